"""Polishing of the incumbent (polish_incumbent 1): what it costs and what it changes.

Config 1 and config 2 of problems.random_miqp (seed 0), rho 0.1 and "auto":
  * the whole tree with polish_incumbent 0 and 1 -- wall time, upper_glob before and after, the node re-solve's time;
  * one device polish of the incumbent with its integers fixed: device time split into classification, rows of the
    reduced matrix, factorisation + inverse, solves + refinement + acceptance;
  * whether the two rho modes end on the same integer assignment, and how far their upper_glob are apart before and
    after polishing.

    python tools/probes/polish.py [--out profiles/polish.txt] [--reps 5]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from miosqp_amd import bnb, problems  # noqa: E402


def tree(pr, rho, on):
    m = bnb.MIOSQP()
    m.setup(pr["P"], pr["q"], pr["A"], np.copy(pr["l"]), np.copy(pr["u"]), pr["i_idx"], pr["i_l"], pr["i_u"],
            dict(problems.BNB_SETTINGS, polish_incumbent=on), dict(problems.QP_SETTINGS, rho=rho))
    t0 = time.time()
    r = m.solve()
    return m, r, time.time() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    out("# polishing of the incumbent (one MI355X), random_miqp seed 0; times are measured, medians of %d" % a.reps)
    for cfg in ("cfg1", "cfg2"):
        c = problems.CONFIGS[cfg]
        pr = problems.random_miqp(c["n"], c["m"], c["p"], density=c["density"], seed=0)
        ints = {}
        for rho in (0.1, "auto"):
            walls = {0: [], 1: []}
            for _ in range(a.reps):
                for on in (0, 1):
                    m, r, wall = tree(pr, rho, on)
                    walls[on].append(wall)
                    if on == 0:
                        plain = r.upper_glob
            w, d = m.work, m.work.data
            st = w.polish_stats
            ints[rho] = (np.round(r.x[d.i_idx]), plain, r.upper_glob)
            out("%s rho %-5r tree wall: off %.4f s, on %.4f s (polish step %.4f s: node re-solve + polish)"
                % (cfg, rho, np.median(walls[0]), np.median(walls[1]), st["time"]))
            out("%s rho %-5r upper_glob: search %.9f -> polished %.9f; accepted %d/%d, %d active rows, pri %.1e dua %.1e"
                % (cfg, rho, plain, r.upper_glob, st["accepted"], st["calls"], st["n_active"], st["pri_after"],
                   st["dua_after"]))
            # one polish call on its own: the fixed node re-solved, then polished `reps` times
            xi = np.round(r.x[d.i_idx])
            l, u = d.l.copy(), d.u.copy()
            l[d.m:] = xi
            u[d.m:] = xi
            node_t, stages, dev = [], [], []
            for _ in range(a.reps):
                t0 = time.time()
                node = w.solver.solve_node(l, u, np.array(r.x), np.zeros(d.m + d.n_int))
                node_t.append(time.time() - t0)
                p = w.solver.polish(l, u, node.x, node.y, w.pol["delta"], w.pol["refine_iter"])
                stages.append(w.solver.polish_stages())
                dev.append(p.device_time)
            s = 1e6 * np.median(np.array(stages), axis=0)
            out("%s rho %-5r node re-solve %.1f us wall (%d iterations); one polish %.1f us device: classify %.1f, "
                "Schur rows %.1f, factor + inverse %.1f, solves + acceptance %.1f"
                % (cfg, rho, 1e6 * np.median(node_t), node.iter, 1e6 * np.median(dev), s[0], s[1], s[2], s[3]))
        same = bool(np.array_equal(ints[0.1][0], ints["auto"][0]))
        out("%s rho 0.1 vs auto: integer parts %s; |upper_glob difference| search %.2e, polished %.2e"
            % (cfg, "agree" if same else "DIFFER", abs(ints[0.1][1] - ints["auto"][1]), abs(ints[0.1][2] - ints["auto"][2])))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
