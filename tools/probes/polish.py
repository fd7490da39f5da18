"""Polishing of the incumbent (polish_incumbent 1): what it costs and what it changes.

Config 1 and config 2 of problems.random_miqp (seed 0), rho 0.1 and "auto":
  * the whole tree with polish_incumbent 0 and 1 -- wall time, upper_glob before and after, the node re-solve's time;
  * one device polish of the incumbent with its integers fixed: device time split into classification, rows of the
    reduced matrix, factorisation + inverse, solves + refinement + acceptance;
  * whether the two rho modes end on the same integer assignment, and how far their upper_glob are apart before and
    after polishing.
With --repair-iter K > 0, for the config-2 root (both rho) and for config-1 incumbents with their integers fixed (seed 0
at rho 0.1, seed 1 at rho "auto"): the device time of a plain polish, of a repair call as a whole and round by round
(a round's time runs up to the revision's counters), and the host's wait for each round's counters.

    python tools/probes/polish.py [--out profiles/polish.txt] [--reps 5] [--repair-iter 5] [--no-trees]
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


def repair_calls(out, reps, repair_iter):
    """plain polish against the repair call on four inputs, each solved by the engine that then polishes it"""
    out("# repair loop, repair_iter %d: device times in us, medians of %d; a round's time runs from the round before's "
        "counters (round 0: from the call's first event) to its own, `wait` is the host's wait for them" % (repair_iter, reps))
    for label, cfg, seed, rho, incumbent in (("cfg2 root", "cfg2", 0, 0.1, False), ("cfg2 root", "cfg2", 0, "auto", False),
                                             ("cfg1 incumbent", "cfg1", 0, 0.1, True),
                                             ("cfg1 incumbent", "cfg1", 1, "auto", True)):
        c = problems.CONFIGS[cfg]
        pr = problems.random_miqp(c["n"], c["m"], c["p"], density=c["density"], seed=seed)
        m = bnb.MIOSQP()
        m.setup(pr["P"], pr["q"], pr["A"], np.copy(pr["l"]), np.copy(pr["u"]), pr["i_idx"], pr["i_l"], pr["i_u"],
                dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS, rho=rho))
        w, d = m.work, m.work.data
        l, u = d.l.copy(), d.u.copy()
        if incumbent:
            r = m.solve()
            xi = np.round(r.x[d.i_idx])
            l[d.m:] = xi
            u[d.m:] = xi
            node = w.solver.solve_node(l, u, np.array(r.x), np.zeros(d.m + d.n_int))
        else:
            node = w.solver.solve_node(l, u, np.zeros(d.n), np.zeros(d.m + d.n_int))
        plain, whole, rounds, waits = [], [], [], []
        for _ in range(reps):
            p0 = w.solver.polish(l, u, node.x, node.y)
            plain.append(p0.device_time)
            p = w.solver.polish(l, u, node.x, node.y, repair_iter=repair_iter)
            whole.append(p.device_time)
            dev, wait = w.solver.polish_rounds()
            rounds.append(dev[:p.rounds + 1])
            waits.append(wait[:p.rounds + 1])
        rs, ws = 1e6 * np.median(np.array(rounds), axis=0), 1e6 * np.median(np.array(waits), axis=0)
        out("%s seed %d rho %-5r plain: accepted %d reason %d, %d rows, %.1f us | repair: accepted %d, rounds %d stop %d "
            "+%d -%d, %d rows, pri %.1e dua %.1e, %.1f us; rounds %s; wait %s"
            % (label, seed, rho, p0.accepted, p0.reason, p0.n_lower + p0.n_upper, 1e6 * np.median(plain), p.accepted,
               p.rounds, p.stop, p.n_added, p.n_dropped, p.n_lower + p.n_upper, p.pri_after, p.dua_after,
               1e6 * np.median(whole), " ".join("%.1f" % v for v in rs), " ".join("%.1f" % v for v in ws)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--repair-iter", type=int, default=0, help="also time the repair loop with this many rounds at most")
    ap.add_argument("--no-trees", action="store_true", help="skip the whole trees: the single calls only")
    a = ap.parse_args()
    f = open(a.out, "w") if a.out else None

    def out(s=""):
        print(s, flush=True)
        if f:
            f.write(s + "\n")
            f.flush()

    if a.repair_iter > 0:
        repair_calls(out, a.reps, a.repair_iter)
    if a.no_trees:
        if f:
            f.close()
        return
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
    if f:
        f.close()


if __name__ == "__main__":
    main()
