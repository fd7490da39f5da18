"""Strong branching (branching_rule 1) and reliability branching (rule 2) against most fractional (rule 0), per tree.

Config 1 (20 MIQPs) and config 2 (5 MIQPs) of problems.random_miqp, rho 0.1 and "auto": nodes, node ADMM iterations,
strong-branching calls and their ADMM iterations, wall time to close.  Rule 0 runs the default path (the hosted search);
rules 1 and 2 run MIOSQP.solve's Python loop (solve_node + strong_branch).  Then the device time of one strong_branch
call on config 2's root for K = 4, 8, 16 and sb_max_iter = 25, 50, 100.

    python tools/probes/strong_branching.py [--out FILE] [--cfg1 20] [--cfg2 5]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from miosqp_amd import bnb, problems  # noqa: E402


def tree(pr, rule, rho):
    m = bnb.MIOSQP()
    m.setup(pr["P"], pr["q"], pr["A"], pr["l"], pr["u"], pr["i_idx"], pr["i_l"], pr["i_u"],
            dict(problems.BNB_SETTINGS, branching_rule=rule), dict(problems.QP_SETTINGS, rho=rho))
    t0 = time.time()
    r = m.solve()
    wall = time.time() - t0
    w = m.work
    return dict(status=r.status, upper=r.upper_glob, nodes=w.iter_num - 1, iters=w.osqp_iter, sb_calls=w.sb_stats["calls"],
                sb_iters=w.sb_stats["osqp_iter"], wall=wall)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cfg1", type=int, default=20)
    ap.add_argument("--cfg2", type=int, default=5)
    a = ap.parse_args()
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    out("# strong / reliability branching vs most fractional, per tree (one MI355X; rule 0 = hosted search)")
    out("# cols: cfg seed rho rule status upper nodes node_iters sb_calls sb_iters wall_ms")
    summary = {}
    for cfg, count in (("cfg1", a.cfg1), ("cfg2", a.cfg2)):
        c = problems.CONFIGS[cfg]
        for seed in range(count):
            pr = problems.random_miqp(c["n"], c["m"], c["p"], density=c["density"], seed=seed)
            for rho in (0.1, "auto"):
                for rule in (0, 1, 2):
                    t = tree(pr, rule, rho)
                    out("%s %2d %-4s %d %-18s %14.8g %6d %8d %5d %8d %10.2f" % (
                        cfg, seed, rho, rule, t["status"].replace(" ", "_"), t["upper"], t["nodes"], t["iters"],
                        t["sb_calls"], t["sb_iters"], 1e3 * t["wall"]))
                    s = summary.setdefault((cfg, rho, rule), np.zeros(6))
                    s += [1, t["nodes"], t["iters"], t["sb_calls"], t["sb_iters"], t["wall"]]
    out()
    out("# totals per (cfg, rho, rule): trees nodes node_iters sb_calls sb_iters wall_s")
    for (cfg, rho, rule), s in summary.items():
        out("%s %-4s %d  %3d %7d %9d %6d %9d %9.3f" % (cfg, rho, rule, s[0], s[1], s[2], s[3], s[4], s[5]))

    out()
    out("# one strong_branch call on config 2's root (seed 0, rho 0.1): device ms / wall ms (median of 5)")
    c = problems.CONFIGS["cfg2"]
    pr = problems.random_miqp(c["n"], c["m"], c["p"], density=c["density"], seed=0)
    m = bnb.MIOSQP()
    m.setup(pr["P"], pr["q"], pr["A"], pr["l"], pr["u"], pr["i_idx"], pr["i_l"], pr["i_u"],
            dict(problems.BNB_SETTINGS, branching_rule=1), dict(problems.QP_SETTINGS))
    w = m.work
    leaf = w.leaves.pop()
    leaf.solve()
    w.is_int_feas(leaf.x, leaf)
    frac = sorted(leaf.frac_idx)
    out("# root: %d fractional positions" % len(frac))
    for K in (4, 8, 16):
        cand = w._most_fractional(leaf, frac, K)
        for cap in (25, 50, 100):
            dev, wall = [], []
            for _ in range(6):
                r = w.solver.strong_branch(leaf.l, leaf.u, leaf.x, leaf.y, leaf.lower, cand, cap, 1e-6)
                dev.append(r.device_time)
                wall.append(r.run_time)
            dev, wall = dev[1:], wall[1:]  # the first call of a shape captures its chunk graphs
            out("K %2d  sb_max_iter %3d  device %7.3f ms  wall %7.3f ms  child iters %d" % (
                K, cap, 1e3 * np.median(dev), 1e3 * np.median(wall), r.iters))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
