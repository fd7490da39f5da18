"""Round and fix (primal_heuristic 1) against the search without it (primal_heuristic 0), per tree.

Config 1 (20 MIQPs) and config 2 (5 MIQPs) of problems.random_miqp, rho 0.1 and "auto": nodes, node ADMM iterations,
heuristic calls, feasible candidates and their ADMM iterations, the node after which the first incumbent exists, wall
time to close.  Three legs per tree: "0h" is primal_heuristic 0 on the default path (the hosted search: the baseline),
"0p" is primal_heuristic 0 in MIOSQP.solve's Python loop (what the heuristic's leg pays for leaving the hosted search),
"1" is primal_heuristic 1 (Python loop, solve_node + round_and_fix).  Then the device time of one round_and_fix call on
config 2's root for rf_max_iter 100, 250 and the default.

    python tools/probes/round_and_fix.py [--out FILE] [--cfg1 20] [--cfg2 5]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from miosqp_amd import bnb, problems  # noqa: E402


def tree(pr, leg, rho):
    settings = dict(problems.BNB_SETTINGS, primal_heuristic=1 if leg == "1" else 0)
    if leg == "0p":
        settings.update(device_search=False, device_tree=False)
    m = bnb.MIOSQP()
    m.setup(pr["P"], pr["q"], pr["A"], pr["l"], pr["u"], pr["i_idx"], pr["i_l"], pr["i_u"], settings,
            dict(problems.QP_SETTINGS, rho=rho))
    first = []

    def obs(w, leaf):
        if not first and np.isfinite(w.upper_glob):
            first.append(w.iter_num)

    t0 = time.time()
    r = m.solve(observer=None if leg == "0h" else obs)
    wall = time.time() - t0
    w = m.work
    rf = w.rf_stats
    return dict(status=r.status, upper=r.upper_glob, nodes=w.iter_num - 1, iters=w.osqp_iter, calls=rf["calls"],
                feasible=rf["feasible"], improved=rf["improved"], rf_iters=rf["osqp_iter"], rf_time=rf["solve_time"],
                first=first[0] if first else -1, wall=wall)


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

    out("# round and fix vs none, per tree (one MI355X; leg 0h = hosted search, 0p / 1 = Python loop without / with)")
    out("# cols: cfg seed rho leg status upper nodes node_iters rf_calls rf_feasible rf_improved rf_iters first_incumbent_node "
        "wall_ms rf_ms")
    summary = {}
    for cfg, count in (("cfg1", a.cfg1), ("cfg2", a.cfg2)):
        c = problems.CONFIGS[cfg]
        for seed in range(count):
            pr = problems.random_miqp(c["n"], c["m"], c["p"], density=c["density"], seed=seed)
            for rho in (0.1, "auto"):
                for leg in ("0h", "0p", "1"):
                    t = tree(pr, leg, rho)
                    out("%s %2d %-4s %-2s %-18s %14.8g %6d %8d %4d %4d %3d %8d %5d %10.2f %9.2f" % (
                        cfg, seed, rho, leg, t["status"].replace(" ", "_"), t["upper"], t["nodes"], t["iters"],
                        t["calls"], t["feasible"], t["improved"], t["rf_iters"], t["first"], 1e3 * t["wall"],
                        1e3 * t["rf_time"]))
                    s = summary.setdefault((cfg, rho, leg), np.zeros(8))
                    s += [1, t["nodes"], t["iters"], t["calls"], t["feasible"], t["rf_iters"], t["wall"], t["rf_time"]]
    out()
    out("# totals per (cfg, rho, leg): trees nodes node_iters rf_calls rf_feasible rf_iters wall_s rf_s")
    for (cfg, rho, leg), s in summary.items():
        out("%s %-4s %-2s  %3d %7d %9d %5d %5d %9d %9.3f %8.3f" % (cfg, rho, leg, s[0], s[1], s[2], s[3], s[4], s[5], s[6],
                                                                 s[7]))

    c = problems.CONFIGS["cfg2"]
    pr = problems.random_miqp(c["n"], c["m"], c["p"], density=c["density"], seed=0)
    for rho in (0.1, "auto"):
        out()
        out("# one round_and_fix call (K = 7) on config 2's root (seed 0, rho %s): device ms / wall ms (median of 5)" % rho)
        m = bnb.MIOSQP()
        m.setup(pr["P"], pr["q"], pr["A"], pr["l"], pr["u"], pr["i_idx"], pr["i_l"], pr["i_u"],
                dict(problems.BNB_SETTINGS, primal_heuristic=1), dict(problems.QP_SETTINGS, rho=rho))
        w = m.work
        leaf = w.leaves.pop()
        leaf.solve()
        for cap in (100, 250, w.rf["max_iter"]):
            dev, wall = [], []
            for _ in range(6):
                r = w.solver.round_and_fix(leaf.l, leaf.u, leaf.x, leaf.y, np.inf, w.rf["K"], cap)
                dev.append(r.device_time)
                wall.append(r.run_time)
            dev, wall = dev[1:], wall[1:]  # the first call of a shape captures its chunk graphs
            best = "none" if r.chosen < 0 else "%.6f" % r.obj[r.chosen]
            out("rf_max_iter %4d  device %8.3f ms  wall %8.3f ms  candidate iters %5d  feasible %d  chosen %2d  objective %s"
                % (cap, 1e3 * np.median(dev), 1e3 * np.median(wall), r.iters, r.feasible, r.chosen, best))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
