"""The exploration rules against each other, per tree: tree_explor_rule 1 (the default: depth first, then the largest
bound), 2 (best bound) and 3 (depth first until the first incumbent, then best bound).

Config 1 (20 MIQPs) and config 2 (5 MIQPs) of problems.random_miqp -- the trees of DESIGN 3g and 3h --, rho 0.1 and
"auto".  Legs per tree: "d1" "d2" "d3" are rules 1, 2, 3 on the default path of MIOSQP.solve (config 1: the one-launch
tree k_tree; config 2: the hosted search); "h1" "h3" are rules 1 and 3 with primal_heuristic 1 (round and fix: the
Python loop).  Per leg: nodes, ADMM iterations, wall time to close, the largest number of open leaves (one-launch tree:
the launch's own max_leaves; hosted search: counted in a second, untimed search that steps node by node; Python loop:
counted by an observer).  Then k_tree's device time per node on config 1 under the rules given by --kernel-rules.

    python tools/probes/explor_rules.py [--out FILE] [--cfg1 20] [--cfg2 5]
    python tools/probes/explor_rules.py --kernel-only --kernel-rules 1 --package-root OTHER_CHECKOUT

--package-root imports miosqp_amd from another checkout (with its library built): the parent commit's k_tree under
rule 1, measured in the same session as this one's.
"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def tree(bnb, problems, pr, leg, rho):
    rule, rf = int(leg[1]), leg[0] == "h"
    m = bnb.MIOSQP()
    m.setup(pr["P"], pr["q"], pr["A"], pr["l"], pr["u"], pr["i_idx"], pr["i_l"], pr["i_u"],
            dict(problems.BNB_SETTINGS, tree_explor_rule=rule, primal_heuristic=1 if rf else 0),
            dict(problems.QP_SETTINGS, rho=rho))
    w = m.work
    longest = [1]

    def obs(work, leaf):
        longest[0] = max(longest[0], len(work.leaves))

    t0 = time.time()
    r = m.solve(observer=obs if rf else None)
    wall = time.time() - t0
    form = "loop"
    info = getattr(w, "tree_info", None)
    if not rf:
        if info is not None and not info.overflow:
            form, longest[0] = "tree", int(info.max_leaves)
        elif getattr(w, "_hosted", None) is not None:
            form = "hosted"
        elif info is not None:
            form, longest[0] = "tree-overflow", -1  # (more than 1024 leaves alive: the Python loop redid the search)
    out = dict(status=r.status, upper=r.upper_glob, nodes=w.iter_num - 1, iters=w.osqp_iter, wall=wall, form=form,
               dev=w.osqp_solve_time)
    if form == "hosted":
        # the same search again, a node per call: the open-leaf count after every node (untimed)
        m.update_vectors(q=pr["q"])
        hs = w._hosted
        hs.begin_instance()
        alive, nodes = 1, 0
        while alive > 0 and nodes < problems.BNB_SETTINGS["max_iter_bb"]:
            alive = hs.step(1)
            nodes += 1
            longest[0] = max(longest[0], int(hs._open))
        if nodes != out["nodes"]:
            out["form"] = "hosted(recount %d nodes)" % nodes
    out["longest"] = longest[0]
    w.solver.close()
    return out


def kernel_time(bnb, problems, rule, rho, count, reps):
    """k_tree's device seconds per node over config 1's `count` trees under `rule`: `reps` passes, each over all trees"""
    c = problems.CONFIGS["cfg1"]
    models = []
    for seed in range(count):
        pr = problems.random_miqp(c["n"], c["m"], c["p"], density=c["density"], seed=seed)
        m = bnb.MIOSQP()
        m.setup(pr["P"], pr["q"], pr["A"], pr["l"], pr["u"], pr["i_idx"], pr["i_l"], pr["i_u"],
                dict(problems.BNB_SETTINGS, tree_explor_rule=rule), dict(problems.QP_SETTINGS, rho=rho))
        models.append((m, pr))
    passes = []
    for rep in range(reps + 1):
        dev, nodes, iters = 0.0, 0, 0
        for m, pr in models:
            m.update_vectors(q=pr["q"])
            m.solve()
            dev += m.work.osqp_solve_time
            nodes += m.work.iter_num - 1
            iters += m.work.osqp_iter
        if rep:  # (the first pass pays the one-time allocations)
            passes.append((dev / nodes, nodes, iters))
    for m, _ in models:
        m.work.solver.close()
    return passes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cfg1", type=int, default=20)
    ap.add_argument("--cfg2", type=int, default=5)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--kernel-rules", default="1,3")
    ap.add_argument("--kernel-reps", type=int, default=5)
    ap.add_argument("--package-root", default=HERE)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    from miosqp_amd import bnb, problems  # noqa: E402
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    out("# package: %s" % os.path.dirname(os.path.abspath(bnb.__file__)))
    if not a.kernel_only:
        out("# exploration rules per tree (one MI355X; legs d1 d2 d3 = rules 1 2 3 on the default path, h1 h3 = rules 1 3 "
            "with round and fix in the Python loop)")
        out("# cols: cfg seed rho leg form status upper nodes iters wall_ms longest_leaf_list")
        summary = {}
        for cfg, count in (("cfg1", a.cfg1), ("cfg2", a.cfg2)):
            c = problems.CONFIGS[cfg]
            for seed in range(count):
                pr = problems.random_miqp(c["n"], c["m"], c["p"], density=c["density"], seed=seed)
                for rho in (0.1, "auto"):
                    for leg in ("d1", "d2", "d3", "h1", "h3"):
                        t = tree(bnb, problems, pr, leg, rho)
                        out("%s %2d %-4s %-2s %-14s %-18s %14.8g %6d %8d %10.2f %5d" % (
                            cfg, seed, rho, leg, t["form"], t["status"].replace(" ", "_"), t["upper"], t["nodes"], t["iters"],
                            1e3 * t["wall"], t["longest"]))
                        s = summary.setdefault((cfg, rho, leg), np.zeros(5))
                        s += [1, t["nodes"], t["iters"], t["wall"], 0]
                        s[4] = max(s[4], t["longest"])
        out()
        out("# totals per (cfg, rho, leg): trees nodes iters wall_s longest_leaf_list")
        for (cfg, rho, leg), s in summary.items():
            out("%s %-4s %-2s  %3d %7d %9d %9.3f %5d" % (cfg, rho, leg, s[0], s[1], s[2], s[3], s[4]))
        out()
    out("# k_tree on config 1 (%d trees, %d passes after one warm-up): device us per node [min median max], nodes, iters"
        % (a.cfg1, a.kernel_reps))
    for rho in (0.1, "auto"):
        for rule in [int(v) for v in a.kernel_rules.split(",")]:
            ps = kernel_time(bnb, problems, rule, rho, a.cfg1, a.kernel_reps)
            us = sorted(1e6 * p[0] for p in ps)
            out("ktree rho %-4s rule %d  %8.2f %8.2f %8.2f  %6d %8d" % (rho, rule, us[0], float(np.median(us)), us[-1],
                                                                        ps[0][1], ps[0][2]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
