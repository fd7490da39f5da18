"""B polishes in one launch (OSQP.polish_many) against B single polishes in a row: what an instance costs either way.

Shapes (50, 100, 10), (18, 27, 6) and (128, 30, 10) of problems.random_miqp (seed 0); B = 1, 8, 64, 256 instances that
share P and A and differ in q (q_b = q + 0.1 N(0, 1), q_0 = q).  The inputs are what MIOSQP.polish_many hands over: the
closed tree of every instance (solve_many), its integers rounded and fixed, y from bnb.primal_guess_multipliers with
tau = 10 eps_abs; repair_iter 20.
  * many: the device time of ONE polish_many call (between the events around its copy down, launch and copy back),
    median of `reps`, and that per instance; its wall time;
  * single: the same B inputs through update(q=q_b) + polish(..., repair_iter=20) one after the other -- the sum of the
    calls' device times, median of `reps`, per instance; the wall time of the whole sequence;
  * the ratio single / many of the device times and of the wall times, and whether both gave the same integer fields.

    python tools/probes/polish_many.py [--out profiles/polish_many.txt] [--reps 7]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from miosqp_amd import bnb, problems  # noqa: E402

SHAPES = [(50, 100, 10), (18, 27, 6), (128, 30, 10)]
BATCHES = [1, 8, 64, 256]
FIELDS = ("accepted", "reason", "rounds", "stop", "n_added", "n_dropped", "n_lower", "n_upper")


def inputs(m, pr, B, tau):
    """(Q, L, U, X, Y) of B closed trees, as MIOSQP.polish_many builds them"""
    d = m.work.data
    n = d.n
    inst = [dict(q=np.array(pr["q"], dtype=float) + (0.1 * np.random.RandomState(1000 + b).standard_normal(n) if b else 0.0))
            for b in range(B)]
    res = m.solve_many(inst)
    Q, L, U, X, Y = [], [], [], [], []
    for i, r in zip(inst, res):
        if r["status"] != bnb.MI_SOLVED:
            continue
        x = np.array(r["x"], dtype=float)
        xi = np.round(x[d.i_idx])
        x[d.i_idx] = xi
        l, u = d.l.copy(), d.u.copy()
        l[d.m:] = xi
        u[d.m:] = xi
        Q.append(i["q"]); L.append(l); U.append(u); X.append(x)
        Y.append(bnb.primal_guess_multipliers(l, u, d.A.dot(x), tau))
    idx = np.arange(B) % len(Q)  # (a tree that did not close is replaced by one that did)
    return tuple(np.array(a)[idx] for a in (Q, L, U, X, Y)), len(Q)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    f = open(a.out, "w") if a.out else None

    def out(s=""):
        print(s, flush=True)
        if f:
            f.write(s + "\n")
            f.flush()

    tau = 10 * problems.QP_SETTINGS["eps_abs"]
    out("# polish_many against B single polishes (one MI355X), random_miqp seed 0, primal-guess inputs of closed trees, "
        "tau %g, repair_iter 20; device times in us, medians of %d" % (tau, a.reps))
    out("# shape            B   many: call   /inst    wall | single: sum   /inst    wall | device ratio  wall ratio | rounds  accepted+fixed  same")
    for shape in SHAPES:
        pr = problems.random_miqp(*shape, seed=0)
        m = bnb.MIOSQP()
        m.setup(pr["P"], pr["q"], pr["A"], np.copy(pr["l"]), np.copy(pr["u"]), pr["i_idx"], pr["i_l"], pr["i_u"],
                dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS))
        eng = m.work.solver
        q0 = np.array(pr["q"], dtype=float)
        for B in BATCHES:
            (Q, L, U, X, Y), closed = inputs(m, pr, B, tau)
            many_dev, many_wall, one_dev, one_wall = [], [], [], []
            eng.polish_many(Q, L, U, X, Y, 1e-6, 3, 20)  # (the first call allocates)
            for _ in range(a.reps):
                t0 = time.time()
                recs = eng.polish_many(Q, L, U, X, Y, 1e-6, 3, 20)
                many_wall.append(time.time() - t0)
                many_dev.append(recs[0].device_time)
                t0 = time.time()
                singles = []
                for b in range(B):
                    eng.update(q=Q[b])
                    singles.append(eng.polish(L[b], U[b], X[b], Y[b], 1e-6, 3, repair_iter=20))
                one_wall.append(time.time() - t0)
                one_dev.append(sum(r.device_time for r in singles))
            eng.update(q=q0)
            same = all(getattr(r, k) == getattr(s, k) for r, s in zip(recs, singles) for k in FIELDS)
            md, mw, sd, sw = (1e6 * np.median(v) for v in (many_dev, many_wall, one_dev, one_wall))
            out("%-16s %4d %11.1f %7.2f %7.1f | %11.1f %7.2f %7.1f | %12.2f %11.2f | %6d %9d/%-4d  %s"
                % ("(%d,%d,%d)" % shape, B, md, md / B, mw, sd, sd / B, sw, sd / md, sw / mw, max(r.rounds for r in recs),
                   sum(1 for r in recs if r.accepted and r.stop == 0), B, "yes" if same else "NO"))
            if closed < B:
                out("#   (%d of %d trees closed; the others were replaced by closed ones)" % (closed, B))
    if f:
        f.close()


if __name__ == "__main__":
    main()
