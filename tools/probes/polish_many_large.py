"""B polishes in one launch beyond one workgroup's LDS (OSQP.polish_many_large, k_pol_many_g) against the two ways the
same work was done before it: (a) B x (update(q=) + polish(..., repair_iter=20)) on the engine, one after the other, and
(b) bnb.polish_restatement per instance on the host -- what solve_many(polish=True) falls back to at these sizes.

Shapes (257, 40, 5) and config 2 (500, 1000, 250) of problems.random_miqp (seed 0); B = 1, 8, 64, 256 instances that share
P and A and differ in q (q_b = q + 0.1 N(0, 1), q_0 = q).  Inputs: the crude root of every instance (25 iterations at
rho 0.1 on a second engine); at config 2 also the incumbents of closed lock-step trees as MIOSQP.polish_many hands them
over (integers rounded and fixed, y from bnb.primal_guess_multipliers with tau = 10 eps_abs), B = 8 and 64.
  * large: the device time of ONE polish_many_large call (between the events around its copy down, launch and copy
    back), median of `reps`, and that per instance; the Python call's wall time;
  * (a): the sum of the B calls' device times and the wall time of the sequence, median of `reps` (of 3 from B = 64);
  * (b): the host's seconds per instance, measured once on the first min(B, 4) instances;
  * the ratios (a) / large of device and wall times, (b) / large per instance on the wall clock, and whether large and
    (a) gave the same integer fields.

    python tools/probes/polish_many_large.py [--out profiles/polish_many_large.txt] [--reps 7]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from miosqp_amd import bnb, problems  # noqa: E402

SHAPES = [(257, 40, 5), (500, 1000, 250)]
BATCHES = [1, 8, 64, 256]
TREE_BATCHES = [8, 64]
FIELDS = ("accepted", "reason", "rounds", "stop", "n_added", "n_dropped", "n_lower", "n_upper")


def model(pr, **qp_extra):
    m = bnb.MIOSQP()
    m.setup(pr["P"], pr["q"], pr["A"], np.copy(pr["l"]), np.copy(pr["u"]), pr["i_idx"], pr["i_l"], pr["i_u"],
            dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS, **qp_extra))
    return m


def costs(pr, B):
    n = len(pr["q"])
    return [np.array(pr["q"], dtype=float) + (0.1 * np.random.RandomState(1000 + b).standard_normal(n) if b else 0.0)
            for b in range(B)]


def crude_inputs(pr, B):
    """(Q, L, U, X, Y): every instance's root after 25 iterations at rho 0.1"""
    m = model(pr, rho=0.1, max_iter=25)
    d, eng = m.work.data, m.work.solver
    M = d.m + d.n_int
    Q, X, Y = costs(pr, B), [], []
    for q in Q:
        eng.update(q=q)
        r = eng.solve_node(d.l, d.u, np.zeros(d.n), np.zeros(M))
        X.append(r.x.copy()); Y.append(r.y.copy())
    eng.close()
    return np.array(Q), np.tile(d.l, (B, 1)), np.tile(d.u, (B, 1)), np.array(X), np.array(Y)


def tree_inputs(m, pr, B, tau):
    """(Q, L, U, X, Y) of B closed lock-step trees, as MIOSQP.polish_many builds them, and the seconds the trees took"""
    d = m.work.data
    inst = [dict(q=q) for q in costs(pr, B)]
    t0 = time.time()
    res = m.solve_many(inst)
    dt = time.time() - t0
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
    return tuple(np.array(a)[idx] for a in (Q, L, U, X, Y)), len(Q), dt


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

    def measure(tag, m, pr, data, B):
        eng, d = m.work.solver, m.work.data
        Q, L, U, X, Y = data
        q0 = np.array(pr["q"], dtype=float)
        eng.polish_many_large(Q, L, U, X, Y, 1e-6, 3, 20)  # (the first call allocates)
        dev, wall = [], []
        for _ in range(a.reps):
            t0 = time.time()
            recs = eng.polish_many_large(Q, L, U, X, Y, 1e-6, 3, 20)
            wall.append(time.time() - t0)
            dev.append(recs[0].device_time)
        one_dev, one_wall = [], []
        for _ in range(a.reps if B < 64 else min(a.reps, 3)):
            t0 = time.time()
            singles = []
            for b in range(B):
                eng.update(q=Q[b])
                singles.append(eng.polish(L[b], U[b], X[b], Y[b], 1e-6, 3, repair_iter=20))
            one_wall.append(time.time() - t0)
            one_dev.append(sum(r.device_time for r in singles))
        eng.update(q=q0)
        nh = min(B, 4)
        t0 = time.time()
        host = [bnb.polish_restatement(d.P, Q[b], d.A, L[b], U[b], X[b], Y[b], 1e-6, 3, repair_iter=20) for b in range(nh)]
        host_s = (time.time() - t0) / nh
        same = all(getattr(r, k) == getattr(s, k) for r, s in zip(recs, singles) for k in FIELDS)
        same_h = all(getattr(r, k) == getattr(s, k) for r, s in zip(recs, host) for k in FIELDS)
        md, mw, sd, sw = (1e3 * np.median(v) for v in (dev, wall, one_dev, one_wall))
        out("%-15s %-6s %4d %10.2f %8.3f %9.2f | %10.2f %8.3f %10.2f | %9.1f | %8.2f %8.2f %9.1f | %3d..%-3d %5d/%-4d %s %s"
            % ("(%d,%d,%d)" % (d.n, d.m, d.n_int), tag, B, md, md / B, mw, sd, sd / B, sw, 1e3 * host_s, sd / md, sw / mw,
               1e3 * host_s * B / mw, min(r.rounds for r in recs), max(r.rounds for r in recs),
               sum(1 for r in recs if r.accepted and r.stop == 0), B, "yes" if same else "NO", "yes" if same_h else "NO"))

    tau = 10 * problems.QP_SETTINGS["eps_abs"]
    out("# polish_many_large (ONE launch, k_pol_many_g) against (a) B x (update(q=) + polish(repair_iter=20)) and (b) the "
        "host's polish_restatement per instance; one MI355X, random_miqp seed 0, delta 1e-6, refine_iter 3, repair_iter 20; "
        "times in ms, medians of %d ((a): of 3 from B = 64; (b): once, on min(B, 4) instances)" % a.reps)
    out("# shape           input     B  large:call    /inst      wall |   (a): sum    /inst       wall | (b) /inst | "
        "(a)/large dev, wall; (b)/large wall | rounds  accepted+fixed  same as (a) (b)")
    for shape in SHAPES:
        pr = problems.random_miqp(*shape, seed=0)
        m = model(pr)
        for B in BATCHES:
            measure("crude", m, pr, crude_inputs(pr, B), B)
        if shape == (500, 1000, 250):
            for B in TREE_BATCHES:
                data, closed, dt = tree_inputs(m, pr, B, tau)
                measure("trees", m, pr, data, B)
                out("#   (the %d lock-step trees took %.2f s, %d closed%s)"
                    % (B, dt, closed, "" if closed == B else "; the others were replaced by closed ones"))
        m.work.solver.close()
    if f:
        f.close()


if __name__ == "__main__":
    main()
