"""Inputs of the polish_many tests (test_polish_many_cpu.py, test_gpu_polish_many.py) and of tools/probes/polish_many.py:
instances that share P and A and differ in q, and their (l, u, x, y) made by the CPU backend, so that the restatement and
the device classify the same numbers."""
import numpy as np

from miosqp_amd import bnb, problems

import polish_repair_inputs as single


def instances(pr, B):
    """q_b = q + 0.1 RandomState(1000 + b).standard_normal(n), q_0 = q"""
    n = len(pr["q"])
    return [dict(q=np.array(pr["q"], dtype=float) + (0.1 * np.random.RandomState(1000 + b).standard_normal(n) if b else 0.0))
            for b in range(B)]


def crude_inputs(backend, shape, seed, B):
    """(Data, Q, L, U, X, Y): the root of every instance after 25 iterations at rho 0.1, each solved with its own q_b"""
    pr = problems.random_miqp(*shape, seed=seed)
    Q, L, U, X, Y = [], [], [], [], []
    for inst in instances(pr, B):
        d, l, u, x, y = single.root_input(backend, dict(pr, q=inst["q"]), rho=0.1, max_iter=25)
        Q.append(inst["q"]); L.append(l); U.append(u); X.append(x); Y.append(y)
    return (d,) + tuple(np.array(a) for a in (Q, L, U, X, Y))


def guess_inputs(backend, shape, seed, B, tau=1e-2):
    """(Data, Q, L, U, X, Y): the closed tree of every instance -- x with the integers rounded, l, u with the integer rows
    fixed to them, y from bnb.primal_guess_multipliers: what MIOSQP.polish_many hands to the polish"""
    pr = problems.random_miqp(*shape, seed=seed)
    m = single.model(backend, pr)
    inst = instances(pr, B)
    res = m.solve_many(inst)
    d = m.work.data
    Q, L, U, X, Y = [], [], [], [], []
    for i, r in zip(inst, res):
        assert r["status"] == bnb.MI_SOLVED
        x = np.array(r["x"], dtype=float)
        xi = np.round(x[d.i_idx])
        x[d.i_idx] = xi
        l, u = d.l.copy(), d.u.copy()
        l[d.m:] = xi
        u[d.m:] = xi
        Q.append(i["q"]); L.append(l); U.append(u); X.append(x)
        Y.append(bnb.primal_guess_multipliers(l, u, d.A.dot(x), tau))
    return (d,) + tuple(np.array(a) for a in (Q, L, U, X, Y))


def residuals(d, q, l, u, x, y):
    """pri, dua of (x, y) from the original matrices"""
    z = d.A.dot(x)
    pri = max(np.max(l - z), np.max(z - u), 0.0)
    return pri, float(np.max(np.abs(d.P.dot(x) + q + d.A.T.dot(y))))
