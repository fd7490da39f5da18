"""Inputs of the polish_many tests (test_polish_many_cpu.py, test_gpu_polish_many.py, test_polish_reference_cpu.py,
test_gpu_polish_many_edges.py) and of tools/probes/polish_many.py: instances that share P and A and differ in q, and
their (l, u, x, y) made by the CPU backend, so that the restatement and the device classify the same numbers.

The second half is the table of edge inputs (EDGES): each case names a problem, how its (x, y) are made, the batch and
the polish settings, and what the long-double reference must say about it (test_polish_reference_cpu.py asserts that on
the CPU; test_gpu_polish_many_edges.py runs the same inputs through k_pol_many)."""
import types

import numpy as np
import scipy.sparse as spa

from miosqp_amd import bnb, problems

import polish_repair_inputs as single


def instances(pr, B):
    """q_b = q + 0.1 RandomState(1000 + b).standard_normal(n), q_0 = q"""
    n = len(pr["q"])
    return [dict(q=np.array(pr["q"], dtype=float) + (0.1 * np.random.RandomState(1000 + b).standard_normal(n) if b else 0.0))
            for b in range(B)]


def crude_inputs(backend, shape, seed, B):
    """(Data, Q, L, U, X, Y): the root of every instance after 25 iterations at rho 0.1, each solved with its own q_b"""
    return crude_inputs_of(backend, problems.random_miqp(*shape, seed=seed), B)


def crude_inputs_of(backend, pr, B):
    """crude_inputs for a problem dict"""
    Q, L, U, X, Y = [], [], [], [], []
    for inst in instances(pr, B):
        d, l, u, x, y = single.root_input(backend, dict(pr, q=inst["q"]), rho=0.1, max_iter=25)
        Q.append(inst["q"]); L.append(l); U.append(u); X.append(x); Y.append(y)
    return (d,) + tuple(np.array(a) for a in (Q, L, U, X, Y))


def guess_inputs(backend, shape, seed, B, tau=1e-2):
    """(Data, Q, L, U, X, Y): the closed tree of every instance -- x with the integers rounded, l, u with the integer rows
    fixed to them, y from bnb.primal_guess_multipliers: what MIOSQP.polish_many hands to the polish"""
    return guess_inputs_of(backend, problems.random_miqp(*shape, seed=seed), B, tau)


def guess_inputs_of(backend, pr, B, tau=1e-2):
    """guess_inputs for a problem dict"""
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


# ---- edge inputs of k_pol_many -----------------------------------------------------------------------------------------
def _random(shape, seed):
    return lambda: problems.random_miqp(*shape, seed=seed)


def _structured(name, **kw):
    def make():
        import structured_problems as sp
        return getattr(sp, name)(**kw)
    return make


def indefinite_problem(n=70, k=66, seed=0):
    """P a random positive definite block, but row and column k zero with P[k][k] = -1; one general row, x_k; variable 0
    the integer.  Held by its row, x_k gives a positive definite S (the row's 1 / delta); released, pivot k of S is
    -1 + delta.  P + sigma I + 2 A'A (extended A, unscaled) has smallest eigenvalue 1: set-up at rho 2 without scaling
    accepts it."""
    rng = np.random.RandomState(seed)
    G = rng.randn(n, n)
    P = G.dot(G.T) / n + np.eye(n)
    P[k, :] = 0.0
    P[:, k] = 0.0
    P[k, k] = -1.0
    A = np.zeros((1, n))
    A[0, k] = 1.0
    q = rng.randn(n)
    q[k] = -1.0
    return dict(P=spa.csc_matrix(P), q=q, A=spa.csc_matrix(A), l=np.array([0.0]), u=np.array([5.0]),
                i_idx=np.array([0]), i_l=np.zeros(1), i_u=np.ones(1), k=k)


def indefinite_batch(pr):
    """(Q, L, U, X, Y) of four instances on indefinite_problem, rows (x_k, x_0): 0 and 3 healthy (q_k = +1, +2: the row
    x_k >= 0 is active with a negative multiplier, a fixed point), 1 the bad pivot in repair round 1 (the row is held in
    round 0, its multiplier comes out +1, the revision drops it), 2 the bad pivot in round 0 (x_k = 1, y = 0: the row is
    inactive from the start)"""
    n, k = len(pr["q"]), pr["k"]
    Q = np.tile(np.array(pr["q"], dtype=float), (4, 1))
    Q[0, k], Q[3, k] = 1.0, 2.0
    L, U = np.tile([0.0, 0.0], (4, 1)), np.tile([5.0, 0.0], (4, 1))
    X, Y = np.zeros((4, n)), np.tile([-0.5, 0.0], (4, 1))
    X[2, k], Y[2, 0] = 1.0, 0.0
    return Q, L, U, X, Y


def two_variable_problem():
    """the smallest model of the same thing (tests/test_polish_repair_cpu.py): P = diag(1, -1), one row x_2 in [0, 5]"""
    return dict(P=spa.csc_matrix(np.diag([1.0, -1.0])), q=np.array([-2.0, -1.0]), A=spa.csc_matrix(np.array([[0.0, 1.0]])),
                l=np.array([0.0]), u=np.array([5.0]), x=np.array([2.0, 0.0]), y=np.array([-0.5]))


PROBLEMS = {
    "r129_s0": _random((129, 30, 10), 0), "r160_s0": _random((160, 20, 5), 0), "r160_s1": _random((160, 20, 5), 1),
    "r180_s0": _random((180, 8, 3), 0), "r191_s0": _random((191, 0, 1), 0), "r192_s0": _random((192, 2, 1), 0),
    "r20x150_s0": _random((20, 150, 10), 0), "r20x150_s1": _random((20, 150, 10), 1), "r10x170_s0": _random((10, 170, 5), 0),
    "r50_s1": _random((50, 100, 10), 1), "r20_s0": _random((20, 10, 5), 0), "r64_s1": _random((64, 20, 5), 1),
    "one_sided": _structured("one_sided_rows", n=60, m=80, p=10, seed=1),
    "equality": _structured("equality_rows", n=60, m=80, p=10, seed=2),
    "sparse5": _structured("sparse_rows", n=60, m=80, p=10, density=0.05, seed=5),
    "low_rank": _structured("low_rank_quadratic", n=60, m=80, p=10, seed=3),
    "milp": _structured("milp_relaxation", n=40, m=80, p=10, seed=4),
}


def _edge(name, group, prob, kind, repair_iter, B=4, pick=None, delta=1e-6, refine_iter=3, **expect):
    return types.SimpleNamespace(name=name, group=group, prob=prob, kind=kind, repair_iter=repair_iter, B=B, pick=pick,
                                 delta=delta, refine_iter=refine_iter, expect=expect)


# expect: accepted (every instance), rounds (lo, hi) per instance, added (lo, hi) per instance, reason0, stop, reason,
# moves (the case's instances together both add and drop rows)
EDGES = [_edge(p, "segment3", p, "crude", 5, accepted=True)
         for p in ("r129_s0", "r160_s1", "r180_s0", "r191_s0", "r192_s0")]
EDGES += [_edge("r160_s0", "segment3", "r160_s0", "crude", 5, accepted=True, rounds=(2, 4))]
EDGES += [_edge(p, "chunk3", p, "crude", 5, accepted=True, moves=True) for p in ("r20x150_s0", "r20x150_s1", "r10x170_s0")]
for _p in ("r160_s1", "r50_s1"):
    EDGES += [_edge("%s_refine0" % _p, "settings", _p, "crude", 5, refine_iter=0, accepted=True),
              _edge("%s_refine10" % _p, "settings", _p, "crude", 5, refine_iter=10, accepted=True),
              _edge("%s_delta1e-4" % _p, "settings", _p, "crude", 5, delta=1e-4, accepted=True),
              _edge("%s_delta1e-8" % _p, "settings", _p, "crude", 5, delta=1e-8, accepted=True)]
EDGES += [_edge("one_sided_crude", "structured", "one_sided", "crude", 5, accepted=True, rounds=(0, 1)),
          _edge("one_sided_guess", "structured", "one_sided", "guess", 20, accepted=True, rounds=(0, 1)),
          _edge("equality_crude", "structured", "equality", "crude", 5, accepted=True, rounds=(0, 1)),
          _edge("equality_guess", "structured", "equality", "guess", 20, accepted=True, rounds=(0, 1)),
          _edge("sparse5_crude", "structured", "sparse5", "crude", 5, accepted=True, rounds=(0, 1)),
          _edge("low_rank_guess", "structured", "low_rank", "guess", 20, accepted=True, rounds=(0, 1)),
          # instance 0 cycles to the round limit at pri about 1 and its counts depend on the order of the sums: it is
          # no input of this case
          _edge("milp_guess", "P0", "milp", "guess", 20, B=3, pick=(1, 2), accepted=True)]
for _p in ("r20_s0", "r64_s1"):
    EDGES += [_edge("%s_empty" % _p, "empty", _p, "empty", 20, B=3, accepted=True, reason0=2, rounds=(5, 9), added=(27, 46)),
              _edge("%s_empty_norepair" % _p, "empty", _p, "empty", 0, B=3, accepted=False, reason=2, stop=1, rounds=(0, 0))]
EDGE = {c.name: c for c in EDGES}
GROUPS = ("segment3", "chunk3", "settings", "structured", "P0", "empty")

_MADE = {}


def empty_inputs_of(backend, pr, B):
    """(Data, Q, L, U, X, Y) at the root's bounds with x = 0 but 0.25 on the integers and y = 0: every row is strictly
    inside its bounds, so the first active set is empty"""
    d = single.model(backend, pr).work.data
    Q = np.array([i["q"] for i in instances(pr, B)])
    X = np.zeros((B, d.n))
    X[:, d.i_idx] = 0.25
    return d, Q, np.tile(d.l, (B, 1)), np.tile(d.u, (B, 1)), X, np.zeros((B, d.m + d.n_int))


def edge_inputs(backend, case):
    """(Data, Q, L, U, X, Y) of one EDGES case, the picked instances only; made once per (problem, kind, B)"""
    key = (case.prob, case.kind, case.B)
    if key not in _MADE:
        make = dict(crude=crude_inputs_of, guess=guess_inputs_of, empty=empty_inputs_of)[case.kind]
        _MADE[key] = make(backend, PROBLEMS[case.prob](), case.B)
    d, arrs = _MADE[key][0], _MADE[key][1:]
    if case.pick is not None:
        arrs = tuple(a[list(case.pick)] for a in arrs)
    return (d,) + tuple(arrs)


def edge_references(case, data):
    """[(long double, float64)] records per instance of the case (polish_reference.both: computed once, not to be
    written to)"""
    import polish_reference as ref
    d, Q, L, U, X, Y = data
    idx = case.pick if case.pick is not None else range(len(Q))
    return [ref.both((case.prob, case.kind, case.B, i), d.P, Q[b], d.A, L[b], U[b], X[b], Y[b], case.delta,
                     case.refine_iter, case.repair_iter) for b, i in enumerate(idx)]


def structure_counts():
    """what the structured problems hold, counted on their general rows: infinite bounds, equality rows, empty rows and
    columns of A, the rank of P"""
    out = {}
    for name in ("one_sided", "equality", "sparse5", "low_rank", "milp"):
        pr = PROBLEMS[name]()
        A, P = np.asarray(pr["A"].todense()), np.asarray(pr["P"].todense())
        l, u = np.asarray(pr["l"]), np.asarray(pr["u"])
        out[name] = dict(n=A.shape[1], M=A.shape[0] + len(pr["i_idx"]), l_inf=int(np.sum(l == -np.inf)),
                         u_inf=int(np.sum(u == np.inf)), free=int(np.sum((l == -np.inf) & (u == np.inf))),
                         eq_general=int(np.sum(l == u)), empty_rows=int(np.sum(~np.any(A != 0.0, axis=1))),
                         empty_cols=int(np.sum(~np.any(A != 0.0, axis=0))), rank_P=int(np.linalg.matrix_rank(P)),
                         nnz_P=int(np.count_nonzero(P)))
    return out
