"""Inputs that take the lock-step batch path (solve_batch / solve_batch_q, the kb_* / kbm_* / kbp kernels) off
`problems.random_miqp`: the `structured_problems` generators at sizes where every tile is ragged and a wave takes seconds,
widened so that single columns of a wave can be made primal or dual infeasible.  Importable without a GPU; the waves are
built on the CPU oracle (tests/test_batch_structured_cpu.py states what they must contain)."""
import numpy as np
import scipy.sparse as spa

import structured_problems as sp
from miosqp_amd import problems

CASES = {
    "milp": (sp.milp_relaxation, dict(n=60, m=100, p=24, density=0.4, seed=11)),
    "low_rank_P": (sp.low_rank_quadratic, dict(n=80, m=120, p=30, density=0.5, seed=12)),
    "equality_rows": (sp.equality_rows, dict(n=60, m=100, p=20, density=0.5, seed=13)),
    "one_sided_rows": (sp.one_sided_rows, dict(n=70, m=140, p=30, density=0.5, seed=14)),
    "A_5pct": (sp.sparse_rows, dict(n=90, m=180, p=30, density=0.05, seed=16)),
    # seed 52, not structured_problems' 17: at seed 17 (and 18, 29, 37, 46, 53, 56) the primal-infeasible columns are
    # detected after 550 .. 1250 iterations and their certificate E dy / ||.||inf, whose rows are unscaled by factors that
    # differ by 1e8, is beyond the stated rtol 1e-6 / atol 1e-8 on the single-node path already: solve_node misses the
    # oracle's by up to 57 x that tolerance, the batch by up to 52 x, the two differ from each other by as much (measured
    # on an MI355X, both factor forms; every other figure of those columns and waves was inside its tolerance).  At seed
    # 52 detection takes 300 .. 500 iterations and both paths stay below 0.18 x the tolerance; 38 does as well.
    "badly_scaled": (sp.badly_scaled_rows, dict(n=60, m=100, p=20, density=0.5, seed=52)),
    "pc_K3": (sp.power_converter_horizon, dict(K=3)),
    "pc_K4": (sp.power_converter_horizon, dict(K=4, step=7)),
}
RANDOM_STRUCTURED = ("milp", "low_rank_P", "equality_rows", "one_sided_rows", "A_5pct", "badly_scaled")
TWO_TILE_CASES = ("milp", "one_sided_rows", "badly_scaled", "pc_K4")  # the forms with max_batch = 128
MAX_ITER_CASES = ("milp", "badly_scaled")  # the waves that are also run under MAX_ITER
TREE_CASES = ("one_sided_rows", "equality_rows", "A_5pct", "milp")
A_1PCT = (sp.sparse_rows, dict(n=130, m=200, p=50, density=0.01, seed=15))
WAVE = 70
MAX_ITER = 200
EPS_INT = EPS_LIN = 1e-3  # what the tests hand set_root
_CACHE = {}


def make(name):
    fn, kw = CASES[name]
    return fn(**kw)


def widen(pr):
    """(widened instance, k, j): the first continuous variable k (None where every variable is an integer: the power
    converter) loses its row and column of P, its column of A and its cost -- with Q[b, k] = 1 a column of a wave is
    unbounded along e_k --, and a copy of the first non-empty general row j with finite two-sided bounds becomes the new
    last general row with bounds (-inf, +inf): free in every ordinary column, contradicting row j where a column sets
    its bounds above u_j.  The factor keeps its structure class (P = 0 stays P = 0, sparse stays sparse ...)."""
    n = pr["A"].shape[1]
    P, A, q = spa.lil_matrix(pr["P"]), spa.lil_matrix(pr["A"]), np.array(pr["q"], dtype=float)
    cont = sorted(set(range(n)) - set(int(i) for i in pr["i_idx"]))
    k = cont[0] if cont else None
    if k is not None:
        P[k, :] = 0.0
        P[:, k] = 0.0
        A[:, k] = 0.0
        q[k] = 0.0
    A = spa.csr_matrix(A)
    A.eliminate_zeros()
    P = spa.csc_matrix(P)
    P.eliminate_zeros()
    nnz_row = np.diff(A.indptr)
    j = next(r for r in range(A.shape[0]) if nnz_row[r] > 0 and np.isfinite(pr["l"][r]) and np.isfinite(pr["u"][r]))
    out = dict(pr)
    out.update(P=P, q=q, A=spa.vstack([A, A.getrow(j)]).tocsc(), l=np.append(pr["l"], -np.inf),
               u=np.append(pr["u"], np.inf))
    return out, k, j


def widened(name):
    """widen(make(name)), once per session"""
    if ("w", name) not in _CACHE:
        _CACHE["w", name] = widen(make(name))
    return _CACHE["w", name]


def mixed_wave(name, oracle_mod):
    """(Q, L, U, X, Y) of 70 columns on the widened instance `name`: the leaves of test_gpu_parity._wave_of_nodes, the
    duplicate row moved above u_j in the columns b % 7 == 3 (primal infeasible), cost 1 on variable k in the columns
    b % 7 == 5 (dual infeasible; none on the power converter, which has no continuous variable), the instance's q in
    every other row of Q.  Built once per session and handed out as copies."""
    if ("mw", name) not in _CACHE:
        from test_gpu_parity import _wave_of_nodes
        pw, k, j = widened(name)
        leaves = _wave_of_nodes(oracle_mod, pw, WAVE)
        assert len(leaves) == WAVE, (name, len(leaves))
        L = np.stack([lf.l for lf in leaves]); U = np.stack([lf.u for lf in leaves])
        X = np.stack([lf.x for lf in leaves]); Y = np.stack([lf.y for lf in leaves])
        Q = np.tile(pw["q"], (WAVE, 1))
        dup = pw["A"].shape[0] - 1
        uj = pw["u"][j]
        s = max(1.0, abs(uj))
        for b in range(WAVE):
            if b % 7 == 3:
                L[b, dup], U[b, dup] = uj + s, uj + 2 * s
            if b % 7 == 5 and k is not None:
                Q[b, k] = 1.0
        _CACHE["mw", name] = (Q, L, U, X, Y)
    return tuple(v.copy() for v in _CACHE["mw", name])


def all_dual(name):
    """(q, L, U, X, Y): 5 copies of the widened root under the shared cost q with q[k] = 1 -- a wave in which every
    column is dual infeasible, for update(q=) + solve_batch (the kernels without a cost per column)."""
    pw, k, _ = widened(name)
    assert k is not None
    A, l, u = problems.extended(pw)
    q = pw["q"].copy()
    q[k] = 1.0
    return q, np.tile(l, (5, 1)), np.tile(u, (5, 1)), np.zeros((5, A.shape[1])), np.zeros((5, A.shape[0]))


def a_1pct():
    """the 1 % instance, un-widened: columns of A are empty under a non-zero cost, the root is dual infeasible as it is"""
    if "a1" not in _CACHE:
        fn, kw = A_1PCT
        _CACHE["a1"] = fn(**kw)
    return _CACHE["a1"]


def a_1pct_wave():
    """(Q, L, U, X, Y): five columns at the 1 % instance's root, row k of Q = q + 0.3 randn"""
    pr = a_1pct()
    A, l, u = problems.extended(pr)
    Q = pr["q"][None, :] + 0.3 * np.random.RandomState(15).randn(5, len(pr["q"]))
    return Q, np.tile(l, (5, 1)), np.tile(u, (5, 1)), np.zeros((5, A.shape[1])), np.zeros((5, A.shape[0]))


def tree_instances(pr):
    """solve_many's five instances: the model's q, then four times q + 0.3 randn"""
    rng = np.random.RandomState(3)
    return [dict(q=pr["q"].copy())] + [dict(q=pr["q"] + 0.3 * rng.randn(len(pr["q"]))) for _ in range(4)]


def oracle_wave(name, oracle_mod, max_iter=None, shared_q=None):
    """The oracle's answer per column of mixed_wave(name): update(q) + update(l, u) + warm_start + solve.  shared_q: every
    column under that cost instead of its row of Q (what solve_batch computes).  Once per session; leave it unchanged."""
    key = ("ow", name, max_iter, None if shared_q is None else shared_q.tobytes())
    if key not in _CACHE:
        pw = widened(name)[0]
        Q, L, U, X, Y = mixed_wave(name, oracle_mod)
        if shared_q is not None:
            Q = np.tile(shared_q, (len(L), 1))
        _CACHE[key] = oracle_columns(oracle_mod, pw, Q, L, U, X, Y, max_iter)
    return _CACHE[key]


def oracle_columns(oracle_mod, pr, Q, L, U, X, Y, max_iter=None):
    A, l, u = problems.extended(pr)
    o = oracle_mod.OSQP()
    st = dict(problems.QP_SETTINGS) if max_iter is None else dict(problems.QP_SETTINGS, max_iter=max_iter)
    o.setup(pr["P"], pr["q"], A, l, u, **st)
    out = []
    for b in range(len(L)):
        o.update(q=Q[b])
        o.update(l=L[b], u=U[b])
        o.warm_start(x=X[b], y=Y[b])
        out.append(o.solve())
    return out
