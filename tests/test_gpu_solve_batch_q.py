"""miosqp_qp_solve_batch_q: the lock-step batch with a linear cost of its own in every column (needs an MI355X).

Parity contract: column k is what the engine computes after update(q=Q[k]) + solve_node(l_k, u_k, x0_k, y0_k), and what
the CPU oracle computes after the same calls: status and iteration count exact, x and y within 1e-8 relative, lower within
1e-9, the rounded candidate's objective within 1e-8 (the tolerances and the guards around ties of
test_gpu_parity.py::test_batch_equals_node_by_node, whose wave builder is used here).  With every row of Q equal to the
engine's q the call leaves the bits of solve_batch -- the engine's q being what update(q=) left there, c D q in one
product, which is what the batch kernel computes per column; straight after setup the engine's scaled q still carries the
roundings of the equilibration's passes (last-bit differences), so the engines here are handed their q through update
first, as MIOSQP.update_vectors hands it to them."""
import numpy as np
import pytest

from miosqp_amd import problems
from test_gpu_parity import SOL_TOL, _wave_of_nodes, rel

pytestmark = pytest.mark.gpu


def _costs(q, B, seed):
    """row k = q + 0.3 randn; row 0 the engine's q itself, row 1 all zeros (||q|| = 0 in the relative tolerance: the
    column ends at an early test while others go on), row 2 = 100 q"""
    Q = q[None, :] + 0.3 * np.random.RandomState(seed).randn(B, len(q))
    Q[0] = q
    Q[1] = 0.0
    Q[2] = 100.0 * q
    return Q


def _same_batch(a, b):
    for key in ("status_val", "iter", "x", "y", "lower"):
        np.testing.assert_array_equal(getattr(a, key), getattr(b, key), err_msg=key)


def _check_column(rq, k, r1, ro, pr, A, l, u, qk, Lk, Uk):
    """column k of the per-column batch against the same node on a second engine (r1) and on the oracle (ro)"""
    ii, k_int = pr["i_idx"], len(pr["i_idx"])
    assert rq.status_val[k] == r1.status_val and rq.iter[k] == r1.iter, k
    assert (rq.status_val[k], rq.iter[k]) == (ro.info.status_val, ro.info.iter), k
    if ro.info.status_val not in (1, -2):
        assert np.isnan(rq.lower[k]) and rq.digest[k] is None
        return
    assert rel(rq.x[k], r1.x) <= SOL_TOL and rel(rq.y[k], r1.y) <= SOL_TOL, k
    xo = ro.x.copy()
    xo[ii] = np.minimum(np.maximum(xo[ii], Lk[-k_int:]), Uk[-k_int:])
    assert rel(rq.x[k], xo) <= SOL_TOL and rel(rq.y[k], ro.y) <= SOL_TOL, k
    lo = 0.5 * xo.dot(pr["P"].dot(xo)) + qk.dot(xo)
    assert abs(rq.lower[k] - lo) <= 1e-9 * max(1.0, abs(lo)), k
    assert abs(rq.lower[k] - r1.lower) <= 1e-9 * max(1.0, abs(lo)), k
    dq, d1 = rq.digest[k], r1.digest
    frac = np.abs(xo[ii] - np.round(xo[ii]))
    assert dq.int_inf == d1.int_inf == int(np.sum(frac > 1e-3)), k
    if frac.max() > 1e-6:
        assert dq.nextvar == d1.nextvar == int(np.argmax(frac)), k
    xr = xo.copy()
    xr[ii] = np.round(xo[ii])
    zz = A.dot(xr)
    margin = np.max(np.maximum(l - 1e-3 - zz, zz - u - 1e-3))
    if abs(margin) > 1e-7:
        assert dq.heur_feasible == d1.heur_feasible == bool(margin <= 0), k
    ho = 0.5 * xr.dot(pr["P"].dot(xr)) + qk.dot(xr)
    assert abs(dq.heur_obj - ho) <= 1e-8 * max(1.0, abs(ho)) and abs(d1.heur_obj - ho) <= 1e-8 * max(1.0, abs(ho)), k


@pytest.mark.parametrize("n,m,p,seed,count,fold,cap", [(20, 40, 10, 1, 7, -1, 64), (50, 100, 25, 2, 70, 0, 64),
                                                        (50, 100, 25, 2, 70, 1, 64), (130, 260, 65, 3, 200, -1, 256),
                                                        (37, 3, 20, 4, 9, 1, 64), (33, 2, 16, 6, 9, 0, 64)])
def test_per_column_cost_equals_update_and_solve_node(oracle_mod, n, m, p, seed, count, fold, cap):
    """cap 64 < count: a sliced wave (both factor forms); cap 256, 200 columns: several tiles and compaction -- the
    columns' costs must follow them; m = 3, 2: bound rows outside the products."""
    from miosqp_amd import qp
    pr = problems.random_miqp(n, m, p, seed=seed)
    leaves = _wave_of_nodes(oracle_mod, pr, count)
    B = len(leaves)
    assert B >= 4
    A, l, u = problems.extended(pr)
    g, g2, o = qp.OSQP(), qp.OSQP(), oracle_mod.OSQP()
    g.setup(pr["P"], pr["q"], A, l, u, max_batch=cap, fold=fold, **problems.QP_SETTINGS)
    g2.setup(pr["P"], pr["q"], A, l, u, fold=fold, **problems.QP_SETTINGS)
    o.setup(pr["P"], pr["q"], A, l, u, **problems.QP_SETTINGS)
    for e in (g, g2):
        e.set_integer_rows(pr["i_idx"], m)
        e.set_root(l, u, 1e-3, 1e-3)
    g.update(q=pr["q"])  # (see the module text)
    L = np.stack([lf.l for lf in leaves]); U = np.stack([lf.u for lf in leaves])
    X = np.stack([lf.x for lf in leaves]); Y = np.stack([lf.y for lf in leaves])
    Q = _costs(pr["q"], B, seed)
    rb0 = g.solve_batch(L, U, X, Y)
    n0 = g.solve_node(L[3], U[3], X[3], Y[3])
    c0 = g.compactions()
    rq = g.solve_batch_q(Q, L, U, X, Y)
    c1 = g.compactions()
    for k in range(B):
        g2.update(q=Q[k])
        r1 = g2.solve_node(L[k], U[k], X[k], Y[k])
        o.update(q=Q[k])
        o.update(l=L[k], u=U[k])
        o.warm_start(x=X[k], y=Y[k])
        _check_column(rq, k, r1, o.solve(), pr, A, l, u, Q[k], L[k], U[k])
    assert len(set(rq.iter.tolist())) > 1  # columns end at different tests
    if cap >= 128 and B > 128:
        assert c1 - c0 >= 1  # the wave was compacted (and every column's lower matched its own q above)
    # a second identical call is bit-identical
    _same_batch(rq, g.solve_batch_q(Q, L, U, X, Y))
    # the engine's own q is untouched, the shared-cost chunk graphs are not mixed up with the per-column ones
    _same_batch(rb0, g.solve_batch(L, U, X, Y))
    n1 = g.solve_node(L[3], U[3], X[3], Y[3])
    assert (n0.status_val, n0.iter, n0.lower) == (n1.status_val, n1.iter, n1.lower)
    np.testing.assert_array_equal(n0.x, n1.x)
    np.testing.assert_array_equal(n0.y, n1.y)
    # every row the engine's q: the bits of solve_batch
    _same_batch(rb0, g.solve_batch_q(np.tile(pr["q"], (B, 1)), L, U, X, Y))
    for e in (g, g2):
        e.close()


@pytest.mark.parametrize("B", [150, 300])
def test_per_column_cost_in_the_persistent_batch(B):
    """Shape (100, 62, 42) of test_batched_persistent_chunks_over_shapes with the persistent batch on and B no multiple of
    64.  150 columns: three tiles, kbp1 (the column's cost is one register per thread, as the shared one is); 300 columns:
    kbp, two tiles per group (one more load per column block).  Outcome: neither was called off for per-column batches --
    both leave the bits of the launches, with no fall-back -- and a sample of columns equals update(q) + solve_node."""
    from miosqp_amd import qp
    n, m, p, dens = 100, 62, 42, 0.4
    pr = problems.random_miqp(n, m, p, density=dens, seed=n + m)
    A, l, u = problems.extended(pr)
    rng = np.random.RandomState(p)
    L = np.tile(l, (B, 1)); U = np.tile(u, (B, 1))
    for b in range(B):
        idx = rng.choice(p, size=min(p, 1 + b % 6), replace=False)
        val = rng.randint(0, 2, size=len(idx)).astype(float)
        L[b, m + idx] = val
        U[b, m + idx] = val
    X = np.zeros((B, n)); Y = np.zeros((B, m + p))
    Q = _costs(pr["q"], B, B)
    out = []
    for bp in (0, 1):
        g = qp.OSQP()
        g.setup(pr["P"], pr["q"], A, l, u, **dict(problems.QP_SETTINGS, max_batch=320, batch_pers=bp, max_iter=500))
        g.set_integer_rows(pr["i_idx"], m)
        g.set_root(l, u, 1e-3, 1e-3)
        g.update(q=pr["q"])
        shared = g.solve_batch(L, U, X, Y)
        out.append(g.solve_batch_q(Q, L, U, X, Y))
        assert g.factor_stats()["batch_pers"] == bool(bp) and g.batch_pers_fallbacks() == 0
        _same_batch(shared, g.solve_batch(L, U, X, Y))
        _same_batch(shared, g.solve_batch_q(np.tile(pr["q"], (B, 1)), L, U, X, Y))
        if bp:
            for k in list(range(4)) + [B // 2, B - 1]:
                g.update(q=Q[k])
                r1 = g.solve_node(L[k], U[k], X[k], Y[k])
                assert (out[1].status_val[k], out[1].iter[k]) == (r1.status_val, r1.iter), k
                if r1.status_val in (1, -2):
                    assert rel(out[1].x[k], r1.x) <= SOL_TOL and rel(out[1].y[k], r1.y) <= SOL_TOL, k
                    assert abs(out[1].lower[k] - r1.lower) <= 1e-9 * max(1.0, abs(r1.lower)), k
        g.close()
    _same_batch(out[0], out[1])
    assert len(set(out[1].iter.tolist())) > 1
