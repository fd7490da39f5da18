"""The inputs of tests/test_gpu_batch_structured.py are what that file takes them for, shown on the CPU oracle alone:
every wave holds the statuses it is meant to mix, its columns end at different tests, and no column stands within 1e-7 of
a decision that two correct arithmetic paths could take differently (a tie for the branching position, a fractionality
at eps_int, a rounded point on the feasibility threshold).  These are conditions on the inputs, not measurements: if a
change to a generator breaks one, change the seed, not the cap.  The long-double reference of tests/batch_reference.py is
checked here against the double expressions of test_gpu_parity.py::test_batch_equals_node_by_node."""
import collections

import numpy as np
import pytest

import batch_reference as br
import batch_structured_inputs as bi
from miosqp_amd import bnb, problems

GUARD = 1e-7
SOLVED, MAX_ITER, PRIMAL_INF, DUAL_INF = 1, -2, -3, -4


def _counts(res):
    return dict(collections.Counter(r.info.status_val for r in res))


def _clamped(pw, r, Lb, Ub):
    ii, p = pw["i_idx"], len(pw["i_idx"])
    xo = r.x.copy()
    xo[ii] = np.minimum(np.maximum(xo[ii], Lb[-p:]), Ub[-p:])
    return xo


def _references(pw, Q, L, U, res):
    """the long-double reference of every column with an x, on the oracle's clamped point"""
    A, l, u = problems.extended(pw)
    Pd, Ad = br.dense_ld(pw["P"]), br.dense_ld(A)
    out = {}
    for b, r in enumerate(res):
        if r.info.status_val in (SOLVED, MAX_ITER):
            xo = _clamped(pw, r, L[b], U[b])
            out[b] = (xo, br.column(xo, Q[b], Pd, Ad, l, u, pw["i_idx"], bi.EPS_INT, bi.EPS_LIN))
    return out


def _assert_no_guard(name, refs):
    for b, (_, c) in refs.items():
        assert c.guard_tie > GUARD, (name, b, c.guard_tie)
        assert c.guard_int > GUARD, (name, b, c.guard_int)
        assert c.guard_viol > GUARD, (name, b, c.guard_viol)


@pytest.mark.parametrize("name", list(bi.CASES))
def test_mixed_wave_holds_what_it_is_meant_to_mix(oracle_mod, name):
    pw, k, j = bi.widened(name)
    Q, L, U, X, Y = bi.mixed_wave(name, oracle_mod)
    res = bi.oracle_wave(name, oracle_mod)
    want = {SOLVED: 50, PRIMAL_INF: 10, DUAL_INF: 10} if k is not None else {SOLVED: 60, PRIMAL_INF: 10}
    assert _counts(res) == want
    for b, r in enumerate(res):
        if b % 7 == 3:
            assert r.info.status_val == PRIMAL_INF
        elif b % 7 == 5 and k is not None:
            assert r.info.status_val == DUAL_INF
        else:
            assert r.info.status_val == SOLVED
    assert len(set(r.info.iter for r in res)) >= 4
    refs = _references(pw, Q, L, U, res)
    assert len(refs) == want[SOLVED]
    _assert_no_guard(name, refs)
    if k is not None:
        # under the shared cost (solve_batch) the columns that were dual infeasible solve
        q0 = pw["q"]
        rs = bi.oracle_wave(name, oracle_mod, shared_q=q0)
        assert _counts(rs) == {SOLVED: 60, PRIMAL_INF: 10}
        _assert_no_guard(name, _references(pw, np.tile(q0, (len(L), 1)), L, U, rs))


@pytest.mark.parametrize("name", bi.MAX_ITER_CASES)
def test_wave_under_an_iteration_limit(oracle_mod, name):
    """max_iter = 200: columns that stop at the limit beside columns decided earlier"""
    pw = bi.widened(name)[0]
    Q, L, U, X, Y = bi.mixed_wave(name, oracle_mod)
    res = bi.oracle_wave(name, oracle_mod, max_iter=bi.MAX_ITER)
    assert _counts(res) == {MAX_ITER: 60, DUAL_INF: 10}
    assert all(r.info.iter == bi.MAX_ITER for r in res if r.info.status_val == MAX_ITER)
    assert all(r.info.iter < bi.MAX_ITER for r in res if r.info.status_val == DUAL_INF)
    _assert_no_guard(name, _references(pw, Q, L, U, res))


@pytest.mark.parametrize("name", bi.RANDOM_STRUCTURED)
def test_all_dual_wave(oracle_mod, name):
    pw = bi.widened(name)[0]
    q, L, U, X, Y = bi.all_dual(name)
    res = bi.oracle_columns(oracle_mod, pw, np.tile(q, (5, 1)), L, U, X, Y)
    assert _counts(res) == {DUAL_INF: 5}


def test_one_percent_instance_is_dual_infeasible_as_it_is(oracle_mod):
    pr = bi.a_1pct()
    A, l, u = problems.extended(pr)
    assert np.any(np.diff(pr["A"].indptr) == 0)  # empty columns of A
    root = bi.oracle_columns(oracle_mod, pr, pr["q"][None], l[None], u[None], np.zeros((1, A.shape[1])),
                             np.zeros((1, A.shape[0])))[0]
    assert (root.info.status_val, root.info.iter) == (DUAL_INF, 25)
    Q, L, U, X, Y = bi.a_1pct_wave()
    assert _counts(bi.oracle_columns(oracle_mod, pr, Q, L, U, X, Y)) == {DUAL_INF: 5}


@pytest.mark.parametrize("name", list(bi.CASES))
def test_long_double_reference_against_the_double_expressions(oracle_mod, name):
    """lower, heur_obj, heur_viol within 1e-12 of the sum of their absolute terms, int_inf and nextvar equal"""
    pw = bi.widened(name)[0]
    Q, L, U, X, Y = bi.mixed_wave(name, oracle_mod)
    A, l, u = problems.extended(pw)
    ii = pw["i_idx"]
    refs = _references(pw, Q, L, U, bi.oracle_wave(name, oracle_mod))
    assert refs
    for b, (xo, c) in refs.items():
        lo = 0.5 * xo.dot(pw["P"].dot(xo)) + Q[b].dot(xo)
        assert abs(lo - c.lower) <= 1e-12 * c.lower_abs, b
        frac = np.abs(xo[ii] - np.round(xo[ii]))
        assert c.int_inf == int(np.sum(frac > 1e-3)) and c.nextvar == int(np.argmax(frac)), b
        xr = xo.copy()
        xr[ii] = np.round(xo[ii])
        np.testing.assert_array_equal(xr, c.x_r.astype(np.float64))
        zz = A.dot(xr)
        margin = np.max(np.maximum(l - 1e-3 - zz, zz - u - 1e-3))
        assert abs(margin - c.heur_viol) <= 1e-12 * c.heur_viol_abs, b
        ho = 0.5 * xr.dot(pw["P"].dot(xr)) + Q[b].dot(xr)
        assert abs(ho - c.heur_obj) <= 1e-12 * c.heur_obj_abs, b


def test_reference_breaks_ties_towards_the_lowest_position():
    P, A = br.dense_ld(np.zeros((4, 4))), br.dense_ld(np.eye(4))
    x = np.array([0.25, 0.75, 0.5, 0.5])
    inf = np.full(4, np.inf)
    c = br.column(x, np.ones(4), P, A, -inf, inf, np.array([1, 0, 3, 2]), 1e-3, 1e-3)
    assert c.nextvar == 2 and c.int_inf == 4 and c.guard_tie == 0.0
    np.testing.assert_array_equal(c.x_r.astype(float), [0.0, 1.0, 0.0, 0.0])  # halves round to even, as rint does
    assert float(c.lower) == 2.0 and float(c.heur_obj) == 1.0 and float(c.heur_viol) == -np.inf


@pytest.mark.parametrize("name", bi.TREE_CASES)
def test_trees_meet_no_branching_tie(oracle_mod, name):
    """the five trees of the lock-step test on the oracle backend: no solved node has its two largest fractionalities
    (above eps_int) within 1e-7 of each other, so every correct driver branches on the same position"""
    pr = bi.make(name)
    ii = pr["i_idx"]
    seen = []

    def observer(work, leaf):
        if leaf.status not in (SOLVED, MAX_ITER):
            return
        frac = np.abs(leaf.x[ii] - np.round(leaf.x[ii]))
        top = np.sort(frac[frac > bi.EPS_INT])[::-1]
        seen.append(len(top))
        if len(top) > 1:
            assert top[0] - top[1] > GUARD, (name, work.iter_num, top[:2])

    mdl = bnb.MIOSQP(backend=oracle_mod)
    mdl.setup(pr["P"], pr["q"], pr["A"], pr["l"].copy(), pr["u"].copy(), pr["i_idx"], pr["i_l"], pr["i_u"],
              dict(problems.BNB_SETTINGS, max_iter_bb=40), dict(problems.QP_SETTINGS))
    nodes = []
    for inst in bi.tree_instances(pr):
        mdl.update_vectors(q=inst["q"].copy())
        mdl.solve(observer=observer)
        nodes.append(mdl.work.iter_num - 1)
    print(name, "nodes per tree", nodes, "ADMM iterations of the last", mdl.work.osqp_iter)
    assert min(nodes) >= 3 and sum(n_ > 1 for n_ in seen) >= 10  # trees that branch, not five roots
