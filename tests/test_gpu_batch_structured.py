"""The lock-step batch path -- kb_prepare / kb_warm_z, the sweeps kb_* (factor form), kbm_* (fp64 matrix-core tiles) and
kbp / kbp1, the tests kb_check_* / kbm_check_* / kb_check_reduce / kb_check_decide, the epilogue kb_finish /
kb_heur_rows / kb_obj_rows / kb_obj_sum -- on matrices that are not `problems.random_miqp` and on waves that mix solved,
primal-infeasible and dual-infeasible columns (needs an MI355X).

Inputs: tests/batch_structured_inputs.py (P = 0, rank-deficient P, equality rows, infinite bounds, A at 5 % and 1 %, row
norms 1e-4 .. 1e4, the power converter's blocks; tests/test_batch_structured_cpu.py shows on the oracle what every wave
holds and that no column stands within 1e-7 of a tie, so nothing here is skipped).  Per column the contract of
tests/test_gpu_solve_batch_q.py: what the oracle computes after update(q) + update(l, u) + warm_start + solve and what a
second engine of the same form computes in update(q) + solve_node -- status and iteration exact, x and y within SOL_TOL.
New here:
  * the numbers of the batched termination test, infos[k].pri_res / dua_res / obj_val, against the oracle's info (the
    tolerances of test_gpu_parity.py::test_solve_matches_oracle);
  * the epilogue's lower, heur_obj, heur_viol, int_inf and nextvar against tests/batch_reference.py (long double) on the
    column's own returned x: 1e-9 relative -- at n <= 150 a row sum carries about 150 roundings of 1.1e-16 on the sum of
    its absolute terms, which leaves four orders of magnitude for cancellation --, the two integers exact;
  * the certificates of infeasible columns: the other vector all NaN, the certificate within rtol 1e-6 / atol 1e-8 of
    the oracle's (test_certificates_on_random_instances) and its largest entry exactly +-1 (kb_finish divides by it).

Forms: L (fold=0, slices of 64 + 6), Linv (fold=1, matrix-core tiles, identity rows left out of the products), Linv_tiles
(max_batch=128: two tiles, compaction), Linv_full (MIOSQP_NO_IDROWS=1: the identity rows inside the products), Linv_pers
(batch_pers=1; MIOSQP_KBP_MIN_COLS=1 as in tests/test_gpu_kbs.py, because below 192 columns the engine would choose the
launches by itself and the form would be Linv_tiles again).  The engines are handed their q through update first, as
tests/test_gpu_solve_batch_q.py explains."""
import collections

import numpy as np
import pytest

import batch_reference as br
import batch_structured_inputs as bi
from miosqp_amd import problems
from test_gpu_lockstep_device import _assert_state, _same, _state
from test_gpu_parity import SOL_TOL, rel

pytestmark = pytest.mark.gpu

SOLVED, MAX_ITER, PRIMAL_INF, DUAL_INF = 1, -2, -3, -4
FORMS = {
    "L": dict(fold=0, max_batch=64),
    "Linv": dict(fold=1, max_batch=64),
    "Linv_tiles": dict(fold=1, max_batch=128),
    "Linv_full": dict(fold=1, max_batch=128),
    "Linv_pers": dict(fold=1, max_batch=128, batch_pers=1),
}
WAVES = [(c, f) for f in ("L", "Linv") for c in bi.CASES] + \
        [(c, f) for f in ("Linv_tiles", "Linv_full", "Linv_pers") for c in bi.TWO_TILE_CASES]
SLICED = [(c, f) for f in ("L", "Linv") for c in bi.CASES]


def _engines(pr, form, monkeypatch, count=2, **qp_extra):
    """`count` engines of one form on the instance, digest on, their q handed to them through update"""
    from miosqp_amd import qp
    if form == "Linv_full":
        monkeypatch.setenv("MIOSQP_NO_IDROWS", "1")
    if form == "Linv_pers":
        monkeypatch.setenv("MIOSQP_KBP_MIN_COLS", "1")
    A, l, u = problems.extended(pr)
    out = []
    for _ in range(count):
        g = qp.OSQP()
        g.setup(pr["P"], pr["q"], A, l, u, **dict(problems.QP_SETTINGS, **dict(FORMS[form], **qp_extra)))
        g.set_integer_rows(pr["i_idx"], pr["A"].shape[0])
        g.set_root(l, u, bi.EPS_INT, bi.EPS_LIN)
        g.update(q=pr["q"])
        assert g.factor_stats()["fold"] == bool(FORMS[form]["fold"])
        out.append(g)
    return out


def _close(g, g2, form):
    """g ran the batches (the persistent form is decided when the batch arrays are made, at the first of them)"""
    if form == "Linv_pers":
        assert g.factor_stats()["batch_pers"] and g.batch_pers_fallbacks() == 0
    g.close()
    g2.close()


def _certificate(got, other, want, k):
    assert np.all(np.isnan(other)), k
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-8, err_msg=str(k))
    assert np.max(np.abs(got)) == 1.0, k


def _check_columns(rb, g2, ros, pr, Q, L, U, X, Y, columns=None, node=True):
    """every column of the batch result rb against the oracle's ros[k], against update(q) + solve_node on g2 and -- where
    it has an x -- against the long-double reference on its own x.  Returns the status counts."""
    A, l, u = problems.extended(pr)
    Pd, Ad = br.dense_ld(pr["P"]), br.dense_ld(A)
    ii, p = pr["i_idx"], len(pr["i_idx"])
    seen = collections.Counter()
    for k in (range(len(L)) if columns is None else columns):
        ro, info = ros[k], rb.infos[k]
        st = ro.info.status_val
        seen[st] += 1
        assert (rb.status_val[k], rb.iter[k]) == (st, ro.info.iter), k
        r1 = None
        if node:
            g2.update(q=Q[k])
            r1 = g2.solve_node(L[k], U[k], X[k], Y[k])
            assert (rb.status_val[k], rb.iter[k]) == (r1.status_val, r1.iter), k
        if st == PRIMAL_INF:
            _certificate(rb.y[k], rb.x[k], ro.y, k)
            if node:
                _certificate(r1.y, r1.x, ro.y, k)
        elif st == DUAL_INF:
            _certificate(rb.x[k], rb.y[k], ro.x, k)
            if node:
                _certificate(r1.x, r1.y, ro.x, k)
        if st in (PRIMAL_INF, DUAL_INF):
            assert np.isnan(rb.lower[k]) and rb.digest[k] is None, k
            continue
        assert st in (SOLVED, MAX_ITER), k
        xo = ro.x.copy()
        xo[ii] = np.minimum(np.maximum(xo[ii], L[k][-p:]), U[k][-p:])
        assert rel(rb.x[k], xo) <= SOL_TOL and rel(rb.y[k], ro.y) <= SOL_TOL, k
        if node:
            assert rel(rb.x[k], r1.x) <= SOL_TOL and rel(rb.y[k], r1.y) <= SOL_TOL, k
            assert abs(rb.lower[k] - r1.lower) <= 1e-9 * max(1.0, abs(r1.lower)), k
        # the termination test's numbers, as the batch kernels left them for this column
        assert abs(info.pri_res - ro.info.pri_res) <= 1e-9 + 1e-6 * ro.info.pri_res, (k, info.pri_res, ro.info.pri_res)
        assert abs(info.dua_res - ro.info.dua_res) <= 1e-9 + 1e-6 * ro.info.dua_res, (k, info.dua_res, ro.info.dua_res)
        assert abs(info.obj_val - ro.info.obj_val) <= 1e-9 * max(1, abs(ro.info.obj_val)), (k, info.obj_val, ro.info.obj_val)
        # the epilogue's arithmetic alone: the reference on the column's own returned x
        c = br.column(rb.x[k], Q[k], Pd, Ad, l, u, ii, bi.EPS_INT, bi.EPS_LIN)
        assert min(c.guard_tie, c.guard_int, c.guard_viol) > 1e-7, k  # (the CPU file shows it on the oracle's x)
        assert abs(info.lower - c.lower) <= 1e-9 * max(1.0, abs(c.lower)), (k, info.lower, c.lower)
        assert rb.lower[k] == info.lower
        assert abs(info.heur_obj - c.heur_obj) <= 1e-9 * max(1.0, abs(c.heur_obj)), (k, info.heur_obj, c.heur_obj)
        assert abs(info.heur_viol - c.heur_viol) <= 1e-9 * max(1.0, c.ax_inf), (k, info.heur_viol, c.heur_viol)
        assert (info.int_inf, info.nextvar) == (c.int_inf, c.nextvar), k
        d = rb.digest[k]
        assert (d.int_inf, d.nextvar, d.heur_obj, d.heur_feasible) == (info.int_inf, info.nextvar, info.heur_obj,
                                                                        bool(c.heur_viol <= 0)), k
    return dict(seen)


def _same_bits(a, b, columns=None):
    s = slice(None) if columns is None else columns
    for key in ("status_val", "iter", "x", "y", "lower"):
        np.testing.assert_array_equal(getattr(a, key)[s], getattr(b, key)[s], err_msg=key)


@pytest.mark.parametrize("name,form", WAVES)
def test_mixed_wave_with_a_cost_per_column(oracle_mod, monkeypatch, name, form):
    pw, k, _ = bi.widened(name)
    Q, L, U, X, Y = bi.mixed_wave(name, oracle_mod)
    g, g2 = _engines(pw, form, monkeypatch)
    rq = g.solve_batch_q(Q, L, U, X, Y)
    seen = _check_columns(rq, g2, bi.oracle_wave(name, oracle_mod), pw, Q, L, U, X, Y)
    print("%s %s: columns compared by status %s, iterations %d .. %d" % (name, form, seen, rq.iter.min(), rq.iter.max()))
    assert seen == ({SOLVED: 50, PRIMAL_INF: 10, DUAL_INF: 10} if k is not None else {SOLVED: 60, PRIMAL_INF: 10})
    assert len(set(rq.iter.tolist())) >= 4
    if form == "Linv_tiles" and name in ("milp", "badly_scaled"):
        assert g.compactions() >= 1  # two tiles, columns decided at different tests: the wave was compacted
    _same_bits(rq, g.solve_batch_q(Q, L, U, X, Y))  # a second identical call is bit-identical
    _close(g, g2, form)


@pytest.mark.parametrize("name,form", SLICED)
def test_mixed_wave_under_the_shared_cost(oracle_mod, monkeypatch, name, form):
    """solve_batch on the engine's own q (the kernels without a cost per column): the columns that were dual infeasible
    under their own cost solve now; the others are the columns of the per-column call, bit for bit (a column is a pure
    function of its q, l, u, x0, y0)."""
    pw, k, _ = bi.widened(name)
    Q, L, U, X, Y = bi.mixed_wave(name, oracle_mod)
    Q0 = np.tile(pw["q"], (len(L), 1))
    g, g2 = _engines(pw, form, monkeypatch)
    rb = g.solve_batch(L, U, X, Y)
    seen = _check_columns(rb, g2, bi.oracle_wave(name, oracle_mod, shared_q=pw["q"]), pw, Q0, L, U, X, Y)
    print("%s %s: columns compared by status %s" % (name, form, seen))
    assert seen == {SOLVED: 60, PRIMAL_INF: 10}
    unchanged = np.array([b for b in range(len(L)) if np.array_equal(Q[b], Q0[b])])
    assert len(unchanged) == (60 if k is not None else 70)
    _same_bits(rb, g.solve_batch_q(Q, L, U, X, Y), unchanged)
    _same_bits(rb, g.solve_batch(L, U, X, Y))
    _close(g, g2, form)


@pytest.mark.parametrize("form", ["L", "Linv"])
@pytest.mark.parametrize("name", bi.RANDOM_STRUCTURED)
def test_wave_of_dual_infeasible_columns_under_the_shared_cost(oracle_mod, monkeypatch, name, form):
    """update(q=) + solve_batch with cost on the free variable: the whole wave is unbounded"""
    pw = bi.widened(name)[0]
    q, L, U, X, Y = bi.all_dual(name)
    g, g2 = _engines(pw, form, monkeypatch)
    g.update(q=q)
    rb = g.solve_batch(L, U, X, Y)
    Q = np.tile(q, (5, 1))
    seen = _check_columns(rb, g2, bi.oracle_columns(oracle_mod, pw, Q, L, U, X, Y), pw, Q, L, U, X, Y)
    assert seen == {DUAL_INF: 5}
    assert np.all(rb.status_val == DUAL_INF)
    _same_bits(rb, g.solve_batch(L, U, X, Y))
    _close(g, g2, form)


@pytest.mark.parametrize("form", ["L", "Linv"])
def test_one_percent_instance(oracle_mod, monkeypatch, form):
    """A at 1 %: empty rows and columns, a root that is dual infeasible as it is, five costs"""
    pr = bi.a_1pct()
    Q, L, U, X, Y = bi.a_1pct_wave()
    g, g2 = _engines(pr, form, monkeypatch)
    rq = g.solve_batch_q(Q, L, U, X, Y)
    seen = _check_columns(rq, g2, bi.oracle_columns(oracle_mod, pr, Q, L, U, X, Y), pr, Q, L, U, X, Y)
    assert seen == {DUAL_INF: 5}
    _same_bits(rq, g.solve_batch_q(Q, L, U, X, Y))
    _close(g, g2, form)


@pytest.mark.parametrize("form", ["L", "Linv"])
@pytest.mark.parametrize("name", bi.MAX_ITER_CASES)
def test_mixed_wave_under_an_iteration_limit(oracle_mod, monkeypatch, name, form):
    """max_iter = 200: columns that stop at the limit (their test's numbers and their epilogue included) beside columns
    that are decided earlier"""
    pw = bi.widened(name)[0]
    Q, L, U, X, Y = bi.mixed_wave(name, oracle_mod)
    g, g2 = _engines(pw, form, monkeypatch, max_iter=bi.MAX_ITER)
    rq = g.solve_batch_q(Q, L, U, X, Y)
    seen = _check_columns(rq, g2, bi.oracle_wave(name, oracle_mod, max_iter=bi.MAX_ITER), pw, Q, L, U, X, Y)
    print("%s %s: columns compared by status %s" % (name, form, seen))
    assert seen == {MAX_ITER: 60, DUAL_INF: 10}
    _same_bits(rq, g.solve_batch_q(Q, L, U, X, Y))
    _close(g, g2, form)


# -- whole trees: lock-step solve_many on structured matrices ------------------------------------------------------------

def _tree_model(pr):
    """device_tree off: two of the four instances have n + M <= 192, where solve_many would otherwise hand every tree to
    the one-launch path and the lock-step driver would not run at all"""
    from miosqp_amd import bnb
    mdl = bnb.MIOSQP()
    mdl.setup(pr["P"], pr["q"], pr["A"], pr["l"].copy(), pr["u"].copy(), pr["i_idx"], pr["i_l"], pr["i_u"],
              dict(problems.BNB_SETTINGS, max_iter_bb=40, device_tree=False), dict(problems.QP_SETTINGS))
    return mdl


_TREES = {}


def _sequential_trees(name):
    if name not in _TREES:
        pr = bi.make(name)
        seq = _tree_model(pr)
        _TREES[name] = (pr, seq.solve_many(bi.tree_instances(pr), lockstep=False))
        seq.work.solver.close()
    return _TREES[name]


@pytest.mark.parametrize("mode", ["device", "refill", "ahead"])
@pytest.mark.parametrize("name", bi.TREE_CASES)
def test_lockstep_trees_on_structured_matrices(name, mode):
    """five trees of at most 40 nodes (tests/test_batch_structured_cpu.py: no branching tie on the oracle) through every
    library driver of the lock-step trees against the sequential calls: status, nodes and ADMM iterations equal, the
    incumbent within 1e-9, its integers exact; the model is left as it was"""
    pr, want = _sequential_trees(name)
    mdl = _tree_model(pr)
    before = _state(mdl)
    got = mdl.solve_many(bi.tree_instances(pr), lockstep=mode)
    assert mdl.work.lockstep["driver"] == mode and mdl.work.lockstep["instances"] == 5
    _assert_state(mdl, before)
    _same(got, want, pr["i_idx"])
    assert sum(g["nodes"] for g in got) >= 100  # (the CPU trees run to the cap of 40 or a little before)
    mdl.work.solver.close()
