"""setup_models on the HIP engine (needs an MI355X): the dense set-up of several DIFFERENT models in one launch
(k_setup_models, one workgroup per model) against the long-double reference of tests/setup_reference.py under the rule of
setup_cases.check -- 8 x max(float64 floor, n 2^-53), no new epsilon --, against the per-model engine where the issue asks
for bit for bit, and, on the trees, against the same models set up by MIOSQP.setup.

One call sets up the six shapes of setup_cases.SHAPES with n + M <= 192 and setup_cases.SMALL; that call and the per-model
engines of the same problems are built once per session and shared, read-only."""
import os

import numpy as np
import pytest
import scipy.sparse as spa

import setup_cases as sc
import setup_models_cpu_body as cb
import setup_reference as sr
from miosqp_amd import problems
from test_gpu_solve_models import BEYOND, TWELVE, _problem

pytestmark = pytest.mark.gpu

SHAPES = [s for s in sc.SHAPES if s[0] + s[1] + s[2] <= 192] + [sc.SMALL]
SOL_TOL = 1e-8           # tests/test_gpu_parity.py: its tolerance for two arithmetics of one algorithm
COOP_GUARD_TOL = 1e-9    # kernels_guard.inc


def _pr(shape):
    return sc.instance(shape)[0]


def _setup(shapes, info=None, qs=None):
    import miosqp_amd
    return miosqp_amd.setup_models([_pr(s) for s in shapes], dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS, **(qs or {})),
                                   info=info)


def _own(shape, **qs):
    from miosqp_amd import bnb
    pr = _pr(shape)
    mdl = bnb.MIOSQP()
    mdl.setup(pr["P"], pr["q"], pr["A"], pr["l"], pr["u"], pr["i_idx"], pr["i_l"], pr["i_u"], dict(problems.BNB_SETTINGS),
              dict(problems.QP_SETTINGS, **qs))
    return mdl


def _close(models):
    for m in models:
        m.work.solver.close()


_SHARED = {}


@pytest.fixture(scope="module", autouse=True)
def _shared_models_are_closed_and_no_group_is_left():
    """after the last test of this file every model is closed: no group of setup_models is alive any more"""
    from miosqp_amd import qp
    assert qp.setup_groups_live() == 0
    yield
    for v in _SHARED.values():
        _close(v[0] if isinstance(v, tuple) else [v])
    _SHARED.clear()
    assert qp.setup_groups_live() == 0


def _batch():
    """(models, info) of ONE setup_models call over SHAPES"""
    if "batch" not in _SHARED:
        assert len(SHAPES) == 7
        info = {}
        _SHARED["batch"] = (_setup(SHAPES, info=info), info)
    return _SHARED["batch"]


def _single(shape):
    key = ("own", shape)
    if key not in _SHARED:
        _SHARED[key] = _own(shape)
    return _SHARED[key]


def _products(g):
    return [g.debug_factor(w)[1] for w in (0, 1, 2, 3)] + [g.debug_product_form(0)[1]]


def _check_f_rows(g, shape, who):
    ld, f64 = sc.reference(shape)
    n, N = shape[0], g.n + g.m
    F, raw = g.debug_product_form(0)
    assert F.shape == (n, N) and raw.shape == (n, (N + 15) & ~15)
    sc.check("f_rows", F, cb.product_form_reference(ld, sc.RHO), cb.product_form_reference(f64, sc.RHO), n)
    assert np.all(raw[:, N:] == 0.0), who
    return F


def test_one_launch_sets_up_all_seven_models():
    models, info = _batch()
    assert info["batched"] == list(range(7)) and info["own"] == {} and info["launches"] == 1
    assert info["device_time"] > 0.0 and info["arena_bytes"] > 0
    groups = {m.work.solver.setup_group() for m in models}
    assert len(groups) == 1 and None not in groups
    for m in models:
        fs = m.work.solver.factor_stats()
        assert fs["fold"] and fs["resident"] and not fs["coop"] and not fs["setup_on_device"]
    print("setup_models: 7 models, device %.3f ms, arena %d bytes" % (1e3 * info["device_time"], info["arena_bytes"]))


@pytest.mark.parametrize("k", range(7), ids=[str(s) for s in SHAPES])
def test_products_against_the_long_double_reference(k):
    shape = SHAPES[k]
    g = _batch()[0][k].work.solver
    ld, f64 = sc.reference(shape)
    n, M = shape[0], g.m
    N = n + M
    d2inv, _ = g.debug_factor(0)
    Linv, Linv_raw = g.debug_factor(1)
    LinvT, LinvT_raw = g.debug_factor(2)
    assert Linv_raw.shape == (n, (n + 15) & ~15) and LinvT_raw.shape == Linv_raw.shape
    sc.check("d2inv", d2inv, ld.d2inv, f64.d2inv, n)
    sc.check("Linv", Linv, ld.Linv, f64.Linv, n)
    assert np.all(np.triu(Linv) == 0.0)
    np.testing.assert_array_equal(LinvT, Linv.T)
    assert np.all(Linv_raw[:, n:] == 0.0) and np.all(LinvT_raw[:, n:] == 0.0)
    W, W_raw = g.debug_factor(3)
    assert W.shape == (N, N) and W_raw.shape == (N, (N + 7) & ~7)
    Kinv = W.astype(np.longdouble)
    Kinv[:M, :M] -= np.longdouble(sc.RHO) * np.eye(M, dtype=np.longdouble)  # as _check_inverse of test_gpu_setup_kernels.py
    sc.check("W", Kinv, ld.Kinv, f64.Kinv, n)
    assert np.all(W_raw[:, N:] == 0.0)
    F = _check_f_rows(g, shape, "batched")
    GmT, GmT_raw = g.debug_product_form(1)
    np.testing.assert_array_equal(GmT, F[:, :M].T)
    assert np.all(GmT_raw[:, n:] == 0.0)
    resid, tol, tripped = g.inverse_guard()
    print("guard residual", shape, resid)
    assert 0.0 <= resid <= COOP_GUARD_TOL and tol == COOP_GUARD_TOL and not tripped
    assert not g.factor_stats()["inverse_guard_tripped"]


def test_f_rows_reference_formula_on_a_per_model_engine():
    shape = (65, 20, 5)
    _check_f_rows(_single(shape).work.solver, shape, "per model")


@pytest.mark.parametrize("k", range(7), ids=[str(s) for s in SHAPES])
def test_copies_and_scalings_bit_for_bit_the_per_model_engine(k):
    shape = SHAPES[k]
    g, o = _batch()[0][k].work.solver, _single(shape).work.solver
    assert o.setup_group() is None and o.factor_stats()["resident"]
    np.testing.assert_array_equal(g.debug_factor(4)[1], o.debug_factor(4)[1])  # Kc
    for which in (2, 3, 4, 5, 6, 7):  # f_Ad, f_Atd, f_Pd, the scaled q, l, u
        np.testing.assert_array_equal(g.debug_product_form(which)[1], o.debug_product_form(which)[1], err_msg=str(which))
    for a, b in zip(g.scaling(), o.scaling()):
        np.testing.assert_array_equal(a, b)


def test_permuting_the_list_gives_the_same_products_bit_for_bit():
    models, _ = _batch()
    order = [3, 6, 0, 5, 1, 4, 2]
    again = _setup([SHAPES[k] for k in order])
    try:
        for j, k in enumerate(order):
            for a, b in zip(_products(again[j].work.solver), _products(models[k].work.solver)):
                np.testing.assert_array_equal(a, b)
    finally:
        _close(again)


def test_a_single_model_and_a_tiny_one_next_to_the_largest():
    from miosqp_amd import qp
    models, _ = _batch()
    live = qp.setup_groups_live()
    one = _setup([(65, 20, 5)])
    two = _setup([(3, 2, 1), (129, 30, 10)])
    try:
        assert qp.setup_groups_live() == live + 2
        for got, k in ((one[0], SHAPES.index((65, 20, 5))), (two[0], SHAPES.index((3, 2, 1))), (two[1], SHAPES.index((129, 30, 10)))):
            for a, b in zip(_products(got.work.solver), _products(models[k].work.solver)):
                np.testing.assert_array_equal(a, b)
    finally:
        _close(one + two)
    assert qp.setup_groups_live() == live


def test_n_plus_m_192_goes_in_and_193_is_set_up_on_its_own():
    at, past = (100, 82, 10), (100, 83, 10)
    info = {}
    import miosqp_amd
    prs = [problems.random_miqp(*s, seed=7) for s in (at, past)]
    models = miosqp_amd.setup_models(prs, dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS), info=info)
    try:
        assert info["batched"] == [0] and list(info["own"]) == [1] and "193" in info["own"][1]
        g = models[0].work.solver
        assert g.n + g.m == 192 and g.setup_group() is not None and models[1].work.solver.setup_group() is None
        A, _, _ = problems.extended(prs[0])
        Pd = np.triu(spa.csc_matrix(prs[0]["P"]).toarray())
        ld, f64 = sr.products(("edge192",), Pd + np.triu(Pd, 1).T, A.toarray(), np.asarray(prs[0]["q"]), rho=sc.RHO, sigma=sc.SIGMA,
                              passes=sc.PASSES)
        n, M = 100, 92
        sc.check("d2inv", g.debug_factor(0)[0], ld.d2inv, f64.d2inv, n)
        sc.check("Linv", g.debug_factor(1)[0], ld.Linv, f64.Linv, n)
        Kinv = g.debug_factor(3)[0].astype(np.longdouble)
        Kinv[:M, :M] -= np.longdouble(sc.RHO) * np.eye(M, dtype=np.longdouble)
        sc.check("W", Kinv, ld.Kinv, f64.Kinv, n)
        sc.check("f_rows", g.debug_product_form(0)[0], cb.product_form_reference(ld, sc.RHO), cb.product_form_reference(f64, sc.RHO), n)
        assert not g.inverse_guard()[2]
        for m in models:  # both are ready: the root relaxation
            d = m.work.data
            assert m.work.solver.solve_node(d.l, d.u, np.zeros(d.n), np.zeros(len(d.l))).status_val in m.work.ok
    finally:
        _close(models)


def test_an_indefinite_p_in_the_middle_raises_with_its_position_and_leaves_nothing():
    import miosqp_amd
    from miosqp_amd import qp
    live = qp.setup_groups_live()
    prs = [_pr((10, 5, 2)), dict(_pr((10, 5, 2))), _pr((63, 20, 5))]
    p = np.ones(10)
    p[4] = -50.0
    prs[1]["P"] = spa.diags(p).tocsc()
    with pytest.raises(RuntimeError, match=r"non-positive pivot.*position 1"):
        miosqp_amd.setup_models(prs, dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS, scaling=0))
    assert qp.setup_groups_live() == live
    with pytest.raises(RuntimeError, match="non-positive pivot"):  # what MIOSQP.setup raises for the same model
        _bad = prs[1]
        from miosqp_amd import bnb
        bnb.MIOSQP().setup(_bad["P"], _bad["q"], _bad["A"], _bad["l"], _bad["u"], _bad["i_idx"], _bad["i_l"], _bad["i_u"],
                           dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS, scaling=0))


def test_an_entry_twice_in_a_is_refused_by_the_library_and_set_up_on_its_own_by_the_package():
    """the launch copies entries where the per-model set-up sums duplicates: such a model does not go in"""
    import miosqp_amd
    from miosqp_amd import qp
    live = qp.setup_groups_live()
    def twice(Mx):  # the last stored entry of the last column a second time
        Mx = spa.csc_matrix(Mx)
        Mx.sort_indices()
        out = spa.csc_matrix((np.append(Mx.data, 0.25), np.append(Mx.indices, Mx.indices[-1]),
                              np.append(Mx.indptr[:-1], Mx.indptr[-1] + 1)), shape=Mx.shape)
        assert not out.has_canonical_format
        return out

    pr = dict(_pr((10, 5, 2)))
    Ae, l, u = problems.extended(pr)
    with pytest.raises(RuntimeError, match="no entry twice.*model 0"):
        qp.setup_models([dict(P=pr["P"], q=pr["q"], A=twice(Ae), l=l, u=u, settings=dict(problems.QP_SETTINGS), i_idx=pr["i_idx"],
                              m_orig=pr["A"].shape[0])])
    assert qp.setup_groups_live() == live
    pr["P"] = twice(pr["P"])
    info = {}
    models = miosqp_amd.setup_models([pr, _pr((10, 5, 2))], dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS), info=info)
    try:
        assert info["batched"] == [1] and "duplicate" in info["own"][0]
    finally:
        _close(models)


def test_a_tripped_guard_leaves_the_product_form_and_the_engines_still_solve():
    shape = (10, 5, 2)
    os.environ["MIOSQP_GUARD_TOL"] = "1e-30"
    try:
        models = _setup([shape, (63, 20, 5)])
        own, own2 = _own(shape), _own((63, 20, 5))
    finally:
        del os.environ["MIOSQP_GUARD_TOL"]
    try:
        for m in models + [own, own2]:
            g = m.work.solver
            assert g.inverse_guard()[2] and g.factor_stats()["inverse_guard_tripped"] and g.factor_stats()["resident"]
            with pytest.raises(RuntimeError, match="did not build"):
                g.debug_factor(3)
        a, b = models[0].solve(), own.solve()
        assert a.status == b.status and abs(a.upper_glob - b.upper_glob) <= SOL_TOL * max(1.0, abs(b.upper_glob))
        a, b = models[1].solve(), own2.solve()
        assert a.status == b.status and abs(a.upper_glob - b.upper_glob) <= SOL_TOL * max(1.0, abs(b.upper_glob))
    finally:
        _close(models + [own, own2])


def test_forty_models_take_three_allocations_and_closing_them_frees_the_group():
    from miosqp_amd import qp
    live = qp.setup_groups_live()
    desc = []
    for seed in range(40):
        pr = problems.random_miqp(10, 5, 2, seed=seed)
        A, l, u = problems.extended(pr)
        desc.append(dict(P=pr["P"], q=pr["q"], A=A, l=l, u=u, settings=dict(problems.QP_SETTINGS), i_idx=pr["i_idx"],
                         m_orig=pr["A"].shape[0]))
    os.environ["MIOSQP_NO_CACHE"] = "1"  # a cold call: the objects of an earlier, freed group are not used again
    try:
        solvers, stats = qp.setup_models(desc)
    finally:
        del os.environ["MIOSQP_NO_CACHE"]
    assert (stats.models, stats.launches) == (40, 1)
    assert (stats.device_mallocs, stats.host_mallocs, stats.streams) == (1, 1, 1)
    assert stats.arena_bytes > 0 and stats.pinned_bytes > 0 and 0 < stats.lds_bytes <= 160 * 1024
    assert qp.setup_groups_live() == live + 1 and len({s.setup_group() for s in solvers}) == 1
    for s in solvers[:-1]:
        s.close()
    assert qp.setup_groups_live() == live + 1  # the last engine keeps the group alive ...
    pr = problems.random_miqp(10, 5, 2, seed=39)
    A, l, u = problems.extended(pr)
    r = solvers[-1].solve_node(l, u, np.zeros(10), np.zeros(len(l)))  # ... and works after its siblings were closed
    assert r.status_val == 1
    solvers[-1].close()
    assert qp.setup_groups_live() == live


# ---- trees ----

def _tree_models(rho=0.1):
    """TWELVE set up by one setup_models call and, separately, by MIOSQP.setup; the instances they solve"""
    import miosqp_amd
    from miosqp_amd import bnb
    built = [_problem(inst) for inst in TWELVE]
    prs = [b[0] for b in built]
    sts = [dict(b[1], tree_explor_rule=(k % 4)) if TWELVE[k] != "pc" else dict(b[1]) for k, b in enumerate(built)]
    qss = [dict(b[2], rho=rho) for b in built]
    insts = [b[3] for b in built]
    info = {}
    got = miosqp_amd.setup_models(prs, [dict(s) for s in sts], qss, info=info)
    ref = []
    for pr, st, qs in zip(prs, sts, qss):
        m = bnb.MIOSQP()
        m.setup(pr["P"], pr["q"], pr["A"], pr["l"].copy(), pr["u"].copy(), pr["i_idx"], pr["i_l"], pr["i_u"], dict(st), dict(qs))
        ref.append(m)
    return got, ref, insts, prs, info


def _same_tree(g, w, pr, who):
    from miosqp_amd import bnb
    print("%s: %s %d nodes %d iterations %.17g | per-model set-up %s %d %d %.17g"
          % (who, g["status"], g["nodes"], g["osqp_iter"], g["upper_glob"], w["status"], w["nodes"], w["osqp_iter"], w["upper_glob"]))
    assert (g["status"], g["nodes"], g["osqp_iter"]) == (w["status"], w["nodes"], w["osqp_iter"]), who
    if w["status"] in (bnb.MI_SOLVED, bnb.MI_MAX_ITER_FEASIBLE):
        ii = np.asarray(pr["i_idx"])
        np.testing.assert_array_equal(g["x"][ii], w["x"][ii], err_msg=who)
        assert np.max(np.abs(g["x"] - w["x"])) <= SOL_TOL * max(1.0, np.max(np.abs(w["x"]))), who
        assert abs(g["upper_glob"] - w["upper_glob"]) <= SOL_TOL * max(1.0, abs(w["upper_glob"])), who
    else:
        assert g["upper_glob"] == w["upper_glob"], who


def test_twelve_models_set_up_in_one_launch_solve_as_the_per_model_set_ups_do():
    """solve_models, solve(), solve_many with three instances and update_vectors on models of one setup_models call
    against the same models set up one by one: status, nodes and iterations equal, x equal at the integer positions, x
    and upper_glob within SOL_TOL"""
    import miosqp_amd
    got, ref, insts, prs, info = _tree_models()
    try:
        assert info["batched"] == list(range(12)) and info["launches"] == 1
        a = miosqp_amd.solve_models(got, insts)
        b = miosqp_amd.solve_models(ref, insts)
        for k in range(12):
            _same_tree(a[k], b[k], prs[k], "solve_models %r" % (TWELVE[k],))
        for k in (1, 7, 8):  # a wavefront model, two workgroup models
            ra, rb = got[k].solve(), ref[k].solve()
            assert ra.status == rb.status and got[k].work.iter_num == ref[k].work.iter_num and got[k].work.osqp_iter == ref[k].work.osqp_iter
            ii = np.asarray(prs[k]["i_idx"])
            np.testing.assert_array_equal(ra.x[ii], rb.x[ii])
            assert abs(ra.upper_glob - rb.upper_glob) <= SOL_TOL * max(1.0, abs(rb.upper_glob))
            rng = np.random.RandomState(5 + k)
            three = [dict(q=prs[k]["q"] + 0.1 * rng.randn(len(prs[k]["q"]))) for _ in range(3)]
            for j, (ga, gb) in enumerate(zip(got[k].solve_many(three), ref[k].solve_many(three))):
                _same_tree(ga, gb, prs[k], "solve_many %r instance %d" % (TWELVE[k], j))
            q2 = prs[k]["q"] + 0.05 * rng.randn(len(prs[k]["q"]))
            for m in (got[k], ref[k]):
                m.update_vectors(q=q2)
            _same_tree(got[k].solve_many([{}])[0], ref[k].solve_many([{}])[0], prs[k], "update_vectors %r" % (TWELVE[k],))
    finally:
        _close(got + ref)


def test_a_mixed_list_two_groups_and_a_model_outliving_its_siblings():
    import miosqp_amd
    from miosqp_amd import qp
    live = qp.setup_groups_live()
    kinds = [(10, 5, 2, 0), BEYOND, (50, 25, 25, 1), (32, 8, 16, 0)]
    prs = [problems.random_miqp(*k[:3], seed=k[3]) for k in kinds]
    qss = [dict(problems.QP_SETTINGS, rho=("auto" if j == 2 else 0.1)) for j in range(4)]
    info = {}
    got = miosqp_amd.setup_models(prs, dict(problems.BNB_SETTINGS), qss, info=info)
    second = _setup([(10, 5, 2), (63, 20, 5)])
    ref = []
    try:
        assert info["batched"] == [0, 3] and sorted(info["own"]) == [1, 2]
        assert "220" in info["own"][1] and "auto" in info["own"][2]
        assert qp.setup_groups_live() == live + 2
        assert got[0].work.solver.setup_group() != second[0].work.solver.setup_group()
        from miosqp_amd import bnb
        for pr, qs in zip(prs, qss):
            m = bnb.MIOSQP()
            m.setup(pr["P"], pr["q"], pr["A"], pr["l"], pr["u"], pr["i_idx"], pr["i_l"], pr["i_u"], dict(problems.BNB_SETTINGS), dict(qs))
            ref.append(m)
        a, b = miosqp_amd.solve_models(got), miosqp_amd.solve_models(ref)
        for k in range(4):
            _same_tree(a[k], b[k], prs[k], "mixed %r" % (kinds[k],))
        got[0].work.solver.close()  # the sibling of got[3] in its group
        second[0].work.solver.close()
        assert qp.setup_groups_live() == live + 2
        _same_tree(got[3].solve_many([{}])[0], b[3], prs[3], "after its sibling was closed")
    finally:
        _close(got + second + ref)
    assert qp.setup_groups_live() == live
