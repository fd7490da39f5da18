"""setup_models(..., large="device") on the HIP engine (needs an MI355X): models beyond n + M = 192 are set up in the same
call by a second launch (k_setup_models_large: one workgroup per model, only the packed triangle in LDS, Abar read from
memory) and come out as the engines MIOSQP.setup builds with coop=0, resident=0, fold=1.

The products are checked against the long-double reference of tests/setup_reference.py under the rule of setup_cases.check
-- 8 x max(float64 floor, n 2^-53), no new epsilon --, the copies and scalings bit for bit against that per-model engine,
the trees (solve_models(large="device")) against the same models set up one by one under the contract of
test_gpu_setup_models.py: status, nodes and iterations equal, x equal at the integer positions, x and upper_glob within
1e-8.  One call over FIVE and the per-model engines of its large shapes are built once per module and shared, read-only."""
import numpy as np
import pytest
import scipy.sparse as spa

import setup_cases as sc
import setup_models_cpu_body as cb
from miosqp_amd import problems
from test_gpu_solve_models_large import LARGE

pytestmark = pytest.mark.gpu

FIVE = [(100, 90, 3), (10, 5, 2), (20, 170, 4), (150, 300, 20), (20, 530, 4)]
BIG = [0, 2, 3, 4]       # positions of the large models in FIVE
SOL_TOL = 1e-8           # tests/test_gpu_setup_models.py: its tolerance for two set-ups of one model
OWN = dict(coop=0, resident=0, fold=1)


def _pr(shape):
    return sc.instance(shape)[0]


def _setup(shapes, info=None, qs=None, **kw):
    import miosqp_amd
    return miosqp_amd.setup_models([_pr(s) for s in shapes], dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS, **(qs or {})),
                                   info=info, **kw)


def _own(pr, st=None, **qs):
    from miosqp_amd import bnb
    mdl = bnb.MIOSQP()
    mdl.setup(pr["P"], pr["q"], pr["A"], pr["l"].copy(), pr["u"].copy(), pr["i_idx"], pr["i_l"], pr["i_u"],
              dict(problems.BNB_SETTINGS, **(st or {})), dict(problems.QP_SETTINGS, **qs))
    return mdl


def _close(models):
    for m in models:
        m.work.solver.close()


_SHARED = {}


@pytest.fixture(scope="module", autouse=True)
def _shared_models_are_closed_and_no_group_is_left():
    from miosqp_amd import qp
    assert qp.setup_groups_live() == 0
    yield
    for v in _SHARED.values():
        _close(v[0] if isinstance(v, tuple) else [v])
    _SHARED.clear()
    assert qp.setup_groups_live() == 0


def _batch():
    """(models, info) of ONE setup_models(large="device") call over FIVE"""
    if "batch" not in _SHARED:
        info = {}
        _SHARED["batch"] = (_setup(FIVE, info=info, large="device"), info)
    return _SHARED["batch"]


def _single(shape):
    """the per-model engine of a large shape: MIOSQP.setup with coop=0, resident=0, fold=1"""
    key = ("own", shape)
    if key not in _SHARED:
        _SHARED[key] = _own(_pr(shape), **OWN)
    return _SHARED[key]


def _products(g):
    return [g.debug_factor(w)[1] for w in (0, 1, 2)] + [g.debug_product_form(w)[1] for w in range(8)]


def test_one_call_two_launches_one_group():
    models, info = _batch()
    assert info["batched"] == list(range(5)) and info["own"] == {} and info["launches"] == 2
    assert info["forms"] == dict(small=1, large=4)
    assert info["device_time"] > 0.0 and info["arena_bytes"] > 0
    groups = {m.work.solver.setup_group() for m in models}
    assert len(groups) == 1 and None not in groups
    for k, m in enumerate(models):
        fs = m.work.solver.factor_stats()
        assert fs["fold"] and not fs["coop"] and not fs["setup_on_device"]
        assert bool(fs["resident"]) == (k == 1)
    for k in BIG:
        # the tree forms are those of the per-model engine: 3 wherever no existing form takes the model -- (20,170,4), 20
        # rows of 194 doubles, still fits the workgroup form and keeps it, so tree_form_large leaves it alone
        g, o = models[k].work.solver, _single(FIVE[k]).work.solver
        assert (g.tree_form(), g.tree_form_large(256)) == (o.tree_form(), o.tree_form_large(256)), FIVE[k]
        assert (g.tree_form(), g.tree_form_large(256)) == ((2, 0) if FIVE[k] == (20, 170, 4) else (0, 3)), FIVE[k]
        with pytest.raises(RuntimeError, match="did not build"):  # no explicit inverse
            g.debug_factor(3)
    print("setup_models large: 5 models, device %.3f ms, arena %d bytes" % (1e3 * info["device_time"], info["arena_bytes"]))


@pytest.mark.parametrize("k", BIG, ids=[str(FIVE[k]) for k in BIG])
def test_products_against_the_long_double_reference(k):
    shape = FIVE[k]
    g = _batch()[0][k].work.solver
    ld, f64 = sc.reference(shape, inverses=False)
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
    F, raw = g.debug_product_form(0)
    assert F.shape == (n, N) and raw.shape == (n, (N + 15) & ~15)
    sc.check("f_rows", F, cb.product_form_reference(ld, sc.RHO), cb.product_form_reference(f64, sc.RHO), n)
    assert np.all(raw[:, N:] == 0.0)
    np.testing.assert_array_equal(F[:, M:], Linv)
    GmT, GmT_raw = g.debug_product_form(1)
    np.testing.assert_array_equal(GmT, F[:, :M].T)
    assert np.all(GmT_raw[:, n:] == 0.0)


@pytest.mark.parametrize("k", BIG, ids=[str(FIVE[k]) for k in BIG])
def test_copies_and_scalings_bit_for_bit_the_per_model_engine(k):
    shape = FIVE[k]
    g, o = _batch()[0][k].work.solver, _single(shape).work.solver
    fs = o.factor_stats()
    assert o.setup_group() is None and fs["fold"] and not fs["coop"] and not fs["resident"]
    for which in (2, 3, 4, 5, 6, 7):  # f_Ad, f_Atd, f_Pd, the scaled q, l, u
        np.testing.assert_array_equal(g.debug_product_form(which)[1], o.debug_product_form(which)[1], err_msg=str(which))
    for a, b in zip(g.scaling(), o.scaling()):
        np.testing.assert_array_equal(a, b)
    assert g.rho() == o.rho() == sc.RHO


def test_the_small_model_is_bit_for_bit_that_of_setup_models_alone():
    models, _ = _batch()
    info = {}
    alone = _setup([FIVE[1]], info=info)
    try:
        assert info["launches"] == 1 and info["batched"] == [0]
        a, b = alone[0].work.solver, models[1].work.solver
        for x, y in zip(_products(a) + [a.debug_factor(3)[1], a.debug_factor(4)[1]],
                        _products(b) + [b.debug_factor(3)[1], b.debug_factor(4)[1]]):
            np.testing.assert_array_equal(x, y)
    finally:
        _close(alone)


@pytest.mark.parametrize("order", ["reversed", "rotated"])
def test_permuting_the_list_gives_the_same_products_bit_for_bit(order):
    models, _ = _batch()
    perm = [4, 3, 2, 1, 0] if order == "reversed" else [3, 4, 0, 1, 2]
    info = {}
    again = _setup([FIVE[k] for k in perm], info=info, large="device")
    try:
        assert info["launches"] == 2 and info["batched"] == list(range(5))
        for j, k in enumerate(perm):
            for a, b in zip(_products(again[j].work.solver), _products(models[k].work.solver)):
                np.testing.assert_array_equal(a, b)
    finally:
        _close(again)


def test_a_large_model_alone_and_two_groups_live_at_once():
    from miosqp_amd import qp
    models, _ = _batch()
    live = qp.setup_groups_live()
    info = {}
    one = _setup([FIVE[3]], info=info, large="device")
    two = _setup([FIVE[2], FIVE[0]], large="device")
    try:
        assert info["launches"] == 1 and info["forms"] == dict(small=0, large=1) and info["batched"] == [0]
        assert qp.setup_groups_live() == live + 2
        assert one[0].work.solver.setup_group() != two[0].work.solver.setup_group()
        assert one[0].work.solver.tree_form_large(256) == 3
        for got, k in ((one[0], 3), (two[0], 2), (two[1], 0)):
            for a, b in zip(_products(got.work.solver), _products(models[k].work.solver)):
                np.testing.assert_array_equal(a, b)
    finally:
        _close(one + two)
    assert qp.setup_groups_live() == live


def _same_tree(g, w, pr, who):
    """the contract of tests/test_gpu_setup_models.py for two set-ups of one model"""
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


def test_trees_of_models_set_up_in_the_call_are_those_of_models_set_up_one_by_one():
    """the eleven models of tests/test_gpu_solve_models_large.py, set up by one call with the keyword and one by one by
    MIOSQP.setup (the cooperative grid's engines), both lists solved by solve_models(large="device")"""
    import miosqp_amd
    prs = [problems.random_miqp(n, m, p, seed=s) for n, m, p, s in LARGE]
    sts = [dict(problems.BNB_SETTINGS, tree_explor_rule=k % 4) for k in range(len(LARGE))]
    info = {}
    got = miosqp_amd.setup_models(prs, [dict(s) for s in sts], dict(problems.QP_SETTINGS, rho=0.1), info=info, large="device")
    ref = []
    try:
        assert info["batched"] == list(range(len(LARGE))) and info["launches"] == 1 and info["forms"] == dict(small=0, large=len(LARGE))
        ref = [_own(pr, st=st, rho=0.1) for pr, st in zip(prs, sts)]
        ia, ib = {}, {}
        a = miosqp_amd.solve_models(got, info=ia, large="device")
        b = miosqp_amd.solve_models(ref, info=ib, large="device")
        assert ia["own"] == {} and ib["own"] == {} and ia["forms"] == ib["forms"] and ia["overflow"] == ib["overflow"] == []
        for k, s in enumerate(LARGE):
            _same_tree(a[k], b[k], prs[k], "solve_models %r rule %d" % (s, k % 4))
    finally:
        _close(got + ref)


def test_a_large_engine_answers_the_sequential_entries_as_the_per_model_engine_does():
    """solve(), solve_many([inst]) and update_vectors on the captured chunks: the per-model engine with coop=0, resident=0,
    fold=1 is the same algorithm on products that differ in their last bits -- equal within the solver's eps"""
    shape = FIVE[0]  # (100,90,3): no one-launch tree form takes it, so solve() and solve_many go node by node
    pr = _pr(shape)
    got = _setup([shape], large="device")[0]
    ref = _own(pr, **OWN)
    for m in (got, ref):
        g = m.work.solver
        assert g.tree_form() == 0, "the sequential path is what is compared"
        fs = g.factor_stats()
        assert fs["fold"] and not fs["coop"] and not fs["resident"]  # the captured chunks run the iterations
    assert got.work.solver.setup_group() is not None and ref.work.solver.setup_group() is None
    d = got.work.data
    ra = got.work.solver.solve_node(d.l, d.u, np.zeros(d.n), np.zeros(len(d.l)))  # one relaxation: full chunks replayed
    rb = ref.work.solver.solve_node(d.l, d.u, np.zeros(d.n), np.zeros(len(d.l)))
    assert ra.status_val == rb.status_val and ra.iter == rb.iter and ra.iter > 0
    assert np.max(np.abs(ra.x - rb.x)) <= SOL_TOL * max(1.0, np.max(np.abs(rb.x)))
    eps = max(problems.QP_SETTINGS["eps_abs"], problems.QP_SETTINGS["eps_rel"])
    ii = np.asarray(pr["i_idx"])

    def same(xa, ua, xb, ub, who):
        np.testing.assert_array_equal(np.round(xa[ii]), np.round(xb[ii]), err_msg=who)
        assert np.max(np.abs(xa - xb)) <= eps * max(1.0, np.max(np.abs(xb))), who
        assert abs(ua - ub) <= eps * max(1.0, abs(ub)), who

    try:
        ra, rb = got.solve(), ref.solve()
        assert ra.status == rb.status
        same(ra.x, ra.upper_glob, rb.x, rb.upper_glob, "solve")
        rng = np.random.RandomState(11)
        inst = dict(q=pr["q"] + 0.1 * rng.randn(len(pr["q"])))
        ga, gb = got.solve_many([inst])[0], ref.solve_many([inst])[0]
        assert ga["status"] == gb["status"]
        same(ga["x"], ga["upper_glob"], gb["x"], gb["upper_glob"], "solve_many")
        q2 = pr["q"] + 0.05 * rng.randn(len(pr["q"]))
        for m in (got, ref):
            m.update_vectors(q=q2)
        ra, rb = got.solve(), ref.solve()
        assert ra.status == rb.status
        same(ra.x, ra.upper_glob, rb.x, rb.upper_glob, "update_vectors")
    finally:
        _close([got, ref])


def test_an_indefinite_p_in_the_middle_raises_with_its_position_and_leaves_nothing():
    import miosqp_amd
    from miosqp_amd import qp
    live = qp.setup_groups_live()
    shape = (20, 170, 4)
    prs = [_pr((10, 5, 2)), dict(_pr(shape)), _pr(shape)]
    p = np.ones(20)
    p[7] = -50.0
    prs[1]["P"] = spa.diags(p).tocsc()
    with pytest.raises(RuntimeError, match=r"non-positive pivot.*model 1, pivot.*position 1"):
        miosqp_amd.setup_models(prs, dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS, scaling=0), large="device")
    assert qp.setup_groups_live() == live


def test_refusals_and_fallbacks():
    import miosqp_amd
    from miosqp_amd import qp
    live = qp.setup_groups_live()
    shape = (20, 170, 4)
    pr = _pr(shape)
    Ae, l, u = problems.extended(pr)
    md = dict(P=pr["P"], q=pr["q"], A=Ae, l=l, u=u, i_idx=pr["i_idx"], m_orig=pr["A"].shape[0])
    small = _pr((10, 5, 2))
    As, ls, us = problems.extended(small)
    ms = dict(P=small["P"], q=small["q"], A=As, l=ls, u=us, settings=dict(problems.QP_SETTINGS), i_idx=small["i_idx"],
              m_orig=small["A"].shape[0])
    # the library: a large model with rho="auto" is refused by name, with either flag; without large=True the size is
    with pytest.raises(RuntimeError, match=r"rho_auto.*\(model 1\)"):
        qp.setup_models([ms, dict(md, settings=dict(problems.QP_SETTINGS, rho="auto"))], rho_auto_in_launch=True, large=True)
    with pytest.raises(RuntimeError, match=r"rho_auto.*\(model 0\)"):
        qp.setup_models([dict(md, settings=dict(problems.QP_SETTINGS, rho="auto"))], large=True)
    with pytest.raises(RuntimeError, match=r"large launch does not take.*\(model 1\)"):
        qp.setup_models([ms, dict(md, settings=dict(problems.QP_SETTINGS, coop=1))], large=True)
    with pytest.raises(RuntimeError, match=r"does not take this model.*\(model 0\)"):
        qp.setup_models([dict(md, settings=dict(problems.QP_SETTINGS))])
    assert qp.setup_groups_live() == live
    assert qp.setup_models_eligible_large(20, 174, dict(problems.QP_SETTINGS))
    assert not qp.setup_models_eligible_large(20, 174, dict(problems.QP_SETTINGS, rho="auto"))
    assert not qp.setup_models_eligible_large(10, 7, dict(problems.QP_SETTINGS))
    assert not qp.setup_models_eligible_large(199, 3, dict(problems.QP_SETTINGS))
    # the package: such models are set up in place, with their reasons; rho_auto="device" and large="device" combine
    qss = [dict(problems.QP_SETTINGS, rho="auto"), dict(problems.QP_SETTINGS, rho="auto"), dict(problems.QP_SETTINGS, coop=1),
           dict(problems.QP_SETTINGS)]
    info = {}
    models = miosqp_amd.setup_models([small, pr, pr, pr], dict(problems.BNB_SETTINGS), qss, info=info, rho_auto="device",
                                     large="device")
    try:
        assert info["batched"] == [0, 3] and sorted(info["own"]) == [1, 2] and info["launches"] == 2
        assert info["forms"] == dict(small=1, large=1)
        assert "auto" in info["own"][1] and "large launch" in info["own"][1]
        assert "another engine form" in info["own"][2]
        assert models[0].work.solver.setup_group() == models[3].work.solver.setup_group() is not None
        assert models[1].work.solver.setup_group() is None and models[2].work.solver.setup_group() is None
        assert models[2].work.solver.factor_stats()["coop"]  # what MIOSQP.setup builds when asked for the grid
    finally:
        _close(models)
    assert qp.setup_groups_live() == live


@pytest.mark.parametrize("var,value", [("MIOSQP_COOP", "1"), ("MIOSQP_PERS", "1"), ("MIOSQP_PERS", "2")])
def test_the_environment_switches_of_another_engine_form_keep_large_models_out(monkeypatch, var, value):
    """MIOSQP_COOP=1 and MIOSQP_PERS ask miosqp_qp_setup for the grid or the persistent kernel: the eligibility entry says
    no, the library refuses the call before anything is queued, the package sets the model up in place with the
    environment named as the reason -- not the size"""
    import miosqp_amd
    from miosqp_amd import qp
    live = qp.setup_groups_live()
    shape = (20, 170, 4)
    pr = _pr(shape)
    Ae, l, u = problems.extended(pr)
    md = dict(P=pr["P"], q=pr["q"], A=Ae, l=l, u=u, i_idx=pr["i_idx"], m_orig=pr["A"].shape[0], settings=dict(problems.QP_SETTINGS))
    assert qp.setup_models_eligible_large(20, 174, dict(problems.QP_SETTINGS))
    assert (qp.setup_models_shape(20, 174), qp.setup_models_shape(10, 7), qp.setup_models_shape(199, 3)) == (2, 1, 0)
    monkeypatch.setenv(var, value)
    assert not qp.setup_models_eligible_large(20, 174, dict(problems.QP_SETTINGS))
    assert (qp.setup_models_shape(20, 174), qp.setup_models_shape(10, 7)) == (2, 1)  # the size rules do not read it
    with pytest.raises(RuntimeError, match="MIOSQP_COOP=1 or MIOSQP_PERS"):
        qp.setup_models([md], large=True)
    assert qp.setup_groups_live() == live
    if var == "MIOSQP_COOP":  # (the package's fallback is MIOSQP.setup under that switch: the grid, which it asks for)
        info = {}
        models = miosqp_amd.setup_models([pr], dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS), info=info, large="device")
        try:
            assert info["batched"] == [] and info["forms"] == dict(small=0, large=0) and info["launches"] == 0
            assert info["own"][0] == "settings or environment that lead to another engine form than the large launch builds"
            assert models[0].work.solver.factor_stats()["coop"] and models[0].work.solver.setup_group() is None
        finally:
            _close(models)
        # a SMALL model under the switch is not sent to the large rule: its reason is the one it has without the keyword
        from miosqp_amd import bnb
        sm = _pr((10, 5, 2))
        data = bnb.Data(spa.csc_matrix(sm["P"]), sm["q"], spa.csc_matrix(sm["A"]), sm["l"], sm["u"], sm["i_idx"], sm["i_l"], sm["i_u"])
        why = bnb._setup_models_own_reason(qp, data, dict(problems.QP_SETTINGS), False, True)
        assert why == bnb._setup_models_own_reason(qp, data, dict(problems.QP_SETTINGS), False, False) and "either" not in why
    monkeypatch.delenv(var)
    assert qp.setup_models_eligible_large(20, 174, dict(problems.QP_SETTINGS))
    assert qp.setup_groups_live() == live


def test_without_the_keyword_the_size_keeps_a_model_out_as_before():
    info = {}
    models = _setup([(10, 5, 2), (20, 170, 4)], info=info)
    try:
        assert info["batched"] == [0] and list(info["own"]) == [1]
        assert info["own"][1] == "n + M = 194: beyond one workgroup of the launch" and info["launches"] == 1
        assert models[1].work.solver.setup_group() is None
    finally:
        _close(models)
