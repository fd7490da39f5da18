"""setup_models(..., large="device", large_rho_auto="device") on the HIP engine (needs an MI355X): a model beyond
n + M = 192 with rho="auto" goes into the call, and the workgroup of the large launch that builds it chooses rho
(k_setup_models_large_auto: the probing iterations on the first factor in LDS with Abar read from L2, the rule, S and the
factor again at the chosen rho).

The chosen rho is asserted EQUAL to the long-double reference's (tests/rho_probe_reference.py), under the condition
asserted from the reference alone that its estimate is away from a rounding boundary and that its own float64 run agrees;
the products against the long-double reference of tests/setup_reference.py at the chosen rho under the rule of
setup_cases.check, and bit for bit against the same models set up by setup_models(large="device") at a FIXED rho equal to
the chosen one; the trees of the two lists bit for bit.  One call over LIST, its fixed-rho twins and the same list without
the keyword are built once per module and shared, read-only, closed at the end."""
import numpy as np
import pytest
import scipy.sparse as spa

import rho_probe_reference as rp
import setup_cases as sc
import setup_models_cpu_body as cb
import setup_reference as sr
from miosqp_amd import problems
from test_setup_models_auto_cpu import chosen_reference

pytestmark = pytest.mark.gpu

# (shape, rho): small auto, large auto, large fixed, large auto, large auto (M above twice the workgroup), small fixed
LIST = [((10, 5, 2), "auto"), ((20, 170, 4), "auto"), ((100, 90, 3), 0.1), ((50, 200, 10), "auto"), ((20, 530, 4), "auto"),
        ((3, 2, 1), 0.1)]
LARGE_AUTO = [1, 3, 4]
KEYS = dict(rho_auto="device", large="device", large_rho_auto="device")
OWN_REASON = 'rho="auto" beyond one workgroup of the launch: the large launch builds a fixed rho only'


def _setup(entries, info=None, **kw):
    import miosqp_amd
    prs = [sc.instance(e[0])[0] for e in entries]
    qss = [dict(problems.QP_SETTINGS, rho=e[1]) for e in entries]
    return miosqp_amd.setup_models(prs, dict(problems.BNB_SETTINGS), qss, info=info, **kw)


def _own(shape, **qs):
    from miosqp_amd import bnb
    pr = sc.instance(shape)[0]
    mdl = bnb.MIOSQP()
    mdl.setup(pr["P"], pr["q"], pr["A"], pr["l"].copy(), pr["u"].copy(), pr["i_idx"], pr["i_l"], pr["i_u"],
              dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS, **qs))
    return mdl


def _close(models):
    for m in models:
        m.work.solver.close()


_SHARED = {}


@pytest.fixture(scope="module", autouse=True)
def _shared_models_are_closed_and_no_group_is_left():
    from miosqp_amd import qp
    live = qp.setup_groups_live()
    yield
    for models, _ in _SHARED.values():
        _close(models)
    _SHARED.clear()
    assert qp.setup_groups_live() == live


def _shared(key, make):
    if key not in _SHARED:
        info = {}
        _SHARED[key] = (make(info), info)
    return _SHARED[key]


def _device():
    """(models, info) of ONE call over LIST with the three keywords"""
    return _shared("device", lambda info: _setup(LIST, info=info, **KEYS))


def _plain():
    """... of the same list without the new keyword: the large rho="auto" models through MIOSQP.setup"""
    return _shared("plain", lambda info: _setup(LIST, info=info, rho_auto="device", large="device"))


def _twins():
    """... of the large rho="auto" models in one setup_models(large="device") call at a FIXED rho equal to the chosen one"""
    rho = _device()[1]["rho"]
    return _shared("twins", lambda info: _setup([(LIST[k][0], rho[k]) for k in LARGE_AUTO], info=info, large="device"))


def _products(g):
    return [g.debug_factor(w)[1] for w in (0, 1, 2)] + [g.debug_product_form(w)[1] for w in range(8)] + \
           [g.debug_panel(w) for w in (0, 1)] + [np.array([g.rho()])]


def _same_products(a, b, who):
    for j, (x, y) in enumerate(zip(_products(a), _products(b))):
        np.testing.assert_array_equal(x, y, err_msg="%s: array %d" % (who, j))


def test_one_call_over_a_mixed_list():
    models, info = _device()
    assert info["batched"] == list(range(6)) and info["own"] == {} and info["launches"] == 2
    assert info["forms"] == dict(small=2, large=4) and info["rho_auto_large"] == LARGE_AUTO
    groups = {m.work.solver.setup_group() for m in models}
    assert len(groups) == 1 and None not in groups
    for k in (1, 2, 3, 4):
        fs = models[k].work.solver.factor_stats()
        assert fs["fold"] and not fs["coop"] and not fs["resident"], k
    for k in (0, 5):
        assert models[k].work.solver.factor_stats()["resident"], k
    print("setup_models large rho auto: 6 models, device %.3f ms, rho %s" % (1e3 * info["device_time"], info["rho"]))


@pytest.mark.parametrize("k", LARGE_AUTO, ids=[str(LIST[k][0]) for k in LARGE_AUTO])
def test_the_chosen_rho_is_the_references_and_the_per_model_paths(k):
    shape = LIST[k][0]
    models, info = _device()
    ld, f64 = chosen_reference(shape)
    assert rp.away_from_a_rounding_boundary(ld.est) and ld.rho64 == f64.rho, (rp.mantissa(ld.est), ld.rho64, f64.rho)
    rho = info["rho"][k]
    own = [_own(shape, rho="auto"), _own(shape, rho="auto", coop=0, resident=0, fold=1)]
    try:
        got = [m.work.solver.rho() for m in own]
        print("rho %s: launch %.17g, reference %.17g (estimate %.17g), MIOSQP.setup %.17g, with coop=0 resident=0 fold=1 %.17g"
              % (shape, rho, ld.rho64, ld.est, got[0], got[1]))
        assert rho == ld.rho64 and rho == got[0] and rho == got[1] and rho != 0.1
        assert models[k].work.solver.rho() == rho
        fs = own[1].work.solver.factor_stats()
        assert fs["fold"] and not fs["coop"] and not fs["resident"]
    finally:
        _close(own)


@pytest.mark.parametrize("k", LARGE_AUTO, ids=[str(LIST[k][0]) for k in LARGE_AUTO])
def test_products_against_the_long_double_reference_at_the_chosen_rho(k):
    shape = LIST[k][0]
    models, info = _device()
    g, rho = models[k].work.solver, info["rho"][k]
    ld, f64 = sc.reference(shape, rho=rho, inverses=False)
    n, M = shape[0], g.m
    N = n + M
    sc.check("d2inv", g.debug_factor(0)[0], ld.d2inv, f64.d2inv, n)
    Linv, Linv_raw = g.debug_factor(1)
    LinvT, LinvT_raw = g.debug_factor(2)
    sc.check("Linv", Linv, ld.Linv, f64.Linv, n)
    assert np.all(np.triu(Linv) == 0.0)
    np.testing.assert_array_equal(LinvT, Linv.T)
    assert np.all(Linv_raw[:, n:] == 0.0) and np.all(LinvT_raw[:, n:] == 0.0)
    F, raw = g.debug_product_form(0)
    assert F.shape == (n, N)
    sc.check("f_rows", F, cb.product_form_reference(ld, rho), cb.product_form_reference(f64, rho), n)
    assert np.all(raw[:, N:] == 0.0)
    np.testing.assert_array_equal(F[:, M:], Linv)
    GmT, GmT_raw = g.debug_product_form(1)
    np.testing.assert_array_equal(GmT, F[:, :M].T)
    assert np.all(GmT_raw[:, n:] == 0.0)
    # the panels: -rho Abar on the device and in the host's mirror
    for dev, host in ((0, 2), (1, 3)):
        np.testing.assert_array_equal(g.debug_panel(dev), g.debug_panel(host))
    Ad = g.debug_product_form(2)[0]
    assert sorted(np.unique(g.debug_panel(1)[g.debug_panel(1) != 0.0])) == sorted(np.unique((-rho * Ad)[Ad != 0.0]))


def test_products_bit_for_bit_those_of_a_fixed_rho_set_up_at_the_chosen_rho():
    models, info = _device()
    twins, tinfo = _twins()
    assert tinfo["batched"] == [0, 1, 2] and tinfo["launches"] == 1 and tinfo["forms"] == dict(small=0, large=3)
    assert tinfo["rho_auto_large"] == []
    for j, k in enumerate(LARGE_AUTO):
        assert tinfo["rho"][j] == info["rho"][k]
        _same_products(models[k].work.solver, twins[j].work.solver, str(LIST[k][0]))


def test_trees_bit_for_bit_those_of_the_fixed_rho_twins():
    """iterates and control block are what a fresh set-up leaves: solve_models(large="device") on the launch's large
    rho="auto" models and on their fixed-rho twins"""
    import miosqp_amd
    models, _ = _device()
    twins, _ = _twins()
    ia, ib = {}, {}
    a = miosqp_amd.solve_models([models[k] for k in LARGE_AUTO], info=ia, large="device")
    b = miosqp_amd.solve_models(twins, info=ib, large="device")
    assert ia["own"] == {} and ib["own"] == {} and ia["forms"] == ib["forms"] and ia["overflow"] == ib["overflow"] == []
    for j, k in enumerate(LARGE_AUTO):
        who = str(LIST[k][0])
        print("%s: %s %d nodes %d iterations %.17g" % (who, a[j]["status"], a[j]["nodes"], a[j]["osqp_iter"], a[j]["upper_glob"]))
        assert (a[j]["status"], a[j]["nodes"], a[j]["osqp_iter"]) == (b[j]["status"], b[j]["nodes"], b[j]["osqp_iter"]), who
        assert a[j]["nodes"] > 0 and a[j]["osqp_iter"] > 0
        np.testing.assert_array_equal(a[j]["x"], b[j]["x"], err_msg=who)
        assert a[j]["upper_glob"] == b[j]["upper_glob"], who


def test_without_the_keyword_such_models_are_set_up_in_place_and_the_neighbours_do_not_move():
    models, info = _device()
    plain, pinfo = _plain()
    assert pinfo["batched"] == [0, 2, 5] and sorted(pinfo["own"]) == LARGE_AUTO and pinfo["rho_auto_large"] == []
    assert all(pinfo["own"][k] == OWN_REASON for k in LARGE_AUTO)
    assert pinfo["forms"] == dict(small=2, large=1) and pinfo["launches"] == 2
    assert all(plain[k].work.solver.setup_group() is None for k in LARGE_AUTO)
    assert pinfo["rho"] == info["rho"]
    for k in (0, 2, 5):  # the small rho="auto" one, the large and the small fixed-rho ones
        _same_products(models[k].work.solver, plain[k].work.solver, "neighbour %d" % k)
    for k in (0, 5):  # ... with the explicit inverse and Kc of the small launch
        a, b = models[k].work.solver, plain[k].work.solver
        for w in (3, 4):
            np.testing.assert_array_equal(a.debug_factor(w)[1], b.debug_factor(w)[1])


def test_permuting_the_list_gives_the_same_products_and_rho_bit_for_bit():
    models, info = _device()
    perm = [4, 0, 3, 5, 1, 2]
    pinfo = {}
    again = _setup([LIST[k] for k in perm], info=pinfo, **KEYS)
    try:
        assert pinfo["batched"] == list(range(6)) and pinfo["launches"] == 2
        assert pinfo["rho_auto_large"] == [0, 2, 4]
        for j, k in enumerate(perm):
            assert pinfo["rho"][j] == info["rho"][k]
            _same_products(again[j].work.solver, models[k].work.solver, "position %d" % k)
    finally:
        _close(again)


def _descriptor(pr, **qs):
    Ae, l, u = problems.extended(pr)
    return dict(P=pr["P"], q=pr["q"], A=Ae, l=l, u=u, i_idx=pr["i_idx"], m_orig=pr["A"].shape[0],
                settings=dict(problems.QP_SETTINGS, **qs))


def test_refusals():
    import miosqp_amd
    from miosqp_amd import qp
    live = qp.setup_groups_live()
    auto, fixed = dict(problems.QP_SETTINGS, rho="auto"), dict(problems.QP_SETTINGS)
    assert qp.setup_models_eligible_large_auto(20, 174, auto) and qp.setup_models_eligible_large_auto(20, 174, fixed)
    assert qp.setup_models_eligible_large_auto(197, 3, auto) and not qp.setup_models_eligible_large_auto(198, 3, auto)
    assert qp.setup_models_eligible_large_auto(198, 3, fixed) and not qp.setup_models_eligible_large_auto(10, 7, auto)
    assert not qp.setup_models_eligible_large_auto(20, 174, dict(auto, coop=1))
    assert not qp.setup_models_eligible_large(20, 174, auto)  # the existing entry keeps its answer
    small, edge = sc.instance((10, 5, 2))[0], problems.random_miqp(198, 2, 1, seed=198)
    # the library: n = 198 at rho="auto" is beyond the rule of the new entry, refused with the rule and the position
    with pytest.raises(RuntimeError, match=r"rho_auto = 1 beyond the large launch that chooses rho.*n <= 197.*\(model 1\)"):
        qp.setup_models([_descriptor(small), _descriptor(edge, rho="auto")], large=True, large_auto=True)
    # ... without large_auto a large rho="auto" model is refused as before
    with pytest.raises(RuntimeError, match=r"builds a fixed rho only \(model 0\)"):
        qp.setup_models([_descriptor(sc.instance((20, 170, 4))[0], rho="auto")], large=True)
    # ... and large_auto decides for the large models only: a small one still needs rho_auto_in_launch
    with pytest.raises(RuntimeError, match=r"does not take this model.*\(model 0\)"):
        qp.setup_models([_descriptor(small, rho="auto")], large=True, large_auto=True)
    assert qp.setup_groups_live() == live
    # the package sets the model beyond the rule up in place, the rule named
    info = {}
    models = miosqp_amd.setup_models([small, edge], dict(problems.BNB_SETTINGS), [fixed, auto], info=info, **KEYS)
    try:
        assert info["batched"] == [0] and list(info["own"]) == [1] and info["rho_auto_large"] == []
        assert "LDS rule" in info["own"][1] and "n <= 197" in info["own"][1]
        assert models[1].work.solver.setup_group() is None and info["forms"] == dict(small=1, large=0)
    finally:
        _close(models)
    assert qp.setup_groups_live() == live


def test_a_bad_pivot_of_the_second_factor_raises_with_the_chosen_rho_and_the_position():
    """the negative-entry recipe of tests/test_setup_models_auto_cpu.py at a large shape: n = 100, diagonal P with one
    negative entry, A = 3 I (n + M = 200), a starting rho of 10; the cost is that recipe's on the first twelve variables
    and zero on the others (the problem separates by variable, so the rule sees the recipe's norms: with the cost spread
    over all hundred, or A stacked twice, the reference chooses a rho above 1 and the second factor exists).  Both facts
    from the reference alone, before the device is asked: the first factor exists, the second does not."""
    from miosqp_amd import qp
    n, start = 100, 10.0
    p = np.ones(n)
    p[5] = -0.5
    q = np.zeros(n)
    q[:12] = 30.0 * np.cos(1.0 + np.arange(12))
    P, A, l, u = spa.diags(p).tocsc(), (3.0 * spa.identity(n, format="csc")).tocsc(), -np.ones(n), np.ones(n)
    ld, f64 = rp.choose(("negative entry large",), P.toarray(), A.toarray(), q, l, u, rho=start, sigma=sc.SIGMA, passes=0)
    assert rp.away_from_a_rounding_boundary(ld.est) and ld.rho64 == f64.rho
    assert sr.run(P.toarray(), A.toarray(), q, start, sc.SIGMA, 0, np.longdouble, inverses=False).bad_pivot is None
    assert sr.run(P.toarray(), A.toarray(), q, ld.rho64, sc.SIGMA, 0, np.longdouble, inverses=False).bad_pivot == 5
    live = qp.setup_groups_live()
    small = _descriptor(sc.instance((10, 5, 2))[0])
    bad = dict(P=P, q=q, A=A, l=l, u=u, settings=dict(problems.QP_SETTINGS, scaling=0, rho=start, rho_auto=1))
    assert qp.setup_models_shape(n, n) == 2
    with pytest.raises(RuntimeError, match=r"non-positive pivot.*\(model 1, pivot 5, at the rho chosen at set-up 0\.0077") as ei:
        qp.setup_models([small, bad], large=True, large_auto=True)
    print(ei.value)
    assert qp.setup_groups_live() == live
    # the first factor fails as it always did, without the chosen rho in the text
    with pytest.raises(RuntimeError, match=r"non-positive pivot.*\(model 0, pivot 5\)"):
        qp.setup_models([dict(bad, settings=dict(problems.QP_SETTINGS, scaling=0, rho=0.01, rho_auto=1))], large=True, large_auto=True)
    assert qp.setup_groups_live() == live
