"""setup_models(rho_auto="device") on the HIP engine (needs an MI355X): rho="auto" models go into the one launch
(k_setup_models_auto) and the workgroup that builds a model chooses its rho.  Checked per position against the long-double
reference of the rho-once recipe (tests/rho_probe_reference.py) and of the set-up products at the CHOSEN rho
(tests/setup_reference.py) under the rule of setup_cases.check, and against the same list set up without the keyword, where
every rho="auto" model goes through MIOSQP.setup's two set-ups.

The chosen rho is asserted EQUAL to the reference's and to the per-model set-up's; the condition that makes that a fact and
not a measurement (the long-double mantissa at least 0.01 away from a rounding boundary) is asserted for every input from
the reference alone.

One call with the keyword and one without, over the same mixed list, are built once per session and shared, read-only."""
import numpy as np
import pytest
import scipy.sparse as spa

import rho_probe_reference as rp
import setup_cases as sc
import setup_models_cpu_body as cb
import setup_reference as sr
from miosqp_amd import problems
from test_setup_models_auto_cpu import chosen_reference, dense

pytestmark = pytest.mark.gpu

AUTO = [(10, 5, 2), (12, 30, 6), (20, 10, 8), (50, 25, 25), (50, 100, 10)]
FIXED = [(63, 20, 5), (3, 2, 1)]
BEYOND = (80, 120, 20)  # n + M = 220: beyond one workgroup
# (shape, rho): two rho-0.1 models between the rho="auto" ones, the one beyond a workgroup before the last
LIST = [(AUTO[0], "auto"), (FIXED[0], 0.1), (AUTO[1], "auto"), (AUTO[2], "auto"), (FIXED[1], 0.1), (AUTO[3], "auto"),
        (BEYOND, "auto"), (AUTO[4], "auto")]
IN_LAUNCH = [0, 1, 2, 3, 4, 5, 7]
SOL_TOL = 1e-8  # tests/test_gpu_parity.py: its tolerance for two arithmetics of one algorithm


def _setup(entries, info=None, **kw):
    import miosqp_amd
    prs = [e[2] if len(e) > 2 else sc.instance(e[0])[0] for e in entries]
    qss = [dict(problems.QP_SETTINGS, rho=e[1]) for e in entries]
    return miosqp_amd.setup_models(prs, dict(problems.BNB_SETTINGS), qss, info=info, **kw)


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


def _device():
    """(models, info) of ONE call over LIST with rho_auto="device" """
    if "device" not in _SHARED:
        info = {}
        _SHARED["device"] = (_setup(LIST, info=info, rho_auto="device"), info)
    return _SHARED["device"]


def _plain():
    """(models, info) of the same list without the keyword: the rho="auto" models through MIOSQP.setup"""
    if "plain" not in _SHARED:
        info = {}
        _SHARED["plain"] = (_setup(LIST, info=info), info)
    return _SHARED["plain"]


def _products(g):
    return [g.debug_factor(w)[1] for w in (0, 1, 2, 3, 4)] + [g.debug_product_form(w)[1] for w in range(8)] + \
           [g.debug_panel(w) for w in (0, 1)] + [np.array([g.rho()])]


def _check_products(g, ld, f64, n, rho):
    M = g.m
    N = n + M
    sc.check("d2inv", g.debug_factor(0)[0], ld.d2inv, f64.d2inv, n)
    Linv, Linv_raw = g.debug_factor(1)
    sc.check("Linv", Linv, ld.Linv, f64.Linv, n)
    assert np.all(np.triu(Linv) == 0.0) and np.all(Linv_raw[:, n:] == 0.0)
    np.testing.assert_array_equal(g.debug_factor(2)[0], Linv.T)
    W, W_raw = g.debug_factor(3)
    Kinv = W.astype(np.longdouble)
    Kinv[:M, :M] -= np.longdouble(rho) * np.eye(M, dtype=np.longdouble)
    sc.check("W", Kinv, ld.Kinv, f64.Kinv, n)
    assert np.all(W_raw[:, N:] == 0.0)
    F, F_raw = g.debug_product_form(0)
    sc.check("f_rows", F, cb.product_form_reference(ld, rho), cb.product_form_reference(f64, rho), n)
    assert np.all(F_raw[:, N:] == 0.0)
    np.testing.assert_array_equal(g.debug_product_form(1)[0], F[:, :M].T)


def test_the_keyword_exists():
    import inspect
    import miosqp_amd
    from miosqp_amd import _lib, qp
    assert inspect.signature(miosqp_amd.setup_models).parameters["rho_auto"].default is None
    assert inspect.signature(qp.setup_models).parameters["rho_auto_in_launch"].default is False
    assert hasattr(_lib.load(), "miosqp_qp_setup_models_auto") and "miosqp_qp_setup_models_auto" in _lib.SYMBOLS


def test_without_the_keyword_a_rho_auto_model_is_still_set_up_on_its_own():
    models, info = _plain()
    assert info["batched"] == [1, 4] and sorted(info["own"]) == [0, 2, 3, 5, 6, 7]
    assert all(info["own"][k] == 'rho="auto"' for k in (0, 2, 3, 5, 6, 7))
    assert all(models[k].work.solver.setup_group() is None for k in info["own"])


def test_one_launch_takes_the_rho_auto_models_and_the_one_beyond_a_workgroup_goes_own():
    models, info = _device()
    assert info["batched"] == IN_LAUNCH and list(info["own"]) == [6] and "220" in info["own"][6]
    assert info["launches"] == 1 and info["device_time"] > 0.0
    groups = {models[k].work.solver.setup_group() for k in IN_LAUNCH}
    assert len(groups) == 1 and None not in groups and models[6].work.solver.setup_group() is None
    for k in IN_LAUNCH:
        fs = models[k].work.solver.factor_stats()
        assert fs["fold"] and fs["resident"] and not fs["coop"] and not fs["setup_on_device"]
    print("setup_models(rho_auto='device'): 7 models, device %.3f ms; rho %s" % (1e3 * info["device_time"], info["rho"]))


@pytest.mark.parametrize("k", [k for k, e in enumerate(LIST) if e[1] == "auto"], ids=[str(e[0]) for e in LIST if e[1] == "auto"])
def test_the_chosen_rho_is_the_references_and_the_per_model_set_ups(k):
    shape = LIST[k][0]
    ld, f64 = chosen_reference(shape)
    assert rp.away_from_a_rounding_boundary(ld.est), rp.mantissa(ld.est)
    got, own = _device()[1]["rho"][k], _plain()[1]["rho"][k]
    print("rho", shape, "device call %.17g, MIOSQP.setup %.17g, long double %.17g -> %.17g" % (got, own, ld.est, ld.rho64))
    assert got == own and got == ld.rho64 and got != rp.RHO0
    assert _device()[0][k].work.solver.rho() == got


@pytest.mark.parametrize("shape", AUTO, ids=str)
def test_products_at_the_chosen_rho_against_the_long_double_reference(shape):
    k = [e[0] for e in LIST].index(shape)
    g = _device()[0][k].work.solver
    rho = g.rho()
    ld, f64 = sc.reference(shape, rho=rho)
    _check_products(g, ld, f64, shape[0], rho)
    resid, tol, tripped = g.inverse_guard()
    assert 0.0 <= resid <= tol and not tripped
    # the panel's values on the device are the host's mirror bit for bit, and they are those of the chosen rho
    at_01 = _plain()[0][1].work.solver  # (a rho-0.1 engine of another shape: only to say what "moved" means below)
    for dev, host in ((0, 2), (1, 3)):
        a, b = g.debug_panel(dev), g.debug_panel(host)
        np.testing.assert_array_equal(a, b)
        assert not np.any(np.signbit(a[a == 0.0])) and np.any(a != 0.0)
    own = _plain()[0][k].work.solver  # MIOSQP.setup at the same rho: the same expression, the same bits
    np.testing.assert_array_equal(g.debug_panel(0), own.debug_panel(0))
    np.testing.assert_array_equal(g.debug_panel(1), own.debug_panel(1))
    assert at_01.rho() == 0.1
    # iterates and control block as a fresh set-up leaves them: the root relaxation solves as on the per-model engine
    d = _device()[0][k].work.data
    ra = g.solve_node(d.l, d.u, np.zeros(d.n), np.zeros(len(d.l)))
    rb = own.solve_node(d.l, d.u, np.zeros(d.n), np.zeros(len(d.l)))
    assert ra.status_val == rb.status_val and ra.iter == rb.iter


def test_the_fixed_rho_models_are_bit_for_bit_what_the_call_without_the_keyword_gives():
    for k in (1, 4):
        a, b = _device()[0][k].work.solver, _plain()[0][k].work.solver
        assert a.rho() == 0.1 and b.rho() == 0.1
        for x, y in zip(_products(a), _products(b)):
            np.testing.assert_array_equal(x, y)


def test_permuting_the_list_gives_the_same_engines_bit_for_bit():
    models, _ = _device()
    order = [7, 4, 0, 5, 1, 3, 2]
    again = _setup([LIST[k] for k in order], rho_auto="device")
    try:
        for j, k in enumerate(order):
            for a, b in zip(_products(again[j].work.solver), _products(models[k].work.solver)):
                np.testing.assert_array_equal(a, b)
    finally:
        _close(again)


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


def test_solve_models_matches_the_trees_of_the_per_model_set_ups():
    import miosqp_amd
    a = miosqp_amd.solve_models(_device()[0])
    b = miosqp_amd.solve_models(_plain()[0])
    for k, e in enumerate(LIST):
        _same_tree(a[k], b[k], sc.instance(e[0])[0], "position %d %r rho=%r" % (k, e[0], e[1]))


def test_a_model_of_n_plus_m_192_chooses_its_rho_in_the_launch():
    shape = (100, 82, 10)
    ld, f64 = chosen_reference(shape)
    assert rp.away_from_a_rounding_boundary(ld.est), rp.mantissa(ld.est)
    info = {}
    models = _setup([(shape, "auto")], info=info, rho_auto="device")
    try:
        g = models[0].work.solver
        assert info["batched"] == [0] and g.n + g.m == 192 and g.setup_group() is not None
        assert info["rho"] == [ld.rho64] and g.rho() == ld.rho64
        rld, r64 = sc.reference(shape, rho=g.rho())
        _check_products(g, rld, r64, shape[0], g.rho())
        assert not g.inverse_guard()[2]
        np.testing.assert_array_equal(g.debug_panel(0), g.debug_panel(2))
        np.testing.assert_array_equal(g.debug_panel(1), g.debug_panel(3))
    finally:
        _close(models)


def test_zero_cost_with_zero_inside_the_bounds_chooses_what_the_per_model_path_chooses():
    pr = dict(sc.instance(sc.SMALL)[0])
    pr["q"] = np.zeros(sc.SMALL[0])
    pr["l"], pr["u"] = np.minimum(pr["l"], -1.0), np.maximum(pr["u"], 1.0)
    A, l, u = problems.extended(pr)
    ld, _ = rp.choose(("zero cost gpu",), dense(pr["P"]), A.toarray(), pr["q"], l, u, sigma=sc.SIGMA, passes=sc.PASSES)
    assert ld.rho64 == 1e-6 and not ld.x.any()
    entry = [(sc.SMALL, "auto", pr)]
    dev_info, own_info = {}, {}
    dev, own = _setup(entry, info=dev_info, rho_auto="device"), _setup(entry, info=own_info)
    try:
        assert dev_info["batched"] == [0] and list(own_info["own"]) == [0]
        print("zero cost: rho in the launch %.17g, per model %.17g" % (dev_info["rho"][0], own_info["rho"][0]))
        assert dev_info["rho"] == own_info["rho"] == [1e-6]
        np.testing.assert_array_equal(dev[0].work.solver.debug_panel(0), own[0].work.solver.debug_panel(0))
    finally:
        _close(dev + own)


def test_an_indefinite_p_in_the_middle_fails_the_whole_call_and_leaves_no_group():
    import miosqp_amd
    from miosqp_amd import bnb, qp
    live = qp.setup_groups_live()
    prs = [sc.instance((10, 5, 2))[0], dict(sc.instance((10, 5, 2))[0]), sc.instance((63, 20, 5))[0]]
    p = np.ones(10)
    p[4] = -50.0
    prs[1]["P"] = spa.diags(p).tocsc()
    qs = dict(problems.QP_SETTINGS, scaling=0, rho="auto")
    with pytest.raises(RuntimeError, match=r"non-positive pivot.*position 1"):
        miosqp_amd.setup_models(prs, dict(problems.BNB_SETTINGS), qs, rho_auto="device")
    assert qp.setup_groups_live() == live
    with pytest.raises(RuntimeError, match="non-positive pivot"):  # what the per-model two-set-up path raises for it
        _bad = prs[1]
        bnb.MIOSQP().setup(_bad["P"], _bad["q"], _bad["A"], _bad["l"], _bad["u"], _bad["i_idx"], _bad["i_l"], _bad["i_u"],
                           dict(problems.BNB_SETTINGS), dict(qs))
    assert sr.run(np.diag(p), np.eye(10), np.zeros(10), sc.RHO, sc.SIGMA, 0, np.longdouble, inverses=False).bad_pivot == 4
