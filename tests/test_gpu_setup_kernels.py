"""The device set-up kernels (miosqp_amd/csrc/dense_setup.hip) against a high-precision reference of their own operation.

Every product is read back from device memory (OSQP.debug_factor) and compared with tests/setup_reference.py run in long
double; the tolerance is no fixed epsilon but the rule of setup_reference.bound: 8 x max(error of the same textbook
algorithm in float64, n 2^-53).  The shapes sit on the edges of the 64-wide tiles (setup_cases.SHAPES); the rule and the
instances are checked against the host set-up, without a GPU, in test_setup_reference_cpu.py.  Every case prints its floor,
measured error and bound (pytest -s): the table in DESIGN.md (set-up section) is made of those lines.
"""
import os

import numpy as np
import pytest
import scipy.sparse as spa

import setup_cases as sc
import setup_reference as sr
from miosqp_amd import problems

pytestmark = pytest.mark.gpu

PLAIN = dict(fold=0, coop=0, resident=0)  # the four-kernel factor form: Linv stays where the device set-up computed it
FORMS = {"plain": PLAIN, "default": {}}   # default: the product form is built on the host, Linv takes the round trip


def _setup(shape, **kw):
    from miosqp_amd import qp
    pr, P, A, l, u = sc.instance(shape)
    g = qp.OSQP()
    g.setup(P, pr["q"], A, l, u, **dict(problems.QP_SETTINGS, **kw))
    return g


def _check_factor(g, shape, ref=None):
    """d2inv, Linv, LinvT and the scaling of engine g against the reference of `shape`"""
    ld, f64 = ref if ref is not None else sc.reference(shape, inverses=False)
    n = shape[0]
    assert ld.bad_pivot is None and f64.bad_pivot is None and np.all(ld.d > 0)
    d2inv, _ = g.debug_factor(0)
    Linv, Linv_raw = g.debug_factor(1)
    LinvT, LinvT_raw = g.debug_factor(2)
    assert d2inv.shape == (n,) and Linv.shape == (n, n) and LinvT.shape == (n, n)
    assert Linv_raw.shape == (n, (n + 15) & ~15) and LinvT_raw.shape == Linv_raw.shape
    out = [sc.check("d2inv", d2inv, ld.d2inv, f64.d2inv, n), sc.check("Linv", Linv, ld.Linv, f64.Linv, n)]
    assert np.all(np.triu(Linv) == 0.0)  # strictly lower: the diagonal and everything above it exactly zero
    np.testing.assert_array_equal(LinvT, Linv.T)
    assert np.all(Linv_raw[:, n:] == 0.0) and np.all(LinvT_raw[:, n:] == 0.0)  # the padding columns
    D, E, c = g.scaling()
    np.testing.assert_allclose(D, ld.D.astype(np.float64), rtol=1e-14)
    np.testing.assert_allclose(E, ld.E.astype(np.float64), rtol=1e-14)
    assert abs(c - float(ld.c)) <= 1e-14 * float(ld.c)
    return out


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("shape", sc.SHAPES, ids=str)
def test_device_factor_against_reference(shape, form):
    """kr_norms / kr_scale / kr_scale_cost, ks_schur_row, ks_diag / ks_panel / ks_update, ks_inv / ks_out"""
    g = _setup(shape, setup_on_device=1, **FORMS[form])
    fs = g.factor_stats()
    assert fs["setup_on_device"]
    if form == "plain":
        assert not (fs["fold"] or fs["coop"] or fs["resident"] or fs["pers"])
    _check_factor(g, shape)


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("shape", sc.SHAPES, ids=str)
def test_host_factor_against_reference(shape, form):
    """the same rule on the same read-backs with the set-up on the host: anchors the rule where this file runs"""
    g = _setup(shape, setup_on_device=0, **FORMS[form])
    assert not g.factor_stats()["setup_on_device"]
    _check_factor(g, shape)


def test_stage_variants_give_the_same_factor_bitwise():
    """equilibration on the device or the host, Schur complement assembled on the device or uploaded, Linv left on the
    device or sent down and up again: the factor itself -- not only the iterates that come of it -- is the same"""
    shape = (129, 30, 10)
    got = []
    for env in ({}, {"MIOSQP_SETUP_HOST_SCHUR": "1"}, {"MIOSQP_SETUP_HOST_RUIZ": "1"},
                {"MIOSQP_SETUP_ROUNDTRIP": "1", "MIOSQP_SETUP_HOST_SCHUR": "1", "MIOSQP_SETUP_HOST_RUIZ": "1"}):
        os.environ.update(env)
        try:
            g = _setup(shape, setup_on_device=1, **PLAIN)
            got.append([g.debug_factor(w)[1] for w in (0, 1, 2)])
        finally:
            for k in env:
                del os.environ[k]
    for other in got[1:]:
        for a, b in zip(got[0], other):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("shape", [(65, 20, 5), (129, 30, 10), sc.DEV2], ids=str)
def test_factor_after_rho_auto(shape):
    """rho="auto" with the set-up on the host: the factor in use is the reference's at the rho the engine reports.  At
    n + M > 400 (the last shape) the probing iterations run on the engine itself and the factor at the chosen rho is
    rebuilt by the device factorisation from the host's Schur complement (engine.hip, `dev2`, reuse_rows); below that
    the engine is set up a second time at the chosen rho."""
    g = _setup(shape, setup_on_device=0, rho="auto")
    rho = g.rho()
    assert rho > 0
    print("rho chosen at", shape, rho)
    _check_factor(g, shape, ref=sc.reference(shape, rho=rho, inverses=False))


def _check_inverse(g, shape):
    ld, f64 = sc.reference(shape)
    n = shape[0]
    N = ld.K.shape[0]
    resid, tol, tripped = g.inverse_guard()
    assert resid >= 0.0 and resid <= tol and not tripped  # W was built and is in use: otherwise nothing is tested
    assert not g.factor_stats()["inverse_guard_tripped"]
    W, W_raw = g.debug_factor(3)
    Kc, Kc_raw = g.debug_factor(4)
    assert W.shape == (N, N) and W_raw.shape == (N, (N + 7) & ~7) and Kc_raw.shape == W_raw.shape
    # W = F^T D22^-1 F is K^-1 without the constant -rho I of its constraint block, which the solvers add themselves
    # (dense_setup.hip: "W [wh ; rx] = [rho A x~ + .. ; x~]", kernels_guard.inc: kg_apply): put back here, in long double
    M = N - n
    Kinv_dev = W.astype(np.longdouble)
    Kinv_dev[:M, :M] -= np.longdouble(sc.RHO) * np.eye(M, dtype=np.longdouble)
    sc.check("W", Kinv_dev, ld.Kinv, f64.Kinv, n)
    np.testing.assert_allclose(Kc, sr.kc(ld.Pbar, ld.Abar).astype(np.float64), rtol=1e-14, atol=0.0)


@pytest.mark.parametrize("on_dev", [0, 1])
@pytest.mark.parametrize("shape", [s for s in sc.SHAPES if sum(s) >= 64], ids=str)
def test_explicit_kkt_inverse_cooperative(shape, on_dev):
    """ks_kkt_inverse (and k_build_kc) as the cooperative solver uses them, compared entry by entry with K^-1 from
    Gauss-Jordan in long double: the first check of W that does not go through the device's own probe kernels"""
    g = _setup(shape, coop=1, resident=0, setup_on_device=on_dev)
    fs = g.factor_stats()
    assert fs["fold"] and not fs["resident"] and fs["setup_on_device"] == bool(on_dev)
    _check_inverse(g, shape)  # (debug_factor(3) raises unless the cooperative set-up built W)


@pytest.mark.parametrize("shape", [sc.SMALL, (3, 2, 1)], ids=str)
def test_explicit_kkt_inverse_resident(shape):
    """the small register-resident loop: one partial tile"""
    g = _setup(shape, resident=1)
    fs = g.factor_stats()
    assert fs["resident"] and not fs["coop"]
    _check_inverse(g, shape)


@pytest.mark.parametrize("shape", [(65, 20, 5), (129, 30, 10)], ids=str)
def test_tail_inverse_of_the_persistent_solver(shape):
    """ks_kkt_inverse with M = 0: S^-1 = Linv^T D^-1 Linv for the persistent streaming solver (pers=2, factor form)"""
    g = _setup(shape, pers=2, fold=0)
    fs = g.factor_stats()
    assert fs["pers"] and fs["tail_inverse"] and not fs["fold"]
    ld, f64 = sc.reference(shape)
    n = shape[0]
    Sinv, raw = g.debug_factor(5)
    assert Sinv.shape == (n, n) and raw.shape[1] >= n
    sc.check("Sinv", Sinv, ld.Sinv, f64.Sinv, n)


def test_read_back_refuses_what_was_not_built_and_changes_nothing():
    """a product the engine did not build is an error, never zeros; reading back leaves the iteration bitwise as it
    was (the multi-kernel form and the one-workgroup form: both run the same sums in the same order every time)"""
    rng = np.random.RandomState(0)
    for shape, kw, built in (((65, 20, 5), dict(setup_on_device=1, **PLAIN), (0, 1, 2)),
                             (sc.SMALL, dict(resident=1), (0, 1, 2, 3, 4))):
        g = _setup(shape, **kw)
        n, M = g.n, g.m
        x0, y0 = rng.randn(n), rng.randn(M)
        g.warm_start(x=x0, y=y0)
        before = g.debug_iterate(20)
        for w in range(6):
            if w in built:
                a, raw = g.debug_factor(w)
                assert np.all(np.isfinite(raw)) and np.any(a != 0.0)
            else:
                with pytest.raises(RuntimeError, match="did not build"):
                    g.debug_factor(w)
        with pytest.raises(RuntimeError, match="bad argument"):
            g.debug_factor(6)
        g.warm_start(x=x0, y=y0)
        after = g.debug_iterate(20)
        for a, b in zip(before, after):
            np.testing.assert_array_equal(a, b)


def test_nonpositive_pivot_on_the_device():
    """ks_diag's flag: a pivot that is not positive in the first block, the second block and the last partial block of
    the device factorisation is reported as an error (nothing faults: the kernels finish on whatever they hold); the
    reference stops at the same index; a valid set-up afterwards is unharmed"""
    from miosqp_amd import qp
    n = 150
    A = spa.identity(n, format="csc")
    for k in (0, 70, 149):
        p = np.ones(n)
        p[k] = -50.0
        with pytest.raises(RuntimeError, match="non-positive pivot"):
            qp.OSQP().setup(spa.diags(p).tocsc(), np.zeros(n), A, -np.ones(n), np.ones(n),
                            **dict(problems.QP_SETTINGS, scaling=0, setup_on_device=1))
        for T in (np.longdouble, np.float64):
            r = sr.run(np.diag(p), np.eye(n), np.zeros(n), sc.RHO, sc.SIGMA, 0, T, inverses=False)
            assert r.bad_pivot == k
    shape = (129, 30, 10)
    g = _setup(shape, setup_on_device=1, **PLAIN)
    assert g.factor_stats()["setup_on_device"]
    _check_factor(g, shape)
