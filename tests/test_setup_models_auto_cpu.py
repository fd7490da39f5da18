"""setup_models with rho chosen inside the launch, on the CPU: the reference of the rho-once recipe
(tests/rho_probe_reference.py) proved against the oracle backend; the ARITHMETIC of k_setup_models_auto -- the phases of
setup_models_body.hpp: body_auto, run by tests/setup_models_auto_body_cpu.cpp with a loop over the thread index, built
with -fsanitize=address,undefined and run as its own executable -- against that reference in long double; the edges of the
rule; the new argument check (tests/setup_plan_auto_fuzz.cpp, sanitized as well); and the keyword's plumbing on the oracle
backend.  Nothing here touches a GPU.

The chosen rho is asserted EQUAL to the reference's.  That rests on a condition, asserted from the reference alone for
every input: the mantissa r / 10^floor(log10 r) * 10 of the long-double estimate has a fractional part at least 0.01
away from .5 (rho_probe_reference.away_from_a_rounding_boundary)."""
import inspect
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as spa

import miosqp_amd
import rho_probe_reference as rp
import setup_cases as sc
import setup_models_auto_cpu_body as ab
import setup_models_cpu_body as cb
import setup_reference as sr
from miosqp_amd import problems
from oracle import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(3, 2, 1), sc.SMALL, (65, 20, 5), (129, 30, 10), (100, 82, 10), (12, 30, 6)]  # n + M = 192 and M > n among them
PROBE_PHASES = 1 + 4 * rp.RHO_ONCE_ITERS + 2   # bounds and zero; four per iteration; the three products, the rule
REFACTOR_EXTRA = 3 + 1                         # clear, Pbar + sigma I, rho Abar^T Abar ... the panel's values


def dense(P):
    Pd = np.triu(spa.csc_matrix(P).toarray())  # the engine reads the upper triangle only
    return Pd + np.triu(Pd, 1).T


def chosen_reference(shape, rho=rp.RHO0):
    """(long double, float64) runs of the recipe on setup_cases.instance(shape)"""
    pr, P, A, l, u = sc.instance(shape)
    return rp.choose(("random_miqp",) + tuple(shape), dense(P), A.toarray(), np.asarray(pr["q"]), l, u, rho=rho, sigma=sc.SIGMA,
                     passes=sc.PASSES)


@pytest.fixture(scope="module")
def body(tmp_path_factory):
    d = tmp_path_factory.mktemp("setup_models_auto_body")
    return ab.build(d), d


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_the_reference_in_float64_chooses_the_rho_the_oracle_backend_reports(shape):
    pr, P, A, l, u = sc.instance(shape)
    ld, f64 = chosen_reference(shape)
    assert rp.away_from_a_rounding_boundary(ld.est), rp.mantissa(ld.est)
    o = oracle.OSQP()
    o.setup(P, pr["q"], A, l, u, rho="auto", **problems.QP_SETTINGS)
    print("rho chosen", shape, "long double %.17g -> %.17g, float64 %.17g, oracle %.17g" % (ld.est, ld.rho64, f64.rho, o.rho()))
    assert f64.rho == o.rho() and ld.rho64 == o.rho() and o.rho() != rp.RHO0


def check_products(o, ld, f64, n, M, rho, l, u, guard_tol=1e-9):
    """the assertions of test_kernel_arithmetic_against_the_long_double_reference, at `rho`"""
    N = n + M
    sc.check("d2inv", o.d2inv, ld.d2inv, f64.d2inv, n)
    sc.check("Linv", o.Linv[:, :n], ld.Linv, f64.Linv, n)
    assert np.all(np.triu(o.Linv[:, :n]) == 0.0)
    np.testing.assert_array_equal(o.LinvT[:, :n], o.Linv[:, :n].T)
    assert np.all(o.Linv[:, n:] == 0.0) and np.all(o.LinvT[:, n:] == 0.0)
    Kinv = o.W[:, :N].astype(np.longdouble)
    Kinv[:M, :M] -= np.longdouble(rho) * np.eye(M, dtype=np.longdouble)
    sc.check("W", Kinv, ld.Kinv, f64.Kinv, n)
    assert np.all(o.W[:, N:] == 0.0) and np.all(o.Kc[:, N:] == 0.0)
    sc.check("f_rows", o.f_rows[:, :N], cb.product_form_reference(ld, rho), cb.product_form_reference(f64, rho), n)
    assert np.all(o.f_rows[:, N:] == 0.0)
    np.testing.assert_array_equal(o.f_GmT[:, :n], o.f_rows[:, :M].T)
    assert np.all(o.f_GmT[:, n:] == 0.0)
    np.testing.assert_allclose(o.Kc[:, :N], sr.kc(ld.Pbar, ld.Abar).astype(np.float64), rtol=1e-14, atol=0.0)
    np.testing.assert_array_equal(o.l, o.E * np.maximum(l, -1e30))
    np.testing.assert_array_equal(o.u, o.E * np.minimum(u, 1e30))
    if guard_tol is not None:
        assert 0.0 <= o.guard <= guard_tol  # COOP_GUARD_TOL (kernels_guard.inc)


def check_panels(o, rho):
    """-rho Abar with the expression of build_factor(reuse_rows); padding exactly +0.0"""
    for got, plain in ((o.pv_L, o.At_val), (o.pc_L, o.A_val)):
        want = np.where(plain == 0.0, 0.0, -rho * plain)
        np.testing.assert_array_equal(got, want)
        assert not np.any(np.signbit(got[plain == 0.0]))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_probe_rule_and_products_against_the_long_double_reference(body, shape):
    """x, z, y after the 50th iteration and the estimate under the rule of setup_cases.check (float64 floor, sr.bound);
    the chosen rho EQUAL to the reference's; every product against the reference at the chosen rho; the panels"""
    exe, d = body
    pr, P, A, l, u = sc.instance(shape)
    n, M = shape[0], A.shape[0]
    ld, f64 = chosen_reference(shape)
    assert rp.away_from_a_rounding_boundary(ld.est), rp.mantissa(ld.est)
    o = ab.run(exe, d, P, pr["q"], A, l, u, rho=rp.RHO0, sigma=sc.SIGMA, alpha=rp.ALPHA, passes=sc.PASSES)
    assert o.bad_pivot == 0 and o.lds_doubles * 8 <= 160 * 1024
    for name in ("x", "z", "y"):
        sc.check(name, getattr(o, name), getattr(ld, name), getattr(f64, name), n)
    floor = abs(float((f64.est - ld.est) / ld.est))
    got = abs(float((np.longdouble(o.rho_est) - ld.est) / ld.est))
    print("rho estimate %s: long double %.17g, float64 floor %.3e, measured %.3e, bound %.3e" % (shape, ld.est, floor, got, sr.bound(floor, n)))
    assert got <= sr.bound(floor, n)
    assert o.rho == ld.rho64 and o.rho == f64.rho and o.rho != rp.RHO0
    rld, r64 = sc.reference(shape, rho=o.rho)
    check_products(o, rld, r64, n, M, o.rho, l, u)
    check_panels(o, o.rho)


def test_zero_cost_with_zero_inside_the_bounds_stays_at_zero_and_clamps_to_1e_minus_6(body):
    exe, d = body
    pr, P, A, l, u = sc.instance(sc.SMALL)
    n, M = sc.SMALL[0], A.shape[0]
    q = np.zeros(n)
    l, u = np.minimum(l, -1.0), np.maximum(u, 1.0)
    ld, f64 = rp.choose(("zero cost",), dense(P), A.toarray(), q, l, u, sigma=sc.SIGMA, passes=sc.PASSES)
    assert not ld.x.any() and not ld.z.any() and not ld.y.any() and ld.est == np.longdouble(1e-6) and ld.rho64 == 1e-6
    o = ab.run(exe, d, P, q, A, l, u, rho=rp.RHO0, sigma=sc.SIGMA, alpha=rp.ALPHA, passes=sc.PASSES)
    assert o.bad_pivot == 0
    assert not o.x.any() and not o.z.any() and not o.y.any()
    assert o.rho_est == 1e-6 and o.rho == 1e-6
    rld, r64 = sr.products(("zero cost",), dense(P), A.toarray(), q, rho=1e-6, sigma=sc.SIGMA, passes=sc.PASSES)
    check_products(o, rld, r64, n, M, 1e-6, l, u, guard_tol=None)  # (K holds -1e6 on its diagonal: the guard is not judged)
    check_panels(o, 1e-6)


def test_an_estimate_equal_to_the_starting_rho_builds_no_second_factor(body):
    """the body is given a starting rho the reference maps to itself: the phases that run are those of the fixed-rho body
    and of the probe, none of the second factor, and the products are the fixed-rho body's bit for bit"""
    exe, d = body
    shape = sc.SMALL
    pr, P, A, l, u = sc.instance(shape)
    start = 0.25  # found by walking the two-digit values with the reference; that it IS a fixed point is asserted here
    ld, f64 = chosen_reference(shape, rho=start)
    assert ld.rho64 == start and f64.rho == start and rp.away_from_a_rounding_boundary(ld.est), (start, ld.est)
    print("fixed point of the rule on", shape, ":", start)
    fixed = ab.run(exe, d, P, pr["q"], A, l, u, rho=start, sigma=sc.SIGMA, alpha=rp.ALPHA, passes=sc.PASSES, rho_auto=0)
    o = ab.run(exe, d, P, pr["q"], A, l, u, rho=start, sigma=sc.SIGMA, alpha=rp.ALPHA, passes=sc.PASSES)
    moved = ab.run(exe, d, P, pr["q"], A, l, u, rho=rp.RHO0, sigma=sc.SIGMA, alpha=rp.ALPHA, passes=sc.PASSES)
    assert o.rho == start and o.bad_pivot == 0 and fixed.rho == 0.0 and fixed.rho_est == 0.0
    assert o.phases == fixed.phases + PROBE_PHASES
    n = shape[0]
    ldl_phases = 2 * n - 1 + 1 + (n - 1) + 1  # phase 3 (two per column, one for the last), phase 4 (first copy, rows), 5a
    assert moved.rho != rp.RHO0 and moved.phases == fixed.phases + PROBE_PHASES + REFACTOR_EXTRA + ldl_phases
    for name in ("d2inv", "Linv", "LinvT", "f_rows", "f_GmT", "W", "Kc", "pv_L", "pc_L", "l", "u"):
        np.testing.assert_array_equal(getattr(o, name), getattr(fixed, name), err_msg=name)
    assert o.guard == fixed.guard


def _negative_entry_problem():
    """diag P with one negative entry, A = 3 I: the sign of pivot 5 of S = P + sigma I + 9 rho I is decided by rho"""
    n = 12
    p = np.ones(n)
    p[5] = -0.5
    q = 30.0 * np.cos(1.0 + np.arange(n))
    return n, spa.diags(p).tocsc(), q, (3.0 * spa.identity(n, format="csc")).tocsc(), -np.ones(n), np.ones(n)


def test_a_bad_pivot_of_the_second_factor_is_reported_with_its_factor(body):
    exe, d = body
    n, P, q, A, l, u = _negative_entry_problem()
    start = 10.0
    ld, f64 = rp.choose(("negative entry",), P.toarray(), A.toarray(), q, l, u, rho=start, sigma=sc.SIGMA, passes=0)
    assert rp.away_from_a_rounding_boundary(ld.est)
    # the reference: the factor at the starting rho exists, the one at the rho the rule chooses does not
    assert sr.run(P.toarray(), A.toarray(), q, start, sc.SIGMA, 0, np.longdouble, inverses=False).bad_pivot is None
    assert sr.run(P.toarray(), A.toarray(), q, ld.rho64, sc.SIGMA, 0, np.longdouble, inverses=False).bad_pivot == 5
    print("negative entry: rho %.3g -> %.17g (%.3g): pivot 5 of the second factor is %.3g" % (start, ld.est, ld.rho64, -0.5 + 9 * ld.rho64))
    o = ab.run(exe, d, P, q, A, l, u, rho=start, sigma=sc.SIGMA, alpha=rp.ALPHA, passes=0)
    assert (o.bad_pivot, o.pivot, o.guard) == (2, 5, -1.0) and o.rho == ld.rho64
    # the first factor fails as it always did, as factor 1
    bad = ab.run(exe, d, P, q, A, l, u, rho=0.01, sigma=sc.SIGMA, alpha=rp.ALPHA, passes=0)
    assert (bad.bad_pivot, bad.pivot) == (1, 5)


def test_the_second_factor_stage_called_on_its_own_at_a_rho_the_reference_says_fails(body):
    """A = I beside the same P: the run from rho = 1 is a good one; the stage is then called once more at 0.1 (pivot 5 of
    S is -0.5 + 1e-6 + 0.1) and at 0.8"""
    exe, d = body
    n, P, _, _, l, u = _negative_entry_problem()
    A, q = spa.identity(n, format="csc"), 0.3 * np.ones(n)
    for again, want in ((0.1, 5), (0.8, None)):
        ref = sr.run(P.toarray(), A.toarray(), q, again, sc.SIGMA, 0, np.longdouble, inverses=False)
        assert ref.bad_pivot == want
        o = ab.run(exe, d, P, q, A, l, u, rho=1.0, sigma=sc.SIGMA, alpha=rp.ALPHA, passes=0, rho_again=again)
        assert o.bad_pivot == 0 and o.rho > 0.5
        if want is None:
            assert (o.again_ok, o.again_bad_pivot) == (1.0, 0.0)
            r64 = sr.run(P.toarray(), A.toarray(), q, again, sc.SIGMA, 0, np.float64, inverses=False)
            sc.check("d2inv", o.again_d2inv, ref.d2inv, r64.d2inv, n)
        else:
            assert (o.again_ok, o.again_bad_pivot, o.again_pivot) == (0.0, 2.0, float(want))


def test_sanitized_argument_check_of_the_new_entry(tmp_path):
    exe = str(tmp_path / "setup_plan_auto_fuzz")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(HERE, "setup_plan_auto_fuzz.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "setup_plan auto ok" in r.stdout


def test_the_keyword_exists():
    from miosqp_amd import _lib, qp
    assert inspect.signature(miosqp_amd.setup_models).parameters["rho_auto"].default is None
    assert inspect.signature(qp.setup_models).parameters["rho_auto_in_launch"].default is False
    assert "miosqp_qp_setup_models_auto" in _lib.SYMBOLS and "miosqp_qp_debug_panel" in _lib.SYMBOLS
    assert _lib.SYMBOLS["miosqp_qp_setup_models_auto"] == _lib.SYMBOLS["miosqp_qp_setup_models"]
    assert callable(qp.OSQP.debug_panel)
    header = open(os.path.join(os.path.dirname(HERE), "include", "miosqp_amd.h")).read()
    assert "int miosqp_qp_setup_models_auto(int32_t B, const miosqp_setup_model *models," in header
    assert "int miosqp_qp_debug_panel(miosqp_qp_engine *e," in header


def test_on_the_oracle_backend_the_keyword_keeps_such_models_in_place_and_other_values_are_refused():
    prs = [problems.random_miqp(n, m, p, seed=s) for n, m, p, s in [(12, 30, 6, 8), (10, 5, 2, 0)]]
    qss = [dict(problems.QP_SETTINGS, rho="auto"), dict(problems.QP_SETTINGS)]
    info = {}
    got = miosqp_amd.setup_models(prs, dict(problems.BNB_SETTINGS), qss, info=info, backend=oracle, rho_auto="device")
    assert info["batched"] == [] and sorted(info["own"]) == [0, 1] and all("backend" in why for why in info["own"].values())
    assert info["rho"] == [got[0].work.solver.rho(), 0.1] and info["rho"][0] != 0.1
    plain = {}
    miosqp_amd.setup_models(prs, dict(problems.BNB_SETTINGS), qss, info=plain, backend=oracle)
    assert plain["rho"] == info["rho"]
    for bad in ("host", True, 1, "auto"):
        with pytest.raises(ValueError, match="rho_auto must be None or"):
            miosqp_amd.setup_models(prs, dict(problems.BNB_SETTINGS), qss, backend=oracle, rho_auto=bad)
