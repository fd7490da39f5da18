"""The reference of the set-up kernel tests (setup_reference.py) and their tolerance rule, made trustworthy on the CPU
before a GPU is involved: the host set-up (miosqp_amd/csrc/factor.cpp through tests/host_harness.cpp, compiled as
test_host_factor.py compiles it) is held to the same rule, at the same shapes, as the device kernels in
test_gpu_setup_kernels.py.  If the host factor could not meet the rule at some shape, the rule or the instance would be
wrong -- and that shows here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import setup_cases as sc
import setup_reference as sr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
ALL = sc.SHAPES + [sc.SMALL]


@pytest.fixture(scope="module")
def hh(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hh") / "libhh.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread",
                           os.path.join(HERE, "host_harness.cpp"),
                           os.path.join(ROOT, "miosqp_amd", "csrc", "factor.cpp"), "-o", out])
    L = C.CDLL(out)
    L.hh_build.restype = C.c_void_p
    L.hh_build.argtypes = [C.c_int, C.c_int, ip, ip, dp, ip, ip, dp, dp, C.c_int, C.c_double, C.c_double]
    L.hh_free.argtypes = [C.c_void_p]
    L.hh_scaling.argtypes = [C.c_void_p, dp, dp, dp, dp]
    L.hh_tail.argtypes = [C.c_void_p, dp, dp, dp]
    return L


def _d(a):
    return a.ctypes.data_as(dp)


def _i(a):
    return a.ctypes.data_as(ip)


def _host(hh, shape):
    pr, P, A, _, _ = sc.instance(shape)
    n, M = A.shape[1], A.shape[0]
    keep = [np.ascontiguousarray(P.indptr, np.int32), np.ascontiguousarray(P.indices, np.int32),
            np.ascontiguousarray(P.data, np.float64), np.ascontiguousarray(A.indptr, np.int32),
            np.ascontiguousarray(A.indices, np.int32), np.ascontiguousarray(A.data, np.float64),
            np.ascontiguousarray(pr["q"], np.float64)]
    h = hh.hh_build(n, M, _i(keep[0]), _i(keep[1]), _d(keep[2]), _i(keep[3]), _i(keep[4]), _d(keep[5]), _d(keep[6]),
                    sc.PASSES, sc.RHO, sc.SIGMA)
    assert h
    try:
        D, E, qs, c = np.empty(n), np.empty(M), np.empty(n), C.c_double()
        hh.hh_scaling(h, _d(D), _d(E), C.byref(c), _d(qs))
        Linv, LinvT, d2inv = np.empty((n, n)), np.empty((n, n)), np.empty(n)
        hh.hh_tail(h, _d(Linv), _d(LinvT), _d(d2inv))
    finally:
        hh.hh_free(h)
    return D, E, c.value, Linv, LinvT, d2inv


@pytest.mark.parametrize("shape", ALL, ids=str)
def test_instances_are_sane(shape):
    """every pivot of the reference factorisation is positive at both precisions and the float64 textbook algorithm
    resolves every product to better than 1e-8: the instance, not the rule, is known to be sane"""
    ld, f64 = sc.reference(shape)
    assert ld.bad_pivot is None and f64.bad_pivot is None
    assert np.all(ld.d > 0) and np.all(f64.d > 0)
    for name in ("d2inv", "Linv", "Kinv", "Sinv"):
        floor = sr.err(getattr(f64, name), getattr(ld, name))
        print("setup-floor %-5s %s %.3e" % (name, shape, floor))
        assert floor < 1e-8, (name, floor)


@pytest.mark.parametrize("shape", ALL, ids=str)
def test_host_scaling_equals_reference(hh, shape):
    D, E, c, _, _, _ = _host(hh, shape)
    ld, f64 = sc.reference(shape)
    for ref in (ld, f64):
        np.testing.assert_allclose(D, ref.D.astype(np.float64), rtol=1e-14)
        np.testing.assert_allclose(E, ref.E.astype(np.float64), rtol=1e-14)
        assert abs(c - float(ref.c)) <= 1e-14 * float(ref.c)


@pytest.mark.parametrize("shape", ALL, ids=str)
def test_host_factor_meets_the_rule(hh, shape):
    _, _, _, Linv, LinvT, d2inv = _host(hh, shape)
    ld, f64 = sc.reference(shape)
    n = shape[0]
    sc.check("d2inv", d2inv, ld.d2inv, f64.d2inv, n)
    sc.check("Linv", Linv, ld.Linv, f64.Linv, n)
    assert np.all(np.triu(Linv) == 0.0)
    np.testing.assert_array_equal(LinvT, Linv.T)


@pytest.mark.parametrize("shape", ALL, ids=str)
def test_reference_inverses_are_inverses(shape):
    """K^-1 K = I to 1e-15 N in long double (and S^-1 S, L^-1 L, L D L^T = S likewise): the reference is right by its
    own residual, whatever it is compared with later"""
    ld, _ = sc.reference(shape)
    n, N = ld.S.shape[0], ld.K.shape[0]
    T = np.longdouble
    assert ld.K.dtype == T and ld.Kinv.dtype == T
    assert np.abs(ld.Kinv @ ld.K - np.eye(N, dtype=T)).max() <= 1e-15 * N
    assert np.abs(ld.Sinv @ ld.S - np.eye(n, dtype=T)).max() <= 1e-15 * n
    X = ld.Linv + np.eye(n, dtype=T)
    assert np.abs(X @ ld.L - np.eye(n, dtype=T)).max() <= 1e-15 * n
    assert np.abs((ld.L * ld.d[None, :]) @ ld.L.T - ld.S).max() <= 1e-15 * n * np.abs(ld.S).max()
    # the two routes to S^-1 agree: Gauss-Jordan on S, and X^T D^-1 X from the factor
    assert sr.err((X.T * ld.d2inv[None, :]) @ X, ld.Sinv) <= 1e-15 * n
    # ... and the ordering of K is the engine's: constraints first, K^-1's variable block is S^-1
    M = N - n
    assert sr.err(ld.Kinv[M:, M:], ld.Sinv) <= 1e-15 * N


def test_reference_reports_the_first_bad_pivot():
    n = 150
    for k in (0, 70, 149):
        p = np.ones(n)
        p[k] = -50.0
        for T in (np.longdouble, np.float64):
            r = sr.run(np.diag(p), np.eye(n), np.zeros(n), sc.RHO, sc.SIGMA, 0, T)
            assert r.bad_pivot == k and r.Linv is None
