"""setup_models(large="device") on the CPU: the ARITHMETIC of k_setup_models_large -- setup_models_large_body.hpp is
written as phases between barriers, and tests/setup_models_large_body_cpu.cpp runs those phases with a loop over the
thread index, built with -fsanitize=address,undefined and run as a child process -- against the long-double reference under
the rule of setup_cases.check; the host logic of the entry with mixed forms (setup_plan.hpp) in a second sanitized
stand-alone program; the keyword's handling on the oracle backend; the declared symbols.  Nothing here touches a GPU."""
import os
import subprocess
import types

import numpy as np
import pytest
import scipy.sparse as spa

import miosqp_amd
import setup_cases as sc
import setup_models_cpu_body as cb
import setup_reference as sr
from miosqp_amd import problems
from oracle import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "miosqp_amd", "csrc")
FLAGS = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-pthread", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all"]  # (the line of setup_models_cpu_body.build)
# (n, m, p) of random_miqp: n + M = 193, the first the launch takes; small n, wide M; the LDS maximum in n; M > 512; two
# shapes of the reference benchmark's grid
SHAPES = [(100, 90, 3), (20, 170, 4), (198, 2, 1), (20, 530, 4), (50, 200, 10), (150, 300, 20)]


@pytest.fixture(scope="module")
def body(tmp_path_factory):
    d = tmp_path_factory.mktemp("setup_models_large_body")
    exe = os.path.join(str(d), "setup_models_large_body_cpu")
    subprocess.check_call(FLAGS + [os.path.join(HERE, "setup_models_large_body_cpu.cpp"), os.path.join(CSRC, "factor.cpp"),
                                   "-o", exe])
    return exe, d


def run(exe, tmp_dir, P, q, A, l, u, rho=0.1, sigma=1e-6, passes=10):
    P = spa.csc_matrix(P)
    A = spa.csc_matrix(A)
    P.sort_indices()
    A.sort_indices()
    n, M = A.shape[1], A.shape[0]
    src, dst = os.path.join(str(tmp_dir), "problem.bin"), os.path.join(str(tmp_dir), "products.bin")
    with open(src, "wb") as f:
        np.array([n, M, P.nnz, A.nnz, passes], dtype=np.int32).tofile(f)
        for a, t in ((P.indptr, np.int32), (P.indices, np.int32), (P.data, np.float64), (A.indptr, np.int32),
                     (A.indices, np.int32), (A.data, np.float64), (q, np.float64), (l, np.float64), (u, np.float64),
                     ([rho, sigma], np.float64)):
            np.ascontiguousarray(a, dtype=t).tofile(f)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    v = np.fromfile(dst, dtype=np.float64)
    N = n + M
    ld, ldf, ldm = (n + 15) & ~15, (N + 15) & ~15, (M + 15) & ~15
    pos = [0]

    def take(rows, cols=None):
        cnt = rows if cols is None else rows * cols
        a = v[pos[0]:pos[0] + cnt]
        pos[0] += cnt
        return a.copy() if cols is None else a.reshape(rows, cols).copy()

    o = types.SimpleNamespace(n=n, M=M)
    o.bad_pivot, o.pivot, o.guard, o.lds_doubles = take(4)
    o.S, o.d2inv, o.Linv, o.LinvT, o.f_rows, o.f_GmT = take(n, ld), take(n), take(n, ld), take(n, ld), take(n, ldf), take(M, ld)
    o.f_Ad, o.f_Atd, o.f_Pd, o.l, o.u = take(M, ld), take(n, ldm), take(n, ld), take(M), take(M)
    o.host_ok = bool(take(1)[0])
    o.h_S = take(n, ld)
    if o.host_ok:
        o.h_d2inv, o.h_Linv, o.h_rows, o.h_GmT = take(n), take(n, ld), take(n, ldf), take(M, ld)
        o.h_Ad, o.h_Atd, o.h_Pd, o.D, o.E = take(M, ld), take(n, ldm), take(n, ld), take(n), take(M)
    assert pos[0] == len(v)
    return o


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_kernel_arithmetic_against_the_long_double_reference(body, shape):
    """d2inv, Linv and f_rows under the rule of the set-up kernels' tests (8 x max(float64 floor, n 2^-53)); LinvT the exact
    transpose; padding exactly zero; S, the dense copies and the scaled bounds bit for bit what the per-model host set-up
    makes; the LDS the phases use is what the size rule counts (the sanitizer watches its end)"""
    exe, d = body
    pr, P, A, l, u = sc.instance(shape)
    n, M = shape[0], A.shape[0]
    N = n + M
    assert N > 192 and not miosqp_amd_small_rule(n, M)
    o = run(exe, d, P, pr["q"], A, l, u, rho=sc.RHO, sigma=sc.SIGMA, passes=sc.PASSES)
    ld, f64 = sc.reference(shape, inverses=False)
    assert o.bad_pivot == 0 and o.pivot == -1 and o.host_ok
    assert o.lds_doubles == n * (n + 1) // 2 + 3 * n + 8 and o.lds_doubles * 8 <= 160 * 1024
    low = np.tril(np.ones((n, n), dtype=bool))
    np.testing.assert_array_equal(o.S[:, :n][low], o.h_S[:, :n][low], err_msg="S")
    assert np.all(o.S[:, :n][~low] == 0.0)
    sc.check("d2inv", o.d2inv, ld.d2inv, f64.d2inv, n)
    sc.check("Linv", o.Linv[:, :n], ld.Linv, f64.Linv, n)
    assert np.all(np.triu(o.Linv[:, :n]) == 0.0)
    np.testing.assert_array_equal(o.LinvT[:, :n], o.Linv[:, :n].T)
    assert np.all(o.Linv[:, n:] == 0.0) and np.all(o.LinvT[:, n:] == 0.0)
    F_ld, F_64 = cb.product_form_reference(ld, sc.RHO), cb.product_form_reference(f64, sc.RHO)
    sc.check("f_rows", o.f_rows[:, :N], F_ld, F_64, n)
    assert np.all(o.f_rows[:, N:] == 0.0)
    np.testing.assert_array_equal(o.f_rows[:, M:M + n], o.Linv[:, :n])
    np.testing.assert_array_equal(o.f_GmT[:, :n], o.f_rows[:, :M].T)
    assert np.all(o.f_GmT[:, n:] == 0.0)
    for name in ("Ad", "Atd", "Pd"):
        np.testing.assert_array_equal(getattr(o, "f_" + name), getattr(o, "h_" + name), err_msg=name)
    np.testing.assert_array_equal(o.l, o.E * np.maximum(l, -1e30))
    np.testing.assert_array_equal(o.u, o.E * np.minimum(u, 1e30))


def miosqp_amd_small_rule(n, M):
    """setup_models_body.hpp's eligible_shape, restated: the dense copy of Abar beside the triangle within 160 KB"""
    t, g = n * (n + 1) // 2, 3 * (n + M) + 256 * 3 + (n + M) + 8
    return n + M <= 192 and (max(t, g) + M * (n | 1) + 3 * n + 8) * 8 <= 160 * 1024


def test_kernel_arithmetic_reports_the_hosts_bad_pivot(body):
    exe, d = body
    n = 120
    A = spa.vstack([spa.identity(n), spa.identity(n, format="csr")[:80]], format="csc")  # n + M = 320
    for k in (0, 57, 119):
        p = np.ones(n)
        p[k] = -50.0
        o = run(exe, d, spa.diags(p).tocsc(), np.zeros(n), A, -np.ones(200), np.ones(200), passes=0)
        assert o.bad_pivot == 1 and o.pivot == k and not o.host_ok
        low = np.tril(np.ones((n, n), dtype=bool))
        np.testing.assert_array_equal(o.S[:, :n][low], o.h_S[:, :n][low])
        assert sr.run(np.diag(p), A.toarray(), np.zeros(n), sc.RHO, sc.SIGMA, 0, np.longdouble, inverses=False).bad_pivot == k


def test_sanitized_plan_and_argument_checks_with_mixed_forms(tmp_path):
    exe = str(tmp_path / "setup_plan_large_fuzz")
    subprocess.check_call(FLAGS + [os.path.join(HERE, "setup_plan_large_fuzz.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "setup_plan_large ok" in r.stdout


def test_the_keyword_on_a_backend_without_the_entry():
    """the oracle backend has no one-launch set-up: every model is set up in place, whatever the keyword says; any other
    value of the keyword raises"""
    prs = [problems.random_miqp(10, 5, 2, seed=0), problems.random_miqp(40, 160, 4, seed=1)]
    st, qs = dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS)
    info = {}
    got = miosqp_amd.setup_models(prs, st, qs, info=info, backend=oracle, large="device")
    assert info["batched"] == [] and sorted(info["own"]) == [0, 1] and info["launches"] == 0
    assert info["forms"] == dict(small=0, large=0)
    assert all("backend" in why for why in info["own"].values())
    ref = miosqp_amd.setup_models(prs, st, qs, backend=oracle)
    for a, b in zip(got, ref):
        ra, rb = a.solve(), b.solve()
        assert ra.status == rb.status and ra.upper_glob == rb.upper_glob
        np.testing.assert_array_equal(ra.x, rb.x)
    for bad in (True, "host", 1, "Device"):
        with pytest.raises(ValueError, match="large must be None or"):
            miosqp_amd.setup_models(prs, st, qs, backend=oracle, large=bad)


def test_the_symbols_are_declared():
    from miosqp_amd import _lib, qp
    for name in ("miosqp_qp_setup_models_large", "miosqp_qp_setup_models_eligible_large", "miosqp_qp_setup_models_shape"):
        assert name in _lib.SYMBOLS
    assert callable(qp.setup_models_eligible_large) and callable(qp.setup_models_shape)
    assert "int miosqp_qp_setup_models_shape(int32_t n, int32_t M);" in open(
        os.path.join(os.path.dirname(HERE), "include", "miosqp_amd.h")).read()
    header = open(os.path.join(os.path.dirname(HERE), "include", "miosqp_amd.h")).read()
    assert "int miosqp_qp_setup_models_large(int32_t B," in header
    assert "int miosqp_qp_setup_models_eligible_large(int32_t n, int32_t M," in header
