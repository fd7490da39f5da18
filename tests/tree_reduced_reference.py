"""Plain dense restatement of the ADMM iteration (oracle/qp_oracle.c: admm_step) from a GIVEN start on GIVEN scaled data,
beside rho_probe_reference.py and in its manner: pure numpy, every operation written once with the number format `T` as
an argument.  The tests run it at np.longdouble (the reference) and at np.float64 (the rounding floor of the iteration in
the format the device computes in).  The KKT system of an iteration is solved with the Gauss-Jordan inverse of the FULL
matrix K = [[-I / rho, Abar], [Abar^T, Pbar + sigma I]], as admm_step states it -- not the reduced form the kernel uses.

Also the plumbing of tests/tree_reduced_body_cpu.cpp: the stand-alone program (built with -fsanitize=address,undefined)
that runs the phases of miosqp_amd/csrc/tree_reduced_body.hpp with a loop over the thread index."""
import os
import subprocess
import types

import numpy as np
import scipy.sparse as spa

import setup_reference as sr

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "miosqp_amd", "csrc")
ALPHA = 1.6
_EXE = {}


def admm(Pbar, Abar, q, l, u, rho, sigma, alpha, x, z, y, marks, T):
    """{k: (x, z, y)} after k iterations of admm_step for every k in `marks`, from (x, z, y), in T"""
    Pbar, Abar = np.asarray(Pbar, dtype=T), np.asarray(Abar, dtype=T)
    q, l, u = np.asarray(q, dtype=T), np.asarray(l, dtype=T), np.asarray(u, dtype=T)
    x, z, y = np.asarray(x, dtype=T), np.asarray(z, dtype=T), np.asarray(y, dtype=T)
    M = Abar.shape[0]
    Kinv = sr.gauss_jordan_inverse(sr.kkt(Pbar, Abar, rho, sigma))
    rho, sigma, alpha = T(rho), T(sigma), T(alpha)
    rho_inv = T(1.0) / rho
    out = {}
    for k in range(1, max(marks) + 1):
        sol = Kinv @ np.concatenate([z - rho_inv * y, sigma * x - q])
        nu, xt = sol[:M], sol[M:]
        zt = z + rho_inv * (nu - y)
        x = alpha * xt + (T(1.0) - alpha) * x
        zr = alpha * zt + (T(1.0) - alpha) * z
        zn = np.minimum(np.maximum(zr + rho_inv * y, l), u)
        y = y + rho * (zr - zn)
        z = zn
        if k in marks:
            out[k] = (x.copy(), z.copy(), y.copy())
    return out


def build(tmp_dir):
    key = str(tmp_dir)
    if key not in _EXE:
        exe = os.path.join(key, "tree_reduced_body_cpu")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-pthread", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", os.path.join(HERE, "tree_reduced_body_cpu.cpp"),
                               os.path.join(CSRC, "factor.cpp"), "-o", exe])
        _EXE[key] = exe
    return _EXE[key]


def run(exe, tmp_dir, P, q, A, l, u, tight, rho=0.1, sigma=1e-6, alpha=ALPHA, passes=10, warm_iters=300, leaf_cap=256,
        must_fit=True):
    """runs the program on one problem; tight: the two rows that are fixed to their lower / upper bound after the warm start"""
    P = spa.csc_matrix(P)
    A = spa.csc_matrix(A)
    P.sort_indices()
    A.sort_indices()
    n, M = A.shape[1], A.shape[0]
    src, dst = os.path.join(str(tmp_dir), "tree_problem.bin"), os.path.join(str(tmp_dir), "tree_results.bin")
    with open(src, "wb") as f:
        np.array([n, M, P.nnz, A.nnz, passes, warm_iters, tight[0], tight[1], leaf_cap, int(must_fit)], dtype=np.int32).tofile(f)
        for a, t in ((P.indptr, np.int32), (P.indices, np.int32), (P.data, np.float64), (A.indptr, np.int32),
                     (A.indices, np.int32), (A.data, np.float64), (q, np.float64), (l, np.float64), (u, np.float64),
                     ([rho, sigma, alpha], np.float64)):
            np.ascontiguousarray(a, dtype=t).tofile(f)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    v = np.fromfile(dst, dtype=np.float64)
    pos = [0]

    def take(rows, cols=None):
        cnt = rows if cols is None else rows * cols
        a = v[pos[0]:pos[0] + cnt]
        pos[0] += cnt
        return a.copy() if cols is None else a.reshape(rows, cols).copy()

    o = types.SimpleNamespace(n=n, M=M, rho=rho, sigma=sigma, alpha=alpha)
    o.lds_doubles, o.tri_ld, ldn, ldm = [int(t) for t in take(4)]
    o.Abar, o.Pbar = take(M, ldn)[:, :n], take(n, ldn)[:, :n]
    o.q, o.l, o.u, o.x0, o.z0, o.y0 = take(n), take(M), take(M), take(n), take(M), take(M)
    o.runs = {}
    for name in ("packed", "dense", "product"):
        o.runs[name] = {k: (take(n), take(M), take(M)) for k in (25, 100)}
    assert pos[0] == len(v)
    return o
