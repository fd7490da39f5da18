"""Builds tests/setup_models_auto_body_cpu.cpp (the phases of k_setup_models_auto on the CPU, with
-fsanitize=address,undefined, run as its own executable) once per session and runs it on one problem; returns the record,
the probing iterations' last iterates, every product and the panel's values as arrays.  Beside setup_models_cpu_body.py."""
import os
import subprocess
import types

import numpy as np
import scipy.sparse as spa

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "miosqp_amd", "csrc")
_EXE = {}


def build(tmp_dir):
    key = str(tmp_dir)
    if key not in _EXE:
        exe = os.path.join(key, "setup_models_auto_body_cpu")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-pthread", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", os.path.join(HERE, "setup_models_auto_body_cpu.cpp"),
                               os.path.join(CSRC, "factor.cpp"), "-o", exe])
        _EXE[key] = exe
    return _EXE[key]


def run(exe, tmp_dir, P, q, A, l, u, rho=0.1, sigma=1e-6, alpha=1.6, passes=10, rho_auto=1, rho_again=0.0):
    P = spa.csc_matrix(P)
    A = spa.csc_matrix(A)
    P.sort_indices()
    A.sort_indices()
    n, M = A.shape[1], A.shape[0]
    src, dst = os.path.join(str(tmp_dir), "problem_auto.bin"), os.path.join(str(tmp_dir), "products_auto.bin")
    with open(src, "wb") as f:
        np.array([n, M, P.nnz, A.nnz, passes, rho_auto], dtype=np.int32).tofile(f)
        for a, t in ((P.indptr, np.int32), (P.indices, np.int32), (P.data, np.float64), (A.indptr, np.int32),
                     (A.indices, np.int32), (A.data, np.float64), (q, np.float64), (l, np.float64), (u, np.float64),
                     ([rho, sigma, alpha, rho_again], np.float64)):
            np.ascontiguousarray(a, dtype=t).tofile(f)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    v = np.fromfile(dst, dtype=np.float64)
    N = n + M
    ld, ldf, ldm, ldw = (n + 15) & ~15, (N + 15) & ~15, (M + 15) & ~15, (N + 7) & ~7
    pos = [0]

    def take(rows, cols=None):
        cnt = rows if cols is None else rows * cols
        a = v[pos[0]:pos[0] + cnt]
        pos[0] += cnt
        return a.copy() if cols is None else a.reshape(rows, cols).copy()

    o = types.SimpleNamespace(n=n, M=M)
    o.bad_pivot, o.pivot, o.guard, o.rho_est, o.rho, o.lds_doubles, o.phases, nv, nc = take(9)
    nv, nc = int(nv), int(nc)
    o.x, o.z, o.y = take(n), take(M), take(M)
    o.d2inv, o.Linv, o.LinvT, o.f_rows, o.f_GmT = take(n), take(n, ld), take(n, ld), take(n, ldf), take(M, ld)
    o.f_Ad, o.f_Atd, o.f_Pd, o.W, o.Kc, o.l, o.u = take(M, ld), take(n, ldm), take(n, ld), take(N, ldw), take(N, ldw), take(M), take(M)
    o.pv_L, o.pc_L, o.At_val, o.A_val, o.q, o.E = take(nv), take(nc), take(nv), take(nc), take(n), take(M)
    o.again_ok, o.again_bad_pivot, o.again_pivot = take(3)
    o.again_d2inv = take(n)
    assert pos[0] == len(v)
    return o
