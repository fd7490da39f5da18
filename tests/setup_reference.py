"""Plain dense restatement of the one-time set-up, for the tests of the set-up kernels.

Pure numpy: no code of the project, no scipy solves.  Every operation is written once and takes the number format `T`
as an argument; the tests run it at np.longdouble (the reference, 64-bit significand) and at np.float64 (the rounding
floor of the textbook algorithm in the format the device computes in).

    scale_problem     Ruiz equilibration and cost scaling, step for step as miosqp_amd/csrc/factor.cpp: scale_problem
    schur             S = Pbar + sigma I + rho Abar^T Abar
    ldl               textbook unblocked LDL^T (right-looking, one column per step), first non-positive pivot reported
    unit_lower_inverse  X = L^-1 by forward substitution, one row per step
    gauss_jordan_inverse  inverse by Gauss-Jordan elimination with partial pivoting (K^-1, S^-1)
    kkt               K = [[-I / rho, Abar], [Abar^T, Pbar + sigma I]], constraints first (the ordering of W)

`products(P, A, q, ...)` runs all of it once per precision and caches the result per instance.
"""
import types

import numpy as np

# the reference precision must carry at least a 64-bit significand (x87 extended); a platform whose long double is a
# plain double would make every "floor" zero and the tests meaningless: fail, do not skip
assert np.finfo(np.longdouble).eps < 2e-19, "np.longdouble is no wider than 64-bit significand here: no reference precision"

MIN_SCALING, MAX_SCALING = 1e-4, 1e4


def _clamp(v, T):
    v = np.array(v, dtype=T, copy=True)
    v[v < T(MIN_SCALING)] = T(1.0)
    v[v > T(MAX_SCALING)] = T(MAX_SCALING)
    return v


def _seq_sum(v):
    """left-to-right sum, the order of the host's loop"""
    return np.cumsum(v)[-1]


def scale_problem(P, A, q, passes, T):
    """(D, E, c, Pbar, Abar, qbar).  P: dense symmetric n x n, A: dense M x n."""
    Pb = np.array(P, dtype=T, copy=True)
    Ab = np.array(A, dtype=T, copy=True)
    qb = np.array(q, dtype=T, copy=True)
    n, M = Pb.shape[0], Ab.shape[0]
    D, E, c = np.ones(n, dtype=T), np.ones(M, dtype=T), T(1.0)
    one = T(1.0)
    for _ in range(passes):
        dt = np.abs(Pb).max(axis=0)
        et = np.zeros(M, dtype=T)
        if M:
            dt = np.maximum(dt, np.abs(Ab).max(axis=0))
            et = np.abs(Ab).max(axis=1)
        dt = one / np.sqrt(_clamp(dt, T))
        et = one / np.sqrt(_clamp(et, T))
        Pb = Pb * (dt[:, None] * dt[None, :])  # t = dt[col] * dt[row], then value * t
        Ab = Ab * (et[:, None] * dt[None, :])
        qb = qb * dt
        D = D * dt
        E = E * et
        # cost normalisation
        dt = np.abs(Pb).max(axis=0)
        mean = _seq_sum(dt) / T(n)
        nq = np.abs(qb).max()
        ct = one / _clamp([max(mean, _clamp([nq], T)[0])], T)[0]
        Pb = Pb * ct
        qb = qb * ct
        c = c * ct
    return D, E, c, Pb, Ab, qb


def schur(Pbar, Abar, rho, sigma):
    T = Pbar.dtype.type
    n = Pbar.shape[0]
    return Pbar + T(sigma) * np.eye(n, dtype=T) + T(rho) * (Abar.T @ Abar)


def ldl(S):
    """Unit-lower L (explicit ones) and d with S = L diag(d) L^T; bad = index of the first pivot that is not positive
    (None when all are; L and d are then complete)."""
    T = S.dtype.type
    W = np.array(S, copy=True)
    n = W.shape[0]
    L, d = np.eye(n, dtype=T), np.zeros(n, dtype=T)
    for j in range(n):
        dj = W[j, j]
        if not dj > 0:
            return L, d, j
        d[j] = dj
        if j + 1 < n:
            col = W[j + 1:, j] / dj
            L[j + 1:, j] = col
            W[j + 1:, j + 1:] -= np.outer(col * dj, col)
    return L, d, None


def unit_lower_inverse(L):
    T = L.dtype.type
    n = L.shape[0]
    X = np.eye(n, dtype=T)
    for i in range(1, n):
        X[i, :i] = -(L[i, :i] @ X[:i, :i])  # row i: e_i - L[i, :i] X[:i, :]; columns >= i of X[:i] are zero but for its diagonal
    return X


def gauss_jordan_inverse(K):
    T = K.dtype.type
    N = K.shape[0]
    Wk = np.concatenate([np.array(K, copy=True), np.eye(N, dtype=T)], axis=1)
    for j in range(N):
        p = j + int(np.argmax(np.abs(Wk[j:, j])))
        if p != j:
            Wk[[j, p]] = Wk[[p, j]]
        Wk[j] = Wk[j] / Wk[j, j]
        f = Wk[:, j].copy()
        f[j] = T(0.0)
        Wk -= np.outer(f, Wk[j])
    return Wk[:, N:].copy()


def kkt(Pbar, Abar, rho, sigma):
    T = Pbar.dtype.type
    n, M = Pbar.shape[0], Abar.shape[0]
    return np.block([[-np.eye(M, dtype=T) / T(rho), Abar], [Abar.T, Pbar + T(sigma) * np.eye(n, dtype=T)]])


def kc(Pbar, Abar):
    """[[0, Abar], [Abar^T, Pbar]]: the rows the termination test reads"""
    T = Pbar.dtype.type
    M = Abar.shape[0]
    return np.block([[np.zeros((M, M), dtype=T), Abar], [Abar.T, Pbar]])


def run(P, A, q, rho, sigma, passes, T, inverses=True):
    """Everything the set-up builds, at precision T."""
    D, E, c, Pbar, Abar, qbar = scale_problem(P, A, q, passes, T)
    S = schur(Pbar, Abar, rho, sigma)
    L, d, bad = ldl(S)
    r = types.SimpleNamespace(D=D, E=E, c=c, Pbar=Pbar, Abar=Abar, S=S, L=L, d=d, bad_pivot=bad, Linv=None, d2inv=None,
                              K=None, Kinv=None, Sinv=None)
    if bad is not None:
        return r
    X = unit_lower_inverse(L)
    r.Linv = X - np.eye(X.shape[0], dtype=T)  # strict lower part, as the engine stores it
    r.d2inv = T(1.0) / d
    if inverses:
        r.K = kkt(Pbar, Abar, rho, sigma)
        r.Kinv = gauss_jordan_inverse(r.K)
        r.Sinv = gauss_jordan_inverse(S)
    return r


def err(Z, Z_ld):
    """max |Z - Z_ld| / max |Z_ld|, taken in long double"""
    Z_ld = np.asarray(Z_ld, dtype=np.longdouble)
    return float(np.abs(np.asarray(Z, dtype=np.longdouble) - Z_ld).max() / np.abs(Z_ld).max())


def bound(floor, n):
    """The tolerance rule: 8 x the larger of the float64 textbook algorithm's own error and n rounding units.  Blocking,
    a fixed summation order and fused multiply-adds change the constant of the rounding error, not its order; an entry
    that is wrong (a tile corner, a padding row) is wrong by many orders more."""
    return 8.0 * max(floor, n * 2.0 ** -53)


_CACHE = {}


def products(key, P, A, q, rho=0.1, sigma=1e-6, passes=10, inverses=True):
    """(long double, float64) results for one instance, computed once per `key` and shared: callers must not write to
    them."""
    k = (key, float(rho), float(sigma), int(passes))
    got = _CACHE.get(k)
    if got is None or (inverses and got[0].Kinv is None and got[0].bad_pivot is None):
        got = tuple(run(P, A, q, rho, sigma, passes, T, inverses) for T in (np.longdouble, np.float64))
        _CACHE[k] = got
    return got
