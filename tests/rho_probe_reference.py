"""Plain dense restatement of the rho-once recipe (oracle/qp_oracle.c: rho_once -- RHO_ONCE_ITERS iterations of admm_step
from x = z = y = 0 on the set-up's own bounds, then rho_estimate and rho_round2), beside setup_reference.py and in its
manner: pure numpy, every operation written once with the number format `T` as an argument.  The tests run it at
np.longdouble (the reference) and at np.float64 (the rounding floor of the recipe in the format the device computes in).

It works on the scaled matrices setup_reference produces (Pbar, Abar, E, and the scaled cost), and solves the KKT system
of an iteration with the Gauss-Jordan inverse of K = [[-I / rho, Abar], [Abar^T, Pbar + sigma I]] -- the full system, as
admm_step states it, not the reduced form the kernel uses.
"""
import types

import numpy as np

import setup_reference as sr

RHO_ONCE_ITERS = 50
ALPHA = 1.6   # the engine's and the oracle's default (miosqp_qp_settings.alpha)
RHO0 = 0.1    # ... and the starting rho of rho="auto"
INFTY = 1e30


def round2(r, T):
    """rho_round2: two significant digits"""
    r = T(r)
    if not r > 0:
        return r
    e = np.floor(np.log10(r))
    p = T(10.0) ** e
    return np.floor(r / p * T(10.0) + T(0.5)) / T(10.0) * p


def rho64(r):
    """the float64 rho of an estimate r whose two digits are decided in r's own format: rho_round2's last line, m / 10 * p,
    in float64 (what the engine and the oracle return for those two digits)"""
    T = type(r)
    if not r > 0:
        return float(r)
    e = np.floor(np.log10(r))
    m = np.floor(r / T(10.0) ** e * T(10.0) + T(0.5))
    return float(np.float64(m) / np.float64(10.0) * np.float64(10.0) ** np.float64(e))


def mantissa(r, T=np.longdouble):
    """r / 10^floor(log10 r) * 10: the number whose rounding to an integer is rho_round2's decision"""
    r = T(r)
    return r / T(10.0) ** np.floor(np.log10(r)) * T(10.0)


def away_from_a_rounding_boundary(r, margin=0.01):
    """the condition under which two number formats must choose the SAME rho: the fractional part of the long-double
    mantissa lies at least `margin` away from .5 (many orders above any rounding difference between the formats)"""
    m = mantissa(r)
    return bool(abs((m - np.floor(m)) - np.longdouble(0.5)) >= margin)


def probe(Pbar, Abar, qbar, E, l, u, rho, sigma, T, alpha=ALPHA, iters=RHO_ONCE_ITERS, Kinv=None):
    """(x, z, y) after `iters` iterations of admm_step from zero, in T"""
    Pbar, Abar = np.asarray(Pbar, dtype=T), np.asarray(Abar, dtype=T)
    q = np.asarray(qbar, dtype=T)
    n, M = Pbar.shape[0], Abar.shape[0]
    E = np.asarray(E, dtype=T)
    ls = E * np.maximum(np.asarray(l, dtype=T), T(-INFTY))
    us = E * np.minimum(np.asarray(u, dtype=T), T(INFTY))
    if Kinv is None:
        Kinv = sr.gauss_jordan_inverse(sr.kkt(Pbar, Abar, rho, sigma))
    rho, sigma, alpha = T(rho), T(sigma), T(alpha)
    rho_inv = T(1.0) / rho
    x, z, y = np.zeros(n, dtype=T), np.zeros(M, dtype=T), np.zeros(M, dtype=T)
    for _ in range(iters):
        sol = Kinv @ np.concatenate([z - rho_inv * y, sigma * x - q])
        nu, xt = sol[:M], sol[M:]
        zt = z + rho_inv * (nu - y)
        x = alpha * xt + (T(1.0) - alpha) * x
        zr = alpha * zt + (T(1.0) - alpha) * z
        zn = np.minimum(np.maximum(zr + rho_inv * y, ls), us)
        y = y + rho * (zr - zn)
        z = zn
    return x, z, y


def rule(Pbar, Abar, qbar, x, z, y, rho, T):
    """(the rule's value before rounding, rho_round2 of it): rho_estimate"""
    Pbar, Abar, q = np.asarray(Pbar, dtype=T), np.asarray(Abar, dtype=T), np.asarray(qbar, dtype=T)
    ninf = lambda v: np.abs(v).max() if len(v) else T(0.0)  # noqa: E731
    Ax, Px, Aty = Abar @ x, Pbar @ x, Abar.T @ y
    pri = ninf(Ax - z) / (max(ninf(z), ninf(Ax)) + T(1e-10))
    dua = ninf(Px + q + Aty) / (max(ninf(q), ninf(Aty), ninf(Px)) + T(1e-10))
    r = T(rho) * np.sqrt(pri / (dua + T(1e-10)))
    r = min(max(r, T(1e-6)), T(1e6))
    return r, round2(r, T)


_CACHE = {}


def choose(key, P, A, q, l, u, rho=RHO0, sigma=1e-6, passes=10, alpha=ALPHA):
    """(long double, float64) runs of the recipe on one instance (P dense symmetric, A dense), computed once per `key` and
    shared, read-only: each has x, z, y, est (before rounding), rho (chosen, in the run's own format) and rho64"""
    k = (key, float(rho), float(sigma), int(passes), float(alpha))
    if k not in _CACHE:
        out = []
        for T in (np.longdouble, np.float64):
            D, E, c, Pbar, Abar, qbar = sr.scale_problem(P, A, q, passes, T)
            x, z, y = probe(Pbar, Abar, qbar, E, l, u, rho, sigma, T, alpha=alpha)
            est, chosen = rule(Pbar, Abar, qbar, x, z, y, rho, T)
            out.append(types.SimpleNamespace(x=x, z=z, y=y, est=est, rho=chosen if chosen > 0 else T(rho), rho64=rho64(est),
                                             Pbar=Pbar, Abar=Abar, qbar=qbar, E=E))
        _CACHE[k] = tuple(out)
    return _CACHE[k]
