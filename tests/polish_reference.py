"""Plain dense restatement of the polish with its repair loop, in a chosen number format, for the tests of k_pol_many.

Pure numpy: no code of the project and no numpy linalg (which is float64 only).  `polish(..., T)` is
`bnb.polish_restatement(..., repair_iter=k)` written once and parametrised by the format `T`: the tests run it at
np.longdouble (the reference, 64-bit significand) and at np.float64 (the rounding floor of the textbook algorithm in the
format the device computes in), and judge the device against the floor.

    classification   OSQP's rule plus "an equality row is always active"; a bound at or beyond 1e30 is never active
    S                P + delta I + A_act' A_act / delta, factorised by setup_reference.ldl (textbook unblocked LDL^T; its
                     first non-positive pivot is the kernel's `!(d > 0)` rule)
    ksolve           dx = S^-1 (r1 + A_act' r2 / delta) by forward substitution, the pivots, back substitution;
                     dy = (A_act dx - r2) / delta
    revision         tol 1e-10; stops 0 (fixed point), 1 (round limit), 2 (bad pivot in a repair round: the round before
                     is kept and judged)
    judging          pri_after <= max(pri_before, 1e-10), then dua_after <= max(dua_before, 1e-10), over all rows

`both(key, ...)` runs it once per format and caches the pair per key.
"""
import types

import numpy as np

import setup_reference as sr

# the reference precision must carry at least a 64-bit significand (x87 extended); a platform whose long double is a
# plain double would make every "floor" zero and the tests meaningless: fail, do not skip
assert np.finfo(np.longdouble).eps < 2e-19, "np.longdouble is no wider than 64-bit significand here: no reference precision"

INFTY = 1e30  # a bound at or beyond it is infinite
TOL = 1e-10   # the revision's tolerance and the floor of the acceptance test
COUNTS = ("rounds", "stop", "n_added", "n_dropped", "accepted0", "reason0", "accepted", "reason", "n_lower", "n_upper")


def _dense(a, T):
    return np.array(a.todense() if hasattr(a, "todense") else a, dtype=T)


def forward(L, r):
    """L w = r, L unit lower: one row per step"""
    w = np.array(r, copy=True)
    for i in range(1, len(w)):
        w[i] = w[i] - L[i, :i] @ w[:i]
    return w


def backward(L, w):
    """L' v = w, L unit lower: one row per step, from the last"""
    v = np.array(w, copy=True)
    for i in range(len(v) - 2, -1, -1):
        v[i] = v[i] - L[i + 1:, i] @ v[i + 1:]
    return v


def polish(P, q, A, l, u, x, y, delta=1e-6, refine_iter=3, repair_iter=0, T=np.longdouble):
    """The record of bnb.polish_restatement(P, q, A, l, u, x, y, delta, refine_iter, repair_iter=repair_iter), every
    operation in the format T.  Besides the record: active, margin, xh, yh as there (xh, yh None after reason 1)."""
    P, A = _dense(P, T), _dense(A, T)
    q, l, u, x, y = (np.array(a, dtype=T) for a in (q, l, u, x, y))
    M, n = A.shape
    delta, tol, inf, zero = T(delta), T(TOL), T(INFTY), T(0.0)
    z = A @ x
    active, margin, b = np.zeros(M, dtype=np.int64), np.full(M, np.inf), np.zeros(M, dtype=T)
    for j in range(M):
        lo_fin, up_fin = l[j] > -inf, u[j] < inf
        if lo_fin and l[j] == u[j]:
            active[j], b[j] = -1, l[j]
            continue
        if lo_fin:
            margin[j] = abs((z[j] - l[j]) + y[j])
            if z[j] - l[j] < -y[j]:
                active[j], b[j] = -1, l[j]
                continue
        if up_fin:
            margin[j] = min(margin[j], abs((u[j] - z[j]) - y[j]))
            if u[j] - z[j] < y[j]:
                active[j], b[j] = 1, u[j]

    def residuals(xv, yv):
        zv = A @ xv
        pri = max(np.max(l - zv), np.max(zv - u), zero) if M else zero
        return pri, np.max(np.abs(P @ xv + q + A.T @ yv))

    def solve_on(active, b):
        rows = np.where(active != 0)[0]
        Aa, ba = A[rows], b[rows]
        S = P + delta * np.eye(n, dtype=T) + (Aa.T @ Aa) / delta
        L, d, bad = sr.ldl(S)
        if bad is not None:
            return None

        def ksolve(r1, r2):
            dx = backward(L, forward(L, r1 + (Aa.T @ r2) / delta) / d)
            return dx, (Aa @ dx - r2) / delta

        xh, ya = ksolve(-q, ba)
        for _ in range(refine_iter):
            dx, dy = ksolve(-q - P @ xh - Aa.T @ ya, ba - Aa @ xh)
            xh, ya = xh + dx, ya + dy
        yh = np.zeros(M, dtype=T)
        yh[rows] = ya
        return xh, yh

    def revise(active, b, xh, yh):
        zh = A @ xh
        act, bb, added, dropped = active.copy(), b.copy(), 0, 0
        for j in range(M):
            if l[j] == u[j]:
                continue
            if active[j] < 0:
                margin[j] = min(margin[j], abs(yh[j] - tol))
                if yh[j] > tol:
                    act[j], bb[j], dropped = 0, zero, dropped + 1
            elif active[j] > 0:
                margin[j] = min(margin[j], abs(-yh[j] - tol))
                if yh[j] < -tol:
                    act[j], bb[j], dropped = 0, zero, dropped + 1
            else:
                if l[j] > -inf:
                    margin[j] = min(margin[j], abs((l[j] - zh[j]) - tol))
                    if l[j] - zh[j] > tol:
                        act[j], bb[j], added = -1, l[j], added + 1
                        continue
                if u[j] < inf:
                    margin[j] = min(margin[j], abs((zh[j] - u[j]) - tol))
                    if zh[j] - u[j] > tol:
                        act[j], bb[j], added = 1, u[j], added + 1
        return act, bb, added, dropped

    def judge(xh, yh):
        pri1, dua1 = residuals(xh, yh)
        if not pri1 <= max(pri0, tol):
            return 2, pri1, dua1
        if not dua1 <= max(dua0, tol):
            return 3, pri1, dua1
        return 0, pri1, dua1

    pri0, dua0 = residuals(x, y)
    nan = T(np.nan)
    out = types.SimpleNamespace(accepted=False, reason=1, n_lower=int(np.sum(active < 0)), n_upper=int(np.sum(active > 0)),
                                pri_before=pri0, dua_before=dua0, pri_after=nan, dua_after=nan, obj=nan,
                                x=x.copy(), y=y.copy(), active=active, margin=margin, xh=None, yh=None,
                                rounds=0, stop=0, n_added=0, n_dropped=0, accepted0=False, reason0=1)
    point = solve_on(active, b)
    if point is None:
        return out
    xh, yh = point
    out.reason0 = judge(xh, yh)[0]
    out.accepted0 = out.reason0 == 0
    k = 0
    while True:
        act, bb, added, dropped = revise(active, b, xh, yh)
        out.n_added, out.n_dropped = out.n_added + added, out.n_dropped + dropped
        if added + dropped == 0:
            out.stop = 0
            break
        if k == repair_iter:
            out.stop = 1
            break
        k += 1
        out.rounds = k
        point = solve_on(act, bb)
        if point is None:
            out.stop = 2
            break
        (xh, yh), active, b = point, act, bb
    out.active, out.n_lower, out.n_upper = active, int(np.sum(active < 0)), int(np.sum(active > 0))
    out.reason, out.pri_after, out.dua_after = judge(xh, yh)
    out.xh, out.yh = xh, yh
    out.obj = T(0.5) * (xh @ (P @ xh)) + q @ xh
    if out.reason == 0:
        out.accepted, out.x, out.y = True, xh.copy(), yh.copy()
    return out


def err(v, v_ld):
    """max |v - v_ld|, taken in long double"""
    v_ld = np.asarray(v_ld, dtype=np.longdouble)
    return float(np.max(np.abs(np.asarray(v, dtype=np.longdouble) - v_ld))) if v_ld.size else 0.0


def bound(floor, v_ld):
    """The tolerance rule: 16 x the float64 restatement's own error, or 64 rounding units of the largest entry where
    that error is smaller still.  The kernel and the float64 restatement are the same algorithm in the same format and
    differ in the order of their sums and in fused multiply-adds: that moves the constant of the rounding error, not its
    order; a wrong index in a substitution misses by many orders."""
    v_ld = np.asarray(v_ld, dtype=np.longdouble)
    top = float(np.max(np.abs(v_ld))) if v_ld.size else 0.0
    return max(16.0 * floor, 64.0 * 2.0 ** -52 * max(1.0, top))


def x_floor(r64, rld):
    """e_floor of the tie rule: max |x_float64 - x_longdouble| of the polished point"""
    if rld.xh is None or r64.xh is None:
        return 0.0
    return err(r64.xh, rld.xh)


def tie_free(rld, r64, A, l, u):
    """(ok, worst row, its margin, its threshold): every row's margin is at least
    max(1e-9 max(1, |bound|), 100 x the row's 1-norm of A x e_floor)"""
    A = _dense(A, np.float64)
    bnd = np.where(rld.active < 0, l, u).astype(float)
    bnd = np.where(np.abs(bnd) < INFTY, bnd, 0.0)
    need = np.maximum(1e-9 * np.maximum(1.0, np.abs(bnd)), 100.0 * np.abs(A).sum(axis=1) * x_floor(r64, rld))
    gap = np.asarray(rld.margin, dtype=float) - need
    j = int(np.argmin(gap)) if len(gap) else -1
    return bool(np.all(gap >= 0.0)), j, (float(rld.margin[j]) if j >= 0 else np.inf), (float(need[j]) if j >= 0 else 0.0)


_CACHE = {}


def both(key, P, q, A, l, u, x, y, delta=1e-6, refine_iter=3, repair_iter=0):
    """(long double, float64) records of one instance, computed once per (key, settings) and shared: callers must not
    write to them."""
    k = (key, float(delta), int(refine_iter), int(repair_iter))
    got = _CACHE.get(k)
    if got is None:
        got = tuple(polish(P, q, A, l, u, x, y, delta, refine_iter, repair_iter, T) for T in (np.longdouble, np.float64))
        _CACHE[k] = got
    return got
