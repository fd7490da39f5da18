"""What the batched epilogue (kb_finish, kb_heur_rows, kb_obj_rows, kb_obj_sum) owes a column, restated in plain numpy
`longdouble` from the column's own returned point: no engine, no oracle, dense matrices, every sum accumulated in long
double.  The operations are those of the reference's node and workspace (bound = .5 x'Px + q'x of the clamped point;
integer infeasibilities, most fractional position, rounded candidate and its violation of the root rows)."""
import types

import numpy as np

LD = np.longdouble


def dense_ld(M):
    return np.asarray(M.todense() if hasattr(M, "todense") else M, dtype=np.float64).astype(LD)


def _quad(P, q, x):
    """(.5 x'Px + q'x, the sum of the absolute values of its terms)"""
    t = 0.5 * (x[:, None] * P * x[None, :])
    lin = q * x
    return t.sum() + lin.sum(), np.abs(t).sum() + np.abs(lin).sum()


def column(x, q, P, A_ext, l_root, u_root, i_idx, eps_int, eps_lin):
    """x: a column's returned point (integers already clamped to the node's bounds); P, A_ext: dense long double
    (dense_ld); l_root, u_root: the bounds handed to set_root, infinities allowed.
    Returns lower, x_r, heur_obj, heur_viol, int_inf, nextvar (position in i_idx, ties to the lowest), ax_inf = ||A x_r||inf,
    the *_abs sums of absolute terms (the scale a double evaluation's rounding is relative to) and the three guards: how
    far the column is from a decision that roundings could turn."""
    x, q = np.asarray(x, dtype=np.float64).astype(LD), np.asarray(q, dtype=np.float64).astype(LD)
    l, u = np.asarray(l_root, dtype=np.float64).astype(LD), np.asarray(u_root, dtype=np.float64).astype(LD)
    ii = np.asarray(i_idx)
    eps_int, eps_lin = LD(eps_int), LD(eps_lin)
    lower, lower_abs = _quad(P, q, x)
    xi = x[ii]
    frac = np.abs(xi - np.rint(xi))
    int_inf = int(np.sum(frac > eps_int))
    nextvar = int(np.argmax(frac)) if len(frac) else -1  # argmax: the first of equal maxima
    xr = x.copy()
    xr[ii] = np.rint(xi)
    heur_obj, heur_obj_abs = _quad(P, q, xr)
    terms = A_ext * xr[None, :]
    z, z_abs = terms.sum(axis=1), np.abs(terms).sum(axis=1)
    viol = np.maximum(l - eps_lin - z, z - u - eps_lin)
    heur_viol = viol.max()
    # scale of the violation's rounding: the widest row sum, its finite bounds and the eps beside it
    fin = lambda v: np.where(np.isfinite(v), np.abs(v), LD(0))
    heur_viol_abs = (z_abs + np.maximum(fin(l), fin(u)) + eps_lin).max()
    top = np.sort(frac)[::-1]
    return types.SimpleNamespace(
        lower=lower, lower_abs=lower_abs, x_r=xr, heur_obj=heur_obj, heur_obj_abs=heur_obj_abs, heur_viol=heur_viol,
        heur_viol_abs=heur_viol_abs, ax_inf=np.abs(z).max(), int_inf=int_inf, nextvar=nextvar, frac=frac,
        guard_tie=float(top[0] - top[1]) if len(top) > 1 else np.inf,
        guard_int=float(np.min(np.abs(frac - eps_int))) if len(frac) else np.inf,
        guard_viol=float(abs(heur_viol)))
