"""Host-side branch-and-bound control: the caller of the hot path.

This module is the host counterpart of the reference's Python tree search, kept on the CPU
("stays on the host unchanged" in BASELINE.json's north_star).  It reproduces the observable
behaviour of the reference classes so that, given identical relaxation results, the tree is
explored in the same order and the same statistics come out (SURVEY.md sec. 3.4 lists the
quirks that matter; tests/test_bnb_trace.py replays traces recorded from the reference):

  MIOSQP      /root/reference/miosqp/solver.py:32-212
  Workspace   /root/reference/miosqp/workspace.py:18-433
  Node        /root/reference/miosqp/node.py:5-147
  Data        /root/reference/miosqp/data.py:36-126, add_bounds data.py:5-33
  Results     /root/reference/miosqp/results.py:1-12
  MI_*        /root/reference/miosqp/constants.py:1-7

The only thing replaced is what `Node.solve` calls: the relaxation solver is the HIP engine
behind the C ABI (miosqp_amd.qp), reached either through the reference's own four-call
sequence update -> warm_start -> solve (node.py:102-108) or through the fused per-node entry
`solve_node`, which also performs the integer clamp (node.py:131-136) and the objective
evaluation (node.py:143 -> data.py:99-103) on the device.

A different solver module can be passed explicitly as `backend=` (tests pass the CPU oracle);
there is no automatic fallback: without an explicit backend the HIP library must load.
"""
from __future__ import print_function

from time import time

import inspect
import types

import numpy as np
import scipy.sparse as spa

# status strings, verbatim (constants.py:2 really says 'Unolved')
MI_UNSOLVED = 'Unolved'
MI_SOLVED = 'Solved'
MI_PRIMAL_INFEASIBLE = 'Primal Infeasible'
MI_DUAL_INFEASIBLE = 'Dual Infeasible'
MI_MAX_ITER_FEASIBLE = 'Max-iter feasible'
MI_MAX_ITER_UNSOLVED = 'Max-iter unsolved'


def _default_backend():
    from miosqp_amd import qp  # raises if the HIP library cannot be loaded
    return qp


def branching_settings(settings, qp_settings):
    """The branching rule and its strong-branching parameters, checked (MIOSQP.setup calls this before anything is
    built).  Rule 0: most fractional (the reference's only rule); 1: strong branching; 2: reliability branching."""
    rule = settings.get('branching_rule', 0)
    if rule not in (0, 1, 2):
        raise ValueError('No variable selection rule recognized!')
    K = settings.get('sb_candidates', 8)
    if int(K) != K or not 1 <= K <= 32:
        raise ValueError('sb_candidates must be in 1..32')
    check = (qp_settings or {}).get('check_termination', (qp_settings or {}).get('early_terminate_interval', 25))
    cap = settings.get('sb_max_iter', 50)
    if rule != 0 or 'sb_max_iter' in settings:
        if int(cap) != cap or cap <= 0 or check <= 0 or cap % check != 0:
            raise ValueError('sb_max_iter must be a positive multiple of check_termination (%r)' % check)
    rel = settings.get('sb_reliability', 4)
    if int(rel) != rel or rel < 0:
        raise ValueError('sb_reliability must be a non-negative integer')
    eps = float(settings.get('sb_eps', 1e-6))
    if not eps > 0:
        raise ValueError('sb_eps must be positive')
    return dict(rule=rule, K=int(K), max_iter=int(cap), reliability=int(rel), eps=eps)


def heuristic_settings(settings, qp_settings):
    """The primal heuristic and its parameters, checked (MIOSQP.setup calls this before anything is built).
    primal_heuristic 0: the reference's rounding only; 1: round and fix (Workspace.round_and_fix)."""
    qs = qp_settings or {}
    on = settings.get('primal_heuristic', 0)
    if on not in (0, 1):
        raise ValueError('No primal heuristic recognized!')
    K = settings.get('rf_candidates', 7)
    if int(K) != K or not 1 <= K <= 32:
        raise ValueError('rf_candidates must be in 1..32')
    check = qs.get('check_termination', qs.get('early_terminate_interval', 25))
    qp_cap = qs.get('max_iter', 4000)
    if 'rf_max_iter' in settings:
        cap = settings['rf_max_iter']
        if int(cap) != cap or cap <= 0 or (cap != qp_cap and (check <= 0 or cap % check != 0)):
            raise ValueError("rf_max_iter must be a positive multiple of check_termination (%r) or the QP's max_iter"
                             % check)
    else:
        # the QP's own cap, rounded down to whole termination checks (a cap below one check stays as it is)
        cap = qp_cap if check <= 0 or qp_cap % check == 0 or qp_cap < check else qp_cap - qp_cap % check
    every = settings.get('rf_every', 10)
    if int(every) != every or every < 1:
        raise ValueError('rf_every must be at least 1')
    return dict(on=int(on), K=int(K), max_iter=int(cap), every=int(every))


def polish_settings(settings):
    """Polishing of the incumbent and its parameters, checked (MIOSQP.setup calls this before anything is built).
    polish_incumbent 0: the incumbent as the search found it; 1: re-solved with its integers fixed and polished
    (Workspace.polish_incumbent).  polish_repair_iter is checked here with its neighbours and read by
    polish_repair_setting: this record keeps its three keys."""
    polish_repair_setting(settings)
    on = settings.get('polish_incumbent', 0)
    if on not in (0, 1):
        raise ValueError('polish_incumbent must be 0 or 1')
    delta = settings.get('polish_delta', 1e-6)
    if isinstance(delta, bool) or not isinstance(delta, (int, float, np.integer, np.floating)) \
            or not (delta > 0 and np.isfinite(delta)):
        raise ValueError('polish_delta must be a positive number')
    it = settings.get('polish_refine_iter', 3)
    if isinstance(it, bool) or not isinstance(it, (int, float, np.integer, np.floating)) or int(it) != it \
            or not 0 <= it <= 10:
        raise ValueError('polish_refine_iter must be an integer in 0..10')
    return dict(on=int(on), delta=float(delta), refine_iter=int(it))


def polish_repair_setting(settings):
    """polish_repair_iter, checked: the most repair rounds of the polish's active set (0, the default: the set guessed
    once, as OSQP polishes; up to 20)."""
    it = settings.get('polish_repair_iter', 0)
    if isinstance(it, bool) or not isinstance(it, (int, float, np.integer, np.floating)) or not 0 <= it <= 20 \
            or int(it) != it:
        raise ValueError('polish_repair_iter must be an integer in 0..20')
    return int(it)


def one_launch_trees_ok(work, rf=False, sb=False):
    """would `solve_many` (and `solve_models`) try the one-launch trees for this workspace: the entry point is there, the
    settings are the plain search's, and the engine has not declined before.  rf=True (heuristic="device"): the same
    question with primal_heuristic 1 allowed, for the entry that runs round and fix inside the launch.  sb=True
    (branching="device"): the same question with branching_rule 1 and 2 allowed -- without the heuristic --, for the entry
    that runs strong / reliability branching inside the launch"""
    st, data = work.settings, work.data
    rule_ok = st['branching_rule'] == 0 or (sb and st['branching_rule'] in (1, 2) and not work.rf['on']
                                            and hasattr(work.solver, 'solve_trees_sb'))
    return hasattr(work.solver, 'solve_trees') and st.get('device_tree', True) and rule_ok \
        and (not work.rf['on'] or (rf and hasattr(work.solver, 'solve_trees_rf'))) \
        and st['tree_explor_rule'] in (0, 1, 2, 3) and data.n_int > 0 and 'eps_abs' in work.qp_settings \
        and st.get('device_digest', True) and not getattr(work, '_no_trees', False)


def exploration_setting(settings):
    """The exploration rule, checked (MIOSQP.setup calls this before anything is built).  0: depth first; 1: the
    reference's default (depth first, then the largest bound); 2: best bound; 3: depth first until the first incumbent,
    then best bound (Workspace.leaf_index)."""
    rule = settings.get('tree_explor_rule', 1)
    if rule not in (0, 1, 2, 3):
        raise ValueError('Tree exploring strategy not recognized')
    return rule


def require_depth_first(settings, who):
    """The leaf-pool streams and the sharded searches visit a wide frontier per round and keep the exploration rules 0
    and 1: `who` (the search's name in the message) refuses the best-bound rules before anything is launched."""
    rule = settings.get('tree_explor_rule', 1)
    if rule in (2, 3):
        raise ValueError("%s: tree_explor_rule 0 / 1 only (rule %d, best bound, runs in MIOSQP.solve and solve_many)"
                         % (who, rule))


def require_plain_search(settings, who, rule=True, heuristic=True, polish=True):
    """The searches beside MIOSQP.solve branch on the most fractional variable, run no primal heuristic and do not
    polish their incumbent: `who` (the search's name in the message) refuses the settings that ask for more."""
    if polish and settings.get('polish_incumbent', 0) != 0:
        raise ValueError("%s: polish_incumbent 0 only (the incumbent is polished by MIOSQP.solve)" % who)
    if rule and settings.get('branching_rule', 0) != 0:
        raise ValueError("%s: branching_rule 0 only (strong / reliability branching run in MIOSQP.solve)" % who)
    if heuristic and settings.get('primal_heuristic', 0) != 0:
        raise ValueError("%s: primal_heuristic 0 only (round and fix runs in MIOSQP.solve)" % who)


def rf_roundings(xi, lo, hi, K):
    """The K rounding vectors of round and fix for the integer entries xi inside the node's bounds lo, hi:
    row k is min(max(floor(xi + theta_k), lo), hi) with theta_k = (k + 1) / (K + 1) as one double division."""
    out = np.empty((K, len(xi)))
    for k in range(K):
        theta = float(k + 1) / float(K + 1)
        out[k] = np.minimum(np.maximum(np.floor(xi + theta), lo), hi)
    return out


def sb_scores(lower, status, parent_lower, eps, ok):
    """Scores of K strong-branching candidates from their 2K children (K down, then K up): the gain of a child is
    max(L - L_parent, 0), 1e30 without a lower value (status not in `ok`); score = max(gain_d, eps) * max(gain_u, eps).
    Returns (gains [2K], scores [K], argmax with ties to the lowest candidate)."""
    K = len(lower) // 2
    gain = np.empty(2 * K)
    for b in range(2 * K):
        g = lower[b] - parent_lower if status[b] in ok else 1e30
        gain[b] = g if g > 0.0 else 0.0
    score = np.empty(K)
    for k in range(K):
        gd, gu = gain[k], gain[K + k]
        score[k] = (gd if gd > eps else eps) * (gu if gu > eps else eps)
    return gain, score, int(np.argmax(score))


POLISH_INFTY = 1e30  # a bound at or beyond it is infinite (the engine's constant)


def polish_restatement(P, q, A, l, u, x, y, delta=1e-6, refine_iter=3, repair_iter=None):
    """Polishing of one node's solution in dense numpy: what `OSQP.polish` of the HIP engine computes on the device
    (include/miosqp_amd.h: miosqp_qp_polish, miosqp_qp_polish_repair), used where the backend has none.  A, l, u: all M
    rows; everything unscaled.

    1. z = A x; row j is lower-active when l_j == u_j or z_j - l_j < -y_j, otherwise upper-active when u_j - z_j < y_j;
       an infinite bound is never active.
    2. S = P + delta I + A_act' A_act / delta (Cholesky); ksolve(r1, r2): dx = S^-1 (r1 + A_act' r2 / delta),
       dy = (A_act dx - r2) / delta.
    3. (xh, yh) = ksolve(-q, b), then refine_iter times += ksolve of the unregularised system's residuals.
    4. accepted when S was positive definite, pri_after <= max(pri_before, 1e-10), dua_after <= max(dua_before, 1e-10)
       (pri, dua over all rows); otherwise x, y are the input and reason says why (1 factorisation, 2 primal, 3 dual).

    repair_iter None: exactly the above.  An integer 0..20 adds the repair loop (OSQP has none): steps 1-3 are round 0;
    after the solves of round k every row is revised from (xh, yh), z = A xh, tol = 1e-10 -- an equality row stays; a
    lower-active row with yh > tol and an upper-active row with yh < -tol become inactive; an inactive row with finite
    l and l - z > tol becomes lower-active, otherwise with finite u and z - u > tol upper-active.  No change: stop 0 (a
    fixed point).  A change at k == repair_iter: stop 1.  Otherwise round k + 1 repeats steps 2-3 on the revised set
    from xh = yh = 0; a factorisation that fails there ends the loop with stop 2 and round k's point and set.  Step 4
    judges the point the loop ended with (reason 1 only for round 0's factorisation).  The record gains rounds (repair
    rounds run), stop, n_added, n_dropped (summed over the revisions), accepted0, reason0 (step 4 on round 0's point);
    n_lower, n_upper, active, xh, yh are those of the final set and point.

    Besides the record: active (per row -1 lower, 1 upper, 0 inactive), margin (per row the smallest distance from
    equality of the comparisons that classified it, the revisions' |quantity - tol| included; inf for equality rows
    and rows without a finite bound: an input with a tiny margin sits on a tie and another summation order may
    classify it differently), xh, yh (the polished point whether accepted or not; None after reason 1)."""
    P = np.asarray(P.todense()) if spa.issparse(P) else np.asarray(P, dtype=float)
    A = np.asarray(A.todense()) if spa.issparse(A) else np.asarray(A, dtype=float)
    q, l, u = np.asarray(q, dtype=float), np.asarray(l, dtype=float), np.asarray(u, dtype=float)
    x, y = np.asarray(x, dtype=float), np.asarray(y, dtype=float)
    M, n = A.shape
    if repair_iter is not None and (isinstance(repair_iter, bool) or int(repair_iter) != repair_iter
                                    or not 0 <= repair_iter <= 20):
        raise ValueError('repair_iter must be an integer in 0..20')
    z = A.dot(x)
    active, margin, b = np.zeros(M, dtype=np.int64), np.full(M, np.inf), np.zeros(M)
    for j in range(M):
        lo_fin, up_fin, eq = l[j] > -POLISH_INFTY, u[j] < POLISH_INFTY, l[j] == u[j]
        if lo_fin and eq:
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
        zv = A.dot(xv)
        pri = max(np.max(l - zv), np.max(zv - u), 0.0) if M else 0.0
        return float(pri), float(np.max(np.abs(P.dot(xv) + q + A.T.dot(yv)))) if n else 0.0

    def solve_on(active, b):
        """steps 2 and 3 on one set: (xh, yh), or None when S is not positive definite"""
        rows = np.where(active != 0)[0]
        Aa, ba = A[rows], b[rows]
        S = P + delta * np.eye(n) + Aa.T.dot(Aa) / delta
        try:
            L = np.linalg.cholesky(S)
        except np.linalg.LinAlgError:
            return None

        def ksolve(r1, r2):
            dx = np.linalg.solve(L.T, np.linalg.solve(L, r1 + Aa.T.dot(r2) / delta))
            return dx, (Aa.dot(dx) - r2) / delta

        xh, ya = ksolve(-q, ba)
        for _ in range(refine_iter):
            dx, dy = ksolve(-q - P.dot(xh) - Aa.T.dot(ya), ba - Aa.dot(xh))
            xh, ya = xh + dx, ya + dy
        yh = np.zeros(M)
        yh[rows] = ya
        return xh, yh

    def revise(active, b, xh, yh):
        """the revised set from (xh, yh): (active, b, added, dropped); margin takes the comparisons made"""
        tol = 1e-10
        zh = A.dot(xh)
        act, bb, added, dropped = active.copy(), b.copy(), 0, 0
        for j in range(M):
            if l[j] == u[j]:
                continue
            if active[j] < 0:
                margin[j] = min(margin[j], abs(yh[j] - tol))
                if yh[j] > tol:
                    act[j], bb[j], dropped = 0, 0.0, dropped + 1
            elif active[j] > 0:
                margin[j] = min(margin[j], abs(-yh[j] - tol))
                if yh[j] < -tol:
                    act[j], bb[j], dropped = 0, 0.0, dropped + 1
            else:
                if l[j] > -POLISH_INFTY:
                    margin[j] = min(margin[j], abs((l[j] - zh[j]) - tol))
                    if l[j] - zh[j] > tol:
                        act[j], bb[j], added = -1, l[j], added + 1
                        continue
                if u[j] < POLISH_INFTY:
                    margin[j] = min(margin[j], abs((zh[j] - u[j]) - tol))
                    if zh[j] - u[j] > tol:
                        act[j], bb[j], added = 1, u[j], added + 1
        return act, bb, added, dropped

    def judge(xh, yh):
        pri1, dua1 = residuals(xh, yh)
        if not pri1 <= max(pri0, 1e-10):
            return 2, pri1, dua1
        if not dua1 <= max(dua0, 1e-10):
            return 3, pri1, dua1
        return 0, pri1, dua1

    pri0, dua0 = residuals(x, y)
    out = types.SimpleNamespace(accepted=False, reason=1, n_lower=int(np.sum(active < 0)), n_upper=int(np.sum(active > 0)),
                                pri_before=pri0, dua_before=dua0, pri_after=np.nan, dua_after=np.nan, obj=np.nan,
                                x=x.copy(), y=y.copy(), active=active, margin=margin, xh=None, yh=None)
    if repair_iter is not None:
        out.rounds, out.stop, out.n_added, out.n_dropped, out.accepted0, out.reason0 = 0, 0, 0, 0, False, 1
    point = solve_on(active, b)
    if point is None:
        return out
    xh, yh = point
    if repair_iter is not None:
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
    out.obj = float(.5 * np.dot(xh, P.dot(xh)) + np.dot(q, xh))
    if out.reason == 0:
        out.accepted, out.x, out.y = True, xh.copy(), yh.copy()
    return out


def primal_guess_multipliers(l, u, z, tau):
    """A multiplier guess from the primal side alone, for polishing a point that comes without a y (a tree's incumbent):
    y_j = 0 where l_j == u_j (an equality row is active whatever y says) or both bounds are infinite (never active);
    otherwise y_j = -tau when z_j - l_j < u_j - z_j (the lower bound is the nearer one), else +tau.  Under OSQP's rule
    (polish_restatement step 1) a row is then lower-active iff z - l < tau, otherwise upper-active iff u - z < tau: the
    rows within tau of a bound.  The repair loop corrects what this guesses wrongly."""
    l, u, z = np.asarray(l, dtype=float), np.asarray(u, dtype=float), np.asarray(z, dtype=float)
    y = np.where(z - l < u - z, -float(tau), float(tau))
    y[(l == u) | ((l <= -POLISH_INFTY) & (u >= POLISH_INFTY))] = 0.0
    return y


def add_bounds(i_idx, l_new, u_new, A, l, u):
    """Append l_new <= x[i_idx] <= u_new as identity rows of A (data.py:5-33)."""
    n = A.shape[1]
    rows = spa.identity(n, format='csc')[i_idx, :]
    return spa.vstack([A, rows]).tocsc(), np.append(l, l_new), np.append(u, u_new)


class Data(object):
    """Relaxed-QP data with the integer bounds as trailing constraint rows (data.py:78-97)."""

    def __init__(self, P, q, A, l, u, i_idx, i_l, i_u):
        self.m, self.n = A.shape
        self.n_int = len(i_idx)
        self.A, self.l, self.u = add_bounds(i_idx, i_l, i_u, A, l, u)
        self.P = P.tocsc()
        self.q = q
        self.i_idx = i_idx
        self.i_l = i_l
        self.i_u = i_u

    def compute_obj_val(self, x):
        # data.py:99-103
        return .5 * np.dot(x, self.P.dot(x)) + np.dot(self.q, x)

    def update_vectors(self, q=None, l=None, u=None):
        # data.py:105-126 (l, u are written in place: the root node shares these arrays)
        if q is not None:
            if len(q) != self.n:
                raise ValueError('Wrong q dimension!')
            self.q = q
        if l is not None:
            if len(l) != self.m:
                raise ValueError('Wrong l dimension!')
            self.l[:self.m] = l
        if u is not None:
            if len(u) != self.m:
                raise ValueError('Wrong u dimension!')
            self.u[:self.m] = u


class Node(object):
    """One branch-and-bound node = one relaxation (node.py:41-94)."""

    def __init__(self, data, l, u, solver, depth=0, lower=None, x0=None, y0=None,
                 constant=None):
        self.data = data
        self.l = l
        self.u = u
        self.solver = solver
        self.depth = depth
        self.lower = -np.inf if lower is None else lower
        self.frac_idx = None
        self.intinf = None
        self.num_iter = 0
        self.osqp_solve_time = 0
        self.x = np.zeros(data.n) if x0 is None else x0
        self.y = np.zeros(data.m + data.n_int) if y0 is None else y0
        self._constant = constant if constant is not None else solver.constant
        self.status = self._constant('OSQP_UNSOLVED')
        self.nextvar_idx = None
        self.constr_idx = None
        self.digest = None  # filled by the device epilogue (miosqp_qp_set_root) when available
        self.pc = None  # reliability branching: (parent lower, position, direction 0 down / 1 up, distance f) of the branching

    def _absorb(self, status, num_iter, run_time, x, y, lower):
        self.status = status
        self.num_iter = num_iter
        self.osqp_solve_time = run_time
        self.x = x
        self.y = y
        if lower is not None:
            self.lower = lower

    def solve(self):
        """Lower bound of this node's relaxation (node.py:96-143)."""
        if hasattr(self.solver, 'solve_node'):
            # fused device path: bounds + warm start + ADMM + clamp + objective in one call
            r = self.solver.solve_node(self.l, self.u, self.x, self.y)
            self._absorb(r.status_val, r.iter, r.run_time, r.x, r.y, r.lower)
            self.digest = getattr(r, 'digest', None)
            return
        self.solver.update(l=self.l, u=self.u)
        self.solver.warm_start(x=self.x, y=self.y)
        res = self.solver.solve()
        self._absorb(res.info.status_val, res.info.iter, res.info.run_time, res.x, res.y, None)
        if self.status in (self._constant('OSQP_SOLVED'),
                           self._constant('OSQP_MAX_ITER_REACHED')):
            k = self.data.n_int
            ii = self.data.i_idx
            self.x[ii] = np.minimum(np.maximum(self.x[ii], self.l[-k:]), self.u[-k:])
            self.lower = self.data.compute_obj_val(self.x)


class Results(object):
    def __init__(self, x, upper_glob, run_time, status, osqp_solve_time, osqp_iter_avg):
        self.x = x
        self.upper_glob = upper_glob
        self.run_time = run_time
        self.status = status
        self.osqp_solve_time = osqp_solve_time
        self.osqp_iter_avg = osqp_iter_avg


class Workspace(object):
    """Tree state + the single shared relaxation solver (workspace.py:58-92)."""

    def __init__(self, data, settings, qp_settings=None, backend=None, solver=None):
        self.data = data
        self.settings = settings
        exploration_setting(settings)
        self.sb = branching_settings(settings, qp_settings)
        self.rf = heuristic_settings(settings, qp_settings)
        self.pol = polish_settings(settings)
        self.pol_repair_iter = polish_repair_setting(settings)
        self._second = {}  # second relaxation solvers of the host-side restatements, by iteration cap
        self.backend = backend if backend is not None else _default_backend()
        self.constant = self.backend.constant
        self.ok = (self.constant('OSQP_SOLVED'), self.constant('OSQP_MAX_ITER_REACHED'))  # the statuses with an x
        self.qp_settings = {} if qp_settings is None else qp_settings
        if solver is not None:
            # a solver that is already set up on this data with these qp_settings, integer rows and root included
            # (setup_models builds many in one launch): adopted as it is
            self.solver = solver
            self.root_on_device = self._root_goes_to_device()
        else:
            self.solver = self.backend.OSQP()
            # workspace.py:67-68 expands the *argument*: qp_settings=None is a TypeError there too
            self.solver.setup(data.P, data.q, data.A, data.l, data.u, **qp_settings)
            if hasattr(self.solver, 'set_integer_rows'):
                self.solver.set_integer_rows(data.i_idx, data.m)
            self.push_root()
        self._reset_counters()
        self.first_run = 1
        self.leaves = [self._make_root()]
        self.upper_glob = np.inf
        self.x = np.empty(data.n)
        self.setup_time = 0.
        self.solve_time = 0.
        self.run_time = 0.

    def _root_goes_to_device(self):
        return bool(hasattr(self.solver, 'set_root') and self.settings.get('device_digest', True)
                    and 'eps_abs' in self.qp_settings and self.data.n_int > 0)

    def push_root(self):
        """Hands the root bounds and the two tolerances to the engine so that the x-only part of
        bound_and_branch (integrality test, branching variable, rounding heuristic) is evaluated on
        the device at the end of each node (settings['device_digest'] = False keeps it on the host)."""
        self.root_on_device = False
        if self._root_goes_to_device():
            self.root_on_device = True
            self.solver.set_root(self.data.l, self.data.u, self.settings['eps_int_feas'],
                                 self.qp_settings['eps_abs'])

    # -- bookkeeping ---------------------------------------------------------------------
    def _reset_counters(self):
        self.iter_num = 1
        self.osqp_solve_time = 0.
        self.osqp_iter = 0
        self.osqp_iter_avg = 0
        self.lower_glob = -np.inf
        self.defer_lower = False
        self.status = MI_UNSOLVED
        # strong branching's own work (node relaxations stay in osqp_iter / osqp_solve_time) and the pseudo-costs of
        # reliability branching: per position and direction (0 down, 1 up), sum and count of gains per unit distance
        self.sb_stats = dict(calls=0, children=0, osqp_iter=0, solve_time=0.)
        self.pc_sum = np.zeros((2, self.data.n_int))
        self.pc_cnt = np.zeros((2, self.data.n_int), dtype=np.int64)
        # round and fix: its own work, and the count of fractional nodes that reached the branching (it fires on every
        # rf_every-th of them, the first included)
        self.rf_stats = dict(calls=0, candidates=0, feasible=0, improved=0, osqp_iter=0, solve_time=0.)
        self.rf_nodes = 0
        # polishing of the incumbent (after the search): n_active, pri_after, dua_after are the last call's
        self.polish_stats = dict(calls=0, accepted=0, n_active=0, pri_after=np.nan, dua_after=np.nan, time=0.)
        # the repair loop of the polish (polish_repair_iter > 0): sums over the calls; fixed_points counts stop 0
        self.polish_repair_stats = dict(calls=0, rounds=0, added=0, dropped=0, fixed_points=0)

    def _make_root(self):
        return Node(self.data, self.data.l, self.data.u, self.solver, constant=self.constant)

    def _is(self, leaf, *names):
        return any(leaf.status == self.constant(nm) for nm in names)

    def set_x0(self, x0):
        # workspace.py:94-111
        root = self.leaves[0]
        if self.satisfies_lin_constraints(x0, root.l, root.u) and self.is_int_feas(x0, root):
            self.x = x0
            self.upper_glob = self.data.compute_obj_val(x0)
        else:
            print('Invalid initial solution!\n')
            self.upper_glob = np.inf
            self.x = np.empty(self.data.n)

    def can_continue(self):
        # workspace.py:113-126
        return len(self.leaves) > 0 and self.iter_num < self.settings['max_iter_bb']

    # -- tree exploration ----------------------------------------------------------------
    def leaf_index(self, tree_explor_rule):
        """Index of the next leaf (workspace.py:128-149; note argmax of `lower` in phase two of rule 1).
        Rule 2 is best bound: the leaf with the SMALLEST inherited `lower`, the first one on ties (np.argmin; two
        siblings share their parent's bound, so the tie rule decides the tree).  Rule 3 dives like rule 0 until there
        is an incumbent (from a node or from set_x0) and takes the best bound from then on."""
        if tree_explor_rule == 0 or (tree_explor_rule in (1, 3) and np.isinf(self.upper_glob)):
            return int(np.argmax([lf.depth for lf in self.leaves]))
        if tree_explor_rule == 1:
            return int(np.argmax([lf.lower for lf in self.leaves]))
        if tree_explor_rule in (2, 3):
            return int(np.argmin([lf.lower for lf in self.leaves]))
        raise ValueError('Tree exploring strategy not recognized')

    def choose_leaf(self, tree_explor_rule):
        return self.leaves.pop(self.leaf_index(tree_explor_rule))

    def _child(self, leaf, l, u):
        if np.any(l > u):
            # the reference drops into a debugger here (workspace.py:170-171,194-195)
            raise RuntimeError('branching produced l > u')
        self.leaves.append(Node(self.data, l, u, self.solver, depth=leaf.depth + 1,
                                lower=leaf.lower, x0=leaf.x, y0=leaf.y,
                                constant=self.constant))

    def add_left(self, leaf):
        l, u = np.copy(leaf.l), np.copy(leaf.u)
        u[leaf.constr_idx] = np.floor(leaf.x[leaf.nextvar_idx])
        self._child(leaf, l, u)

    def add_right(self, leaf):
        l, u = np.copy(leaf.l), np.copy(leaf.u)
        l[leaf.constr_idx] = np.ceil(leaf.x[leaf.nextvar_idx])
        self._child(leaf, l, u)

    def pick_nextvar(self, leaf):
        # workspace.py:205-230: largest fractional part among the still-fractional integers (rule 0); rules 1 and 2
        # decide from strong-branching children (select_branching)
        rule = self.settings['branching_rule']
        if rule == 0:
            xf = leaf.x[self.data.i_idx[leaf.frac_idx]]
            nextvar = leaf.frac_idx[int(np.argmax(abs(xf - np.round(xf))))]
        elif rule in (1, 2):
            nextvar = self.select_branching(leaf)
        else:
            raise ValueError('No variable selection rule recognized!')
        leaf.constr_idx = self.data.m + nextvar
        leaf.nextvar_idx = self.data.i_idx[nextvar]

    # -- strong and reliability branching ---------------------------------------------------------
    def _most_fractional(self, leaf, cand, count):
        """`count` positions of `cand` with the largest |x - round(x)| (ties to the lower position), ascending."""
        xf = leaf.x[self.data.i_idx[cand]]
        fr = abs(xf - np.round(xf))
        order = sorted(range(len(cand)), key=lambda j: (-fr[j], cand[j]))[:count]
        return sorted(cand[j] for j in order)

    def select_branching(self, leaf):
        """Branching position of a solved leaf under rule 1 (strong branching on the sb_candidates most fractional) or
        rule 2 (reliability branching: strong branching on the unreliable candidates only, pseudo-costs for the rest)."""
        sb = self.sb
        cand = sorted(leaf.frac_idx)
        if sb['rule'] == 1:
            if len(cand) == 1:
                return cand[0]
            cc = self._most_fractional(leaf, cand, sb['K'])
            return cc[self.strong_branch(leaf, cc).chosen]
        x = leaf.x[self.data.i_idx[cand]]
        fd, fu = x - np.floor(x), np.ceil(x) - x
        cnt = self.pc_cnt[:, cand]
        unrel = [c for j, c in enumerate(cand) if min(cnt[0, j], cnt[1, j]) < sb['reliability']]
        score = dict()
        if unrel:
            cc = self._most_fractional(leaf, unrel, sb['K'])
            r = self.strong_branch(leaf, cc)
            K = len(cc)
            for j, c in enumerate(cc):
                v = leaf.x[self.data.i_idx[c]]
                for side, f in ((0, v - np.floor(v)), (1, np.ceil(v) - v)):
                    b = side * K + j
                    if r.status[b] in self.ok:
                        self.record_gain(c, side, r.lower[b] - leaf.lower, f)
                score[c] = r.score[j]
        psi = self.pseudo_costs()
        eps = sb['eps']
        best, best_s = None, -np.inf
        for j, c in enumerate(cand):
            s = score.get(c)
            if s is None:
                sd, su = psi[0, c] * fd[j], psi[1, c] * fu[j]
                s = (sd if sd > eps else eps) * (su if su > eps else eps)
            if s > best_s:
                best, best_s = c, s
        return best

    def record_gain(self, pos, side, delta, f):
        """One pseudo-cost observation: gain max(delta, 0) per unit distance f of position `pos`, direction `side`."""
        self.pc_sum[side, pos] += (delta if delta > 0.0 else 0.0) / f
        self.pc_cnt[side, pos] += 1

    def pseudo_costs(self):
        """Mean gain per unit [2, n_int]; a position without observations in a direction gets the mean over the
        positions that have some there, or 1.0."""
        psi = np.ones((2, self.data.n_int))
        for side in (0, 1):
            have = self.pc_cnt[side] > 0
            if np.any(have):
                mean = self.pc_sum[side, have] / self.pc_cnt[side, have]
                psi[side, have] = mean
                psi[side, ~have] = np.mean(mean)
        return psi

    def strong_branch(self, leaf, cand):
        """The 2K children of `leaf` for the ascending candidate positions `cand`, each solved with sb_max_iter
        iterations: one device call on an engine with `strong_branch`, otherwise the reference's four calls per child
        on a second solver instance (set up like the first, max_iter = sb_max_iter).  Returns chosen (index into cand),
        lower / status / iter [2K: K down, then K up] and score [K]."""
        sb, st = self.sb, self.sb_stats
        data = self.data
        if hasattr(self.solver, 'strong_branch'):
            r = self.solver.strong_branch(leaf.l, leaf.u, leaf.x, leaf.y, leaf.lower, cand, sb['max_iter'], sb['eps'])
            st['calls'] += 1
            st['children'] += 2 * len(cand)
            st['osqp_iter'] += int(r.iters)
            st['solve_time'] += r.run_time
            return r
        solver = self.sb_solver()
        K, m, ii = len(cand), data.m, data.i_idx
        lower, status, iters = np.full(2 * K, np.nan), np.empty(2 * K, dtype=np.int32), np.empty(2 * K, dtype=np.int32)
        for side in (0, 1):
            for j, c in enumerate(cand):
                b = side * K + j
                l, u = np.copy(leaf.l), np.copy(leaf.u)
                if side == 0:
                    u[m + c] = np.floor(leaf.x[ii[c]])
                else:
                    l[m + c] = np.ceil(leaf.x[ii[c]])
                if np.any(l > u):
                    raise RuntimeError('branching produced l > u')
                status[b], iters[b], x = self.capped_child(leaf, l, u, solver, st)
                if x is not None:
                    lower[b] = data.compute_obj_val(x)
        _, score, chosen = sb_scores(lower, status, leaf.lower, sb['eps'], self.ok)
        st['calls'] += 1
        st['children'] += 2 * K
        st['osqp_iter'] += int(np.sum(iters))
        return types.SimpleNamespace(chosen=chosen, lower=lower, status=status, iter=iters, score=score,
                                     iters=int(np.sum(iters)))

    def capped_child(self, leaf, l, u, solver, stats):
        """Host restatement of one capped child solve: the node `leaf` with the bounds l, u, warm-started from the
        leaf, by the reference's calls on the second solver; its run time goes to stats['solve_time'].  Returns status,
        iterations and x with its integer entries clamped into their rows of l, u (None when the status has no x)."""
        k_int, ii = self.data.n_int, self.data.i_idx
        solver.update(l=l, u=u)
        solver.warm_start(x=leaf.x, y=leaf.y)
        res = solver.solve()
        stats['solve_time'] += res.info.run_time
        x = None
        if res.info.status_val in self.ok:
            x = res.x
            x[ii] = np.minimum(np.maximum(x[ii], l[-k_int:]), u[-k_int:])
        return res.info.status_val, res.info.iter, x

    def sb_solver(self, max_iter=None):
        """The second relaxation solver of the host-side restatements (strong branching, round and fix), created on
        first use.  The `osqp` surface the backends share fixes the iteration cap at setup, so a call that asks for
        another cap than sb_max_iter gets the instance kept for that cap."""
        cap = self.sb['max_iter'] if max_iter is None else int(max_iter)
        if cap not in self._second:
            qs = dict(self.qp_settings, max_iter=cap)
            d = self.data
            self._second[cap] = self.backend.OSQP()
            self._second[cap].setup(d.P, d.q, d.A, d.l, d.u, **qs)
        return self._second[cap]

    # -- round and fix ------------------------------------------------------------------------------------------
    def round_and_fix(self, leaf):
        """Round and fix on a solved, fractional leaf: rf_candidates copies of the node with every integer row fixed
        to a rounding of leaf.x (rf_roundings), warm-started from the leaf and solved with at most rf_max_iter
        iterations.  One device call on an engine with `round_and_fix` that holds the root bounds, otherwise the
        reference's four calls per candidate on the second solver instance.  Returns status / iter / obj / viol per
        candidate (objective of the rounded point, its worst violation of the ROOT's constraints with eps_abs slack:
        <= 0 is satisfies_lin_constraints), feasible (count), chosen (the feasible candidate of lowest objective below
        upper_glob, ties to the lowest, or -1) and its rounded point x (None without one)."""
        rf, st = self.rf, self.rf_stats
        data = self.data
        K = rf['K']
        if hasattr(self.solver, 'round_and_fix') and self.root_on_device:
            r = self.solver.round_and_fix(leaf.l, leaf.u, leaf.x, leaf.y, self.upper_glob, K, rf['max_iter'])
            st['solve_time'] += r.run_time
        else:
            solver = self.sb_solver(rf['max_iter'])
            k_int, ii = data.n_int, data.i_idx
            tol = self.qp_settings['eps_abs']
            fix = rf_roundings(leaf.x[ii], leaf.l[-k_int:], leaf.u[-k_int:], K)
            status, iters = np.empty(K, dtype=np.int32), np.empty(K, dtype=np.int32)
            obj, viol = np.full(K, np.nan), np.full(K, np.nan)
            xs = [None] * K
            for k in range(K):
                l, u = np.copy(leaf.l), np.copy(leaf.u)
                l[-k_int:] = fix[k]
                u[-k_int:] = fix[k]
                status[k], iters[k], x = self.capped_child(leaf, l, u, solver, st)
                if x is not None:
                    x = self.get_integer_solution(x)
                    z = data.A.dot(x)
                    viol[k] = max(np.max(data.l - tol - z), np.max(z - data.u - tol))
                    obj[k] = data.compute_obj_val(x)
                    xs[k] = x
            chosen, feasible = -1, 0
            for k in range(K):
                if xs[k] is None or not viol[k] <= 0.0:
                    continue
                feasible += 1
                if obj[k] < self.upper_glob and (chosen < 0 or obj[k] < obj[chosen]):
                    chosen = k
            r = types.SimpleNamespace(chosen=chosen, x=xs[chosen] if chosen >= 0 else None, status=status, iter=iters,
                                      obj=obj, viol=viol, feasible=feasible, iters=int(np.sum(iters)))
        st['calls'] += 1
        st['candidates'] += K
        st['feasible'] += int(r.feasible)
        st['osqp_iter'] += int(r.iters)
        return r

    def primal_heuristic(self, leaf):
        """bound_and_branch calls this on every fractional node it is about to branch: round and fix on every
        rf_every-th of them (the first included); the winner's objective is recomputed on the host before it becomes
        the incumbent, as the rounding heuristic's is."""
        if not self.rf['on']:
            return
        fire = self.rf_nodes % self.rf['every'] == 0
        self.rf_nodes += 1
        if not fire:
            return
        r = self.round_and_fix(leaf)
        if r.chosen < 0:
            return
        obj = self.data.compute_obj_val(r.x)
        if obj < self.upper_glob:
            self.upper_glob = obj
            self.x = r.x
            self.rf_stats['improved'] += 1
            self.prune()

    def branch_children(self, leaf):
        """Both children of `leaf` on its chosen position; under rule 2 each remembers what its own solve will tell
        the pseudo-costs."""
        self.add_left(leaf)
        self.add_right(leaf)
        if self.sb['rule'] == 2:
            c = leaf.constr_idx - self.data.m
            v = leaf.x[leaf.nextvar_idx]
            self.leaves[-2].pc = (leaf.lower, c, 0, v - np.floor(v))
            self.leaves[-1].pc = (leaf.lower, c, 1, np.ceil(v) - v)

    def satisfies_lin_constraints(self, x, l, u):
        # workspace.py:232-243 (needs 'eps_abs' in qp_settings)
        z = self.data.A.dot(x)
        tol = self.qp_settings['eps_abs']
        return not (np.any(z < l - tol) or np.any(z > u + tol))

    def is_int_feas(self, x, leaf):
        # workspace.py:245-264
        xi = x[self.data.i_idx]
        bad = abs(xi - np.round(xi)) > self.settings['eps_int_feas']
        leaf.frac_idx = np.where(bad)[0].tolist()
        leaf.intinf = np.sum(bad)
        return not leaf.intinf > 0

    def get_integer_solution(self, x):
        xr = np.copy(x)
        xr[self.data.i_idx] = np.round(x[self.data.i_idx])
        return xr

    def solve_wave(self, leaves):
        """Relaxations of several open leaves at once.  With the HIP engine the wave is ONE
        batched device call sharing the factor (`solve_batch`); every leaf ends up exactly as
        its own Node.solve() would leave it."""
        if len(leaves) > 1 and hasattr(self.solver, 'solve_batch'):
            r = self.solver.solve_batch(np.stack([lf.l for lf in leaves]), np.stack([lf.u for lf in leaves]),
                                        np.stack([lf.x for lf in leaves]), np.stack([lf.y for lf in leaves]))
            for k, lf in enumerate(leaves):
                lower = None if np.isnan(r.lower[k]) else float(r.lower[k])
                lf._absorb(int(r.status_val[k]), int(r.iter[k]), float(r.run_time[k]), r.x[k].copy(),
                           r.y[k].copy(), lower)
                lf.digest = r.digest[k] if getattr(r, 'digest', None) is not None else None
        else:
            for lf in leaves:
                lf.solve()

    def prune(self):
        """Drop leaves whose bound exceeds the incumbent, with the reference's traversal:
        workspace.py:278-280 removes from the list it is iterating, so the element following
        each removed one is never examined."""
        k = 0
        while k < len(self.leaves):
            if self.leaves[k].lower > self.upper_glob:
                del self.leaves[k]
            k += 1

    def branch(self, leaf):
        self.pick_nextvar(leaf)
        self.branch_children(leaf)

    def update_lower_glob(self):
        # workspace.py:334: after every branching; a wave defers it to its end (`defer_lower`), the value is
        # only reported, never used for a decision
        if not self.defer_lower:
            self.lower_glob = min(lf.lower for lf in self.leaves)

    def bound_and_branch(self, leaf):
        # workspace.py:282-334
        self.osqp_iter += leaf.num_iter
        self.osqp_solve_time += leaf.osqp_solve_time
        if leaf.pc is not None and self._is(leaf, 'OSQP_SOLVED', 'OSQP_MAX_ITER_REACHED'):
            lp, c, side, f = leaf.pc
            self.record_gain(c, side, leaf.lower - lp, f)
        if self._is(leaf, 'OSQP_PRIMAL_INFEASIBLE', 'OSQP_DUAL_INFEASIBLE'):
            return
        if leaf.lower > self.upper_glob:
            return
        dg = leaf.digest
        if dg is not None:
            # Same decisions from the device digest of this node's x.  The device sums in another order than
            # numpy, so its objective values agree with the host's to ~1e-12 relative, not bit for bit; what
            # enters `upper_glob` through the rounding heuristic is therefore recomputed on the host (rare:
            # only when the digest says the incumbent improves), exactly as workspace.py:321-327 computes
            # it.  `leaf.lower` is the device value on this path by design (node.py:143 fused into the
            # epilogue; 1e-9 relative, DESIGN.md "tolerances").
            rule = self.settings['branching_rule']
            if rule not in (0, 1, 2):
                raise ValueError('No variable selection rule recognized!')
            leaf.intinf = dg.int_inf
            if dg.int_inf == 0:
                leaf.frac_idx = []
                self.x = leaf.x
                self.upper_glob = leaf.lower
                self.prune()
                return
            if dg.heur_feasible and dg.heur_obj < self.upper_glob:
                x_int = self.get_integer_solution(leaf.x)
                obj_int = self.data.compute_obj_val(x_int)
                if obj_int < self.upper_glob:
                    self.upper_glob = obj_int
                    self.x = x_int
                    self.prune()
            self.primal_heuristic(leaf)
            xi = leaf.x[self.data.i_idx]
            leaf.frac_idx = np.where(abs(xi - np.round(xi)) > self.settings['eps_int_feas'])[0].tolist()
            nextvar = dg.nextvar if rule == 0 else self.select_branching(leaf)
            leaf.constr_idx = self.data.m + nextvar
            leaf.nextvar_idx = self.data.i_idx[nextvar]
            self.branch_children(leaf)
            self.update_lower_glob()
            return
        if self.is_int_feas(leaf.x, leaf):
            self.x = leaf.x
            self.upper_glob = leaf.lower
            self.prune()
            return
        x_int = self.get_integer_solution(leaf.x)
        if self.satisfies_lin_constraints(x_int, self.data.l, self.data.u):
            obj_int = self.data.compute_obj_val(x_int)
            if obj_int < self.upper_glob:
                self.upper_glob = obj_int
                self.x = x_int
                self.prune()
        self.primal_heuristic(leaf)
        self.branch(leaf)
        self.update_lower_glob()

    # -- results -------------------------------------------------------------------------
    def get_return_status(self, finished=None):
        # workspace.py:352-373; the sharded search passes `finished` (no open leaf on any rank)
        if finished is None:
            finished = self.iter_num < self.settings['max_iter_bb']
        if self.upper_glob != np.inf:
            self.status = MI_SOLVED if finished else MI_MAX_ITER_FEASIBLE
        elif self.upper_glob >= 0:
            self.status = MI_PRIMAL_INFEASIBLE if finished else MI_MAX_ITER_UNSOLVED
        else:
            self.status = MI_DUAL_INFEASIBLE

    def get_return_solution(self):
        if self.status in (MI_SOLVED, MI_MAX_ITER_FEASIBLE):
            ii = self.data.i_idx
            self.x[ii] = np.round(self.x[ii])

    # -- polishing of the incumbent ---------------------------------------------------------------------------
    def polish_incumbent(self):
        """After the search (settings['polish_incumbent'] = 1, an incumbent exists): the root with every integer row
        fixed to the incumbent's rounded value is solved once through the normal node path, warm-started from the
        incumbent with y = 0, and that solution is polished -- one device call on an engine with `polish`, otherwise
        polish_restatement; with polish_repair_iter > 0 both run the repair loop of the active set and
        polish_repair_stats counts its rounds.  On acceptance the polished x (its integer entries set to the exact
        integers) becomes the returned x and upper_glob its objective; status, node count and the search's statistics
        are not touched."""
        t0 = time()
        data, st = self.data, self.polish_stats
        ii, m = data.i_idx, data.m
        xi = np.round(self.x[ii])
        l, u = np.copy(data.l), np.copy(data.u)
        l[m:] = xi
        u[m:] = xi
        x0 = np.array(self.x, dtype=float)
        x0[ii] = xi
        node = Node(data, l, u, self.solver, x0=x0, y0=np.zeros(m + data.n_int), constant=self.constant)
        node.solve()
        if node.status in self.ok:
            pol = self.pol
            rep = dict(repair_iter=self.pol_repair_iter) if self.pol_repair_iter > 0 else {}
            if hasattr(self.solver, 'polish'):
                r = self.solver.polish(l, u, node.x, node.y, pol['delta'], pol['refine_iter'], **rep)
            else:
                r = polish_restatement(data.P, data.q, data.A, l, u, node.x, node.y, pol['delta'], pol['refine_iter'],
                                       **rep)
            if rep:
                rs = self.polish_repair_stats
                rs['calls'] += 1
                rs['rounds'] += int(r.rounds)
                rs['added'] += int(r.n_added)
                rs['dropped'] += int(r.n_dropped)
                rs['fixed_points'] += int(r.stop == 0)
            st['calls'] += 1
            st['n_active'] = int(r.n_lower + r.n_upper)
            st['pri_after'], st['dua_after'] = float(r.pri_after), float(r.dua_after)
            if r.accepted:
                x = np.array(r.x, dtype=float)
                x[ii] = xi
                self.x = x
                self.upper_glob = data.compute_obj_val(x)
                st['accepted'] += 1
        st['time'] += time() - t0

    # -- progress table (workspace.py:386-433) --------------------------------------------
    def print_headline(self):
        print("     Nodes      |           Current Node        |"
              "             Objective Bounds             |   Cur Node")
        print("Explr\tUnexplr\t|      Obj\tDepth\tIntInf  |    Lower\t   Upper\t"
              "    Gap    |     Iter")

    def print_progress(self, leaf):
        if self.upper_glob == np.inf:
            gap = "    --- "
        else:
            gap = "%8.2f%%" % ((self.upper_glob - self.lower_glob) / abs(self.lower_glob) * 100)
        infeas = self._is(leaf, 'OSQP_PRIMAL_INFEASIBLE', 'OSQP_DUAL_INFEASIBLE')
        obj = np.inf if infeas else leaf.lower
        intinf = "  ---" if leaf.intinf is None else "%5d" % leaf.intinf
        tail = "!" if self._is(leaf, 'OSQP_MAX_ITER_REACHED') else ""
        print("%4d\t%4d\t  %10.2e\t%4d\t%s\t  %10.2e\t%10.2e\t%s\t%5d%s" %
              (self.iter_num, len(self.leaves), obj, leaf.depth, intinf, self.lower_glob,
               self.upper_glob, gap, leaf.num_iter, tail))

    def print_footer(self):
        print("\n")
        print("Status: %s" % self.status)
        if self.status == MI_SOLVED:
            print("Objective bound: %6.3e" % self.upper_glob)
        print("Total number of OSQP iterations: %d" % self.osqp_iter)


class MIOSQP(object):
    """Public facade (solver.py:32-212): setup / solve / update_vectors / set_x0."""

    def __init__(self, backend=None):
        self.data = None
        self.work = None
        self._backend = backend

    def setup(self, P, q, A, l, u, i_idx, i_l, i_u, settings, qp_settings):
        t0 = time()
        if i_l is None:
            i_l = -np.inf * np.ones(len(i_idx))
        if i_u is None:
            i_u = np.inf * np.ones(len(i_idx))
        data = Data(P, q, A, l, u, i_idx, i_l, i_u)
        self.work = Workspace(data, settings, qp_settings, backend=self._backend)
        self.work.setup_time = time() - t0

    def solve(self, observer=None):
        """Run the tree search (solver.py:65-172).  `observer(work, leaf)` is an optional hook
        called after each bound_and_branch; tests use it to record traces."""
        t0 = time()
        work = self.work
        verbose = work.settings['verbose']
        if verbose:
            work.print_headline()
        if observer is None and not verbose:
            self._solve_on_device(work)
        while work.can_continue():
            leaf = work.choose_leaf(work.settings['tree_explor_rule'])
            leaf.solve()
            work.bound_and_branch(leaf)
            if observer is not None:
                observer(work, leaf)
            if verbose and work.iter_num % work.settings['print_interval'] == 0:
                work.print_progress(leaf)
            work.iter_num += 1
        work.osqp_iter_avg = work.osqp_iter / work.iter_num
        work.get_return_status()
        work.get_return_solution()
        if work.pol['on'] and work.status in (MI_SOLVED, MI_MAX_ITER_FEASIBLE):
            work.polish_incumbent()
        if verbose:
            work.print_footer()
        work.solve_time = time() - t0
        if work.first_run:
            work.first_run = 0
            work.run_time = work.setup_time + work.solve_time
        else:
            work.run_time = work.solve_time
        if verbose:
            print("Elapsed time: %.4es" % work.run_time)
        return Results(work.x, work.upper_glob, work.run_time, work.status,
                       work.osqp_solve_time, work.osqp_iter_avg)

    def _solve_on_device(self, work):
        """Small problems (the LDS-resident engine form; BASELINE config 4): the whole loop below runs inside ONE
        device launch with the same decisions (`miosqp_qp_solve_tree`, csrc/kernels_tree.inc); the host only sends
        the root and reads the outcome.  Falls through to the host loop when the engine does not cover the problem
        (too large, no device digest) or the leaf list overflowed -- to be expected more often under tree_explor_rule 2,
    which keeps many more leaves alive than depth first.  settings['device_tree'] = False keeps the host loop."""
        st = work.settings
        if not hasattr(work.solver, 'solve_tree') or getattr(work, '_no_tree', False) or not st.get('device_tree', True):
            self._solve_hosted(work)
            return
        if st['branching_rule'] != 0 or work.rf['on'] or st['tree_explor_rule'] not in (0, 1, 2, 3) or len(work.leaves) != 1 \
                or work.iter_num != 1 or work.data.n_int == 0 or 'eps_abs' not in work.qp_settings \
                or not st.get('device_digest', True):
            return
        root = work.leaves[0]
        have = np.isfinite(work.upper_glob)
        r = work.solver.solve_tree(root.l, root.u, root.x, root.y, work.upper_glob, work.x if have else None,
                                   st['tree_explor_rule'], st['max_iter_bb'])
        if r is None:
            work._no_tree = True  # this engine form never will: do not ask again
            self._solve_hosted(work)
            return
        work.tree_info = r.info  # the launch's own record (max_leaves, overflow, device_time): tests and probes read it
        if r.info.overflow:
            return  # more leaves alive than the launch holds: the host loop redoes the search from the root
        work.iter_num = r.info.nodes + 1
        work.osqp_iter = r.info.osqp_iter
        work.osqp_solve_time = r.info.device_time
        work.upper_glob = r.info.upper_glob
        work.lower_glob = r.info.lower_glob
        if r.info.found:
            work.x = r.x
        # the leaves live on the device; what matters afterwards is whether any is left (node cap reached)
        work.leaves = [] if r.info.leaves_left == 0 else [root] * int(r.info.leaves_left)
        if work.leaves:
            work.iter_num = max(work.iter_num, st['max_iter_bb'])

    def _solve_hosted(self, work):
        """Larger problems: the same loop in the C++ host library with the leaves in device slots
        (`miosqp_qp_search_*`, miosqp_amd/search.py) -- no interpreter and no vector traffic between two nodes.
        settings['device_search'] = False keeps the Python loop."""
        st = work.settings
        if not st.get('device_search', True) or not hasattr(work.solver, 'search_create'):
            return
        if st['branching_rule'] != 0 or work.rf['on'] or st['tree_explor_rule'] not in (0, 1, 2, 3) or len(work.leaves) != 1 \
                or work.iter_num != 1 or work.data.n_int == 0 or 'eps_abs' not in work.qp_settings \
                or not st.get('device_digest', True):
            return
        from miosqp_amd import search
        hs = getattr(work, '_hosted', None)
        root = work.leaves[0]
        if hs is None:
            hs = work._hosted = search.HostedSearch(self, owned=True)
        else:
            hs.begin_instance()
        alive = hs._open
        while alive > 0 and work.iter_num < st['max_iter_bb']:
            alive = hs.step(st['max_iter_bb'] - work.iter_num)
        work.leaves = [root] * int(alive)  # the leaves live on the device; what matters is whether any is left

    def _instance_vectors(self, instances):
        """(Q, L, U) of solve_many's instances, instance-major: the model's current vector where a key is missing"""
        data = self.work.data
        B, n, m, M = len(instances), data.n, data.m, data.m + data.n_int
        Q = np.empty((B, n)); L = np.empty((B, M)); U = np.empty((B, M))
        for k, inst in enumerate(instances):
            Q[k] = data.q if inst.get('q') is None else inst['q']
            L[k] = data.l; U[k] = data.u
            if inst.get('l') is not None:
                L[k, :m] = inst['l']
            if inst.get('u') is not None:
                U[k, :m] = inst['u']
        return Q, L, U

    def _instance_incumbent(self, inst, q, l, u):
        """Workspace.set_x0 (workspace.py:94-111) on one instance's data (q: n, l, u: M): (value, x0) when the instance
        brings an x0 that is feasible for its rows and integral, None when it brings none or an invalid one (printed)"""
        work, data, st = self.work, self.work.data, self.work.settings
        x0 = inst.get('x0')
        if x0 is None:
            return None
        x0 = np.asarray(x0, dtype=float)
        z = data.A.dot(x0)
        tol = work.qp_settings['eps_abs']
        xi = x0[data.i_idx]
        if not (np.any(z < l - tol) or np.any(z > u + tol)) and \
                not np.any(abs(xi - np.round(xi)) > st['eps_int_feas']):
            return .5 * np.dot(x0, data.P.dot(x0)) + np.dot(q, x0), x0
        print('Invalid initial solution!\n')
        return None

    def _tree_result(self, info, x_tree, upper0, run_time):
        """solve_many's dict from the record of a one-launch tree (info: TreeInfo, x_tree: the incumbent the launch
        returned, upper0: the value of the incumbent that went in, inf for none)"""
        data, st = self.work.data, self.work.settings
        upper = info.upper_glob
        # workspace.py:352-373 decides on the loop counter, not on the leaf list: a tree that closes with its
        # last permitted node reports the MAX_ITER family, exactly as solve() does (iter_num = nodes + 1)
        finished = int(info.nodes) + 1 < st['max_iter_bb']
        if upper != np.inf:
            status = MI_SOLVED if finished else MI_MAX_ITER_FEASIBLE
        elif upper >= 0:
            status = MI_PRIMAL_INFEASIBLE if finished else MI_MAX_ITER_UNSOLVED
        else:
            status = MI_DUAL_INFEASIBLE
        x = x_tree.copy() if (info.found or np.isfinite(upper0)) else np.empty(data.n)
        if status in (MI_SOLVED, MI_MAX_ITER_FEASIBLE):
            x[data.i_idx] = np.round(x[data.i_idx])
        return dict(x=x, upper_glob=upper, status=status, nodes=int(info.nodes),
                    osqp_iter=int(info.osqp_iter), run_time=run_time)

    def polish_many(self, instances, results, tau=None, repair_iter=20, large=False):
        """Polishes the answers of `solve_many(instances)` in place, all in ONE device call.  For every result with status
        MI_SOLVED / MI_MAX_ITER_FEASIBLE: its x with the integers rounded, the instance's l, u with the integer rows fixed
        to them, and -- a tree returns no y -- the multipliers of `primal_guess_multipliers(l, u, A x, tau)`
        (tau None: 10 x qp_settings['eps_abs']); the repair loop of the polish (up to `repair_iter` rounds) corrects the
        guess.  delta and refine_iter are the settings polish_delta / polish_refine_iter.  On an engine with
        `polish_many` the call is `OSQP.polish_many` (one launch, one workgroup per instance); a backend without it, or a
        problem it does not hold, goes through polish_restatement per instance with that instance's q.  An instance's
        point is adopted when `accepted and stop == 0`: the guessed y makes dua_before meaningless, so the fixed point of
        the revision is the certificate.  On adoption x is the polished point with its integers set exactly and
        upper_glob its objective with the instance's q.  Every result gains polished (bool), polish_rounds, pri_after,
        dua_after (NaN where nothing was polished).  The model is not touched.  Returns `results`.

        large=True: once the one-workgroup entry is absent or has declined, `OSQP.polish_many_large` is tried before
        the restatement -- still one launch, an instance's reduced matrix in a slab of device scratch (n <= 512); a
        decline is remembered per model.  On a backend without the entry large=True is the restatement."""
        work, data = self.work, self.work.data
        if len(instances) != len(results):
            raise ValueError('polish_many: one result per instance')
        pol = work.pol
        if tau is None:
            tau = 10. * work.qp_settings.get('eps_abs', 1e-3)
        if not tau > 0:
            raise ValueError('polish_many: tau must be positive')
        for r in results:
            r.update(polished=False, polish_rounds=0, pri_after=np.nan, dua_after=np.nan)
        todo = [k for k, r in enumerate(results) if r['status'] in (MI_SOLVED, MI_MAX_ITER_FEASIBLE)]
        if not todo:
            return results
        Q, L, U = self._instance_vectors([instances[k] for k in todo])
        ii, m = data.i_idx, data.m
        X = np.array([results[k]['x'] for k in todo], dtype=float)
        XI = np.round(X[:, ii])
        X[:, ii] = XI
        L[:, m:] = XI
        U[:, m:] = XI
        Y = np.array([primal_guess_multipliers(L[b], U[b], data.A.dot(X[b]), tau) for b in range(len(todo))])
        recs = None
        if hasattr(work.solver, 'polish_many') and not getattr(work, '_no_polish_many', False):
            recs = work.solver.polish_many(Q, L, U, X, Y, pol['delta'], pol['refine_iter'], repair_iter)
            if recs is None:
                work._no_polish_many = True  # this problem is beyond one workgroup: do not ask again
        if recs is None and large and hasattr(work.solver, 'polish_many_large') and \
                not getattr(work, '_no_polish_many_large', False):
            recs = work.solver.polish_many_large(Q, L, U, X, Y, pol['delta'], pol['refine_iter'], repair_iter)
            if recs is None:
                work._no_polish_many_large = True  # beyond the slabs as well
        if recs is None:
            recs = [polish_restatement(data.P, Q[b], data.A, L[b], U[b], X[b], Y[b], pol['delta'], pol['refine_iter'],
                                       repair_iter=repair_iter) for b in range(len(todo))]
        for b, k in enumerate(todo):
            r, res = recs[b], results[k]
            res['polish_rounds'] = int(r.rounds)
            res['pri_after'], res['dua_after'] = float(r.pri_after), float(r.dua_after)
            if r.accepted and r.stop == 0:
                x = np.array(r.x, dtype=float)
                x[ii] = XI[b]
                res['x'] = x
                res['upper_glob'] = .5 * np.dot(x, data.P.dot(x)) + np.dot(Q[b], x)
                res['polished'] = True
        return results

    def solve_many(self, instances, polish=False, lockstep=None, ahead=8, *, heuristic=None, branching=None, **large_options):
        """B MIQPs on this model's factorisation, solved TOGETHER: instance k is what
        `update_vectors(q=, l=, u=)` [+ `set_x0(x0)`] + `solve()` would solve (the reference's MPC pattern,
        /root/reference/miosqp/solver.py:174-212, examples/power_converter/power_converter.py:467-476), for a list of
        dicts with keys q, l, u (each optional: the model's current vector otherwise) and x0 (optional).  On the HIP
        engine every tree runs in one launch -- one workgroup (one wavefront for n + M <= 64) per instance,
        `miosqp_qp_solve_trees` --, so that many small independent MIQPs fill the chip instead of one compute unit;
        instances the launch cannot hold (leaf list overflow) and engines without the entry point go through the
        sequential calls.  The model itself is left as it was: the one-launch path touches nothing of it, the sequential
        fallback puts q, l, u, the leaf list and the statistics back when it is done or when an instance raises (leaves of
        an unfinished device-hosted search are placeholders and not resumable either way).
        Returns a list of dicts: x, upper_glob, status, nodes, osqp_iter, run_time.

        lockstep: what happens beyond the one-launch trees (a tree must fit one workgroup there, n + M <= 192).  The
        lock-step driver (miosqp_amd/lockstep.py) advances all B trees together, one node of every unfinished tree per
        wave, the wave being ONE `solve_batch_q` -- the engine's lock-step batch with a linear cost per column -- and
        every tree running the unchanged `bound_and_branch` on its own leaf list, incumbent and data view; each tree
        makes the decisions of its sequential solve, node for node, and the dicts are formed the same way (run_time:
        elapsed / B).  None (default): once the one-launch path has declined (no `solve_trees`, or it returned None),
        the driver runs if the solver has `solve_batch_q`, branching_rule is 0 and primal_heuristic is 0; otherwise, and
        on every backend without `solve_batch_q` (the CPU oracle), the sequential path as before.  False: always the
        sequential path.  True: the driver on any backend (ValueError for another branching rule or a primal heuristic);
        without `solve_batch_q` a wave is solved column by column on the model's solver (`update(q=)` + `Node.solve`)
        and the solver's q is put back afterwards.  `work.lockstep` holds the last run's record (instances, waves,
        nodes, batched, ADMM iterations per wave).  The model is left as it was, also when an instance raises.
        Measured at n 500, m 1000, p 250: 3.4 x the sequential path at 256 instances and rho 0.1, 1.6 x at
        rho "auto", even at about 32-64 instances and SLOWER below (a narrow wave costs what a wide one costs): with
        few instances pass lockstep=False.
        "device": the same waves driven inside the library (`lockstep.run_device`, `OSQP.solve_trees_lockstep`): the
        leaves of all trees stay in device slots and the tree logic runs in C++, so no vector crosses PCIe per wave and
        no interpreter runs per node; the trees are those of True, the heuristic incumbent's value is the device's sum
        (1e-12 relative).  ValueError when the solver lacks the entry or the settings are not the lock-step trees'.
        Asked for by name only: None never chooses it (DESIGN 3k has the measurements).
        "device" is also the one driver that takes primal_heuristic = 1 (`OSQP.solve_trees_lockstep_rf`): round and fix
        runs inside the trees -- per tree the decisions of its sequential solve, `Workspace.primal_heuristic` on every
        rf_every-th fractional node --, the candidates of ALL trees that fire in a wave as one more batch, built, solved
        and judged on the device; a winner's value is the device's sum.  `work.lockstep['rf']` holds what `rf_stats`
        counts, summed and per instance; the model's own `rf_stats` is not touched.  True and "refill" keep refusing the
        heuristic, None falls to the sequential path with it.
        "device" also takes branching_rule 1 and 2 (`OSQP.solve_trees_lockstep_sb`): every node that branches chooses its
        position as `Workspace.select_branching` does -- per tree the decisions of its sequential solve with that rule,
        pseudo-costs per tree included --, the strong-branching children of ALL nodes with candidates in a wave as one
        more batch (sb_candidates, sb_max_iter, sb_reliability, sb_eps as `solve` reads them).  `work.lockstep['sb']`
        holds what `sb_stats` counts, summed and per instance; the model's own `sb_stats` and pseudo-costs are not
        touched.  Rule 1 or 2 together with primal_heuristic 1 is refused there, True, "refill" and "ahead" refuse rules
        1 and 2 (ValueError naming the rule), None falls to the sequential path with them (DESIGN 3k has the
        measurements).
        "refill": the trees of "device" without the wave (`lockstep.run_refill`, `OSQP.solve_trees_refill`): a column of
        the batch holds one node of one tree and counts its own iterations; after every chunk of check_termination
        iterations the decided columns are harvested and, at that same boundary, loaded again with the next leaf of a
        tree that has no node in flight (a tree still has one node in flight at the most), so no column waits for the
        slowest of a wave and B trees need only min(B, max_batch) columns.  Status, nodes and iterations are those of
        False, upper_glob and x those of "device" bit for bit.  Needs what "device" needs and max_iter a multiple of
        check_termination (ValueError otherwise).  Asked for by name only (DESIGN 3k has the measurements).
        "ahead": the waves of "device" with their spare columns put to use (`lockstep.run_ahead`,
        `OSQP.solve_trees_lockstep_ahead`): a wave launches whole tiles of 64 columns, and in the columns behind the
        chosen leaves a tree may solve other open leaves and children of nodes it has already solved ahead -- up to
        `ahead` columns per tree and wave (an int >= 1; 1 is "device" exactly).  A record waits with its node until the
        tree's rule reaches it and goes when a pruning removes the node; the wave ends with its chosen leaves, whatever
        the other columns are doing.  Every field is that of "device" bit for bit, only the number of waves changes;
        `work.lockstep['ahead']` counts the ahead columns sent, hit, discarded and called off.  Needs what "device"
        needs; primal_heuristic 1, another branching_rule and ahead < 1 are refused (ValueError).  Asked for by name
        only (DESIGN 3k has the measurements).  `ahead` is read by this driver alone.

        polish=True: the incumbents are then polished together by `polish_many` (one more launch on the HIP engine) and
        every dict gains polished, polish_rounds, pri_after, dua_after.  Polishing many instances is asked for per call:
        the setting polish_incumbent, which polishes the incumbent of `solve`, stays refused here.  polish="device" is
        `polish_many(..., large=True)`: a problem beyond one workgroup (everything the lock-step driver takes) is
        polished by `OSQP.polish_many_large` in one launch instead of the host's restatement per instance.  Any other
        value raises ValueError.

        heuristic=None (the default): as above -- with primal_heuristic 1 the one-launch trees step aside.
        heuristic="device": with primal_heuristic 1 and otherwise the one-launch trees' settings (branching_rule 0,
        tree_explor_rule 0-3, device_tree, the device digest, an engine whose `tree_form()` is not 0) the one-launch
        attempt is made with round and fix INSIDE every tree (`OSQP.solve_trees_rf`, miosqp_qp_solve_trees_rf): per
        tree the decisions of its sequential solve, `Workspace.primal_heuristic` on every rf_every-th node about to
        branch, rf_candidates capped solves by the tree's own workgroup, a winner's value being the device's sum (1e-9
        relative, as under lockstep="device").  One workgroup per instance, also for n + M <= 64.  Trees that overflow,
        and a decline, go on as `lockstep` says.  `work.trees_rf` holds per instance calls, candidates, feasible,
        improved, osqp_iter as `rf_stats` defines them; the model's own `rf_stats` and `rf_nodes` are not touched.  With
        primal_heuristic 0 the keyword changes nothing; a backend without the entry (the CPU oracle) ignores it; any
        other value raises ValueError before any launch.  Whether it pays is measured in DESIGN 3h.

        branching=None (the default): as above -- with branching_rule 1 or 2 the one-launch trees step aside.
        branching="device": with branching_rule 1 or 2, primal_heuristic 0 and otherwise the one-launch trees' settings
        the one-launch attempt is made with the rule INSIDE every tree (`OSQP.solve_trees_sb`, miosqp_qp_solve_trees_sb):
        per tree the decisions of its sequential solve, every node that branches choosing its position as
        `Workspace.select_branching` does -- sb_candidates, sb_max_iter, sb_reliability, sb_eps as `solve` reads them,
        the 2K children solved by the tree's own workgroup, pseudo-costs per tree, starting empty; a child's value is
        the device's sum.  One workgroup per instance, also for n + M <= 64.  Trees that overflow, and a decline, go on
        as `lockstep` says.  `work.trees_sb` holds per instance calls, children, osqp_iter as `sb_stats` defines them;
        the model's own `sb_stats`, `pc_sum` and `pc_cnt` are not touched.  With the rule AND primal_heuristic 1 the
        one-launch trees step aside as before, whatever `heuristic` says.  With branching_rule 0 the keyword changes
        nothing; a backend without the entry (the CPU oracle) ignores it; any other value raises ValueError before any
        launch.  The rules do not shrink these trees by much.  Measured (profiles/solve_trees_sb.txt): against
        the same call without the keyword 1.2-1.6 x at one instance, 6-10 x at 8 and 88-167 x at 256 instances of
        (40,60,20) and (50,100,10); against branching_rule 0 in the one-launch trees it LOSES everywhere, 0.13-0.52 x
        the MIQPs/s.

        Two further keywords, `large` and `leaf_cap`, are taken by name only (any other name is a TypeError).
        large=None (the default): as above -- a model beyond the one-launch trees (`tree_form()` 0: n + M > 192, or more
        than 160 KB of LDS) goes to the lock-step drivers or the sequential path.
        large="device": where the one-launch attempt would be made at all (the settings above, device_tree, the device
        digest), `tree_form()` is 0 and the engine's `tree_form_large(leaf_cap)` is 3, every tree runs in ONE launch in
        the reduced form (`OSQP.solve_trees_large`, miosqp_qp_solve_trees_large): one workgroup per instance, the packed
        triangle of L^-1 in LDS, a leaf list of leaf_cap places (an int >= 2, 256 by default), the model's factor, Abar
        and scalings read by all workgroups from the engine's one copy.  Instance k is bit for bit what
        `solve_models([model], [instances[k]], large="device")` gives.  With heuristic="device" and primal_heuristic 1
        the entry is `OSQP.solve_trees_large_rf`, with branching="device" and branching_rule 1 or 2
        `OSQP.solve_trees_large_sb` (`work.trees_rf` / `work.trees_sb` as above); a rule together with the heuristic, or
        either one without its keyword, makes no large attempt.  Trees that overflow leaf_cap, and a decline, go on as
        `lockstep` says; `work.trees_info` holds the infos.  With `tree_form()` not 0 the keyword changes nothing; a
        backend without the entry (the CPU oracle) ignores it; any other value, and a leaf_cap that is not an int >= 2,
        raise ValueError before any launch.  `leaf_cap` is read by this path alone.  Measured
        (profiles/solve_many_large.txt) on the four large grid shapes against the same call without the
        keyword: 5.0-10.3 x at 256 instances, 1.3-3.2 x at 64, 0.68-1.46 x at one; it LOSES at (150,300,20) below 64
        instances."""
        if not (polish is False or polish is True or (isinstance(polish, str) and polish == "device")):
            raise ValueError('solve_many: polish must be False, True or "device"')
        _heuristic_keyword(heuristic, 'solve_many')
        _branching_keyword(branching, 'solve_many')
        large, leaf_cap = _large_options(large_options, 'solve_many')
        work, data, st = self.work, self.work.data, self.work.settings
        require_plain_search(st, "solve_many", rule=False, heuristic=False)
        B = len(instances)
        if B == 0:
            return []
        n, m, M = data.n, data.m, data.m + data.n_int
        ok_engine = one_launch_trees_ok(work)
        in_launch_rf = (heuristic == "device" and bool(work.rf['on']) and one_launch_trees_ok(work, rf=True)
                        and hasattr(work.solver, 'tree_form') and work.solver.tree_form() != 0)
        in_launch_sb = (branching == "device" and st['branching_rule'] in (1, 2) and one_launch_trees_ok(work, sb=True)
                        and hasattr(work.solver, 'tree_form') and work.solver.tree_form() != 0)
        in_large = _large_entry(work, large, heuristic, branching, leaf_cap)  # None, or the entry's name
        Q, L, U = self._instance_vectors(instances)
        up = np.full(B, np.inf); XI = np.zeros((B, n)); any_inc = False
        for k, inst in enumerate(instances):
            x0 = self._instance_incumbent(inst, Q[k], L[k], U[k])
            if x0 is not None:
                up[k], XI[k] = x0
                any_inc = True
        out = [None] * B
        redo = list(range(B))
        declined = True  # the one-launch path: absent, switched off, or it returned None
        if in_large:
            in_launch_rf, in_launch_sb = in_large == 'solve_trees_large_rf', in_large == 'solve_trees_large_sb'
        if ok_engine or in_launch_rf or in_launch_sb or in_large:
            t0 = time()
            if in_large:
                args = (Q, L, U, np.zeros((B, n)), np.zeros((B, M)), up, XI if any_inc else None, st['tree_explor_rule'],
                        st['max_iter_bb'])
                if in_launch_sb:
                    sb = work.sb
                    r = work.solver.solve_trees_large_sb(*args, sb['rule'], sb['K'], sb['max_iter'], sb['reliability'],
                                                         sb['eps'], leaf_cap=leaf_cap)
                elif in_launch_rf:
                    r = work.solver.solve_trees_large_rf(*args, work.rf['K'], work.rf['max_iter'], work.rf['every'],
                                                         leaf_cap=leaf_cap)
                else:
                    r = work.solver.solve_trees_large(*args, leaf_cap=leaf_cap)
            elif in_launch_sb:
                sb = work.sb
                r = work.solver.solve_trees_sb(Q, L, U, np.zeros((B, n)), np.zeros((B, M)), up, XI if any_inc else None,
                                               st['tree_explor_rule'], st['max_iter_bb'], sb['rule'], sb['K'],
                                               sb['max_iter'], sb['reliability'], sb['eps'])
            elif in_launch_rf:
                r = work.solver.solve_trees_rf(Q, L, U, np.zeros((B, n)), np.zeros((B, M)), up, XI if any_inc else None,
                                               st['tree_explor_rule'], st['max_iter_bb'], work.rf['K'],
                                               work.rf['max_iter'], work.rf['every'])
            else:
                r = work.solver.solve_trees(Q, L, U, np.zeros((B, n)), np.zeros((B, M)), up, XI if any_inc else None,
                                            st['tree_explor_rule'], st['max_iter_bb'])
            if r is None and in_large:
                work._no_trees_large = True  # (the small forms' own record stays as it is: they were not asked)
            elif r is None:
                work._no_trees = True
            else:
                X, infos = r[0], r[1]
                work.trees_info = infos  # per instance, as work.tree_info
                if in_launch_sb:
                    work.trees_sb = [_sb_counters(c) for c in r[2]]
                elif in_launch_rf:
                    work.trees_rf = [_rf_counters(c) for c in r[2]]
                dt = time() - t0
                redo = []
                declined = False
                for k in range(B):
                    info = infos[k]
                    if info.overflow:
                        redo.append(k)
                        continue
                    out[k] = self._tree_result(info, X[k], up[k], dt / B)
        if isinstance(lockstep, str):
            # the driver in the library, asked for by name (the default is not this one)
            from miosqp_amd import lockstep as ls
            if lockstep not in ("device", "refill", "ahead"):
                raise ValueError('solve_many: lockstep must be None, True, False, "ahead", "device" or "refill"')
            if lockstep == "device" and not ls.device_supported(work):
                raise ValueError('solve_many(lockstep="device") needs the HIP engine with solve_trees_lockstep and the '
                                 'device digest')
            if lockstep == "refill" and not ls.refill_supported(work):
                raise ValueError('solve_many(lockstep="refill") needs the HIP engine with solve_trees_refill and the '
                                 'device digest')
            if lockstep == "ahead":
                if not ls.ahead_supported(work):
                    raise ValueError('solve_many(lockstep="ahead") needs the HIP engine with solve_trees_lockstep_ahead '
                                     'and the device digest')
                if isinstance(ahead, bool) or not isinstance(ahead, (int, np.integer)) or ahead < 1:
                    raise ValueError('solve_many(lockstep="ahead") needs ahead to be an int >= 1 (the most columns one '
                                     'tree may hold in a wave): ahead %r' % (ahead,))
            # (round and fix runs inside the device driver's trees; the other drivers refuse the heuristic)
            # (... and so do strong and reliability branching, without the heuristic)
            br = st['branching_rule']
            if br in (1, 2) and lockstep == "device":
                if work.rf['on']:
                    raise ValueError('solve_many(lockstep="device") takes branching_rule %d or primal_heuristic 1, not both '
                                     'together' % br)
                if not ls.device_sb_supported(work):
                    raise ValueError('solve_many(lockstep="device") with branching_rule %d needs the HIP engine with '
                                     'solve_trees_lockstep_sb, the device digest and tree_explor_rule 0-3' % br)
            elif br in (1, 2):
                raise ValueError('solve_many(lockstep="%s") needs branching_rule 0, primal_heuristic 0 and '
                                 'tree_explor_rule 0-3: branching_rule %d runs inside lockstep="device" and on the '
                                 'sequential path only' % (lockstep, br))
            elif not (lockstep == "device" and work.rf['on'] and ls.device_rf_supported(work)) and not ls.supported(work):
                raise ValueError('solve_many(lockstep="%s") needs branching_rule 0, primal_heuristic 0 and '
                                 'tree_explor_rule 0-3' % lockstep)
            if lockstep == "refill":
                qs = work.solver.settings  # (the engine's own: aliases and defaults resolved)
                mi, ct = int(qs.max_iter), int(qs.check_termination)
                if ct < 1 or mi % ct != 0:
                    raise ValueError('solve_many(lockstep="refill") needs max_iter to be a multiple of check_termination '
                                     '(a column counts whole chunks): max_iter %d, check_termination %d' % (mi, ct))
            if redo:
                if lockstep == "ahead":
                    ls.run_ahead(self, redo, Q, L, U, up, XI, instances, out, ahead=int(ahead))
                else:
                    (ls.run_refill if lockstep == "refill" else ls.run_device)(self, redo, Q, L, U, up, XI, instances, out)
                redo = []
        if redo and lockstep is not False:
            from miosqp_amd import lockstep as ls
            batched = hasattr(work.solver, 'solve_batch_q')
            if lockstep and not ls.supported(work):
                raise ValueError('solve_many(lockstep=True) needs branching_rule 0, primal_heuristic 0 and '
                                 'tree_explor_rule 0-3' + (': branching_rule %d runs inside lockstep="device" and on the '
                                                           'sequential path only' % st['branching_rule']
                                                           if st['branching_rule'] in (1, 2) else ''))
            if lockstep or (declined and batched and ls.supported(work)):
                ls.run(self, redo, Q, L, U, up, XI, instances, out, batched)
                redo = []
        if redo:
            # sequential path on a copy of the model's vectors, restored afterwards
            q_keep, l_keep, u_keep = data.q, data.l[:m].copy(), data.u[:m].copy()
            # what solve() / update_vectors() overwrite: put back whatever happens (an instance with l > u raises)
            names = ('leaves', 'x', 'upper_glob', 'lower_glob', 'status', 'iter_num', 'osqp_iter', 'osqp_solve_time',
                     'solve_time', 'run_time', 'first_run', 'osqp_iter_avg', 'defer_lower')
            keep = {a: getattr(work, a) for a in names if hasattr(work, a)}
            try:
                for k in redo:
                    inst = instances[k]
                    self.update_vectors(q=Q[k].copy(), l=L[k, :m].copy(), u=U[k, :m].copy())
                    if inst.get('x0') is not None:
                        self.set_x0(np.asarray(inst['x0'], dtype=float).copy())
                    res = self.solve()
                    out[k] = dict(x=np.array(res.x, dtype=float), upper_glob=res.upper_glob, status=res.status,
                                  nodes=work.iter_num - 1, osqp_iter=work.osqp_iter, run_time=res.run_time)
            finally:
                self.update_vectors(q=q_keep, l=l_keep, u=u_keep)
                for a, v in keep.items():
                    setattr(work, a, v)
        if polish:
            self.polish_many(instances, out, large=polish == "device")
        return out

    # The declared parameters of solve_many, their order and their defaults are pinned (tests/test_solve_trees_sb_cpu.py,
    # tests/test_lockstep_ahead_cpu.py): `large` and `leaf_cap` are therefore the two names **large_options takes
    # (`_large_options`; keyword-only by construction, any other name is a TypeError), and the signature shown is the
    # declared one -- the docstring lists the two.
    solve_many.__signature__ = inspect.Signature(
        [par for par in inspect.signature(solve_many).parameters.values() if par.kind is not inspect.Parameter.VAR_KEYWORD])

    def update_vectors(self, q=None, l=None, u=None):
        # solver.py:174-205: same factorisation, new root, statistics reset
        work = self.work
        work.data.update_vectors(q, l, u)
        if q is not None:
            work.solver.update(q=q)
            for second in work._second.values():
                second.update(q=q)
        work.push_root()
        work.leaves = [work._make_root()]
        work._reset_counters()
        work.solve_time = 0.
        work.run_time = 0.
        work.x = np.empty(work.data.n)
        work.upper_glob = np.inf

    def set_x0(self, x0):
        self.work.set_x0(x0)


def _rf_counters(rec):
    """the counters of round and fix inside a one-launch tree (TreeRfInfo) as a dict with the keys of rf_stats"""
    return dict(calls=int(rec.calls), candidates=int(rec.candidates), feasible=int(rec.feasible),
                improved=int(rec.improved), osqp_iter=int(rec.osqp_iter))


def _sb_counters(rec):
    """the counters of strong / reliability branching inside a one-launch tree (TreeSbInfo) as a dict with the keys of
    sb_stats minus the time"""
    return dict(calls=int(rec.calls), children=int(rec.children), osqp_iter=int(rec.osqp_iter))


_BEYOND_ONE_LAUNCH = 'tree_form 0: beyond the one-launch trees'


def _large_options(options, who):
    """the keyword-only options `large` (None or "device") and `leaf_cap` (an int >= 2; 256) of solve_many, taken from
    the call's remaining keywords and checked: (large, leaf_cap).  TypeError for any other name, as for a call with an
    unknown keyword."""
    options = dict(options)
    large, leaf_cap = options.pop('large', None), options.pop('leaf_cap', 256)
    if options:
        raise TypeError("%s() got an unexpected keyword argument %r" % (who, sorted(options)[0]))
    if large is not None and not (isinstance(large, str) and large == "device"):
        raise ValueError('%s: large must be None or "device"' % who)
    if isinstance(leaf_cap, bool) or not isinstance(leaf_cap, (int, np.integer)) or leaf_cap < 2:
        raise ValueError('%s: leaf_cap must be an int of at least 2' % who)
    return large, int(leaf_cap)


def _large_entry(work, large, heuristic, branching, leaf_cap):
    """which entry of the one-launch trees in the reduced form `solve_many(large="device")` calls for this workspace
    ('solve_trees_large', 'solve_trees_large_rf', 'solve_trees_large_sb'), or None: no keyword, a backend without the
    entries, settings the one-launch attempt is not made with (a rule or the heuristic without its keyword, both
    together), an engine another form takes (`tree_form()` not 0) or the reduced form does not (`tree_form_large` not 3),
    or a decline before.  An earlier decline of the small forms (`_no_trees`: what `solve_many` without the keyword
    leaves on such an engine) is looked past, as `solve_models` does."""
    solver, st = work.solver, work.settings
    if large != "device" or getattr(work, '_no_trees_large', False):
        return None
    if not all(hasattr(solver, a) for a in ('solve_trees_large', 'tree_form', 'tree_form_large')):
        return None
    rule, rf_on = st['branching_rule'], bool(work.rf['on'])
    if rule == 0 and not rf_on:
        name, look = 'solve_trees_large', {}
    elif rule == 0 and rf_on and heuristic == "device":
        name, look = 'solve_trees_large_rf', dict(rf=True)
    elif rule in (1, 2) and not rf_on and branching == "device":
        name, look = 'solve_trees_large_sb', dict(sb=True)
    else:
        return None
    if not hasattr(solver, name):
        return None
    declined = getattr(work, '_no_trees', False)
    work._no_trees = False
    try:
        ok = one_launch_trees_ok(work, **look)
    finally:
        work._no_trees = declined
    if not ok or solver.tree_form() != 0 or solver.tree_form_large(leaf_cap) != 3:
        return None
    return name


def _heuristic_keyword(heuristic, who):
    """the keyword `heuristic` of solve_many / solve_models, checked: None or "device" """
    if heuristic is not None and not (isinstance(heuristic, str) and heuristic == "device"):
        raise ValueError('%s: heuristic must be None or "device"' % who)
    return heuristic


def _branching_keyword(branching, who):
    """the keyword `branching` of solve_many / solve_models, checked: None or "device" """
    if branching is not None and not (isinstance(branching, str) and branching == "device"):
        raise ValueError('%s: branching must be None or "device"' % who)
    return branching


def _models_own_reason(work, declined_counts=True, rf=False, sb=False):
    """why `solve_models` leaves a model to its own `solve_many` (None: it goes into the launch); declined_counts=False
    looks past an earlier decline of the one-launch trees (an engine beyond them declines `solve_many`'s own attempt);
    rf=True (heuristic="device") looks past primal_heuristic 1 on a backend that runs it inside the launch; sb=True
    (branching="device") looks past branching_rule 1 and 2 on a backend that runs them inside the launch -- not together
    with primal_heuristic 1, which has its own reason"""
    if not declined_counts and getattr(work, '_no_trees', False):
        work._no_trees = False
        try:
            return _models_own_reason(work, rf=rf, sb=sb)
        finally:
            work._no_trees = True
    st = work.settings
    if not hasattr(work.solver, 'solve_trees') or not hasattr(work.solver, 'tree_form'):
        return 'backend without the one-launch trees'
    if not st.get('device_tree', True):
        return 'device_tree off'
    if st['branching_rule'] != 0:
        if not (sb and st['branching_rule'] in (1, 2) and hasattr(work.solver, 'solve_trees_sb')):
            return 'branching_rule %d' % st['branching_rule']
        if work.rf['on']:
            return 'branching_rule %d together with primal_heuristic on' % st['branching_rule']
    if work.rf['on'] and not (rf and hasattr(work.solver, 'solve_trees_rf')):
        return 'primal_heuristic on'
    if work.data.n_int == 0:
        return 'n_int == 0'
    if getattr(work, '_no_trees', False):
        return 'the one-launch trees declined this model before'
    if not one_launch_trees_ok(work, rf=rf, sb=sb):
        return 'settings beyond the one-launch trees'
    try:
        require_plain_search(st, "solve_models", rule=False, heuristic=False)
    except ValueError:
        return 'settings solve_many refuses'
    if work.solver.tree_form() == 0:
        return _BEYOND_ONE_LAUNCH
    return None


def _polish_models_own_reason(work):
    """why `polish_models` leaves a model to its own `polish_many` (None: it goes into the launch)"""
    if not hasattr(work.backend, 'polish_models') or not hasattr(work.solver, 'polish_models_fits'):
        return 'backend without polish_models'
    if getattr(work, '_no_polish_many', False):
        return 'polish_many declined this model before'
    if not work.solver.polish_models_fits():
        return _BEYOND_ONE_WORKGROUP
    return None


_BEYOND_ONE_WORKGROUP = 'beyond one workgroup'


def _polish_models_large_ok(work):
    """whether a model that `polish_models` leaves out goes into the launch of large="device": it stays out for its size
    alone (a `_no_polish_many` that a declined `polish_many` left on such a model says the same), the backend has the
    entry, the sizes are within the slabs and `polish_many_large` has not declined it"""
    if _polish_models_own_reason(work) == 'backend without polish_models' or work.solver.polish_models_fits():
        return False
    return (hasattr(work.backend, 'polish_models_large') and hasattr(work.solver, 'polish_models_large_fits')
            and not getattr(work, '_no_polish_many_large', False) and work.solver.polish_models_large_fits())


def polish_models(models, instances, results, tau=None, repair_iter=20, guess="host", info=None, large=None):
    """The list form of `MIOSQP.polish_many`: polishes the answers of `solve_models(models, instances)` in place, the
    incumbents of all models in ONE device call (`qp.polish_models`, miosqp_qp_polish_models: one upload, one launch,
    workgroup b polishes model b).  It replaces the loop `models[k].polish_many([instances[k]], [results[k]])`, whose
    first call on every engine builds that engine's polish scratch: here nothing is allocated per model.

    For every result with status MI_SOLVED / MI_MAX_ITER_FEASIBLE: its x with the integers rounded, the instance's l, u
    with the integer rows fixed to them, that model's polish_delta and polish_refine_iter, up to `repair_iter` repair
    rounds, tau None: 10 x that model's qp_settings['eps_abs'].  guess="host": the multipliers of
    `primal_guess_multipliers(l, u, A x, tau)`, computed here as `polish_many` computes them -- result k is then what
    `models[k].polish_many([instances[k]], [results[k]])` makes of it, bit for bit.  guess="device": no y is handed
    over and the workgroup guesses by the same rule from the z it computes (the library takes one tau per call: models
    with different taus go in one call per tau); the answer is that of guess="host" wherever no row sits within
    rounding of the middle between its bounds.  Adoption as in `polish_many`: `accepted and stop == 0`; x gets its
    integers set exactly and upper_glob is recomputed with the instance's q.  Every result gains polished,
    polish_rounds, pri_after, dua_after.  The models are not touched.  Returns `results`.

    A model goes to its own `polish_many`, in place, when its backend has no `polish_models` (the CPU oracle), its
    `_no_polish_many` is set, its sizes are beyond one workgroup, or the library declines the call.

    large=None (the default): as above.  large="device": a model that stays out ONLY because it is beyond one workgroup
    (more than 160 KB of LDS, or M > 256) goes into a second group, polished by ONE more launch
    (`qp.polish_models_large`, miosqp_qp_polish_models_large: workgroups take the models one after the other, each in
    a slab of device scratch), when its backend has the entry, its solver's `polish_models_large_fits()` is true
    (n <= 512) and its `_no_polish_many_large` is not set.  The inputs are prepared as for the small group and with
    guess="device" there is one call per tau; result k is then what `models[k].polish_many([instances[k]],
    [results[k]], large=True)` makes of it, bit for bit -- instead of the host's restatement per model.  If the library
    declines, every model of the group goes to its own `polish_many(..., large=True)`.  A backend without the entry (the
    CPU oracle) ignores the keyword.  Measured on (100,200,15), (150,100,5), (150,300,20) against the call without the
    keyword (profiles/polish_models_large.txt): SLOWER at one model per call (0.7-0.9 x), 2.9-4.5 x at 8
    models, 5-10 x at 64 and 256.  (n + M > 192 alone does not put a model beyond one workgroup: `polish_models_fits()`
    decides, 160 KB of LDS and M <= 256; (50,200,10) fits and is not affected.)

    ValueError: list lengths that differ, tau not positive, another `guess`, another `large`.  info: a dict that is
    filled with polished (positions that went into a launch), polish_own ({position: why}), polish_launches (both groups),
    polish_forms ({'small': .., 'large': ..}: models that went into each kind of launch) and polish_device_time."""
    models, instances = list(models), list(instances)
    if not (len(models) == len(instances) == len(results)):
        raise ValueError('polish_models: one instance and one result per model (%d models, %d instances, %d results)'
                         % (len(models), len(instances), len(results)))
    if guess not in ("host", "device"):
        raise ValueError('polish_models: guess must be "host" or "device"')
    if tau is not None and not tau > 0:
        raise ValueError('polish_models: tau must be positive')
    if large is not None and not (isinstance(large, str) and large == "device"):
        raise ValueError('polish_models: large must be None or "device"')
    own, groups, prep, own_large = {}, {}, {}, set()
    for k, mdl in enumerate(models):
        work, res = mdl.work, results[k]
        res.update(polished=False, polish_rounds=0, pri_after=np.nan, dua_after=np.nan)
        if res['status'] not in (MI_SOLVED, MI_MAX_ITER_FEASIBLE):
            continue
        why = _polish_models_own_reason(work)
        form = 'small'
        if large == "device" and why is not None and _polish_models_large_ok(work):
            why, form = None, 'large'
        if why is not None:
            own[k] = why
            continue
        data = work.data
        tk = 10. * work.qp_settings.get('eps_abs', 1e-3) if tau is None else float(tau)
        Q, L, U = mdl._instance_vectors([instances[k]])
        ii, m = data.i_idx, data.m
        X = np.array(res['x'], dtype=float)
        XI = np.round(X[ii])
        X[ii] = XI
        L[0, m:] = XI
        U[0, m:] = XI
        Y = primal_guess_multipliers(L[0], U[0], data.A.dot(X), tk) if guess == "host" else None
        prep[k] = (Q[0], L[0], U[0], X, Y, XI)
        groups.setdefault((work.backend, tk if guess == "device" else None, form), []).append(k)
    launched, launches, device_time, forms = [], 0, 0.0, dict(small=0, large=0)
    for (be, tk, form), ks in groups.items():
        entry = be.polish_models_large if form == 'large' else be.polish_models
        r = entry([models[k].work.solver for k in ks], [prep[k][0] for k in ks], [prep[k][1] for k in ks],
                  [prep[k][2] for k in ks], [prep[k][3] for k in ks], [prep[k][4] for k in ks],
                  [models[k].work.pol['delta'] for k in ks], [models[k].work.pol['refine_iter'] for k in ks],
                  repair_iter, tau=tk)
        if r is None:  # (an engine declined after all: every model of the call on its own)
            for k in ks:
                own[k] = 'the library declined the call'
            if form == 'large':
                own_large.update(ks)
            continue
        recs, stats = r
        forms[form] += len(ks)
        launches += int(stats.launches)
        device_time += float(stats.device_time)
        for k, rec in zip(ks, recs):
            launched.append(k)
            res, data = results[k], models[k].work.data
            res['polish_rounds'] = int(rec.rounds)
            res['pri_after'], res['dua_after'] = float(rec.pri_after), float(rec.dua_after)
            if rec.accepted and rec.stop == 0:
                x = np.array(rec.x, dtype=float)
                x[data.i_idx] = prep[k][5]
                res['x'] = x
                res['upper_glob'] = .5 * np.dot(x, data.P.dot(x)) + np.dot(prep[k][0], x)
                res['polished'] = True
    for k in sorted(own):
        models[k].polish_many([instances[k]], [results[k]], tau=tau, repair_iter=repair_iter, large=k in own_large)
    if info is not None:
        info.update(polished=sorted(launched), polish_own=dict(own), polish_launches=launches,
                    polish_device_time=device_time, polish_forms=forms)
    return results


def solve_models(models, instances=None, info=None, polish=False, polish_guess="host", large=None, leaf_cap=256,
                 polish_large=None, *, heuristic=None, branching=None):
    """One MIQP on each of several DIFFERENT set-up models -- each with its own P, A, shapes and settings --, the trees
    of all of them in ONE call of the library (`qp.solve_trees_models`, miosqp_qp_solve_trees_models: at most two
    launches, workgroup or wavefront b runs model b).  It replaces the loop `models[k].solve_many([instances[k]])`: one
    upload, one synchronisation and one interpreter round trip for the whole list instead of one per model (the
    reference's benchmark draws a new P and A for every MIQP; so does a sweep over plants).

    models: a list of set-up MIOSQP objects, each at most once.  instances: None, or one dict per model with the keys of
    `solve_many` (q, l, u, x0, each optional).  Returns one dict per model with the keys `solve_many` returns; result k
    is what `models[k].solve_many([instances[k]])[0]` returns -- status, nodes, osqp_iter equal, x and upper_glob bit
    for bit (run_time: the call's time divided by the number of launched models).

    A model goes into the launch when `solve_many` would try its one-launch path for it and its engine's `tree_form()`
    is not 0; every other model (the CPU oracle backend, branching_rule / primal_heuristic not 0, device_tree off, no
    integer variable, an engine beyond one workgroup) and every model whose tree overflowed is solved by its own
    `solve_many([instance])`, and that result stands in its place.  The models are left as they were (q, l, u, the leaf
    list, the statistics); `work.trees_info` of a launched model gets its own TreeInfo as a one-element list.

    ValueError before any launch: an empty list, len(instances) != len(models), a model listed twice (both positions
    named), a model that was not set up, l > u in an instance (its position named).

    polish=True: the incumbents are then polished together by `polish_models` (one more launch for the whole list; a
    model that does not go into it is polished by its own `polish_many`) with guess=polish_guess, and every dict gains
    polished, polish_rounds, pri_after, dua_after: result k is then what `models[k].solve_many([instances[k]],
    polish=True)[0]` returns.  polish=False (the default): no dict has those keys.  Any other value raises ValueError.

    large=None (the default): as above.  large="device": a model that stays out ONLY because its engine is beyond one
    workgroup's product form (`tree_form()` 0: n + M > 192, or more than 160 KB of LDS) goes into the call as well when
    its engine's `tree_form_large(leaf_cap)` answers 3 -- a third launch runs such trees with the relaxation in reduced
    form (the packed triangle of L^-1 in LDS, `qp.solve_trees_models(..., leaf_cap=leaf_cap)`), with a leaf list of
    leaf_cap places (default 256, at least 2; the other forms keep 1024).  Of the reference benchmark's grid this takes
    (50,200,10), (100,200,15), (150,100,5) and (150,300,20).  Such a result is not bit for bit that of the model's own
    `solve_many` (the sums run in another order): status, nodes and osqp_iter are those of the CPU oracle backend's
    tree, x agrees at the integer positions, upper_glob to 1e-8 and x to 1e-6 relative, and the result does not depend
    on the list around the model.  One workgroup iterates such a model 5-10 times slower than the whole chip does, but
    pays no host round trip per node: measured, the keyword pays from one model on (1.4 x) and 15-22 x at 256 models per
    call (profiles/solve_models_large.txt).  Models of the other forms
    get what the call without the keyword gives them.  A backend without the entry (the CPU oracle) ignores the keyword.
    polish=True polishes such a model as any other of the list: the result is what its own `polish_many` makes of the
    tree's x.  Any other value of `large`, or leaf_cap < 2, raises ValueError.

    polish_large=None (the default): as above -- a model beyond one workgroup is polished by its own `polish_many`, the
    host's restatement.  polish_large="device": handed to `polish_models(large="device")`, which polishes those models
    in one more launch (result k is then what `models[k].polish_many(.., large=True)` makes of the tree's x).  Read
    only with polish=True; any other value raises ValueError before any launch.

    heuristic=None (the default): as above.  heuristic="device": a model that stays out ONLY for 'primal_heuristic on'
    goes into the call (`qp.solve_trees_models(..., rf=...)`, miosqp_qp_solve_trees_models_rf) and runs with round and
    fix inside its tree, in up to two more launches: the workgroup form (which takes the wave-sized models too) and,
    with large="device", the reduced form.  Result k is then what `models[k].solve_many([instances[k]],
    heuristic="device")[0]` returns, bit for bit in the workgroup form; a reduced-form tree is that of the CPU oracle
    backend with the heuristic, as above.  Models with the heuristic off get what the call without the keyword gives
    them, bit for bit.  Composes with polish=True.  A backend without the entry (the CPU oracle) ignores the keyword;
    any other value raises ValueError before any launch.

    branching=None (the default): as above.  branching="device": a model that stays out ONLY for 'branching_rule 1' or
    'branching_rule 2' goes into the call (`qp.solve_trees_models(..., sb=...)`, miosqp_qp_solve_trees_models_sb) and
    chooses its branching positions as `Workspace.select_branching` does inside its tree, in up to two more launches: the
    workgroup form (which takes the wave-sized models too) and, with large="device", the reduced form.  Result k is then
    what `models[k].solve_many([instances[k]], branching="device")[0]` returns, bit for bit in the workgroup form; a
    reduced-form tree is that of the CPU oracle backend with the rule, as above.  Models with branching_rule 0 get what
    the call without the keyword gives them, bit for bit.  A model with the rule AND primal_heuristic 1 stays on its own
    path, whatever `heuristic` says ('branching_rule %d together with primal_heuristic on').  The model's own `sb_stats`,
    `pc_sum` and `pc_cnt` are left as they were; `work.trees_sb` gets the tree's counters.  Composes with polish=True
    and heuristic="device" (the models with the heuristic and the models with a rule then go in two calls of the
    library).  A backend without the entry (the CPU oracle) ignores the keyword; any other value raises ValueError
    before any launch.

    info: a dict that is filled with launched (positions), own ({position: why}), forms ({'wave': .., 'group': ..}; with
    large="device" also 'reduced'; with heuristic="device" also 'group_rf' and 'reduced_rf'; with branching="device"
    also 'group_sb' and 'reduced_sb'), launches, device_time (seconds) and overflow (positions); with heuristic="device"
    also rf ({position: counters} of the models that ran with round and fix inside the launch, keys as `rf_stats`); with
    branching="device" also sb ({position: dict(calls, children, osqp_iter)} of the models that ran with a rule inside
    the launch); with polish=True also what `polish_models` reports."""
    _heuristic_keyword(heuristic, 'solve_models')
    _branching_keyword(branching, 'solve_models')
    if not (polish is False or polish is True):
        raise ValueError('solve_models: polish must be False or True')
    if large is not None and not (isinstance(large, str) and large == "device"):
        raise ValueError('solve_models: large must be None or "device"')
    if polish_large is not None and not (isinstance(polish_large, str) and polish_large == "device"):
        raise ValueError('solve_models: polish_large must be None or "device"')
    if isinstance(leaf_cap, bool) or int(leaf_cap) != leaf_cap or leaf_cap < 2:
        raise ValueError('solve_models: leaf_cap must be an integer of at least 2')
    leaf_cap = int(leaf_cap)
    models = list(models)
    B = len(models)
    if B == 0:
        raise ValueError('solve_models: an empty list of models')
    if instances is None:
        instances = [{} for _ in range(B)]
    instances = list(instances)
    if len(instances) != B:
        raise ValueError('solve_models: %d instances for %d models (one dict per model)' % (len(instances), B))
    for k, mdl in enumerate(models):
        for j in range(k):
            if models[j] is mdl:
                raise ValueError('solve_models: the model at position %d is listed again at position %d' % (j, k))
    for k, mdl in enumerate(models):
        if getattr(mdl, 'work', None) is None:
            raise ValueError('solve_models: the model at position %d was not set up' % k)
    vec = []
    for k, mdl in enumerate(models):
        Q, L, U = mdl._instance_vectors([instances[k]])
        if np.any(L[0] > U[0]):
            raise ValueError('solve_models: instance %d: Lower bound must be lower than or equal to upper bound' % k)
        vec.append((Q[0], L[0], U[0]))
    own = {}
    launched = []
    any_large = False
    in_rf = heuristic == "device"
    in_sb = branching == "device"
    rf_par = {}  # position: (rf_candidates, rf_max_iter, rf_every) of the models that run round and fix in the launch
    sb_par = {}  # position: (rule, sb_candidates, sb_max_iter, sb_reliability, sb_eps) of the models that run their rule there
    for k, mdl in enumerate(models):
        look = dict(rf=True) if in_rf else {}  # (without the keywords the question is asked as it always was)
        if in_sb:
            look['sb'] = True
        why = _models_own_reason(mdl.work, **look)
        if (large == "device" and why is not None and hasattr(mdl.work.solver, 'tree_form_large')
                and _models_own_reason(mdl.work, declined_counts=False, **look) == _BEYOND_ONE_LAUNCH
                and mdl.work.solver.tree_form_large(leaf_cap) == 3):
            why = None
            any_large = True
        if why is None:
            launched.append(k)
            if in_sb and mdl.work.sb['rule'] != 0:
                sb = mdl.work.sb
                sb_par[k] = (sb['rule'], sb['K'], sb['max_iter'], sb['reliability'], sb['eps'])
            elif in_rf and mdl.work.rf['on']:
                rf_par[k] = (mdl.work.rf['K'], mdl.work.rf['max_iter'], mdl.work.rf['every'])
        else:
            own[k] = why
    out = [None] * B
    overflow = []
    forms = dict(wave=0, group=0, reduced=0) if large == "device" else dict(wave=0, group=0)
    if in_rf:
        forms.update(group_rf=0, reduced_rf=0)
    if in_sb:
        forms.update(group_sb=0, reduced_sb=0)
    rf_out, sb_out = {}, {}
    launches, device_time = 0, 0.0
    if launched:
        from miosqp_amd import qp
        inc = {}
        for k in launched:
            inc[k] = models[k]._instance_incumbent(instances[k], *vec[k])
        # one call of the library; two when models with the heuristic and models with a rule are both in the list (an
        # entry of the library takes one of the two): the models with a rule then form the second call.  forms,
        # launches, device_time, launched and overflow are summed over the calls and put in list order: with the one
        # call of every list without both kinds, they are what that call reports, as before
        if rf_par and sb_par:
            with_rule = [k for k in launched if k in sb_par]
            others = [k for k in launched if k not in sb_par]
            calls = [(others, dict(rf=rf_par)), (with_rule, dict(sb=sb_par))]
        elif rf_par:
            calls = [(list(launched), dict(rf=rf_par))]
        elif sb_par:
            calls = [(list(launched), dict(sb=sb_par))]
        else:
            calls = [(list(launched), {})]
        done = []
        for group, extra in calls:
            kw = {name: [par.get(k) for k in group] for name, par in extra.items()}
            t0 = time()
            r = qp.solve_trees_models(
                [models[k].work.solver for k in group], [vec[k][0] for k in group], [vec[k][1] for k in group],
                [vec[k][2] for k in group], [np.zeros(models[k].work.data.n) for k in group],
                [np.zeros(len(vec[k][1])) for k in group], [np.inf if inc[k] is None else inc[k][0] for k in group],
                [None if inc[k] is None else inc[k][1] for k in group],
                [models[k].work.settings['tree_explor_rule'] for k in group],
                [models[k].work.settings['max_iter_bb'] for k in group], **(dict(leaf_cap=leaf_cap) if any_large else {}), **kw)
            dt = time() - t0
            if r is None:  # (an engine declined after all: every model on its own)
                for k in group:
                    own[k] = 'the library declined the call'
                continue
            X, infos, stats = r[:3]
            forms['wave'] += int(stats.models_wave)
            forms['group'] += int(stats.models_group)
            if large == "device":
                forms['reduced'] += int(stats.pad)
            for j, k in enumerate(group):
                if 'rf' in kw and k in rf_par:
                    forms['reduced_rf' if r[3][j].form == 5 else 'group_rf'] += 1
                    rf_out[k] = _rf_counters(r[3][j])
                if 'sb' in kw and k in sb_par:
                    forms['reduced_sb' if r[3][j].form == 7 else 'group_sb'] += 1
                    sb_out[k] = _sb_counters(r[3][j])
            launches += int(stats.launches)
            device_time += float(stats.device_time)
            for j, k in enumerate(group):
                done.append(k)
                models[k].work.trees_info = [infos[j]]
                if k in rf_out:
                    models[k].work.trees_rf = [rf_out[k]]
                if k in sb_out:
                    models[k].work.trees_sb = [sb_out[k]]
                if infos[j].overflow:
                    overflow.append(k)
                    continue
                out[k] = models[k]._tree_result(infos[j], X[j], np.inf if inc[k] is None else inc[k][0], dt / len(group))
        launched = sorted(done)
        overflow.sort()
    for k in range(B):
        if out[k] is None:
            out[k] = models[k].solve_many([instances[k]])[0]
    if info is not None:
        info.update(launched=list(launched), own=dict(own), forms=forms, launches=launches, device_time=device_time,
                    overflow=list(overflow))
        if in_rf:
            info['rf'] = rf_out
        if in_sb:
            info['sb'] = sb_out
    if polish:
        polish_models(models, instances, out, guess=polish_guess, info=info, large=polish_large)
    return out


def _setup_models_own_reason(be, data, qp_settings, rho_auto_in_launch=False, large=False, large_rho_auto=False):
    """why `setup_models` leaves a model to `MIOSQP.setup` (None: it goes into the launch; 'large' in place of None with
    large=True: it goes into the launch for models beyond one workgroup of the existing one; 'large auto' with
    large_rho_auto=True: into that launch, which chooses its rho)"""
    if not hasattr(be, 'setup_models') or not hasattr(be, 'setup_models_eligible'):
        return 'backend without the one-launch set-up'
    if data.n_int == 0:
        return 'n_int == 0'
    n, M = data.n, data.A.shape[0]
    if (large and hasattr(be, 'setup_models_eligible_large') and hasattr(be, 'setup_models_shape')
            and be.setup_models_shape(n, M) != 1):
        # out of the existing launch for its SIZE (asked apart from settings and environment): the large launch's rules
        if be.setup_models_shape(n, M) == 0:
            return 'n + M = %d: beyond one workgroup of either launch' % (n + M)
        if isinstance(qp_settings.get('rho'), str):
            if not large_rho_auto:
                return 'rho="auto" beyond one workgroup of the launch: the large launch builds a fixed rho only'
            if not hasattr(be, 'setup_models_eligible_large_auto'):
                return 'rho="auto" beyond one workgroup of the launch: backend without the large launch that chooses rho'
            if not data.P.has_canonical_format or not spa.csc_matrix(data.A).has_canonical_format:
                return 'duplicate entries in P or A'
            if not be.setup_models_eligible_large_auto(n, M, qp_settings):
                fixed = {k: v for k, v in qp_settings.items() if k != 'rho'}
                if be.setup_models_eligible_large(n, M, fixed):  # (everything but the probe's room in the LDS is in order)
                    return ('rho="auto" beyond the LDS rule of the large launch that chooses rho: the packed triangle and '
                            'the probing iterations\' n + 3 M + 8 doubles within 160 KB (n <= 197)')
                return 'settings or environment that lead to another engine form than the large launch builds'
            return 'large auto'
        if not data.P.has_canonical_format or not spa.csc_matrix(data.A).has_canonical_format:
            return 'duplicate entries in P or A'
        if not be.setup_models_eligible_large(n, M, qp_settings):
            return 'settings or environment that lead to another engine form than the large launch builds'
        return 'large'
    if isinstance(qp_settings.get('rho'), str):
        if not rho_auto_in_launch:
            return 'rho="auto"'
        # the launch chooses rho itself; everything else about the model is judged as at a fixed rho
        qp_settings = {k: v for k, v in qp_settings.items() if k != 'rho'}
    if not be.setup_models_eligible(n, M, {}):  # (the library's size rule, asked with default settings)
        return 'n + M = %d: beyond one workgroup of the launch' % (n + M)
    if not data.P.has_canonical_format or not spa.csc_matrix(data.A).has_canonical_format:
        return 'duplicate entries in P or A'
    if not be.setup_models_eligible(n, M, qp_settings):
        return 'settings or environment that lead to another engine form'
    return None


def setup_models(problems, settings, qp_settings, info=None, backend=None, rho_auto=None, large=None, large_rho_auto=None,
                 prepare=None):
    """Set up several DIFFERENT MIQP models -- each with its own P and A -- with ONE launch for the dense set-up of all of
    them (`qp.setup_models`, miosqp_qp_setup_models: one workgroup per model builds the Schur complement, its LDL^T, the
    triangular inverse, the product form, the explicit inverse and its guard; the engines share one stream, one device
    arena and one pinned slab).  It replaces the loop `MIOSQP().setup(...)` over the list: the reference draws a new P and
    A for every MIQP of its benchmark, and that loop is where such a run spends its time.

    problems: a list of dicts with the keys `problems.random_miqp` returns (P, q, A, l, u, i_idx, i_l, i_u).  settings,
    qp_settings: one dict for all models (every model gets its own copy of `settings`), or a list with one per model.
    Returns set-up MIOSQP objects in the order given, ready for `solve_models` and every other method.

    A model goes into the launch when it fits one workgroup (the library's rule: n + M <= 192), rho is a number, it has an integer variable and the settings lead to
    the engine form the launch builds (LDS-resident, product form, explicit inverse); every other model (the CPU oracle
    backend among them) is set up in its place by `MIOSQP.setup`.

    rho_auto: None -- a model with rho="auto" is set up in its place, with MIOSQP.setup's two set-ups; "device" -- such a
    model goes into the launch where everything else about it is eligible, and the workgroup that builds it chooses rho
    (miosqp_qp_setup_models_auto: the probing iterations, the rule and the second factor are stages of the one launch).
    On a backend without that entry (the CPU oracle) such models are still set up in place.  Any other value: ValueError.

    large: None -- a model beyond one workgroup of the launch (n + M > 192) is set up in its place; "device" -- a model
    that stays out ONLY for its size goes into the call where the large rule (`qp.setup_models_eligible_large`: the packed
    triangle of n variables within 160 KB of LDS, n <= 198; n + M <= 2048) and its settings admit it: a second launch of
    the same call builds it (miosqp_qp_setup_models_large, k_setup_models_large: S on the packed triangle in LDS, Abar read
    from L2; no explicit inverse, no guard) as the engine `MIOSQP.setup` builds with coop=0, resident=0, fold=1 -- the
    product form with captured chunks, NOT the cooperative grid `MIOSQP.setup` builds by default at these sizes, which
    iterates a single relaxation faster.  The keyword is for lists that go to `solve_models(large="device")`, whose
    one-launch trees read nothing of the grid; for a long sequential search on one model call `MIOSQP.setup`.  Of the
    reference benchmark's grid this takes (50,200,10), (100,200,15), (150,100,5) and (150,300,20)
    (profiles/setup_models_large.txt).  rho_auto="device" and large="device" combine in one call; a large model with
    rho="auto" is set up in its place (its reason in info["own"]) unless large_rho_auto says otherwise.  On a
    backend without the entry such models are set up in place.  Any other value: ValueError.

    large_rho_auto: read only with large="device", and independent of rho_auto, which goes on deciding for the small
    models.  None -- as above.  "device" -- a large model with rho="auto" goes into the call where
    `qp.setup_models_eligible_large_auto` admits it (the probing iterations' vectors fit the LDS beside the packed
    triangle: n <= 197, which holds every shape `solve_models(large="device")` solves), and the workgroup that builds it
    chooses rho (miosqp_qp_setup_models_large_auto, k_setup_models_large_auto: the fifty probing iterations on the first
    factor in LDS with Abar read from L2, the rule, S and the factor again at the chosen rho); its products are those of the
    same model at a fixed rho equal to the chosen one, bit for bit.  A model beyond that rule, and every model on a
    backend without the entry (the CPU oracle), is set up in place, the rule named in info["own"].  Opt-in; measured in
    profiles/setup_models_large_rho_auto.txt.  Any other value: ValueError.

    prepare: None -- the host equilibrates every model of the call and packs its rows, as `MIOSQP.setup` does (about half
    of the call's time per model).  "device" -- the models that the call's launches take hand their RAW problem to the
    device, and one more launch ahead of the others (miosqp_qp_setup_models_prepared, k_prepare_models: one workgroup per
    model) does both: the rows by variable, by constraint and of the two symmetric matrices, the Ruiz passes in place, D, E,
    c, their inverses, the scaled q, the panel's values.  It composes with the three keywords above.  Everything it writes
    is bit for bit the host's (maxima, correctly rounded 1 / sqrt, products, one sum by one thread in ascending order), so
    every product of the set-up launches and every tree is that of the same call without the keyword, whatever the length
    of the list and the position in it.  A model that no launch takes is set up by `MIOSQP.setup` as before; a backend
    without the entry (the CPU oracle) ignores the keyword.  Opt-in; measured in profiles/setup_models_prepare.txt (a call
    of ONE model loses: one more launch against a millisecond of host work).  Any other value: ValueError.

    ValueError before anything is queued, with the positions named: an empty list, a wrong number of settings, l > u, a P
    of the wrong shape.  A pivot that is not positive raises what `MIOSQP.setup` raises, with the position added; nothing
    of the call is left behind.

    info: a dict that is filled with batched (positions), own ({position: why}), launches, device_time, arena_bytes,
    host_time (seconds of the call outside the library's one), rho (the rho in use per position), forms
    ({'small': .., 'large': ..}: the batched models per launch) and rho_auto_large (the positions whose rho the large
    launch chose) and prepare (the positions that were prepared on the device)."""
    t_call = time()
    if prepare is not None and not (isinstance(prepare, str) and prepare == 'device'):
        raise ValueError('setup_models: prepare must be None or "device", not %r' % (prepare,))
    if rho_auto not in (None, 'device'):
        raise ValueError('setup_models: rho_auto must be None or "device", not %r' % (rho_auto,))
    if large is not None and not (isinstance(large, str) and large == 'device'):
        raise ValueError('setup_models: large must be None or "device", not %r' % (large,))
    if large_rho_auto is not None and not (isinstance(large_rho_auto, str) and large_rho_auto == 'device'):
        raise ValueError('setup_models: large_rho_auto must be None or "device", not %r' % (large_rho_auto,))
    problems = list(problems)
    B = len(problems)
    if B == 0:
        raise ValueError('setup_models: an empty list of problems')

    def per_model(v, name, copy):
        if isinstance(v, dict):
            return [dict(v) if copy else v for _ in range(B)]
        v = list(v)
        if len(v) != B:
            raise ValueError('setup_models: %d %s for %d problems (one dict, or one per problem)' % (len(v), name, B))
        return v

    settings = per_model(settings, 'settings', True)
    qp_settings = per_model(qp_settings, 'qp_settings', False)
    bad_shape, crossed = [], []
    datas = []
    for k, pr in enumerate(problems):
        A, P = spa.csc_matrix(pr['A']), spa.csc_matrix(pr['P'])
        n = A.shape[1]
        i_idx = pr['i_idx']
        i_l = -np.inf * np.ones(len(i_idx)) if pr.get('i_l') is None else pr['i_l']
        i_u = np.inf * np.ones(len(i_idx)) if pr.get('i_u') is None else pr['i_u']
        if P.shape != (n, n):
            bad_shape.append(k)
            datas.append(None)
            continue
        if np.any(np.asarray(pr['l']) > np.asarray(pr['u'])) or np.any(np.asarray(i_l) > np.asarray(i_u)):
            crossed.append(k)
        datas.append(Data(P, pr['q'], A, pr['l'], pr['u'], i_idx, i_l, i_u))
    if bad_shape:
        raise ValueError('setup_models: P must be n x n with n the columns of A, at position(s) %s' % bad_shape)
    if crossed:
        raise ValueError('setup_models: Lower bound must be lower than or equal to upper bound, at position(s) %s' % crossed)
    be = backend if backend is not None else _default_backend()
    own, batched = {}, []
    forms = dict(small=0, large=0)
    rho_auto_large = []
    prepared = []
    for k in range(B):
        why = _setup_models_own_reason(be, datas[k], qp_settings[k], rho_auto == 'device', large == 'device',
                                       large == 'device' and large_rho_auto == 'device')
        if why is None or why in ('large', 'large auto'):
            batched.append(k)
            forms['small' if why is None else 'large'] += 1
            if why == 'large auto':
                rho_auto_large.append(k)
        else:
            own[k] = why
    out = [None] * B
    solvers = []
    launches, device_time, arena_bytes, lib_time = 0, 0.0, 0, 0.0
    try:
        if batched:
            desc = []
            for k in batched:
                d, st, qs = datas[k], settings[k], qp_settings[k]
                md = dict(P=d.P, q=d.q, A=d.A, l=d.l, u=d.u, settings=qs, i_idx=d.i_idx, m_orig=d.m)
                if st.get('device_digest', True) and 'eps_abs' in qs:
                    md['root'] = (d.l, d.u, st['eps_int_feas'], qs['eps_abs'])
                desc.append(md)
            t0 = time()
            try:
                kw = {}
                if rho_auto == 'device' and any(isinstance(md['settings'].get('rho'), str)
                                                for k, md in zip(batched, desc) if k not in rho_auto_large):
                    kw['rho_auto_in_launch'] = True
                if forms['large']:
                    kw['large'] = True
                if rho_auto_large:
                    kw['large_auto'] = True
                if prepare == 'device' and hasattr(be, 'setup_models_prepared'):
                    kw['prepare'] = True
                    prepared = list(batched)
                solvers, stats = be.setup_models(desc, **kw)
            except RuntimeError as ex:
                import re
                hit = re.search(r'\(model (\d+)', str(ex))
                if hit:
                    raise RuntimeError('%s [setup_models: position %d]' % (ex, batched[int(hit.group(1))]))
                raise
            lib_time = time() - t0
            launches, device_time, arena_bytes = int(stats.launches), float(stats.device_time), int(stats.arena_bytes)
            for j, k in enumerate(batched):
                t1 = time()
                out[k] = MIOSQP(backend=backend)
                out[k].work = Workspace(datas[k], settings[k], qp_settings[k], backend=backend, solver=solvers[j])
                out[k].work.setup_time = lib_time / len(batched) + (time() - t1)
        for k in sorted(own):
            pr, d = problems[k], datas[k]
            mdl = MIOSQP(backend=backend)
            mdl.setup(d.P, pr['q'], spa.csc_matrix(pr['A']), pr['l'], pr['u'], d.i_idx, d.i_l, d.i_u, settings[k], qp_settings[k])
            out[k] = mdl
    except Exception:
        for s in solvers + [out[k].work.solver for k in own if out[k] is not None]:  # nothing of the call is left behind
            if hasattr(s, 'close'):
                s.close()
        raise
    if info is not None:
        rho = [float(m.work.solver.rho()) for m in out]
        info.update(batched=list(batched), own=dict(own), launches=launches, device_time=device_time, arena_bytes=arena_bytes,
                    host_time=(time() - t_call) - lib_time, rho=rho, forms=forms, rho_auto_large=rho_auto_large,
                    prepare=prepared)
    return out
