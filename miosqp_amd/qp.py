"""`osqp`-shaped front of the HIP relaxation engine.

Presents exactly the surface the reference's branch-and-bound layer uses on its `osqp` module
(SURVEY.md sec. 8b):

    osqp.OSQP().setup(P, q, A, l, u, **qp_settings)      /root/reference/miosqp/workspace.py:63-68
      (for many models at once: setup_models below, one launch for the dense part of all of them)
    solver.update(l=, u=) / solver.update(q=)            node.py:102 / solver.py:185
    solver.warm_start(x=, y=)                            node.py:105
    solver.solve() -> .x .y .info.status_val .iter .run_time          node.py:108-125
    osqp.constant(name)                                  node.py:88,128-129

plus the fused / batched extensions `solve_node`, `solve_batch`.  Everything numeric happens in
libmiosqp_hip.so through the C ABI of include/miosqp_amd.h; this file only marshals arrays.
"""
import ctypes as C
import types

import numpy as np
import scipy.sparse as spa

from miosqp_amd import _lib

# accepted spellings from older OSQP releases (the reference's own fixtures use them:
# /root/reference/max_iter_examples/*.pickle carry 'eps_inf' and 'polishing')
_ALIASES = {"eps_inf": "eps_prim_inf", "eps_unb": "eps_dual_inf",
            "early_terminate_interval": "check_termination"}
# accepted and ignored: no effect on the iteration
_IGNORED = {"verbose", "polish", "polishing", "linsys_solver", "time_limit", "scaled_termination",
            "delta", "polish_refine_iter", "early_terminate"}


def constant(name):
    """osqp.constant(name)."""
    v = _lib.load().miosqp_qp_constant(name.encode())
    if v == 0:
        raise ValueError("Constant %s not found" % name)
    return v


def default_settings():
    s = _lib.Settings()
    _lib.load().miosqp_qp_default_settings(C.byref(s))
    return s


def _settings_from_kwargs(kw):
    s = default_settings()
    for k, v in kw.items():
        k = _ALIASES.get(k, k)
        if k in _IGNORED:
            continue
        if k == "adaptive_rho":
            if v:
                raise ValueError("adaptive_rho is not supported: rho is one fixed scalar so that "
                                 "the KKT factor is shared by every node (DESIGN.md)")
            continue
        if k == "rho" and isinstance(v, str):
            if v != "auto":
                raise ValueError("rho: a number or 'auto'")
            s.rho_auto = 1  # chosen once at setup (miosqp_qp_settings.rho_auto), from the default starting value
            continue
        if k not in dict(s._fields_) or k == "reserved":
            raise TypeError("setup() got an unexpected setting %r" % k)
        setattr(s, k, v)
    return s


def _check(rc, what):
    if rc < 0:
        raise RuntimeError("%s failed (%d): %s" % (what, rc, _lib.last_error()))
    return rc


def _f64(a, size, name):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != (size,):
        raise ValueError("%s must have %d entries" % (name, size))
    return a


def solve_trees_models(solvers, q, l, u, x0, y0, upper0, x_inc0, rules, max_iter_bb, leaf_cap=None, rf=None, sb=None):
    """One MIQP on each of B DIFFERENT engines, every tree in one launch per kernel form (miosqp_qp_solve_trees_models):
    model b is what `solvers[b].solve_trees(q[b][None], ...)` solves, bit for bit.  Lists of per-model arrays (q, x0: n_b;
    l, u, y0: M_b), upper0: B incumbent values (inf: none), x_inc0: per model an array or None, rules / max_iter_bb: per
    model.  Returns ([x_b], [TreeInfo], stats) -- stats: launches, models_wave, models_group, lds_bytes, device_time,
    run_time -- or None when the library declines (MIOSQP_EUNSUPPORTED: some engine's tree_form() is 0).  ValueError for
    l > u in a root, RuntimeError (with the library's text, which names the model) for every other refusal.

    leaf_cap (None: the call above, exactly): an int >= 2 sends the call to miosqp_qp_solve_trees_models_large, which also
    takes engines whose `tree_form_large(leaf_cap)` is 3 -- the reduced form for models beyond one workgroup's product
    form, with a leaf list of leaf_cap places -- in a third launch; stats.pad then counts them.  Engines of forms 1 and 2
    get what the call without leaf_cap gives them, bit for bit.

    rf (None: the calls above, exactly): one entry per model, None (round and fix off for that model: it goes into the
    launch it goes into without `rf`, with that result bit for bit) or (rf_candidates 1..32, rf_max_iter >= 1,
    rf_every >= 1) -- the call goes to miosqp_qp_solve_trees_models_rf, where such a model runs with
    `Workspace.primal_heuristic` inside its tree, as `solvers[b].solve_trees_rf(q[b][None], ...)` runs it, in up to two
    more launches (the workgroup form, which takes the wave-sized models too, and with leaf_cap the reduced form).
    Returns ([x_b], [TreeInfo], stats, [TreeRfInfo]): per model calls, candidates, feasible, improved, osqp_iter and form
    (1 wave, 2 group, 3 reduced, 4 group with round and fix, 5 reduced with it).

    sb (None: the calls above, exactly; not together with `rf`): one entry per model, None (the most-fractional rule for
    that model: it goes into the launch it goes into without `sb`, with that result bit for bit) or (branching_rule 1 or
    2, sb_candidates 1..32, sb_max_iter >= 1, sb_reliability >= 0, sb_eps > 0) -- the call goes to
    miosqp_qp_solve_trees_models_sb, where such a model chooses its branching positions as `Workspace.select_branching`
    does, as `solvers[b].solve_trees_sb(q[b][None], ...)` runs it, in up to two more launches (the workgroup form, which
    takes the wave-sized models too, and with leaf_cap the reduced form).  Returns ([x_b], [TreeInfo], stats,
    [TreeSbInfo]): per model calls, children, osqp_iter and form (1 wave, 2 group, 3 reduced, 6 group with the rule,
    7 reduced with it)."""
    B = len(solvers)
    if rf is not None and sb is not None:
        raise ValueError("solve_trees_models: rf or sb, not both in one call")
    if (rf is not None and len(rf) != B) or (sb is not None and len(sb) != B):
        raise ValueError("solve_trees_models: one entry per model in every list")
    if leaf_cap is not None and int(leaf_cap) < 2:
        raise ValueError("solve_trees_models: leaf_cap must be at least 2")
    if not (len(q) == len(l) == len(u) == len(x0) == len(y0) == len(upper0) == len(x_inc0) == len(rules) == len(max_iter_bb) == B):
        raise ValueError("solve_trees_models: one entry per model in every list")
    lib = _lib.load()

    def ptrs(arrs):
        return (_lib.dp * max(B, 1))(*[None if a is None else _lib.as_d(a) for a in arrs])

    for s in solvers:
        if s._h is None:
            raise ValueError("solve_trees_models: an engine that was not set up (or was closed)")
    q = [_f64(a, s.n, "q") for a, s in zip(q, solvers)]
    l = [_f64(a, s.m, "l") for a, s in zip(l, solvers)]
    u = [_f64(a, s.m, "u") for a, s in zip(u, solvers)]
    x0 = [_f64(a, s.n, "x0") for a, s in zip(x0, solvers)]
    y0 = [_f64(a, s.m, "y0") for a, s in zip(y0, solvers)]
    up = np.minimum(np.ascontiguousarray(upper0, dtype=np.float64).reshape(B), 1.7e308)
    xin = [None if (a is None or not up[b] < 1.7e308) else _f64(a, solvers[b].n, "x_inc0") for b, a in enumerate(x_inc0)]
    x = [np.zeros(s.n) for s in solvers]
    rl = np.ascontiguousarray(rules, dtype=np.int32).reshape(B)
    mi = np.array([2 ** 31 - 1 if not np.isfinite(v) else int(min(int(v), 2 ** 31 - 1)) for v in max_iter_bb],
                  dtype=np.int32).reshape(B)
    infos = (_lib.TreeInfo * max(B, 1))()
    stats = _lib.ModelsStats()
    hs = (C.c_void_p * max(B, 1))(*[s._h.value for s in solvers])
    rfs = None
    if rf is not None:
        par = np.array([(0, 1, 1) if r is None else tuple(int(v) for v in r) for r in rf], dtype=np.int32).reshape(B, 3)
        rk, ri, re = (np.ascontiguousarray(par[:, c]) for c in range(3))
        rfs = (_lib.TreeRfInfo * max(B, 1))()
        rc = lib.miosqp_qp_solve_trees_models_rf(B, hs, ptrs(q), ptrs(l), ptrs(u), ptrs(x0), ptrs(y0), _lib.as_d(up), ptrs(xin),
                                                 _lib.as_i(rl), _lib.as_i(mi), 0 if leaf_cap is None else int(leaf_cap),
                                                 _lib.as_i(rk), _lib.as_i(ri), _lib.as_i(re), ptrs(x), infos, rfs,
                                                 C.byref(stats))
    elif sb is not None:
        par = [(0, 1, 1, 0, 1.0) if r is None else r for r in sb]
        sr, sk, si, sl = (np.array([int(r[c]) for r in par], dtype=np.int32).reshape(B) for c in range(4))
        se = np.array([float(r[4]) for r in par], dtype=np.float64).reshape(B)
        rfs = (_lib.TreeSbInfo * max(B, 1))()
        rc = lib.miosqp_qp_solve_trees_models_sb(B, hs, ptrs(q), ptrs(l), ptrs(u), ptrs(x0), ptrs(y0), _lib.as_d(up), ptrs(xin),
                                                 _lib.as_i(rl), _lib.as_i(mi), 0 if leaf_cap is None else int(leaf_cap),
                                                 _lib.as_i(sr), _lib.as_i(sk), _lib.as_i(si), _lib.as_i(sl), _lib.as_d(se),
                                                 ptrs(x), infos, rfs, C.byref(stats))
    elif leaf_cap is None:
        rc = lib.miosqp_qp_solve_trees_models(B, hs, ptrs(q), ptrs(l), ptrs(u), ptrs(x0), ptrs(y0), _lib.as_d(up), ptrs(xin),
                                              _lib.as_i(rl), _lib.as_i(mi), ptrs(x), infos, C.byref(stats))
    else:
        rc = lib.miosqp_qp_solve_trees_models_large(B, hs, ptrs(q), ptrs(l), ptrs(u), ptrs(x0), ptrs(y0), _lib.as_d(up),
                                                    ptrs(xin), _lib.as_i(rl), _lib.as_i(mi), int(leaf_cap), ptrs(x), infos,
                                                    C.byref(stats))
    if rc == -5:
        return None
    _check(rc, "solve_trees_models")
    if rc == 1:
        raise ValueError("Lower bound must be lower than or equal to upper bound (%s)" % _lib.last_error())
    if rfs is not None:
        return x, list(infos)[:B], stats, list(rfs)[:B]
    return x, list(infos)[:B], stats


def polish_models(solvers, q, l, u, x, y, delta, refine_iter, repair_iter, tau=None):
    """One polish on each of B DIFFERENT engines in ONE launch (miosqp_qp_polish_models): model b is what
    `solvers[b].polish_many(q[b][None], l[b][None], ..., delta_b, refine_iter_b, repair_iter_b)[0]` answers, bit for bit,
    without building or touching any engine's polish scratch.  Lists of per-model arrays (q, x: n_b; l, u, y: M_b); an
    entry of q may be None (that engine's current linear cost), an entry of y may be None: the device then guesses the
    multipliers from z = A x (0 on equality and free rows, otherwise -tau / +tau by the nearer bound), which needs
    tau > 0.  delta, refine_iter, repair_iter: a scalar or one per model.  Returns (records, stats): one record per model
    shaped like `OSQP.polish_many`'s, `active` included (device_time / run_time are the call's totals), and stats with
    launches, models, lds_bytes, arena_bytes, device_time (and its parts upload_time, launch_time, download_time),
    run_time -- or None when the library declines
    (MIOSQP_EUNSUPPORTED: some model is beyond one workgroup).  ValueError for list lengths that differ and for l > u,
    RuntimeError (with the library's text, which names the model) for every other refusal."""
    return _polish_models_call("polish_models", _lib.PolishModelsStats, solvers, q, l, u, x, y, delta, refine_iter,
                               repair_iter, tau)


def polish_models_large(solvers, q, l, u, x, y, delta, refine_iter, repair_iter, tau=None):
    """`polish_models` beyond one workgroup's LDS (miosqp_qp_polish_models_large): the same arguments, the same way of
    returning.  Model b is what `solvers[b].polish_many_large(q[b][None], l[b][None], ..., delta_b, refine_iter_b,
    repair_iter_b)[0]` answers, bit for bit, without building or touching any engine's polish scratch: W workgroups
    (stats.workgroups = min(B, two per compute unit, what 1 GiB of slabs allows)) take the models one after the other,
    each in its workgroup's slab of device scratch (stats.slab_bytes, sized for the call's largest model).  Every engine
    form `OSQP.polish_many_large` takes goes in, small models as well.  Returns (records, stats) -- stats with launches,
    models, workgroups, slab_bytes, arena_bytes, device_time (upload_time, launch_time, download_time), run_time -- or
    None when the library declines (MIOSQP_EUNSUPPORTED: some model has n > 512 or M > 65536).  ValueError for list
    lengths that differ and for l > u, RuntimeError (the library's text names the model) for every other refusal."""
    return _polish_models_call("polish_models_large", _lib.PolishModelsLargeStats, solvers, q, l, u, x, y, delta,
                               refine_iter, repair_iter, tau)


def _polish_models_call(name, stats_type, solvers, q, l, u, x, y, delta, refine_iter, repair_iter, tau):
    """`polish_models` / `polish_models_large`: the two entries take the same arguments (name: the entry's, as the
    messages say it; stats_type: its stats structure)"""
    B = len(solvers)

    def per_model(v, what):
        if np.ndim(v) == 0:
            return [v] * B
        if len(v) != B:
            raise ValueError("%s: %s must be a scalar or have one entry per model" % (name, what))
        return list(v)

    if not (len(q) == len(l) == len(u) == len(x) == len(y) == B):
        raise ValueError("%s: one entry per model in every list" % name)
    dl = np.ascontiguousarray(per_model(delta, "delta"), dtype=np.float64).reshape(B)
    ri = np.ascontiguousarray(per_model(refine_iter, "refine_iter"), dtype=np.int32).reshape(B)
    pi = np.ascontiguousarray(per_model(repair_iter, "repair_iter"), dtype=np.int32).reshape(B)
    lib = _lib.load()

    def ptrs(arrs):
        return (_lib.dp * max(B, 1))(*[None if a is None else _lib.as_d(a) for a in arrs])

    for s in solvers:
        if s._h is None:
            raise ValueError("%s: an engine that was not set up (or was closed)" % name)
    q = [None if a is None else _f64(a, s.n, "q") for a, s in zip(q, solvers)]
    l = [_f64(a, s.m, "l") for a, s in zip(l, solvers)]
    u = [_f64(a, s.m, "u") for a, s in zip(u, solvers)]
    x = [_f64(a, s.n, "x") for a, s in zip(x, solvers)]
    y = [None if a is None else _f64(a, s.m, "y") for a, s in zip(y, solvers)]
    xo = [np.empty(s.n) for s in solvers]
    yo = [np.empty(s.m) for s in solvers]
    cls = [np.zeros(s.m, dtype=np.int8) for s in solvers]
    infos = (_lib.PolishRepairInfo * max(B, 1))()
    stats = stats_type()
    hs = (C.c_void_p * max(B, 1))(*[s._h.value for s in solvers])
    cp = (C.c_void_p * max(B, 1))(*[c.ctypes.data for c in cls])
    rc = getattr(lib, "miosqp_qp_" + name)(B, hs, ptrs(q), ptrs(l), ptrs(u), ptrs(x), ptrs(y), 0.0 if tau is None else float(tau),
                                           _lib.as_d(dl), _lib.as_i(ri), _lib.as_i(pi), ptrs(xo), ptrs(yo), cp, infos,
                                           C.byref(stats))
    if rc == -5:
        return None
    _check(rc, name)
    if rc == 1:
        raise ValueError("Lower bound must be lower than or equal to upper bound (%s)" % _lib.last_error())
    out = []
    for b in range(B):
        rep, info = infos[b], infos[b].polish
        out.append(types.SimpleNamespace(
            x=xo[b], y=yo[b], accepted=bool(info.accepted), reason=info.reason, n_lower=info.n_lower,
            n_upper=info.n_upper, pri_before=info.pri_before, dua_before=info.dua_before, pri_after=info.pri_after,
            dua_after=info.dua_after, obj=info.obj, device_time=info.device_time, run_time=info.run_time,
            rounds=rep.rounds, stop=rep.stop, n_added=rep.n_added, n_dropped=rep.n_dropped,
            accepted0=bool(rep.accepted0), reason0=rep.reason0, active=cls[b].astype(np.int64)))
    return out, stats


def _csc_arrays(P, A):
    """(n, m, [Pp, Pi, Px, Ap, Ai, Ax]) as OSQP.setup hands them to the library"""
    P = spa.csc_matrix(P)
    A = spa.csc_matrix(A)
    P.sort_indices()
    A.sort_indices()
    n, m = A.shape[1], A.shape[0]
    if P.shape != (n, n):
        raise ValueError("P must be %d x %d" % (n, n))
    return n, m, [np.ascontiguousarray(P.indptr, dtype=np.int32), np.ascontiguousarray(P.indices, dtype=np.int32),
                  np.ascontiguousarray(P.data, dtype=np.float64), np.ascontiguousarray(A.indptr, dtype=np.int32),
                  np.ascontiguousarray(A.indices, dtype=np.int32), np.ascontiguousarray(A.data, dtype=np.float64)]


def setup_models_eligible(n, m, settings):
    """Does the one-launch set-up take a model of n variables and m rows under these settings (a dict as for OSQP.setup,
    or a Settings structure) and this environment?  (miosqp_qp_setup_models_eligible)"""
    s = settings if isinstance(settings, _lib.Settings) else _settings_from_kwargs(settings)
    return bool(_lib.load().miosqp_qp_setup_models_eligible(int(n), int(m), C.byref(s)))


def setup_models_eligible_large(n, m, settings):
    """Does the large launch of setup_models(..., large=True) take a model of n variables and m rows under these
    settings and this environment: a model beyond n + M = 192 whose packed triangle one workgroup holds, with a fixed rho
    and settings that allow the engine of coop=0, resident=0, fold=1?  (miosqp_qp_setup_models_eligible_large)"""
    s = settings if isinstance(settings, _lib.Settings) else _settings_from_kwargs(settings)
    return bool(_lib.load().miosqp_qp_setup_models_eligible_large(int(n), int(m), C.byref(s)))


def setup_models_eligible_large_auto(n, m, settings):
    """Does the large launch of setup_models(..., large=True, large_auto=True) take a model of n variables and m rows under
    these settings and this environment: what setup_models_eligible_large asks, with rho="auto" taken where the probing
    iterations' vectors fit the LDS beside the triangle (n <= 197)?  (miosqp_qp_setup_models_eligible_large_auto)"""
    s = settings if isinstance(settings, _lib.Settings) else _settings_from_kwargs(settings)
    return bool(_lib.load().miosqp_qp_setup_models_eligible_large_auto(int(n), int(m), C.byref(s)))


def setup_models_shape(n, m):
    """The size rules of setup_models alone, whatever settings and environment say: 1 a shape of the existing launch
    (n + M <= 192), 2 a shape of the large launch (n <= 198, n + M <= 2048), 0 neither (miosqp_qp_setup_models_shape)"""
    return int(_lib.load().miosqp_qp_setup_models_shape(int(n), int(m)))


def setup_groups_live():
    """groups of setup_models that are alive in this process (miosqp_qp_setup_groups_live)"""
    return int(_lib.load().miosqp_qp_setup_groups_live())


def setup_models(models, rho_auto_in_launch=False, large=False, large_auto=False, prepare=False):
    """The set-up of several DIFFERENT small models in ONE launch (miosqp_qp_setup_models): the dense part of every
    model -- Schur complement, LDL^T, triangular inverse, product form, explicit inverse, its guard -- by one workgroup
    per model; the engines share one stream, one device arena and one pinned slab.

    rho_auto_in_launch=True (miosqp_qp_setup_models_auto): models whose settings say rho="auto" are taken too, mixed with
    fixed-rho ones as they come; the workgroup that builds such a model runs the fifty probing iterations, applies the
    rule and builds the factor again at the rho it chose (OSQP.rho() reports it).  Without it such a model is refused.

    large=True (miosqp_qp_setup_models_large): a model beyond n + M = 192 (setup_models_eligible_large) is taken too, by a
    second launch of the same call that keeps only the packed triangle in LDS; it comes out as the engine that
    OSQP.setup(..., coop=0, resident=0, fold=1) builds (product form, no explicit inverse; tree_form_large answers 3 for
    it where it does for that engine).  One group, one upload, at most two launches (stats.launches).  Such a model with
    rho="auto" is refused.

    large_auto=True (read with large=True; miosqp_qp_setup_models_large_auto): a large model with rho="auto" is taken too
    (setup_models_eligible_large_auto); the workgroup that builds it chooses rho as the small launch does, on the triangle
    in LDS with Abar read from L2, and every product is that of the same model at a fixed rho equal to the chosen one.

    prepare=True (miosqp_qp_setup_models_prepared, with the three keywords above as its flag bits): the raw problem goes
    up and one more launch ahead of the others (k_prepare_models, one workgroup per model) equilibrates it and packs the
    rows, where the host does both otherwise (about as long per model as everything else of the call together); what
    it writes is bit for bit the host's, and so is every engine.  stats.launches counts the additional launch.

    models: dicts with P, q, A, l, u (as OSQP.setup takes them), settings (a dict of OSQP.setup's keywords), and
    optionally i_idx with m_orig (set_integer_rows is applied) and root = (l_root, u_root, eps_int_feas, eps_lin)
    (set_root is applied).  Returns (a list of set-up OSQP objects in the order given, the call's SetupModelsStats).
    ValueError for l > u or a P of the wrong shape (the position named), RuntimeError with the library's text for every
    other refusal -- a model the launch does not take (setup_models_eligible), a pivot that is not positive."""
    lib = _lib.load()
    B = len(models)
    desc = (_lib.SetupModel * max(B, 1))()
    keep = []
    shapes = []
    for k, md in enumerate(models):
        try:
            n, m, arrs = _csc_arrays(md["P"], md["A"])
        except ValueError as ex:
            raise ValueError("setup_models: model %d: %s" % (k, ex))
        q, l, u = _f64(md["q"], n, "q"), _f64(md["l"], m, "l"), _f64(md["u"], m, "u")
        if np.any(l > u):
            raise ValueError("setup_models: model %d: Lower bound must be lower than or equal to upper bound" % k)
        s = _settings_from_kwargs(md.get("settings", {}))
        d = desc[k]
        d.n, d.M = n, m
        d.Pp, d.Pi, d.Px = _lib.as_i(arrs[0]), _lib.as_i(arrs[1]), _lib.as_d(arrs[2])
        d.Ap, d.Ai, d.Ax = _lib.as_i(arrs[3]), _lib.as_i(arrs[4]), _lib.as_d(arrs[5])
        d.q, d.l, d.u = _lib.as_d(q), _lib.as_d(l), _lib.as_d(u)
        d.settings = C.pointer(s)
        d.n_int = -1
        held = [arrs, q, l, u, s]
        if md.get("i_idx") is not None:
            ii = np.ascontiguousarray(md["i_idx"], dtype=np.int32)
            d.n_int, d.m_orig, d.i_idx = len(ii), int(md["m_orig"]), _lib.as_i(ii)
            held.append(ii)
            if md.get("root") is not None:
                lr, ur, eps_int, eps_lin = md["root"]
                lr, ur = _f64(lr, m, "l_root"), _f64(ur, m, "u_root")
                d.l_root, d.u_root, d.eps_int_feas, d.eps_lin = _lib.as_d(lr), _lib.as_d(ur), float(eps_int), float(eps_lin)
                held += [lr, ur]
        keep.append(held)
        shapes.append((n, m, s))
    hs = (C.c_void_p * max(B, 1))()
    stats = _lib.SetupModelsStats()
    if prepare:
        flags = (1 if rho_auto_in_launch else 0) | (2 if large else 0) | (4 if large and large_auto else 0)
        _check(lib.miosqp_qp_setup_models_prepared(B, desc, hs, C.byref(stats), flags), "setup_models")
    elif large:
        entry = lib.miosqp_qp_setup_models_large_auto if large_auto else lib.miosqp_qp_setup_models_large
        _check(entry(B, desc, hs, C.byref(stats), 1 if rho_auto_in_launch else 0), "setup_models")
    else:
        entry = lib.miosqp_qp_setup_models_auto if rho_auto_in_launch else lib.miosqp_qp_setup_models
        _check(entry(B, desc, hs, C.byref(stats)), "setup_models")
    out = []
    for k, (n, m, s) in enumerate(shapes):
        g = OSQP()
        g._h, g.n, g.m, g.settings = C.c_void_p(hs[k]), n, m, s
        out.append(g)
    return out, stats


def setup_models_prepared(models, **kw):
    """setup_models(models, prepare=True, ...): equilibration and packed rows by a launch of the call
    (miosqp_qp_setup_models_prepared)"""
    return setup_models(models, prepare=True, **kw)


class DevicePtr(object):
    """`count` doubles at address `addr` of DEVICE memory (a slice of a torch tensor, say): accepted wherever a leaf's
    vectors go in or come out (search_add_leaf / search_take_leaf, stream_*, pool_write_node / pool_read_node) -- the
    library copies device to device, a leaf moves between ranks without visiting the host (dist.ShardedStream)."""

    def __init__(self, addr, count):
        self.addr, self.count = int(addr), int(count)

    def __len__(self):
        return self.count


def leaf_record_views(tensor, n_int, n, m):
    """DevicePtr views (l_int, u_int, x0, y0) of a device tensor of >= 2 n_int + n + m doubles"""
    base = tensor.data_ptr()
    offs = (0, n_int, 2 * n_int, 2 * n_int + n)
    cnts = (n_int, n_int, n, m)
    return tuple(DevicePtr(base + 8 * o, c) for o, c in zip(offs, cnts))


def _digest(info):
    """The node digest of a miosqp_qp_info (None from an engine without root bounds: miosqp_qp_set_root)."""
    if info.int_inf < 0:
        return None
    return types.SimpleNamespace(int_inf=info.int_inf, nextvar=info.nextvar, heur_feasible=info.heur_viol <= 0.0,
                                 heur_obj=info.heur_obj, info_viol=info.heur_viol)


def _vec(a, size, name):
    """ctypes pointer of a leaf vector given as an array (host) or a DevicePtr"""
    if isinstance(a, DevicePtr):
        if a.count != size:
            raise ValueError("%s must have %d entries" % (name, size))
        return C.cast(C.c_void_p(a.addr), _lib.dp)
    return _lib.as_d(_f64(a, size, name))


class OSQP(object):
    def __init__(self):
        self._h = None
        self._lib = _lib.load()
        self.n = self.m = 0

    # -- setup -----------------------------------------------------------------------------
    def setup(self, P=None, q=None, A=None, l=None, u=None, **settings):
        if self._h is not None:
            raise RuntimeError("setup() called twice")
        n, m, arrs = _csc_arrays(P, A)
        s = _settings_from_kwargs(settings)
        arrs += [_f64(q, n, "q"), _f64(l, m, "l"), _f64(u, m, "u")]
        if np.any(arrs[7] > arrs[8]):
            raise ValueError("Lower bound must be lower than or equal to upper bound")
        h = C.c_void_p()
        rc = self._lib.miosqp_qp_setup(C.byref(h), n, m, _lib.as_i(arrs[0]), _lib.as_i(arrs[1]),
                                       _lib.as_d(arrs[2]), _lib.as_i(arrs[3]), _lib.as_i(arrs[4]),
                                       _lib.as_d(arrs[5]), _lib.as_d(arrs[6]), _lib.as_d(arrs[7]),
                                       _lib.as_d(arrs[8]), C.byref(s))
        _check(rc, "setup")
        self._h, self.n, self.m, self.settings = h, n, m, s

    def set_integer_rows(self, i_idx, m_orig):
        ii = np.ascontiguousarray(i_idx, dtype=np.int32)
        _check(self._lib.miosqp_qp_set_integer_rows(self._h, len(ii), _lib.as_i(ii), int(m_orig)),
               "set_integer_rows")

    def set_root(self, l_root, u_root, eps_int_feas, eps_lin):
        """Enable the on-device node digest (see miosqp_qp_set_root)."""
        l_root, u_root = _f64(l_root, self.m, "l_root"), _f64(u_root, self.m, "u_root")
        _check(self._lib.miosqp_qp_set_root(self._h, _lib.as_d(l_root), _lib.as_d(u_root),
                                            float(eps_int_feas), float(eps_lin)), "set_root")

    # -- the reference's four calls ------------------------------------------------------------
    def update(self, q=None, l=None, u=None):
        if q is not None:
            _check(self._lib.miosqp_qp_update_lin_cost(self._h, _lib.as_d(_f64(q, self.n, "q"))),
                   "update(q)")
        if l is not None or u is not None:
            if l is None or u is None:
                raise ValueError("update() needs both l and u")
            l, u = _f64(l, self.m, "l"), _f64(u, self.m, "u")
            rc = _check(self._lib.miosqp_qp_update_bounds(self._h, _lib.as_d(l), _lib.as_d(u)),
                        "update(l,u)")
            if rc == 1:
                raise ValueError("Lower bound must be lower than or equal to upper bound")

    def warm_start(self, x=None, y=None):
        if x is None or y is None:
            raise ValueError("warm_start() needs both x and y")
        _check(self._lib.miosqp_qp_warm_start(self._h, _lib.as_d(_f64(x, self.n, "x")),
                                              _lib.as_d(_f64(y, self.m, "y"))), "warm_start")

    def solve(self):
        x, y, info = np.empty(self.n), np.empty(self.m), _lib.Info()
        _check(self._lib.miosqp_qp_solve(self._h, _lib.as_d(x), _lib.as_d(y), C.byref(info)), "solve")
        return types.SimpleNamespace(x=x, y=y, info=info)

    # -- fused / batched extensions ------------------------------------------------------------
    def solve_node(self, l, u, x0, y0):
        """Whole body of Node.solve() (node.py:96-143) in one device round trip."""
        l, u = _f64(l, self.m, "l"), _f64(u, self.m, "u")
        x0, y0 = _f64(x0, self.n, "x0"), _f64(y0, self.m, "y0")
        x, y, info = np.empty(self.n), np.empty(self.m), _lib.Info()
        rc = _check(self._lib.miosqp_qp_solve_node(self._h, _lib.as_d(l), _lib.as_d(u), _lib.as_d(x0),
                                                   _lib.as_d(y0), _lib.as_d(x), _lib.as_d(y),
                                                   C.byref(info)), "solve_node")
        if rc == 1:
            raise ValueError("Lower bound must be lower than or equal to upper bound")
        lower = None if np.isnan(info.lower) else info.lower
        return types.SimpleNamespace(x=x, y=y, status_val=info.status_val, iter=info.iter,
                                     run_time=info.run_time, lower=lower, info=info, digest=_digest(info))

    def solve_batch(self, l, u, x0, y0):
        """B independent nodes sharing the factor; arrays are [B, .]."""
        return self._solve_batch(None, l, u, x0, y0)

    def solve_batch_q(self, q, l, u, x0, y0):
        """B independent nodes sharing the factor, each with a linear cost of its own (q is [B, n]): column k is
        update(q=q[k]) + solve_node(l[k], u[k], x0[k], y0[k]); the solver's own q stays as it is.  Returns what
        solve_batch returns."""
        return self._solve_batch(q, l, u, x0, y0)

    def _solve_batch(self, q, l, u, x0, y0):
        l = np.ascontiguousarray(l, dtype=np.float64)
        B = l.shape[0]
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(B, self.m)
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(B, self.n)
        y0 = np.ascontiguousarray(y0, dtype=np.float64).reshape(B, self.m)
        x, y = np.empty((B, self.n)), np.empty((B, self.m))
        infos = (_lib.Info * B)()
        if q is None:
            rc = _check(self._lib.miosqp_qp_solve_batch(self._h, B, _lib.as_d(l), _lib.as_d(u),
                                                        _lib.as_d(x0), _lib.as_d(y0), _lib.as_d(x),
                                                        _lib.as_d(y), infos), "solve_batch")
        else:
            q = np.ascontiguousarray(q, dtype=np.float64).reshape(B, self.n)
            rc = _check(self._lib.miosqp_qp_solve_batch_q(self._h, B, _lib.as_d(q), _lib.as_d(l), _lib.as_d(u),
                                                          _lib.as_d(x0), _lib.as_d(y0), _lib.as_d(x),
                                                          _lib.as_d(y), infos), "solve_batch_q")
        if rc == 1:
            raise ValueError("Lower bound must be lower than or equal to upper bound")
        return types.SimpleNamespace(
            digest=[_digest(i) for i in infos],
            x=x, y=y, status_val=np.array([i.status_val for i in infos]),
            iter=np.array([i.iter for i in infos]), lower=np.array([i.lower for i in infos]),
            run_time=np.array([i.run_time for i in infos]), infos=infos)

    def strong_branch(self, l, u, x, y, parent_lower, cand, max_iter, eps):
        """The 2K children of one solved node (bounds l, u; clamped x; y) for the K candidate positions `cand` (ascending
        positions in i_idx), solved together with `max_iter` iterations each and scored on the device
        (miosqp_qp_strong_branch).  lower / status / iter: K down children, then K up children; score: per candidate;
        chosen: the argmax, an index into cand."""
        l, u = _f64(l, self.m, "l"), _f64(u, self.m, "u")
        x, y = _f64(x, self.n, "x"), _f64(y, self.m, "y")
        c = np.ascontiguousarray(cand, dtype=np.int32)
        K = len(c)
        lower, score = np.empty(2 * K), np.empty(max(K, 1))
        status, iters = np.empty(2 * K, dtype=np.int32), np.empty(2 * K, dtype=np.int32)
        info = _lib.SbInfo()
        rc = _check(self._lib.miosqp_qp_strong_branch(self._h, _lib.as_d(l), _lib.as_d(u), _lib.as_d(x), _lib.as_d(y),
                                                      float(parent_lower), K, _lib.as_i(c), int(max_iter), float(eps),
                                                      _lib.as_d(lower), _lib.as_i(status), _lib.as_i(iters),
                                                      _lib.as_d(score), C.byref(info)), "strong_branch")
        if rc == 1:
            raise ValueError("Lower bound must be lower than or equal to upper bound")
        return types.SimpleNamespace(chosen=info.chosen, lower=lower, status=status, iter=iters, score=score[:K],
                                     iters=info.iters, device_time=info.device_time, run_time=info.run_time)

    def round_and_fix(self, l, u, x, y, upper, K, max_iter):
        """The round-and-fix heuristic on one solved node (bounds l, u; clamped x; y): K candidates with every integer
        row fixed to min(max(floor(x_i + (k + 1) / (K + 1)), l), u), solved together with at most `max_iter` iterations
        each and judged on the device (miosqp_qp_round_and_fix).  status / iter / obj / viol: per candidate (objective of
        the rounded point and its worst violation of the root's constraints, <= 0 feasible); chosen: the feasible
        candidate of lowest objective below `upper`, -1 without one; x: its rounded point, None without one."""
        l, u = _f64(l, self.m, "l"), _f64(u, self.m, "u")
        x, y = _f64(x, self.n, "x"), _f64(y, self.m, "y")
        K = int(K)
        kk = max(K, 1)
        xo, obj, viol = np.empty(self.n), np.empty(kk), np.empty(kk)
        status, iters = np.empty(kk, dtype=np.int32), np.empty(kk, dtype=np.int32)
        info = _lib.RfInfo()
        rc = _check(self._lib.miosqp_qp_round_and_fix(self._h, _lib.as_d(l), _lib.as_d(u), _lib.as_d(x), _lib.as_d(y),
                                                      float(upper), K, int(max_iter), _lib.as_d(xo), _lib.as_i(status),
                                                      _lib.as_i(iters), _lib.as_d(obj), _lib.as_d(viol),
                                                      C.byref(info)), "round_and_fix")
        if rc == 1:
            raise ValueError("Lower bound must be lower than or equal to upper bound")
        return types.SimpleNamespace(chosen=info.chosen, x=xo if info.chosen >= 0 else None, status=status[:K],
                                     iter=iters[:K], obj=obj[:K], viol=viol[:K], feasible=info.feasible,
                                     iters=info.iters, device_time=info.device_time, run_time=info.run_time)

    def polish(self, l, u, x, y, delta=1e-6, refine_iter=3, repair_iter=None):
        """Polishing of one node's solution (bounds l, u; approximate x, y) on the device (miosqp_qp_polish): the active
        set guessed from (x, y), the regularised KKT system on it solved through a dense factorisation of the reduced
        matrix and refined `refine_iter` times.  Returns the record (accepted, reason 0 ok / 1 factorisation / 2 primal
        / 3 dual, n_lower, n_upper, pri / dua before and after, obj of the polished point, device_time, run_time) plus
        x, y: the polished point when accepted, the input otherwise.  The QP setting `polish` stays ignored: this is a
        call of its own.

        repair_iter None: as above.  An integer 0..20 calls miosqp_qp_polish_repair: up to that many rounds that revise
        the set from the polished point and solve again; the record is that of the point the loop ended with and gains
        rounds, stop (0 fixed point, 1 round limit, 2 bad pivot in a repair round), n_added, n_dropped, accepted0,
        reason0 (round 0's answer) and active (per row -1 lower, 1 upper, 0 inactive in the final set)."""
        l, u = _f64(l, self.m, "l"), _f64(u, self.m, "u")
        x, y = _f64(x, self.n, "x"), _f64(y, self.m, "y")
        xo, yo = np.empty(self.n), np.empty(self.m)
        args = (self._h, _lib.as_d(l), _lib.as_d(u), _lib.as_d(x), _lib.as_d(y), float(delta), int(refine_iter))
        if repair_iter is None:
            rep, info = None, _lib.PolishInfo()
            rc = _check(self._lib.miosqp_qp_polish(*args, _lib.as_d(xo), _lib.as_d(yo), C.byref(info)), "polish")
        else:
            rep = _lib.PolishRepairInfo()
            rc = _check(self._lib.miosqp_qp_polish_repair(*args, int(repair_iter), _lib.as_d(xo), _lib.as_d(yo),
                                                          C.byref(rep)), "polish_repair")
            info = rep.polish
        if rc == 1:
            raise ValueError("Lower bound must be lower than or equal to upper bound")
        out = types.SimpleNamespace(x=xo, y=yo, accepted=bool(info.accepted), reason=info.reason, n_lower=info.n_lower,
                                    n_upper=info.n_upper, pri_before=info.pri_before, dua_before=info.dua_before,
                                    pri_after=info.pri_after, dua_after=info.dua_after, obj=info.obj,
                                    device_time=info.device_time, run_time=info.run_time)
        if rep is not None:
            out.rounds, out.stop, out.n_added, out.n_dropped = rep.rounds, rep.stop, rep.n_added, rep.n_dropped
            out.accepted0, out.reason0 = bool(rep.accepted0), rep.reason0
            cls = np.zeros(self.m, dtype=np.int8)
            _check(self._lib.miosqp_qp_get_polish_repair_trace(self._h, cls.ctypes.data_as(C.POINTER(C.c_int8)), None,
                                                               None), "get_polish_repair_trace")
            out.active = cls.astype(np.int64)
        return out

    def polish_many(self, q, l, u, x, y, delta=1e-6, refine_iter=3, repair_iter=0):
        """B polishes in ONE launch, one workgroup per instance (miosqp_qp_polish_many): q, x B x n (q None: the engine's
        current linear cost for every instance), l, u, y B x M.  Instance b is answered as
        `update(q=q[b])` + `polish(l[b], u[b], x[b], y[b], delta, refine_iter, repair_iter=repair_iter)` would, up to the
        order of the sums, without touching the engine's q.  Returns a list of B records shaped like
        `polish(..., repair_iter=)`'s, `active` included (device_time / run_time are the call's totals), or None when the
        problem is beyond what one workgroup holds."""
        return self._polish_many("polish_many", q, l, u, x, y, delta, refine_iter, repair_iter)

    def polish_many_large(self, q, l, u, x, y, delta=1e-6, refine_iter=3, repair_iter=0):
        """`polish_many` beyond one workgroup's LDS (miosqp_qp_polish_many_large): the same arguments, the same records,
        the same contract per instance up to the order of the sums; an instance's reduced matrix lives in a slab of
        device scratch, min(B, 2 x compute units, 1 GiB / slab) workgroups take the instances in turn.  No lower size
        limit; None for n > 512 or M > 65536."""
        return self._polish_many("polish_many_large", q, l, u, x, y, delta, refine_iter, repair_iter)

    def _polish_many(self, entry, q, l, u, x, y, delta, refine_iter, repair_iter):
        run = getattr(self._lib, "miosqp_qp_" + entry)
        get_classes = getattr(self._lib, "miosqp_qp_get_%s_classes" % entry)
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim != 2:
            raise ValueError(entry + ": instance-major arrays (B x n, B x M)")
        B = x.shape[0]
        l, u = np.ascontiguousarray(l, dtype=np.float64), np.ascontiguousarray(u, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        q = None if q is None else np.ascontiguousarray(q, dtype=np.float64)
        if x.shape != (B, self.n) or l.shape != (B, self.m) or u.shape != (B, self.m) or y.shape != (B, self.m) or \
                (q is not None and q.shape != (B, self.n)):
            raise ValueError(entry + ": instance-major arrays (B x n, B x M)")
        xo, yo = np.empty((B, self.n)), np.empty((B, self.m))
        infos = (_lib.PolishRepairInfo * max(B, 1))()
        rc = run(self._h, B, None if q is None else _lib.as_d(q), _lib.as_d(l), _lib.as_d(u), _lib.as_d(x), _lib.as_d(y),
                 float(delta), int(refine_iter), int(repair_iter), _lib.as_d(xo), _lib.as_d(yo), infos)
        if rc == -5:
            return None
        _check(rc, entry)
        if rc == 1:
            raise ValueError("Lower bound must be lower than or equal to upper bound")
        out = []
        for b in range(B):
            rep, info = infos[b], infos[b].polish
            cls = np.zeros(self.m, dtype=np.int8)
            _check(get_classes(self._h, b, cls.ctypes.data_as(C.POINTER(C.c_int8))), "get_%s_classes" % entry)
            out.append(types.SimpleNamespace(
                x=xo[b].copy(), y=yo[b].copy(), accepted=bool(info.accepted), reason=info.reason, n_lower=info.n_lower,
                n_upper=info.n_upper, pri_before=info.pri_before, dua_before=info.dua_before, pri_after=info.pri_after,
                dua_after=info.dua_after, obj=info.obj, device_time=info.device_time, run_time=info.run_time,
                rounds=rep.rounds, stop=rep.stop, n_added=rep.n_added, n_dropped=rep.n_dropped,
                accepted0=bool(rep.accepted0), reason0=rep.reason0, active=cls.astype(np.int64)))
        return out

    def polish_models_large_fits(self):
        """whether `qp.polish_models_large` takes this engine's sizes (miosqp_qp_polish_models_large_fits)"""
        return bool(self._lib.miosqp_qp_polish_models_large_fits(self._h))

    def polish_models_fits(self):
        """whether `qp.polish_models` takes this engine's sizes (miosqp_qp_polish_models_fits)"""
        return bool(self._lib.miosqp_qp_polish_models_fits(self._h))

    def polish_rounds(self):
        """Of the last polish call with repair_iter: per round (round 0 first, 21 entries, zeros for rounds not run) the
        device seconds up to the revision's counters, and the host's wait for them."""
        dev, wait = np.zeros(21), np.zeros(21)
        _check(self._lib.miosqp_qp_get_polish_repair_trace(self._h, None, _lib.as_d(dev), _lib.as_d(wait)),
               "get_polish_repair_trace")
        return dev, wait

    def polish_stages(self):
        """Device seconds of the last polish call: classification, rows of the reduced matrix, factorisation, solves."""
        out = np.zeros(4)
        _check(self._lib.miosqp_qp_get_polish_stages(self._h, _lib.as_d(out)), "get_polish_stages")
        return tuple(float(v) for v in out)

    def solve_tree(self, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb):
        """A whole tree search in one launch (small problems); None when the engine does not cover this size."""
        l, u = _f64(l, self.m, "l"), _f64(u, self.m, "u")
        x0, y0 = _f64(x0, self.n, "x0"), _f64(y0, self.m, "y0")
        have = x_inc0 is not None and np.isfinite(upper0)
        xin = _f64(x_inc0, self.n, "x_inc0") if have else None
        x, info = np.empty(self.n), _lib.TreeInfo()
        # the launch counts nodes in 32 bits; the reference accepts any number here (also inf): clamp
        max_iter_bb = 2 ** 31 - 1 if not np.isfinite(max_iter_bb) else int(min(int(max_iter_bb), 2 ** 31 - 1))
        rc = self._lib.miosqp_qp_solve_tree(self._h, _lib.as_d(l), _lib.as_d(u), _lib.as_d(x0), _lib.as_d(y0),
                                            float(upper0) if have else float("inf"), _lib.as_d(xin) if have else None,
                                            int(tree_explor_rule), int(max_iter_bb), _lib.as_d(x), C.byref(info))
        if rc == -5:
            return None
        _check(rc, "solve_tree")
        if rc == 1:
            raise ValueError("Lower bound must be lower than or equal to upper bound")
        return types.SimpleNamespace(x=x, info=info)

    def solve_trees(self, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb):
        """B MIQPs on this engine's factor (q, l, u, x0, y0 instance-major: B x n / B x M), every tree in one launch.
        upper0: B incumbent values (inf: none), x_inc0: B x n or None.  Returns (x B x n, [TreeInfo]) or None when the
        engine does not cover this size."""
        q = np.ascontiguousarray(q, dtype=np.float64)
        B = q.shape[0]
        l, u = np.ascontiguousarray(l, dtype=np.float64), np.ascontiguousarray(u, dtype=np.float64)
        x0, y0 = np.ascontiguousarray(x0, dtype=np.float64), np.ascontiguousarray(y0, dtype=np.float64)
        if q.shape != (B, self.n) or x0.shape != (B, self.n) or l.shape != (B, self.m) or u.shape != (B, self.m) or y0.shape != (B, self.m):
            raise ValueError("solve_trees: instance-major arrays (B x n, B x M)")
        up = np.minimum(np.ascontiguousarray(upper0, dtype=np.float64).reshape(B), 1.7e308)
        xin = None if x_inc0 is None else np.ascontiguousarray(x_inc0, dtype=np.float64).reshape(B, self.n)
        x = np.zeros((B, self.n))
        infos = (_lib.TreeInfo * B)()
        max_iter_bb = 2 ** 31 - 1 if not np.isfinite(max_iter_bb) else int(min(int(max_iter_bb), 2 ** 31 - 1))
        rc = self._lib.miosqp_qp_solve_trees(self._h, B, _lib.as_d(q), _lib.as_d(l), _lib.as_d(u), _lib.as_d(x0), _lib.as_d(y0),
                                             _lib.as_d(up), None if xin is None else _lib.as_d(xin), int(tree_explor_rule),
                                             max_iter_bb, _lib.as_d(x), infos)
        if rc == -5:
            return None
        _check(rc, "solve_trees")
        if rc == 1:
            raise ValueError("Lower bound must be lower than or equal to upper bound")
        return x, list(infos)

    def solve_trees_rf(self, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, rf_candidates, rf_max_iter,
                       rf_every):
        """`solve_trees` with round and fix inside every tree (miosqp_qp_solve_trees_rf, `Workspace.primal_heuristic`):
        on every rf_every-th node a tree is about to branch (the first included) its workgroup solves rf_candidates
        rounded-and-fixed copies of the node, at most rf_max_iter iterations each, and adopts the best feasible one below
        the incumbent.  One workgroup per instance, also for n + M <= 64.  rf_candidates in 1..32, rf_max_iter >= 1,
        rf_every >= 1 (RuntimeError with the library's text otherwise).  Returns (x B x n, [TreeInfo], [TreeRfInfo]) --
        TreeInfo.osqp_iter counts the nodes' iterations, TreeRfInfo has calls, candidates, feasible, improved, osqp_iter
        per instance -- or None when the engine does not cover this size."""
        q = np.ascontiguousarray(q, dtype=np.float64)
        B = q.shape[0]
        l, u = np.ascontiguousarray(l, dtype=np.float64), np.ascontiguousarray(u, dtype=np.float64)
        x0, y0 = np.ascontiguousarray(x0, dtype=np.float64), np.ascontiguousarray(y0, dtype=np.float64)
        if q.shape != (B, self.n) or x0.shape != (B, self.n) or l.shape != (B, self.m) or u.shape != (B, self.m) or y0.shape != (B, self.m):
            raise ValueError("solve_trees_rf: instance-major arrays (B x n, B x M)")
        up = np.minimum(np.ascontiguousarray(upper0, dtype=np.float64).reshape(B), 1.7e308)
        xin = None if x_inc0 is None else np.ascontiguousarray(x_inc0, dtype=np.float64).reshape(B, self.n)
        x = np.zeros((B, self.n))
        infos = (_lib.TreeInfo * B)()
        rfs = (_lib.TreeRfInfo * B)()
        max_iter_bb = 2 ** 31 - 1 if not np.isfinite(max_iter_bb) else int(min(int(max_iter_bb), 2 ** 31 - 1))
        rc = self._lib.miosqp_qp_solve_trees_rf(self._h, B, _lib.as_d(q), _lib.as_d(l), _lib.as_d(u), _lib.as_d(x0),
                                                _lib.as_d(y0), _lib.as_d(up), None if xin is None else _lib.as_d(xin),
                                                int(tree_explor_rule), max_iter_bb, int(rf_candidates), int(rf_max_iter),
                                                int(rf_every), _lib.as_d(x), infos, rfs)
        if rc == -5:
            return None
        _check(rc, "solve_trees_rf")
        if rc == 1:
            raise ValueError("Lower bound must be lower than or equal to upper bound")
        return x, list(infos), list(rfs)

    def solve_trees_sb(self, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, branching_rule, sb_candidates,
                       sb_max_iter, sb_reliability, sb_eps):
        """`solve_trees` with strong (branching_rule 1) or reliability branching (2) inside every tree
        (miosqp_qp_solve_trees_sb, `Workspace.select_branching`): a node that is about to branch has its workgroup solve
        the 2K children of its candidates, at most sb_max_iter iterations each, and branches on the position the rule
        picks; rule 2 keeps pseudo-costs per tree, starting empty.  One workgroup per instance, also for n + M <= 64.
        sb_candidates in 1..32, sb_max_iter >= 1, sb_reliability >= 0, sb_eps > 0 (RuntimeError with the library's text
        otherwise).  Returns (x B x n, [TreeInfo], [TreeSbInfo]) -- TreeInfo.osqp_iter counts the nodes' iterations,
        TreeSbInfo has calls, children, osqp_iter per instance -- or None when the engine does not cover this size."""
        q = np.ascontiguousarray(q, dtype=np.float64)
        B = q.shape[0]
        l, u = np.ascontiguousarray(l, dtype=np.float64), np.ascontiguousarray(u, dtype=np.float64)
        x0, y0 = np.ascontiguousarray(x0, dtype=np.float64), np.ascontiguousarray(y0, dtype=np.float64)
        if q.shape != (B, self.n) or x0.shape != (B, self.n) or l.shape != (B, self.m) or u.shape != (B, self.m) or y0.shape != (B, self.m):
            raise ValueError("solve_trees_sb: instance-major arrays (B x n, B x M)")
        up = np.minimum(np.ascontiguousarray(upper0, dtype=np.float64).reshape(B), 1.7e308)
        xin = None if x_inc0 is None else np.ascontiguousarray(x_inc0, dtype=np.float64).reshape(B, self.n)
        x = np.zeros((B, self.n))
        infos = (_lib.TreeInfo * B)()
        sbs = (_lib.TreeSbInfo * B)()
        max_iter_bb = 2 ** 31 - 1 if not np.isfinite(max_iter_bb) else int(min(int(max_iter_bb), 2 ** 31 - 1))
        rc = self._lib.miosqp_qp_solve_trees_sb(self._h, B, _lib.as_d(q), _lib.as_d(l), _lib.as_d(u), _lib.as_d(x0),
                                                _lib.as_d(y0), _lib.as_d(up), None if xin is None else _lib.as_d(xin),
                                                int(tree_explor_rule), max_iter_bb, int(branching_rule), int(sb_candidates),
                                                int(sb_max_iter), int(sb_reliability), float(sb_eps), _lib.as_d(x), infos, sbs)
        if rc == -5:
            return None
        _check(rc, "solve_trees_sb")
        if rc == 1:
            raise ValueError("Lower bound must be lower than or equal to upper bound")
        return x, list(infos), list(sbs)

    def tree_form(self):
        """Which one-launch tree kernel takes this engine (miosqp_qp_tree_form): 0 none -- `solve_trees` would return
        None --, 1 one wavefront (n + M <= 64), 2 one workgroup.  Builds what the first tree launch would build."""
        if self._h is None:
            return 0
        return int(self._lib.miosqp_qp_tree_form(self._h))

    def tree_form_large(self, leaf_cap=256):
        """3 when `solve_trees_models(..., leaf_cap=leaf_cap)` runs this engine's tree in the reduced form
        (miosqp_qp_tree_form_large): `tree_form()` is 0, the engine has its integer rows, root, digest and product-form
        rows, and the packed triangle of L^-1, the iterates and a leaf list of leaf_cap places fit 160 KB of LDS; else 0."""
        if self._h is None:
            return 0
        return int(self._lib.miosqp_qp_tree_form_large(self._h, int(leaf_cap)))

    def _trees_large_args(self, who, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, leaf_cap):
        """the arrays of solve_trees, checked and laid out, for the three entries of solve_trees_large"""
        q = np.ascontiguousarray(q, dtype=np.float64)
        B = q.shape[0]
        l, u = np.ascontiguousarray(l, dtype=np.float64), np.ascontiguousarray(u, dtype=np.float64)
        x0, y0 = np.ascontiguousarray(x0, dtype=np.float64), np.ascontiguousarray(y0, dtype=np.float64)
        if q.shape != (B, self.n) or x0.shape != (B, self.n) or l.shape != (B, self.m) or u.shape != (B, self.m) or y0.shape != (B, self.m):
            raise ValueError("%s: instance-major arrays (B x n, B x M)" % who)
        if isinstance(leaf_cap, bool) or int(leaf_cap) != leaf_cap or leaf_cap < 2:
            raise ValueError("%s: leaf_cap must be an integer of at least 2" % who)
        up = np.minimum(np.ascontiguousarray(upper0, dtype=np.float64).reshape(B), 1.7e308)
        xin = None if x_inc0 is None else np.ascontiguousarray(x_inc0, dtype=np.float64).reshape(B, self.n)
        max_iter_bb = 2 ** 31 - 1 if not np.isfinite(max_iter_bb) else int(min(int(max_iter_bb), 2 ** 31 - 1))
        keep = (q, l, u, x0, y0, up, xin)  # (the arrays behind the pointers live as long as the call)
        head = (self._h, B, _lib.as_d(q), _lib.as_d(l), _lib.as_d(u), _lib.as_d(x0), _lib.as_d(y0), _lib.as_d(up),
                None if xin is None else _lib.as_d(xin), int(tree_explor_rule), max_iter_bb, int(leaf_cap))
        return types.SimpleNamespace(B=B, head=head, keep=keep, x=np.zeros((B, self.n)), infos=(_lib.TreeInfo * B)())

    def _trees_large_done(self, who, rc, *ret):
        if rc == -5:
            return None
        _check(rc, who)
        if rc == 1:
            raise ValueError("Lower bound must be lower than or equal to upper bound")
        return tuple(ret)

    def solve_trees_large(self, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, leaf_cap=256):
        """`solve_trees` for an engine BEYOND one workgroup's product form (miosqp_qp_solve_trees_large): `tree_form()` is 0
        and `tree_form_large(leaf_cap)` is 3.  B MIQPs on this engine's factor, every tree in one launch, one workgroup
        per instance in the reduced form (the packed triangle of L^-1 in LDS) with a leaf list of leaf_cap places (an int
        >= 2; ValueError otherwise); the factor, Abar and the scalings are read by all workgroups from the engine's own
        arrays.  Arrays and return as `solve_trees`: (x B x n, [TreeInfo]) -- instance b bit for bit what
        `solve_trees_models([self], ..., leaf_cap=leaf_cap)` gives it alone; TreeInfo.overflow marks a tree that needed
        more than leaf_cap leaves at once -- or None when the library declines (another form takes the engine, or none).
        RuntimeError with the library's text when the arrays of B instances are beyond what the device has free."""
        t = self._trees_large_args("solve_trees_large", q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, leaf_cap)
        rc = self._lib.miosqp_qp_solve_trees_large(*t.head, _lib.as_d(t.x), t.infos)
        return self._trees_large_done("solve_trees_large", rc, t.x, list(t.infos))

    def solve_trees_large_rf(self, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, rf_candidates, rf_max_iter,
                             rf_every, leaf_cap=256):
        """`solve_trees_rf` for an engine beyond one workgroup's product form (miosqp_qp_solve_trees_large_rf; see
        `solve_trees_large`): round and fix inside every tree of the reduced form.  Returns (x B x n, [TreeInfo],
        [TreeRfInfo]) -- instance b and its counters as `solve_trees_models([self], ..., leaf_cap=leaf_cap, rf=...)` gives
        them alone -- or None when the library declines."""
        t = self._trees_large_args("solve_trees_large_rf", q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb,
                                   leaf_cap)
        rfs = (_lib.TreeRfInfo * t.B)()
        rc = self._lib.miosqp_qp_solve_trees_large_rf(*t.head, int(rf_candidates), int(rf_max_iter), int(rf_every),
                                                      _lib.as_d(t.x), t.infos, rfs)
        return self._trees_large_done("solve_trees_large_rf", rc, t.x, list(t.infos), list(rfs))

    def solve_trees_large_sb(self, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, branching_rule,
                             sb_candidates, sb_max_iter, sb_reliability, sb_eps, leaf_cap=256):
        """`solve_trees_sb` for an engine beyond one workgroup's product form (miosqp_qp_solve_trees_large_sb; see
        `solve_trees_large`): strong (branching_rule 1) or reliability branching (2) inside every tree of the reduced
        form.  Returns (x B x n, [TreeInfo], [TreeSbInfo]) -- instance b and its counters as
        `solve_trees_models([self], ..., leaf_cap=leaf_cap, sb=...)` gives them alone -- or None when the library
        declines."""
        t = self._trees_large_args("solve_trees_large_sb", q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb,
                                   leaf_cap)
        sbs = (_lib.TreeSbInfo * t.B)()
        rc = self._lib.miosqp_qp_solve_trees_large_sb(*t.head, int(branching_rule), int(sb_candidates), int(sb_max_iter),
                                                      int(sb_reliability), float(sb_eps), _lib.as_d(t.x), t.infos, sbs)
        return self._trees_large_done("solve_trees_large_sb", rc, t.x, list(t.infos), list(sbs))

    def solve_trees_lockstep(self, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, capacity=0,
                             node_hviol=0):
        """B MIQPs on this engine's factor for problems of any size (arrays as for solve_trees): the trees advance in lock
        step, one node of every unfinished tree per wave, driven in C++ on device-resident leaves
        (miosqp_qp_solve_trees_lockstep).  capacity: starting number of node slots (0: the engine's default).
        node_hviol: debug, > 0 records the rounded point's violation at each tree's first `node_hviol` nodes.
        Returns (x B x n, [TreeInfo], stats): stats has waves, nodes, max_width, grown, iters_slowest, iters_all,
        device_time, run_time, host_time (the tree logic between the waves), the per-wave lists width, iters_max, iters_mean (the first 65536 waves), finished_at
        (per instance) and node_hviol (B x node_hviol, NaN where there was no node; None when not asked for)."""
        return self._trees_lockstep(q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, capacity, node_hviol, None)

    def solve_trees_lockstep_rf(self, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, rf_candidates,
                                rf_max_iter, rf_every, capacity=0, first_call=False):
        """solve_trees_lockstep with round and fix inside the trees (miosqp_qp_solve_trees_lockstep_rf): on every
        rf_every-th fractional node a tree is about to branch (the first included) rf_candidates rounded-and-fixed copies
        of the node, at most rf_max_iter iterations each; the candidates of all trees that fire in a wave are ONE more
        batch, built, solved and judged on the device.  rf_candidates in 1..32, rf_max_iter a positive multiple of
        check_termination or max_iter, rf_every >= 1 (ValueError otherwise).
        Returns (x, [TreeInfo], stats, rf): stats as solve_trees_lockstep's (TreeInfo.osqp_iter and the iteration counts
        there are the node relaxations'), rf has batches, columns, iters_slowest, device_time and per instance calls,
        candidates, feasible, improved, iters (lists).  first_call: debug, rf.first_call is then a namespace of
        B x rf_candidates arrays status, iter, obj, viol -- the candidates of every tree's first call as
        `round_and_fix` reports them (status -1 and NaN for a tree that never fired); None otherwise."""
        return self._trees_lockstep(q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, capacity, 0,
                                    (int(rf_candidates), int(rf_max_iter), int(rf_every), bool(first_call)))

    def solve_trees_lockstep_sb(self, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, branching_rule,
                                sb_candidates, sb_max_iter, sb_reliability, sb_eps, capacity=0, first_call=False):
        """solve_trees_lockstep with strong (branching_rule 1) or reliability branching (2) inside the trees
        (miosqp_qp_solve_trees_lockstep_sb): every node that branches chooses its position as
        `Workspace.select_branching` does; the 2K children of all nodes with candidates in a wave are ONE more batch,
        built, solved (at most sb_max_iter iterations each) and read off on the device.  sb_candidates in 1..32,
        sb_max_iter a positive multiple of check_termination, sb_reliability >= 0, sb_eps > 0 (ValueError otherwise).
        Returns (x, [TreeInfo], stats, sb): stats as solve_trees_lockstep's (TreeInfo.osqp_iter and the iteration counts
        there are the node relaxations'), sb has batches, columns, iters_slowest, device_time and per instance calls,
        children, iters (lists).  first_call: debug, sb.first_call is then a namespace of k, chosen (B), cand
        (B x sb_candidates), status, iter, lower (B x 2 sb_candidates: K down then K up in the first 2K entries) --
        every tree's first call as `strong_branch` reports it (k = 0 for a tree that never called); None otherwise."""
        return self._trees_lockstep(q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, capacity, 0, None,
                                    (int(branching_rule), int(sb_candidates), int(sb_max_iter), int(sb_reliability),
                                     float(sb_eps), bool(first_call)))

    # -- what the five tree drivers of the library share on this side ---------------------------------
    def _trees_args(self, who, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, capacity):
        """The drivers' common arguments, normalised: instance-major float64 arrays (ValueError otherwise), upper0 capped
        at what the library reads as "none", max_iter_bb clamped to 32 bits; x and infos for the call to fill.  `head`
        is the C argument list up to `capacity`; `keep` holds the arrays it points into."""
        q = np.ascontiguousarray(q, dtype=np.float64)
        B = q.shape[0]
        l, u = np.ascontiguousarray(l, dtype=np.float64), np.ascontiguousarray(u, dtype=np.float64)
        x0, y0 = np.ascontiguousarray(x0, dtype=np.float64), np.ascontiguousarray(y0, dtype=np.float64)
        if B < 1 or q.shape != (B, self.n) or x0.shape != (B, self.n) or l.shape != (B, self.m) or u.shape != (B, self.m) \
                or y0.shape != (B, self.m):
            raise ValueError(who + ": instance-major arrays (B x n, B x M)")
        up = np.minimum(np.ascontiguousarray(upper0, dtype=np.float64).reshape(B), 1.7e308)
        xin = None if x_inc0 is None else np.ascontiguousarray(x_inc0, dtype=np.float64).reshape(B, self.n)
        max_iter_bb = 2 ** 31 - 1 if not np.isfinite(max_iter_bb) else int(min(int(max_iter_bb), 2 ** 31 - 1))
        head = (self._h, B, _lib.as_d(q), _lib.as_d(l), _lib.as_d(u), _lib.as_d(x0), _lib.as_d(y0), _lib.as_d(up),
                None if xin is None else _lib.as_d(xin), int(tree_explor_rule), max_iter_bb, int(capacity))
        return types.SimpleNamespace(B=B, max_iter_bb=max_iter_bb, head=head, keep=(q, l, u, x0, y0, up, xin),
                                     x=np.zeros((B, self.n)), infos=(_lib.TreeInfo * B)())

    @staticmethod
    def _trees_refused(rc):
        """rc 1 of a tree driver: a root with l > u (nothing was queued), or a branching that produced l > u"""
        if rc == 1:
            if "branching" in _lib.last_error():
                raise RuntimeError("branching produced l > u")
            raise ValueError("Lower bound must be lower than or equal to upper bound")

    @staticmethod
    def _lockstep_stats_in(t, node_hviol=0):
        """(LockstepStats, its arrays): per wave (the first 65536), per instance, and node_hviol where asked for"""
        wcap = max(1, min(t.max_iter_bb, 65536))
        buf = types.SimpleNamespace(wcap=wcap, width=np.zeros(wcap, dtype=np.int32), imax=np.zeros(wcap, dtype=np.int32),
                                    imean=np.zeros(wcap), fin=np.zeros(t.B, dtype=np.int32),
                                    hv=np.full((t.B, int(node_hviol)), np.nan) if node_hviol > 0 else None)
        st = _lib.LockstepStats()
        st.wave_cap = wcap
        st.wave_width, st.wave_iter_max, st.wave_iter_mean = _lib.as_i(buf.width), _lib.as_i(buf.imax), _lib.as_d(buf.imean)
        st.finished_at = _lib.as_i(buf.fin)
        if buf.hv is not None:
            st.node_hviol, st.node_cap = _lib.as_d(buf.hv), int(node_hviol)
        return st, buf

    @staticmethod
    def _lockstep_stats(st, buf):
        """the `stats` namespace of the wave drivers from a filled LockstepStats"""
        k = min(st.waves, buf.wcap)
        return types.SimpleNamespace(
            waves=st.waves, nodes=st.nodes, max_width=st.max_width, grown=st.grown, iters_slowest=st.iters_slowest,
            iters_all=st.iters_all, device_time=st.device_time, run_time=st.run_time, host_time=st.host_time,
            width=buf.width[:k].tolist(), iters_max=buf.imax[:k].tolist(), iters_mean=buf.imean[:k].tolist(),
            finished_at=buf.fin.tolist(), node_hviol=buf.hv)

    def _trees_lockstep(self, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, capacity, node_hviol, rf,
                        sb=None):
        who = "solve_trees_lockstep" if rf is None else "solve_trees_lockstep_rf"
        if sb is not None:
            who = "solve_trees_lockstep_sb"
        t = self._trees_args(who, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, capacity)
        B = t.B
        st, buf = self._lockstep_stats_in(t, node_hviol)
        if sb is not None:
            cnt = [np.zeros(B, dtype=np.int32) for _ in range(2)]
            sb_it = np.zeros(B, dtype=np.int64)
            bs = _lib.LockstepSbStats()
            bs.calls, bs.children = (_lib.as_i(a) for a in cnt)
            bs.iters = sb_it.ctypes.data_as(_lib.i64p)
            first = None
            if sb[5]:
                Kc = max(sb[1], 1)
                first = types.SimpleNamespace(k=np.zeros(B, dtype=np.int32), chosen=np.full(B, -1, dtype=np.int32),
                                              cand=np.full((B, Kc), -1, dtype=np.int32),
                                              status=np.full((B, 2 * Kc), -1, dtype=np.int32),
                                              iter=np.zeros((B, 2 * Kc), dtype=np.int32), lower=np.full((B, 2 * Kc), np.nan))
                bs.first_k, bs.first_chosen, bs.first_cand = _lib.as_i(first.k), _lib.as_i(first.chosen), _lib.as_i(first.cand)
                bs.first_status, bs.first_iter, bs.first_lower = _lib.as_i(first.status), _lib.as_i(first.iter), \
                    _lib.as_d(first.lower)
            rc = self._lib.miosqp_qp_solve_trees_lockstep_sb(*t.head, sb[0], sb[1], sb[2], sb[3], sb[4], _lib.as_d(t.x), t.infos,
                                                             C.byref(st), C.byref(bs))
            if rc == -1 and "solve_trees_lockstep_sb: " in _lib.last_error() and \
                    any(w in _lib.last_error() for w in ("branching_rule", "sb_")):
                raise ValueError(_lib.last_error())
        elif rf is None:
            rc = self._lib.miosqp_qp_solve_trees_lockstep(*t.head, _lib.as_d(t.x), t.infos, C.byref(st))
        else:
            cnt = [np.zeros(B, dtype=np.int32) for _ in range(4)]
            rf_it = np.zeros(B, dtype=np.int64)
            rs = _lib.LockstepRfStats()
            rs.calls, rs.candidates, rs.feasible, rs.improved = (_lib.as_i(a) for a in cnt)
            rs.iters = rf_it.ctypes.data_as(_lib.i64p)
            first = None
            if rf[3]:
                Kc = max(rf[0], 1)
                first = types.SimpleNamespace(status=np.full((B, Kc), -1, dtype=np.int32), iter=np.zeros((B, Kc), dtype=np.int32),
                                              obj=np.full((B, Kc), np.nan), viol=np.full((B, Kc), np.nan))
                rs.cand_status, rs.cand_iter = _lib.as_i(first.status), _lib.as_i(first.iter)
                rs.cand_obj, rs.cand_viol = _lib.as_d(first.obj), _lib.as_d(first.viol)
            rc = self._lib.miosqp_qp_solve_trees_lockstep_rf(*t.head, rf[0], rf[1], rf[2], _lib.as_d(t.x), t.infos, C.byref(st),
                                                             C.byref(rs))
            if rc == -1 and "solve_trees_lockstep_rf: rf_" in _lib.last_error():
                raise ValueError(_lib.last_error())
        _check(rc, who)
        self._trees_refused(rc)
        stats = self._lockstep_stats(st, buf)
        if sb is not None:
            sbs = types.SimpleNamespace(
                batches=bs.batches, columns=bs.columns, iters_slowest=bs.iters_slowest, device_time=bs.device_time,
                calls=cnt[0].tolist(), children=cnt[1].tolist(), iters=sb_it.tolist(), first_call=first)
            return t.x, list(t.infos), stats, sbs
        if rf is not None:
            rfs = types.SimpleNamespace(
                batches=rs.batches, columns=rs.columns, iters_slowest=rs.iters_slowest, device_time=rs.device_time,
                calls=cnt[0].tolist(), candidates=cnt[1].tolist(), feasible=cnt[2].tolist(), improved=cnt[3].tolist(),
                iters=rf_it.tolist(), first_call=first)
            return t.x, list(t.infos), stats, rfs
        return t.x, list(t.infos), stats

    def solve_trees_lockstep_ahead(self, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, ahead, capacity=0):
        """solve_trees_lockstep (same arrays) with the spare columns of every wave solving open leaves early
        (miosqp_qp_solve_trees_lockstep_ahead): a tree may hold up to `ahead` columns of a wave -- its chosen leaf and,
        in the free columns of the tiles the wave launches anyway, other open leaves and children of nodes solved
        ahead --, keeps those records until its exploration rule reaches the node and drops them when a pruning removes
        it.  Results are solve_trees_lockstep's bit for bit; ahead = 1 runs its launches.  ahead >= 1 (ValueError
        otherwise).
        Returns (x B x n, [TreeInfo], stats, ahead): stats as solve_trees_lockstep's (width counts all columns, the
        iteration figures the mandatory columns; node_hviol None), ahead has waves, columns, sent, hits, discarded,
        called_off, hit_iters, discarded_iters, called_off_iters, free_slots, slot_cap and per wave (the first 65536)
        width, iter_mandatory, chunks."""
        who = "solve_trees_lockstep_ahead"
        if int(ahead) != ahead or int(ahead) < 1:
            raise ValueError(who + ": ahead must be at least 1")
        t = self._trees_args(who, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, capacity)
        st, buf = self._lockstep_stats_in(t)
        awidth, amand, achunks = (np.zeros(buf.wcap, dtype=np.int32) for _ in range(3))
        ah = _lib.LockstepAheadStats()
        ah.wave_cap = buf.wcap
        ah.wave_width, ah.wave_iter_mandatory, ah.wave_chunks = _lib.as_i(awidth), _lib.as_i(amand), _lib.as_i(achunks)
        rc = self._lib.miosqp_qp_solve_trees_lockstep_ahead(*t.head, int(ahead), _lib.as_d(t.x), t.infos, C.byref(st), C.byref(ah))
        _check(rc, who)
        self._trees_refused(rc)
        k = min(st.waves, buf.wcap)
        ahs = types.SimpleNamespace(
            waves=ah.waves, columns=ah.columns, sent=ah.sent, hits=ah.hits, discarded=ah.discarded, called_off=ah.called_off,
            hit_iters=ah.hit_iters, discarded_iters=ah.discarded_iters, called_off_iters=ah.called_off_iters,
            free_slots=ah.free_slots, slot_cap=ah.slot_cap, width=awidth[:k].tolist(), iter_mandatory=amand[:k].tolist(),
            chunks=achunks[:k].tolist())
        return t.x, list(t.infos), self._lockstep_stats(st, buf), ahs

    def solve_trees_refill(self, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, capacity=0):
        """The trees of solve_trees_lockstep (same arrays) on columns that are refilled between chunks
        (miosqp_qp_solve_trees_refill): a column holds one node of one tree, every tree has at most one node in flight, and
        at every chunk boundary the decided columns are harvested and loaded again with the next leaf of a waiting tree.
        capacity: starting number of node slots (0: the engine's default).  Needs max_iter to be a multiple of
        check_termination (ValueError otherwise).
        Returns (x B x n, [TreeInfo], stats): stats has chunks, nodes, columns, grown, iters_all, busy and total
        (column-chunks: busy / total is the occupancy), device_time, run_time, host_time (the tree logic between the
        chunks), chunk_time (device seconds inside the chunks), nodes_max_iter and iters_max_iter (the nodes that ended
        MAX_ITER_REACHED and their iterations), chunk_busy (busy columns per chunk, the first 65536) and
        finished_at (per instance, a chunk number)."""
        t = self._trees_args("solve_trees_refill", q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, capacity)
        ccap = 65536
        busy, fin = np.zeros(ccap, dtype=np.int32), np.zeros(t.B, dtype=np.int32)
        st = _lib.RefillStats()
        st.chunk_cap = ccap
        st.chunk_busy, st.finished_at = _lib.as_i(busy), _lib.as_i(fin)
        rc = self._lib.miosqp_qp_solve_trees_refill(*t.head, _lib.as_d(t.x), t.infos, C.byref(st))
        if rc == -1 and "multiple of check_termination" in _lib.last_error():
            raise ValueError("solve_trees_refill: max_iter must be a multiple of check_termination")
        _check(rc, "solve_trees_refill")
        self._trees_refused(rc)
        stats = types.SimpleNamespace(
            chunks=st.chunks, nodes=st.nodes, columns=st.columns, grown=st.grown, iters_all=st.iters_all,
            busy=st.col_chunks_busy, total=st.col_chunks_total, device_time=st.device_time, run_time=st.run_time,
            host_time=st.host_time, chunk_time=st.chunk_time, nodes_max_iter=st.nodes_max_iter,
            iters_max_iter=st.iters_max_iter, chunk_busy=busy[:min(st.chunks, ccap)].tolist(),
            finished_at=fin.tolist())
        return t.x, list(t.infos), stats

    # -- node-at-a-time branch and bound driven from the host in C++ (miosqp_qp_search_*) --------------
    def search_create(self, capacity):
        _check(self._lib.miosqp_qp_search_create(self._h, int(capacity)), "search_create")
        self._search_info = _lib.SearchInfo()

    def search_reset(self):
        _check(self._lib.miosqp_qp_search_reset(self._h), "search_reset")

    def search_add_leaf(self, l_int, u_int, x0, y0, depth, lower):
        k = len(l_int)
        rc = _check(self._lib.miosqp_qp_search_add_leaf(
            self._h, _vec(l_int, k, "l_int"), _vec(u_int, k, "u_int"), _vec(x0, self.n, "x0"), _vec(y0, self.m, "y0"),
            int(depth), float(lower)), "search_add_leaf")
        if rc == 1:
            raise ValueError("Lower bound must be lower than or equal to upper bound")

    def search_take_leaf(self, n_int, into=None):
        """(l_int, u_int, x0, y0, depth, lower) of the shallowest open leaf, removed from the list; None if none.
        into: four DevicePtr (l_int, u_int, x0, y0) the vectors are copied to instead (device to device)."""
        l, u, x, y = into if into is not None else (np.empty(n_int), np.empty(n_int), np.empty(self.n), np.empty(self.m))
        depth, lower = C.c_int32(), C.c_double()
        rc = _check(self._lib.miosqp_qp_search_take_leaf(self._h, _vec(l, n_int, "l_int"), _vec(u, n_int, "u_int"),
                                                         _vec(x, self.n, "x0"), _vec(y, self.m, "y0"),
                                                         C.byref(depth), C.byref(lower)), "search_take_leaf")
        return None if rc == 1 else (l, u, x, y, depth.value, lower.value)

    def search_set_incumbent(self, upper, x):
        """x None: only the VALUE of the incumbent the search already holds is replaced (a rounding-heuristic value
        recomputed on the host, see SearchInfo.improved == 2)."""
        _check(self._lib.miosqp_qp_search_set_incumbent(self._h, float(upper),
                                                        None if x is None else _lib.as_d(_f64(x, self.n, "x"))),
               "search_set_incumbent")

    def search_get_incumbent(self):
        """(upper, x); x is None while there is no incumbent."""
        upper, x = C.c_double(), np.empty(self.n)
        _check(self._lib.miosqp_qp_search_get_incumbent(self._h, C.byref(upper), _lib.as_d(x)), "search_get_incumbent")
        return (upper.value, x) if upper.value < 1.7e308 else (float("inf"), None)

    def search_run(self, tree_explor_rule, max_nodes, budget_s=0.0):
        """Returns the info record; `info.full` is set when the slot store could not grow any further (the device is
        out of memory): the counters of the nodes done in this call are valid, the caller decides what to do."""
        info = self._search_info
        max_nodes = 2 ** 62 if not np.isfinite(max_nodes) else int(min(int(max_nodes), 2 ** 62))
        rc = self._lib.miosqp_qp_search_run(self._h, int(tree_explor_rule), max_nodes, float(budget_s), C.byref(info))
        info.full = rc == -6
        if not info.full:
            _check(rc, "search_run")
        return info

    # -- the host side of the streaming search, compiled (miosqp_qp_stream_*) ---------------------------
    def stream_create(self, capacity, columns, ring_margin=0):
        _check(self._lib.miosqp_qp_stream_create(self._h, int(capacity), int(columns), int(ring_margin)), "stream_create")
        self._stream_info = _lib.StreamInfo()

    def stream_begin(self):
        _check(self._lib.miosqp_qp_stream_begin(self._h), "stream_begin")

    def stream_add_leaf(self, l_int, u_int, x0, y0, depth, lower):
        k = len(l_int)
        rc = _check(self._lib.miosqp_qp_stream_add_leaf(
            self._h, _vec(l_int, k, "l_int"), _vec(u_int, k, "u_int"), _vec(x0, self.n, "x0"), _vec(y0, self.m, "y0"),
            int(depth), float(lower)), "stream_add_leaf")
        if rc == 1:
            raise ValueError("Lower bound must be lower than or equal to upper bound")

    def stream_take_leaf(self, n_int, into=None):
        l, u, x, y = into if into is not None else (np.empty(n_int), np.empty(n_int), np.empty(self.n), np.empty(self.m))
        depth, lower = C.c_int32(), C.c_double()
        rc = _check(self._lib.miosqp_qp_stream_take_leaf(self._h, _vec(l, n_int, "l_int"), _vec(u, n_int, "u_int"),
                                                         _vec(x, self.n, "x0"), _vec(y, self.m, "y0"),
                                                         C.byref(depth), C.byref(lower)), "stream_take_leaf")
        return None if rc == 1 else (l, u, x, y, depth.value, lower.value)

    def stream_set_incumbent(self, upper, x):
        _check(self._lib.miosqp_qp_stream_set_incumbent(self._h, float(min(upper, 1.7e308)),
                                                        _lib.as_d(_f64(x, self.n, "x"))), "stream_set_incumbent")

    def stream_get_incumbent(self):
        upper, x = C.c_double(), np.empty(self.n)
        _check(self._lib.miosqp_qp_stream_get_incumbent(self._h, C.byref(upper), _lib.as_d(x)), "stream_get_incumbent")
        return (upper.value, x) if upper.value < 1.7e308 else (float("inf"), None)

    def stream_step(self, tree_explor_rule, chunks=1, rounds=1, max_nodes=0):
        info = self._stream_info
        _check(self._lib.miosqp_qp_stream_step(self._h, int(tree_explor_rule), int(chunks), int(rounds), int(max_nodes),
                                               C.byref(info)), "stream_step")
        return info

    # -- device-resident leaf pool + streaming batch (miosqp_qp_pool_*) ------------------------------
    POOL_PRUNED = -100

    def pool_create(self, capacity, columns):
        _check(self._lib.miosqp_qp_pool_create(self._h, int(capacity), int(columns)), "pool_create")

    def _digest_buffer(self):
        if getattr(self, "_dg", None) is None:
            self._dg = (_lib.PoolDigest * 8192)()
            self._dg_np = np.frombuffer(self._dg, dtype=np.dtype(
                [("slot", "i4"), ("status_val", "i4"), ("iter", "i4"), ("int_inf", "i4"), ("nextvar", "i4"),
                 ("reserved", "i4"), ("lower", "f8"), ("heur_viol", "f8"), ("heur_obj", "f8"), ("pri_res", "f8"),
                 ("dua_res", "f8")]))
        return self._dg

    def pool_reset(self):
        _check(self._lib.miosqp_qp_pool_reset(self._h), "pool_reset")

    def pool_write_node(self, slot, l_int, u_int, x0, y0):
        k = len(l_int)
        rc = _check(self._lib.miosqp_qp_pool_write_node(
            self._h, int(slot), _vec(l_int, k, "l_int"), _vec(u_int, k, "u_int"), _vec(x0, self.n, "x0"),
            _vec(y0, self.m, "y0")), "pool_write_node")
        if rc == 1:
            raise ValueError("Lower bound must be lower than or equal to upper bound")

    def pool_read_node(self, slot, n_int, want=("l", "u", "x", "y"), into=None):
        """into: dict of DevicePtr by the same keys: those vectors are copied there (device to device) instead"""
        out = dict(l=np.empty(n_int), u=np.empty(n_int), x=np.empty(self.n), y=np.empty(self.m))
        if into:
            out.update(into)
        size = dict(l=n_int, u=n_int, x=self.n, y=self.m)
        ptr = [(_vec(out[k], size[k], k) if k in want else None) for k in ("l", "u", "x", "y")]
        _check(self._lib.miosqp_qp_pool_read_node(self._h, int(slot), *ptr), "pool_read_node")
        return types.SimpleNamespace(**{k: out[k] for k in want})

    def pool_push(self, slot, child0, child1, lower):
        s = np.ascontiguousarray(slot, dtype=np.int32)
        c0 = np.ascontiguousarray(child0, dtype=np.int32)
        c1 = np.ascontiguousarray(child1, dtype=np.int32)
        lo = np.ascontiguousarray(lower, dtype=np.float64)
        _check(self._lib.miosqp_qp_pool_push(self._h, len(s), _lib.as_i(s), _lib.as_i(c0), _lib.as_i(c1),
                                             _lib.as_d(lo)), "pool_push")

    def pool_set_upper(self, upper):
        _check(self._lib.miosqp_qp_pool_set_upper(self._h, float(min(upper, 1.7e308))), "pool_set_upper")

    def pool_launch(self, chunks=1):
        _check(self._lib.miosqp_qp_pool_launch(self._h, int(chunks)), "pool_launch")

    def pool_collect(self, keep_in_flight=0):
        """Waits until at most `keep_in_flight` launches are still running; returns (digests as a numpy record
        array (a copy), active columns, ready-ring entries not yet taken)."""
        n, act, left = C.c_int32(), C.c_int32(), C.c_int64()
        _check(self._lib.miosqp_qp_pool_collect(self._h, int(keep_in_flight), self._digest_buffer(), 8192, C.byref(n),
                                                C.byref(act), C.byref(left)), "pool_collect")
        return self._dg_np[:n.value].copy(), act.value, left.value

    # -- introspection ------------------------------------------------------------------------
    def debug_iterate(self, k):
        x, z, y = np.empty(self.n), np.empty(self.m), np.empty(self.m)
        _check(self._lib.miosqp_qp_debug_iterate(self._h, k, _lib.as_d(x), _lib.as_d(z), _lib.as_d(y)),
               "debug_iterate")
        return x, z, y

    def debug_factor(self, which):
        """One device-resident product of the set-up read back (miosqp_qp_debug_factor): 0 d2inv, 1 Linv, 2 LinvT, 3 W,
        4 Kc, 5 the persistent solver's tail inverse.  Returns (the logical part, the raw padded array): d2inv as a
        vector of n, Linv / LinvT / the tail inverse n x n, W / Kc N x N; raw is rows x ld as it lies in device memory.
        RuntimeError when this engine did not build the product."""
        rows, ld = C.c_int32(), C.c_int32()
        _check(self._lib.miosqp_qp_debug_factor(self._h, int(which), None, 0, C.byref(rows), C.byref(ld)), "debug_factor")
        raw = np.empty((rows.value, ld.value))
        _check(self._lib.miosqp_qp_debug_factor(self._h, int(which), _lib.as_d(raw), raw.size, C.byref(rows), C.byref(ld)),
               "debug_factor")
        if which == 0:
            return raw[:, 0].copy(), raw
        return raw[:, :rows.value].copy(), raw

    def debug_panel(self, which):
        """The values of the factor's panel L21 = -rho Abar as stored, padding included (miosqp_qp_debug_panel): 0 by
        variable and 1 by constraint as they lie in device memory, 2 and 3 the host's mirror of the two."""
        count = C.c_int64()
        _check(self._lib.miosqp_qp_debug_panel(self._h, int(which), None, 0, C.byref(count)), "debug_panel")
        out = np.empty(count.value)
        _check(self._lib.miosqp_qp_debug_panel(self._h, int(which), _lib.as_d(out), out.size, C.byref(count)), "debug_panel")
        return out

    def debug_product_form(self, which):
        """One array of the product form read back (miosqp_qp_debug_product_form): 0 f_rows (n x (M + n): [-G | strict
        lower of Linv]), 1 f_GmT (M x n), 2 f_Ad (M x n), 3 f_Atd (n x M), 4 f_Pd (n x n); 5, 6, 7: the scaled q, l, u as
        vectors.  Returns (the logical part, the raw padded array as it lies in device memory).  RuntimeError for an engine without the product form."""
        rows, ld = C.c_int32(), C.c_int32()
        _check(self._lib.miosqp_qp_debug_product_form(self._h, int(which), None, 0, C.byref(rows), C.byref(ld)),
               "debug_product_form")
        raw = np.empty((rows.value, ld.value))
        _check(self._lib.miosqp_qp_debug_product_form(self._h, int(which), _lib.as_d(raw), raw.size, C.byref(rows),
                                                      C.byref(ld)), "debug_product_form")
        if which >= 5:
            return raw[:, 0].copy(), raw
        cols = (self.n + self.m, self.n, self.n, self.m, self.n)[int(which)]
        return raw[:, :cols].copy(), raw

    def setup_group(self):
        """the group of setup_models this engine belongs to (a positive number, shared by the engines of one call), None
        for an engine of setup()"""
        g = int(self._lib.miosqp_qp_setup_group(self._h)) if self._h is not None else 0
        return g if g > 0 else None

    def scaling(self):
        D, E, c = np.empty(self.n), np.empty(self.m), C.c_double()
        _check(self._lib.miosqp_qp_get_scaling(self._h, _lib.as_d(D), _lib.as_d(E), C.byref(c)),
               "get_scaling")
        return D, E, c.value

    def factor_stats(self):
        out = np.zeros(10, dtype=np.int64)
        _check(self._lib.miosqp_qp_get_factor_stats(self._h, out.ctypes.data_as(_lib.i64p)),
               "get_factor_stats")
        return dict(nnz_L=int(out[0]), nnz_panel=int(out[1]), tail_order=int(out[2]),
                    bytes_per_iter=int(out[3]), bytes_moved_per_iter=int(out[8]), coop_fallbacks=int(out[9]),
                    tpr=(int(out[4]), int(out[5]), int(out[6])),
                    fold=bool(out[7] & 1), resident=bool(out[7] & 2), setup_on_device=bool(out[7] & 4), coop=bool(out[7] & 8), pers=bool(out[7] & 16), tail_inverse=bool(out[7] & 32), pers_small=bool(out[7] & 64), coop_nap=(out[7] >> 8) & 0xff,
                    batch_pers=bool(out[7] & (1 << 16)), inverse_guard_tripped=bool(out[7] & (1 << 17)),
                    search_grid_resident=bool(out[7] & (1 << 18)))

    def rho(self):
        """the rho in use (differs from the setting after rho="auto")"""
        out = np.zeros(1)
        _check(self._lib.miosqp_qp_get_rho(self._h, out.ctypes.data_as(_lib.dp)), "get_rho")
        return float(out[0])

    def inverse_guard(self):
        """(residual, threshold, tripped) of the set-up check of the explicit KKT inverse; residual -1: none was built."""
        out = np.zeros(3)
        _check(self._lib.miosqp_qp_get_inverse_guard(self._h, out.ctypes.data_as(_lib.dp)), "get_inverse_guard")
        return float(out[0]), float(out[1]), bool(out[2])

    def loop_stats(self, reset=False):
        ms, it = C.c_double(), C.c_int64()
        _check(self._lib.miosqp_qp_get_loop_stats(self._h, C.byref(ms), C.byref(it), int(reset)),
               "get_loop_stats")
        return ms.value, it.value

    def node_stats(self):
        """(min, median, max) microseconds of device time per ADMM iteration over the nodes of the hosted search since the
        last loop_stats(reset=True), and the number of nodes."""
        v, k = np.zeros(3), C.c_int32()
        _check(self._lib.miosqp_qp_get_node_stats(self._h, _lib.as_d(v), C.byref(k)), "get_node_stats")
        return float(v[0]), float(v[1]), float(v[2]), k.value

    def loop_launches(self):
        """Launches of the hosted search's solver kernel since the last loop_stats(reset=True): one per node, or one per
        search_run where the cooperative grid stays resident (k_coop_run)."""
        k = C.c_int64()
        _check(self._lib.miosqp_qp_get_loop_launches(self._h, C.byref(k)), "get_loop_launches")
        return k.value

    def batch_stats(self, reset=False):
        ms, bi, ni = C.c_double(), C.c_int64(), C.c_int64()
        _check(self._lib.miosqp_qp_get_batch_stats(self._h, C.byref(ms), C.byref(bi), C.byref(ni), int(reset)),
               "get_batch_stats")
        return ms.value, bi.value, ni.value

    def compactions(self):
        return int(self._lib.miosqp_qp_debug_counter(self._h, 0))

    def batch_pers_fallbacks(self):
        """Times a chunk's persistent launch (kbp) was called off and the engine went back to the launches."""
        return int(self._lib.miosqp_qp_debug_counter(self._h, 1))

    def stream_chunks_by_form(self):
        """(launches of the stream's persistent kernel kbs, chunks queued through them, chunks queued as the chunk graph)"""
        return tuple(int(self._lib.miosqp_qp_debug_counter(self._h, k)) for k in (7, 8, 9))

    def resident_grid_poll_delay(self):
        """(poll delay the resident search grid ran with last, or -1; synthetic nodes its calibration ran on this engine)"""
        return int(self._lib.miosqp_qp_debug_counter(self._h, 10)), int(self._lib.miosqp_qp_debug_counter(self._h, 11))

    def chip_turn_waits(self):
        """Whole-chip launches on this engine's device that were ordered behind another engine's (they take turns)."""
        return int(self._lib.miosqp_qp_debug_counter(self._h, 2))

    def chip_turn_users(self):
        return int(self._lib.miosqp_qp_debug_counter(self._h, 4))

    def tail_inverse_resident_columns(self):
        """Columns of every row of S^-1 the persistent streaming solver keeps in LDS for a whole launch (0: none)."""
        return int(self._lib.miosqp_qp_debug_counter(self._h, 5))

    def tail_inverse_tiles(self):
        """Tiles of S^-1 (on and above the diagonal, one per workgroup) the persistent streaming solver reads per iteration
        when it takes the matrix as symmetric; 0: it streams whole rows."""
        return int(self._lib.miosqp_qp_debug_counter(self._h, 6))

    def polish_many_large_slab_bytes(self):
        """Bytes of device scratch the slabs of `polish_many_large` hold on this engine (0 before its first call)."""
        return int(self._lib.miosqp_qp_debug_counter(self._h, 12))

    def call_off_word(self):
        """The control block's call-off / time-out word once the engine's stream is idle (0: nothing happened)."""
        return int(self._lib.miosqp_qp_debug_counter(self._h, 3))

    def time_kernel(self, which, reps=200):
        us, by = C.c_double(), C.c_double()
        _check(self._lib.miosqp_qp_time_kernel(self._h, which, reps, C.byref(us), C.byref(by)),
               "time_kernel")
        return us.value, by.value

    def close(self):
        if self._h is not None:
            self._lib.miosqp_qp_cleanup(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
