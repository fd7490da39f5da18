"""Round and fix on the device (miosqp_qp_round_and_fix, csrc/kernels_derived.inc) against its CPU restatement
(Workspace with the oracle backend: the reference's four calls per candidate on a second solver with
max_iter = rf_max_iter, the acceptance rule in numpy), and settings["primal_heuristic"] = 1 over whole trees.

Feasibility flags can only be compared where no candidate sits on the threshold.  In the restatement the smallest
|viol| over the candidates of the roots used below is 6.2e-5 -- entries of -0.001 = -eps_abs are rows exactly on a
root bound --; a deeper node with a candidate within 1e-5 of the threshold is passed over for the next one (one such
node exists: random_miqp (30, 150, 15, 4), rho "auto", 3.8e-6), which leaves 1.7e-4 or more.  The whole-tree cases
have 6.2e-5, 3.2e-4 and 1.5e-4 over all their calls.  The device agrees within 1e-6, so no flag can flip."""
import ctypes as C

import numpy as np
import pytest

from golden_cases import load_case
from miosqp_amd import problems

pytestmark = pytest.mark.gpu

SOLVED, MAX_ITER = 1, -2


def _pair(oracle_mod, pr, qp_extra=None, **settings):
    from miosqp_amd import bnb, qp
    st = dict(problems.BNB_SETTINGS, primal_heuristic=1, **settings)
    qs = dict(problems.QP_SETTINGS, **(qp_extra or {}))
    out = []
    for backend in (qp, oracle_mod):
        m = bnb.MIOSQP(backend=backend)
        m.setup(pr["P"], pr["q"], pr["A"], pr["l"], pr["u"], pr["i_idx"], pr["i_l"], pr["i_u"], dict(st), dict(qs))
        out.append(m)
    return out


def _nodes(w, count, depths=(0, 2)):
    """The root and nodes two levels down (both children of the root's most fractional position, then both of theirs),
    solved with the CPU workspace: those that are solved and still fractional."""
    root = w.leaves.pop()
    root.solve()
    level, out = [root], []
    for depth in range(3):
        nxt = []
        for leaf in level:
            if leaf.status not in (SOLVED, MAX_ITER) or w.is_int_feas(leaf.x, leaf):
                continue
            if depth in depths:
                out.append(leaf)
            if depth < 2:
                w.pick_nextvar(leaf)
                w.branch_children(leaf)
                for child in w.leaves[-2:]:
                    child.solve()
                    nxt.append(child)
                del w.leaves[-2:]
        level = nxt
    return out[:count]


def _rel(a, b):
    return abs(a - b) / max(1.0, abs(b))


def _same_record(rg, ro, i_idx):
    K = len(ro.status)
    np.testing.assert_array_equal(rg.status, ro.status)
    np.testing.assert_array_equal(rg.iter, ro.iter)
    for k in range(K):
        if ro.status[k] in (SOLVED, MAX_ITER):
            assert _rel(rg.obj[k], ro.obj[k]) <= 1e-9, (k, rg.obj[k], ro.obj[k])
            assert abs(rg.viol[k] - ro.viol[k]) <= 1e-6, (k, rg.viol[k], ro.viol[k])
            assert abs(ro.viol[k]) > 1e-5, (k, ro.viol[k])  # the node was chosen with a margin: see the module docstring
            assert (rg.viol[k] <= 0.0) == (ro.viol[k] <= 0.0)
        else:
            assert np.isnan(rg.obj[k]) and np.isnan(rg.viol[k])
    assert rg.feasible == ro.feasible
    assert rg.chosen == ro.chosen
    if ro.chosen >= 0:
        assert np.max(np.abs(rg.x - ro.x)) <= 1e-8 * max(1.0, np.max(np.abs(ro.x)))
        np.testing.assert_array_equal(rg.x[i_idx], ro.x[i_idx])
    else:
        assert rg.x is None and ro.x is None
    assert rg.iters == int(np.sum(ro.iter)) and rg.device_time > 0


def _raw_call(eng, leaf, upper, K, max_iter, x_out):
    """The C entry itself, with the caller's x_out"""
    from miosqp_amd import _lib
    l, u = np.ascontiguousarray(leaf.l, dtype=float), np.ascontiguousarray(leaf.u, dtype=float)
    x, y = np.ascontiguousarray(leaf.x, dtype=float), np.ascontiguousarray(leaf.y, dtype=float)
    status, iters = np.empty(K, dtype=np.int32), np.empty(K, dtype=np.int32)
    obj, viol = np.empty(K), np.empty(K)
    info = _lib.RfInfo()
    rc = eng._lib.miosqp_qp_round_and_fix(eng._h, _lib.as_d(l), _lib.as_d(u), _lib.as_d(x), _lib.as_d(y), float(upper), K,
                                          int(max_iter), _lib.as_d(x_out), _lib.as_i(status), _lib.as_i(iters),
                                          _lib.as_d(obj), _lib.as_d(viol), C.byref(info))
    return rc, info, status, iters, obj, viol


INSTANCES = [(50, 100, 10, 0), (60, 80, 30, 3), (30, 150, 15, 4)]


@pytest.mark.parametrize("rho", [0.1, "auto"])
@pytest.mark.parametrize("inst", INSTANCES)
def test_device_entry_equals_the_cpu_restatement(oracle_mod, inst, rho):
    n, m, p, seed = inst
    pr = problems.random_miqp(n, m, p, seed=seed)
    g, o = _pair(oracle_mod, pr, qp_extra=dict(rho=rho))
    nodes = _nodes(o.work, 5)
    assert len(nodes) >= 2 and nodes[0].depth == 0 and any(lf.depth == 2 for lf in nodes)
    ii = pr["i_idx"]
    used = 0
    for leaf in nodes:
        if used == 4:
            break
        for w in (g.work, o.work):
            w.upper_glob = np.inf
        ro = o.work.round_and_fix(leaf)
        if leaf.depth > 0 and np.nanmin(np.abs(ro.viol)) < 1e-5:
            continue  # a candidate on the feasibility threshold: another node (module docstring)
        used += 1
        rg = g.work.round_and_fix(leaf)
        _same_record(rg, ro, ii)
        if leaf.depth == 0 and inst == (50, 100, 10, 0) and rho == "auto":
            # no candidate of this root keeps the root's constraints: nothing is chosen and x_out stays as it was
            assert ro.chosen == -1 and ro.feasible == 0
            x_out = np.full(n, -77.0)
            rc, info, _, _, _, viol = _raw_call(g.work.solver, leaf, np.inf, 7, g.work.rf["max_iter"], x_out)
            assert rc == 0 and info.chosen == -1 and info.feasible == 0 and np.all(viol > 0.0)
            np.testing.assert_array_equal(x_out, np.full(n, -77.0))
        # a caller's upper between two objectives moves the choice, one below all of them leaves none
        feas = sorted({float(ro.obj[k]) for k in range(len(ro.obj)) if ro.viol[k] <= 0.0})
        uppers = [feas[0] - 1.0] if feas else []
        if len(feas) > 1 and feas[-1] - feas[0] > 1e-6:
            uppers.append(0.5 * (feas[0] + feas[-1]))
        for upper in uppers:
            for w in (g.work, o.work):
                w.upper_glob = upper
            rg2, ro2 = g.work.round_and_fix(leaf), o.work.round_and_fix(leaf)
            _same_record(rg2, ro2, ii)
            assert ro2.feasible == ro.feasible
            if upper < feas[0]:
                assert ro2.chosen == -1
    assert used >= 2 and g.work.rf_stats["calls"] >= used


def test_config2_root_equals_the_cpu_restatement(oracle_mod):
    c = problems.CONFIGS["cfg2"]
    pr = problems.random_miqp(c["n"], c["m"], c["p"], density=c["density"], seed=0)
    g, o = _pair(oracle_mod, pr, qp_extra=dict(rho="auto"))
    root = _nodes(o.work, 1, depths=(0,))[0]
    rg, ro = g.work.round_and_fix(root), o.work.round_and_fix(root)
    _same_record(rg, ro, pr["i_idx"])
    assert ro.chosen >= 0 and ro.feasible >= 1
    print("config 2 root, rho auto: %d of 7 feasible, chosen %d, objective %.6f, %d iterations, device %.4f s"
          % (rg.feasible, rg.chosen, rg.obj[rg.chosen], rg.iters, rg.device_time))


def _run(case, backend):
    """golden_cases.run_case with the heuristic's statistics next to each solve"""
    from miosqp_amd import bnb
    prob = case["prob"]
    model = bnb.MIOSQP(backend=backend)
    model.setup(prob["P"], prob["q"], prob["A"], np.copy(prob["l"]), np.copy(prob["u"]), prob["i_idx"], prob["i_l"],
                prob["i_u"], case["settings"], case["qp_settings"])
    rows, out = [], []

    def one():
        del rows[:]
        res = model.solve(observer=lambda w, lf: rows.append(-1 if lf.nextvar_idx is None else lf.nextvar_idx))
        out.append(dict(nextvar=list(rows), upper_glob=res.upper_glob, status=res.status,
                        iter_num=model.work.iter_num, rf=dict(model.work.rf_stats)))

    if case["x0"] is not None:
        model.set_x0(np.copy(case["x0"]))
    one()
    for (q, l, u, x0u) in case["updates"]:
        model.update_vectors(q=q, l=l, u=u)
        if x0u is not None:
            model.set_x0(np.copy(x0u))
        one()
    return out


@pytest.mark.parametrize("name", ["cfg1_n50m100p10_s0", "n30m150p15_s4", "mpc_n12m30p6_s8"])
def test_whole_trees_gpu_equal_cpu(oracle_mod, name):
    from miosqp_amd import qp
    runs = []
    for backend in (qp, oracle_mod):
        case = load_case(name)
        case["settings"] = dict(case["settings"], primal_heuristic=1)
        runs.append(_run(case, backend))
    assert len(runs[0]) == len(runs[1])
    calls = 0
    for a, b in zip(*runs):
        assert a["status"] == b["status"]
        assert a["iter_num"] == b["iter_num"]
        assert a["nextvar"] == b["nextvar"]
        if np.isfinite(b["upper_glob"]):
            assert abs(a["upper_glob"] - b["upper_glob"]) <= 1e-9 * max(1.0, abs(b["upper_glob"]))
        else:
            assert a["upper_glob"] == b["upper_glob"]
        for key in ("calls", "candidates", "feasible", "improved", "osqp_iter"):
            assert a["rf"][key] == b["rf"][key], key
        calls += b["rf"]["calls"]
    assert calls > 0


def test_config2_closes_with_the_heuristic():
    from miosqp_amd import bnb
    c = problems.CONFIGS["cfg2"]
    pr = problems.random_miqp(c["n"], c["m"], c["p"], density=c["density"], seed=0)
    res = {}
    for on in (0, 1):
        m = bnb.MIOSQP()
        m.setup(pr["P"], pr["q"], pr["A"], pr["l"], pr["u"], pr["i_idx"], pr["i_l"], pr["i_u"],
                dict(problems.BNB_SETTINGS, primal_heuristic=on), dict(problems.QP_SETTINGS))
        uppers = []
        r = m.solve(observer=(lambda w, lf: uppers.append(w.upper_glob)) if on else None)
        res[on] = (r, m.work.iter_num, dict(m.work.rf_stats), uppers)
    (r0, n0, _, _), (r1, n1, rf1, uppers) = res[0], res[1]
    assert r0.status == "Solved" and r1.status == "Solved"
    assert abs(r1.upper_glob - r0.upper_glob) <= 1e-3 * max(1.0, abs(r0.upper_glob))
    assert np.isfinite(uppers[0])  # an incumbent after node 1
    assert rf1["calls"] > 0 and rf1["improved"] >= 1 and rf1["feasible"] <= rf1["candidates"]
    print("config 2 seed 0: %d nodes without the heuristic, %d with; rf_stats %r" % (n0, n1, rf1))


def test_round_and_fix_leaves_no_state_behind(oracle_mod):
    pr = problems.random_miqp(50, 100, 10, seed=0)
    g, o = _pair(oracle_mod, pr)
    leaf = _nodes(o.work, 1)[0]
    eng = g.work.solver
    r1 = eng.solve_node(leaf.l, leaf.u, leaf.x, leaf.y)
    rf = eng.round_and_fix(leaf.l, leaf.u, leaf.x, leaf.y, np.inf, 7, 250)
    assert len(rf.status) == 7 and rf.chosen >= 0
    r2 = eng.solve_node(leaf.l, leaf.u, leaf.x, leaf.y)
    np.testing.assert_array_equal(r1.x, r2.x)
    np.testing.assert_array_equal(r1.y, r2.y)
    assert (r1.status_val, r1.iter, r1.lower) == (r2.status_val, r2.iter, r2.lower)
    assert (r1.digest.int_inf, r1.digest.nextvar, r1.digest.heur_obj) == (r2.digest.int_inf, r2.digest.nextvar,
                                                                          r2.digest.heur_obj)
    # and a second identical call is bit-identical
    rf2 = eng.round_and_fix(leaf.l, leaf.u, leaf.x, leaf.y, np.inf, 7, 250)
    for key in ("status", "iter", "obj", "viol", "x"):
        np.testing.assert_array_equal(getattr(rf, key), getattr(rf2, key))
    assert (rf.chosen, rf.feasible, rf.iters) == (rf2.chosen, rf2.feasible, rf2.iters)


def _fresh_engine(pr):
    from miosqp_amd import qp
    A, l, u = problems.extended(pr)
    eng = qp.OSQP()
    eng.setup(pr["P"], pr["q"], A, l, u, **problems.QP_SETTINGS)
    eng.set_integer_rows(pr["i_idx"], pr["A"].shape[0])
    eng.set_root(l, u, problems.BNB_SETTINGS["eps_int_feas"], problems.QP_SETTINGS["eps_abs"])
    return eng


# The second has M = 270: two blocks in x of the builder grid; the third n > M: n sizes that grid.  On the CPU oracle
# all three have a SOLVED, fractional root and two such nodes at depth 2 (fractional integers 5, 1, 2 / 6, 8, 4 /
# 3, 1, 1); the third at seed 2 because seeds 0 and 1 of its shape leave one and two nodes.
SHARED_STAGING = [dict(problems.CONFIGS["cfg1"], seed=0), dict(n=40, m=250, p=20, seed=0),
                  dict(n=300, m=20, p=8, seed=2)]


@pytest.mark.parametrize("kw", SHARED_STAGING)
def test_both_features_share_one_staging_block(oracle_mod, kw):
    """Round and fix and strong branching stage through the same device and pinned blocks: interleaved on ONE engine,
    each call returns bit for bit what it returns as the first call of a fresh engine, and so does the solve_batch
    that follows them."""
    from miosqp_amd import bnb
    pr = problems.random_miqp(**kw)
    o = bnb.MIOSQP(backend=oracle_mod)
    o.setup(pr["P"], pr["q"], pr["A"], pr["l"], pr["u"], pr["i_idx"], pr["i_l"], pr["i_u"], dict(problems.BNB_SETTINGS),
            dict(problems.QP_SETTINGS))
    nodes = _nodes(o.work, 3)
    assert len(nodes) == 3 and nodes[0].depth == 0 and all(lf.depth == 2 for lf in nodes[1:])
    cap = 2 * 25  # two termination checks

    def rf(K):
        return lambda eng, lf: eng.round_and_fix(lf.l, lf.u, lf.x, lf.y, np.inf, K, cap)

    def sb(largest):
        def call(eng, lf):
            cand = sorted(lf.frac_idx)[:32 if largest else 1]
            return eng.strong_branch(lf.l, lf.u, lf.x, lf.y, lf.lower, cand, cap, 1e-6)
        return call

    def batch(eng, _):
        return eng.solve_batch(*(np.stack([getattr(lf, key) for lf in nodes]) for key in ("l", "u", "x", "y")))

    keys = {"rf": ("status", "iter", "obj", "viol", "x", "chosen", "feasible", "iters"),
            "sb": ("lower", "status", "iter", "score", "chosen", "iters"),
            "batch": ("x", "y", "status_val", "iter", "lower")}
    sequence = (("rf", rf(32)), ("sb", sb(False)), ("rf", rf(1)), ("sb", sb(True)))
    calls = [(kind, fn, lf) for lf in nodes for kind, fn in sequence]
    calls.append(("batch", batch, None))
    shared = _fresh_engine(pr)
    for kind, fn, lf in calls:
        got, want = fn(shared, lf), fn(_fresh_engine(pr), lf)
        for key in keys[kind]:
            a, b = getattr(got, key), getattr(want, key)
            if b is None:
                assert a is None, (kind, key)
            else:
                assert np.array_equal(a, b, equal_nan=True), (kind, key, a, b)


def test_round_and_fix_argument_checks(oracle_mod):
    from miosqp_amd import qp
    pr = problems.random_miqp(50, 100, 10, seed=0)
    g, o = _pair(oracle_mod, pr)
    leaf = _nodes(o.work, 1)[0]
    eng = g.work.solver
    assert eng.settings.check_termination == 25 and eng.settings.max_iter == 4000
    for bad in (dict(K=0), dict(K=33), dict(max_iter=30), dict(max_iter=0), dict(max_iter=-25)):
        kw = dict(K=7, max_iter=250)
        kw.update(bad)
        with pytest.raises(RuntimeError):
            eng.round_and_fix(leaf.l, leaf.u, leaf.x, leaf.y, np.inf, kw["K"], kw["max_iter"])
    lbad = leaf.l.copy()
    lbad[0] = leaf.u[0] + 1.0
    with pytest.raises(ValueError):
        eng.round_and_fix(lbad, leaf.u, leaf.x, leaf.y, np.inf, 7, 250)
    # the engine's own max_iter is accepted although it is no multiple of check_termination (the tail runs), and
    # an engine that was never given the root refuses
    A, l, u = problems.extended(pr)
    bare = qp.OSQP()
    bare.setup(pr["P"], pr["q"], A, l, u, **dict(problems.QP_SETTINGS, max_iter=110))
    with pytest.raises(RuntimeError, match="set_integer_rows"):
        bare.round_and_fix(leaf.l, leaf.u, leaf.x, leaf.y, np.inf, 7, 100)
    bare.set_integer_rows(pr["i_idx"], pr["A"].shape[0])
    with pytest.raises(RuntimeError, match="set_root"):
        bare.round_and_fix(leaf.l, leaf.u, leaf.x, leaf.y, np.inf, 7, 100)
    bare.set_root(l, u, 1e-3, 1e-3)
    with pytest.raises(RuntimeError):
        bare.round_and_fix(leaf.l, leaf.u, leaf.x, leaf.y, np.inf, 7, 60)
    r = bare.round_and_fix(leaf.l, leaf.u, leaf.x, leaf.y, np.inf, 7, 110)
    assert np.all(r.iter <= 110) and np.all(np.isin(r.status, (SOLVED, MAX_ITER)))
    ob = oracle_mod.OSQP()
    ob.setup(pr["P"], pr["q"], A, l, u, **dict(problems.QP_SETTINGS, max_iter=110))
    from miosqp_amd import bnb
    p = len(pr["i_idx"])
    fix = bnb.rf_roundings(leaf.x[pr["i_idx"]], leaf.l[-p:], leaf.u[-p:], 7)
    for k in range(7):
        lk, uk = leaf.l.copy(), leaf.u.copy()
        lk[-p:] = uk[-p:] = fix[k]
        ob.update(l=lk, u=uk)
        ob.warm_start(x=leaf.x, y=leaf.y)
        res = ob.solve()
        assert (res.info.status_val, res.info.iter) == (r.status[k], r.iter[k])


def test_searches_without_the_heuristic_refuse_it():
    from miosqp_amd import bnb, dist, search, stream
    pr = problems.random_miqp(50, 100, 10, seed=0)
    m = bnb.MIOSQP()
    m.setup(pr["P"], pr["q"], pr["A"], pr["l"], pr["u"], pr["i_idx"], pr["i_l"], pr["i_u"],
            dict(problems.BNB_SETTINGS, primal_heuristic=1), dict(problems.QP_SETTINGS))
    with pytest.raises(ValueError):
        stream.StreamSearch(m, columns=64, capacity=4096)
    with pytest.raises(ValueError):
        stream.NativeStreamSearch(m, columns=64, capacity=4096)
    with pytest.raises(ValueError):
        dist.ShardedSearch(m)
    with pytest.raises(ValueError):
        dist.ShardedStream(m)
    with pytest.raises(ValueError):
        search.HostedSearch(m)
    # MIOSQP.solve keeps its Python loop and solve_many its sequential path
    r = m.solve()
    assert r.status == "Solved" and m.work.rf_stats["calls"] > 0 and getattr(m.work, "_hosted", None) is None
    out = m.solve_many([dict(), dict(q=pr["q"] * 1.01)])
    assert [o["status"] for o in out] == ["Solved", "Solved"]
