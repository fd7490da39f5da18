"""MIOSQP.solve_many(lockstep="device") with primal_heuristic = 1 on the HIP engine (needs an MI355X): round and fix
inside the lock-step trees (miosqp_qp_solve_trees_lockstep_rf -- the candidates of all trees that fire in a wave as one
more batch, built, solved and judged on the device) against the sequential path on a fresh model:
`solve_many(..., lockstep=False)`, which is update_vectors + set_x0 + solve() per instance, with `work.rf_stats` read
after every solve().  Every tree must make the decisions of its sequential solve: status, nodes and node iterations
equal, the heuristic's calls, candidates, feasible candidates, improvements and iterations equal, the incumbent's value
within 1e-9 relative (the value is the device's sum; the sequential path recomputes it with numpy), its integers exact.
Common settings: rf_max_iter 250, rf_every 3 (a tree of about 80 nodes fires some 25 times)."""
import ctypes as C

import numpy as np
import pytest

from miosqp_amd import problems

pytestmark = pytest.mark.gpu

_CACHE = {}
RF_KEYS = ("calls", "candidates", "feasible", "improved", "osqp_iter")


def _problem(n=100, m=200, p=50):
    key = ("pr", n, m, p)
    if key not in _CACHE:
        _CACHE[key] = problems.random_miqp(n, m, p, seed=0)
    return _CACHE[key]


def _model(pr, rule, rho, qp=None, **st):
    from miosqp_amd import bnb
    settings = dict(problems.BNB_SETTINGS, tree_explor_rule=rule, primal_heuristic=1, rf_max_iter=250, rf_every=3)
    settings.update(st)
    mdl = bnb.MIOSQP()
    mdl.setup(pr["P"], pr["q"], pr["A"], pr["l"].copy(), pr["u"].copy(), pr["i_idx"], pr["i_l"], pr["i_u"], settings,
              dict(problems.QP_SETTINGS, rho=rho, **(qp or {})))
    return mdl


def _instances(pr):
    """the seven of tests/test_gpu_lockstep_device.py, restated: four with their own q, one with its own l, u, one with
    an x0 that passes set_x0, one infeasible by its bounds (alternating equalities, more rows than variables)"""
    n, m = len(pr["q"]), len(pr["l"])
    rng = np.random.RandomState(3)
    inst = [dict(q=pr["q"] + 0.3 * rng.randn(n)) for _ in range(4)]
    inst.append(dict(l=pr["l"] - 0.5 * rng.rand(m), u=pr["u"] - 0.5 * rng.rand(m)))
    x0 = np.zeros(n)
    x0[pr["i_idx"][0]] = 1.0  # A has entries in [0, 1): 0 <= A x0 < 1 lies inside [l, u]
    inst.append(dict(x0=x0))
    b = 50.0 * (1 - 2 * (np.arange(m) % 2))
    inst.append(dict(l=b, u=b.copy()))
    return inst


def _seventy(pr):
    """the seven recipes x 10 cost perturbations from a fixed seed"""
    n = len(pr["q"])
    rng = np.random.RandomState(17)
    out = []
    for _ in range(10):
        for rec in _instances(pr):
            it = dict(rec)
            it["q"] = np.asarray(rec.get("q", pr["q"]), dtype=float) + 0.05 * rng.randn(n)
            out.append(it)
    return out


def _four(pr):
    """for the small shapes: two with their own q, one with its own l, u, one with an x0 (accepted or not, as set_x0 says)"""
    n, m = len(pr["q"]), len(pr["l"])
    rng = np.random.RandomState(5)
    inst = [dict(q=pr["q"] + 0.3 * rng.randn(n)) for _ in range(2)]
    inst.append(dict(l=pr["l"] - 0.2 * rng.rand(m), u=pr["u"] + 0.2 * rng.rand(m)))
    x0 = np.zeros(n)
    x0[pr["i_idx"][0]] = 1.0
    inst.append(dict(q=pr["q"] + 0.3 * rng.randn(n), x0=x0))
    return inst


def _sequential(mdl, inst):
    """solve_many(lockstep=False) -- update_vectors + set_x0 + solve() per instance -- with work.rf_stats read after
    every solve(): (dicts, per-instance rf_stats)"""
    from miosqp_amd import bnb
    stats = []
    solve0 = bnb.MIOSQP.solve

    def solve(self, *a, **kw):
        res = solve0(self, *a, **kw)
        stats.append({k: int(self.work.rf_stats[k]) for k in RF_KEYS})
        return res

    bnb.MIOSQP.solve = solve
    try:
        out = mdl.solve_many(inst, lockstep=False)
    finally:
        bnb.MIOSQP.solve = solve0
    assert len(stats) == len(inst)
    return out, stats


def _reference(key, make, inst):
    """the sequential path on a fresh model, once per session"""
    if key not in _CACHE:
        mdl = make()
        _CACHE[key] = _sequential(mdl, inst)
        mdl.work.solver.close()
    return _CACHE[key]


def _same(got, rf, want, want_rf, ii):
    """the device driver's dicts and work.lockstep['rf'] against the sequential path's"""
    from miosqp_amd import bnb
    assert len(got) == len(want) == len(want_rf)
    per = rf["per_instance"]
    for k, (g, w) in enumerate(zip(got, want)):
        print("instance %d: device %s %d nodes %d iterations %.12g rf %s | sequential %s %d %d %.12g rf %s"
              % (k, g["status"], g["nodes"], g["osqp_iter"], g["upper_glob"], [per[k][a] for a in RF_KEYS], w["status"],
                 w["nodes"], w["osqp_iter"], w["upper_glob"], [want_rf[k][a] for a in RF_KEYS]))
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g["status"], g["nodes"], g["osqp_iter"]) == (w["status"], w["nodes"], w["osqp_iter"]), k
        assert {a: per[k][a] for a in RF_KEYS} == want_rf[k], k
        if w["status"] in (bnb.MI_SOLVED, bnb.MI_MAX_ITER_FEASIBLE):
            assert abs(g["upper_glob"] - w["upper_glob"]) <= 1e-9 * max(1.0, abs(w["upper_glob"])), k
            np.testing.assert_array_equal(g["x"][ii], w["x"][ii])
        else:
            assert g["upper_glob"] == w["upper_glob"], k
    for a in RF_KEYS:
        assert rf[a] == sum(s[a] for s in want_rf), a


def _identical(a, ra, b, rb):
    """bit for bit: the same trees however the batches were cut"""
    assert len(a) == len(b)
    for k, (g, w) in enumerate(zip(a, b)):
        assert (g["status"], g["nodes"], g["osqp_iter"], g["upper_glob"]) == (w["status"], w["nodes"], w["osqp_iter"], w["upper_glob"]), k
        if np.isfinite(w["upper_glob"]):
            np.testing.assert_array_equal(g["x"], w["x"])
        assert ra["per_instance"][k] == rb["per_instance"][k], k


def _state(mdl):
    w = mdl.work
    return dict(q=w.data.q.copy(), l=w.data.l.copy(), u=w.data.u.copy(), leaves=list(w.leaves), iter_num=w.iter_num,
                osqp_iter=w.osqp_iter, upper_glob=w.upper_glob, lower_glob=w.lower_glob, status=w.status,
                first_run=w.first_run, rf_stats=dict(w.rf_stats), rf_nodes=w.rf_nodes)


def _assert_state(mdl, s):
    w = mdl.work
    for key in ("q", "l", "u"):
        np.testing.assert_array_equal(getattr(w.data, key), s[key])
    assert len(w.leaves) == len(s["leaves"]) and all(a is b for a, b in zip(w.leaves, s["leaves"]))
    for key in ("iter_num", "osqp_iter", "upper_glob", "lower_glob", "status", "first_run", "rf_stats", "rf_nodes"):
        assert getattr(w, key) == s[key], key


def _vectors(mdl, inst):
    data = mdl.work.data
    Q, L, U = mdl._instance_vectors(inst)
    up, XI = np.full(len(inst), np.inf), np.zeros((len(inst), data.n))
    for k, it in enumerate(inst):
        if it.get("x0") is not None:
            x0 = np.asarray(it["x0"], dtype=float)
            up[k] = .5 * np.dot(x0, data.P.dot(x0)) + np.dot(Q[k], x0)
            XI[k] = x0
    return Q, L, U, up, XI


@pytest.mark.parametrize("rho", [0.1, "auto"])
@pytest.mark.parametrize("rule", [1, 3])
def test_round_and_fix_in_the_device_trees_equals_the_sequential_solve(rule, rho):
    from miosqp_amd import bnb
    pr = _problem()
    inst = _instances(pr)
    want, want_rf = _reference(("seven", rule, rho), lambda: _model(pr, rule, rho), inst)
    mdl = _model(pr, rule, rho)
    before = _state(mdl)
    got = mdl.solve_many(inst, lockstep="device")  # (ValueError before round and fix ran in this driver)
    rec = mdl.work.lockstep
    assert rec["driver"] == "device" and rec["instances"] == len(inst) and rec["waves"] == max(g["nodes"] for g in got)
    rf = rec["rf"]
    _assert_state(mdl, before)
    _same(got, rf, want, want_rf, pr["i_idx"])
    assert got[6]["status"] == bnb.MI_PRIMAL_INFEASIBLE and got[5]["upper_glob"] < np.inf
    # the run means something: every feasible tree fires more than once, winners are adopted, and a batch holds the
    # candidates of several trees
    assert all(want_rf[k]["calls"] >= 2 for k in range(6)) and want_rf[6]["calls"] == 0
    assert rf["improved"] >= 1 and rf["feasible"] >= 1
    assert rf["columns"] == rf["candidates"] == mdl.work.rf["K"] * rf["calls"]
    assert 0 < rf["batches"] < rf["calls"]
    mdl.work.solver.close()


@pytest.mark.parametrize("K", [1, 7, 32])
@pytest.mark.parametrize("shape", [(10, 5, 2), (65, 130, 33)])
def test_small_and_ragged_shapes(shape, K):
    """tiles of 64 rows and 64 columns partly filled: n = 10 (one partial tile), n = 65 (a tile and one row), 4 K columns
    (128 in two tiles at K = 32).  The larger shape's trees have hundreds of nodes: cut at 60, every one of them asking"""
    pr = _problem(*shape)
    inst = _four(pr)
    st = dict(rf_candidates=K, rf_every=1, max_iter_bb=60)
    want, want_rf = _reference(("small", shape, K), lambda: _model(pr, 1, 0.1, **st), inst)
    mdl = _model(pr, 1, 0.1, **st)
    got = mdl.solve_many(inst, lockstep="device")
    assert mdl.work.lockstep["driver"] == "device"
    _same(got, mdl.work.lockstep["rf"], want, want_rf, pr["i_idx"])
    assert sum(s["calls"] for s in want_rf) >= 2
    mdl.work.solver.close()


def test_candidate_groups_straddle_the_slices():
    """70 trees x 7 candidates: up to 490 columns per heuristic batch, cut at 64 (groups of 7 straddle every boundary:
    64 = 9 * 7 + 1), at the default width and at 128 (compaction inside a slice: the judge finds a candidate's column
    through c_node).  A candidate is a pure function of its node: every tree is the same bit for bit however the batch is
    cut; the first seven are their sequential solves."""
    pr = _problem()
    inst = _seventy(pr)
    st = dict(max_iter_bb=12)
    runs = {}
    for name, qp in (("64", dict(max_batch=64)), ("default", {}), ("128", dict(max_batch=128))):
        mdl = _model(pr, 1, 0.1, qp=qp, **st)
        runs[name] = (mdl.solve_many(inst, lockstep="device"), mdl.work.lockstep["rf"])
        rf = runs[name][1]
        print("max_batch %s: %d heuristic batches, %d columns, widest %d trees" % (name, rf["batches"], rf["columns"],
                                                                                  mdl.work.lockstep["max_width"]))
        assert rf["columns"] > 64 * rf["batches"]  # batches wider than one slice at 64
        mdl.work.solver.close()
    _identical(*runs["64"], *runs["default"])
    _identical(*runs["64"], *runs["128"])
    want, want_rf = _reference(("seventy7",), lambda: _model(pr, 1, 0.1, **st), inst[:7])
    got, rf = runs["64"]
    seven = dict(rf, per_instance={k: rf["per_instance"][k] for k in range(7)})
    for a in RF_KEYS:
        seven[a] = sum(seven["per_instance"][k][a] for k in range(7))
    _same(got[:7], seven, want, want_rf, pr["i_idx"])


def test_first_call_candidate_by_candidate():
    """What kls_rf_keep leaves per candidate (through c_node, in candidate order) for every tree's first call, against
    what `OSQP.round_and_fix` returns per candidate at the same node of the sequential solve: status and iterations equal,
    objective 1e-9 relative, violation 1e-6 -- the bounds DESIGN 3h holds the device entry to.  K = 32 and max_batch = 64:
    the 6 x 32 = 192 columns of the first batch run in three slices, groups across their boundaries."""
    from miosqp_amd import bnb
    pr = _problem()
    inst = _instances(pr)
    st, K = dict(rf_candidates=32, max_iter_bb=4), 32
    seq = _model(pr, 1, 0.1, **st)
    calls = []
    rf0, solve0 = bnb.Workspace.round_and_fix, bnb.MIOSQP.solve

    def rf(self, leaf):
        r = rf0(self, leaf)
        if calls[-1] is None:
            calls[-1] = (np.array(r.status), np.array(r.iter), np.array(r.obj), np.array(r.viol))
        return r

    def solve(self, *a, **kw):
        calls.append(None)
        return solve0(self, *a, **kw)

    bnb.Workspace.round_and_fix, bnb.MIOSQP.solve = rf, solve
    try:
        seq.solve_many(inst, lockstep=False)
    finally:
        bnb.Workspace.round_and_fix, bnb.MIOSQP.solve = rf0, solve0
    seq.work.solver.close()
    mdl = _model(pr, 1, 0.1, qp=dict(max_batch=64), **st)
    data, s = mdl.work.data, mdl.work.solver
    Q, L, U, up, XI = _vectors(mdl, inst)
    B, M = len(inst), data.m + data.n_int
    x, infos, stats, r = s.solve_trees_lockstep_rf(Q, L, U, np.zeros((B, data.n)), np.zeros((B, M)), up, XI, 1, 4, K, 250, 3,
                                                   first_call=True)
    fc = r.first_call
    assert len(calls) == B and calls[6] is None and all(c is not None for c in calls[:6])
    assert np.all(fc.status[6] == -1) and np.all(np.isnan(fc.obj[6]))  # the infeasible tree never fired
    for k in range(6):
        status, iters, obj, viol = calls[k]
        print("instance %d: worst objective difference %.3g, worst violation difference %.3g, iterations %s"
              % (k, np.nanmax(np.abs(fc.obj[k] - obj)), np.nanmax(np.abs(fc.viol[k] - viol)), fc.iter[k].tolist()))
        np.testing.assert_array_equal(fc.status[k], status)
        np.testing.assert_array_equal(fc.iter[k], iters)
        has = np.isfinite(obj)
        assert np.sum(has) >= 1 and np.array_equal(has, np.isfinite(fc.obj[k]))
        assert np.all(np.abs(fc.obj[k][has] - obj[has]) <= 1e-9 * np.maximum(1.0, np.abs(obj[has])))
        assert np.all(np.abs(fc.viol[k][has] - viol[has]) <= 1e-6)
    s.close()


def test_incumbents_an_x0_and_an_instance_judged_by_its_own_root():
    """(a) A tree that starts from an x0 nobody improves: the heuristic's winners are feasible again and again, and none
    replaces the incumbent -- only a strictly better one does.  (b) The instance with l, u of its own (built as
    tests/test_gpu_lockstep_device.py::test_rounded_point_is_judged_against_the_instances_root builds it): its
    candidates are judged against ITS root rows, as its sequential solve judges them after update_vectors; the same cost
    under the model's rows counts other candidates."""
    pr = _problem()
    base_inst = _instances(pr)
    first, _ = _reference(("seven", 1, 0.1), lambda: _model(pr, 1, 0.1), base_inst)
    best = np.array(first[0]["x"], dtype=float)  # the optimum of instance 0 as ITS x0: upper0 is the optimal value
    inst = [dict(q=base_inst[0]["q"], x0=best), base_inst[4], dict()]
    want, want_rf = _reference(("incumbents",), lambda: _model(pr, 1, 0.1), inst)
    mdl = _model(pr, 1, 0.1)
    got = mdl.solve_many(inst, lockstep="device")
    rf = mdl.work.lockstep["rf"]
    _same(got, rf, want, want_rf, pr["i_idx"])
    per = rf["per_instance"]
    data = mdl.work.data
    z = data.A.dot(best)  # (set_x0's test: the optimum the sequential solve reported is accepted as a starting point)
    assert not (np.any(z < data.l - 1e-3) or np.any(z > data.u + 1e-3))
    up0 = .5 * np.dot(best, data.P.dot(best)) + np.dot(base_inst[0]["q"], best)  # solve_many's expression
    assert per[0]["calls"] >= 1 and per[0]["improved"] == 0
    assert got[0]["upper_glob"] == up0
    np.testing.assert_array_equal(got[0]["x"], best)
    # (b): equal to its sequential solve (above), and bit for bit the tree of a model whose OWN root these rows are --
    # there the engine's root and the instance's coincide, here only the instance's rows can have given that verdict;
    # the same cost under the model's rows is another tree
    assert per[1]["calls"] >= 2 and per[2]["calls"] >= 2
    assert (per[1]["feasible"], got[1]["nodes"], got[1]["upper_glob"]) != (per[2]["feasible"], got[2]["nodes"], got[2]["upper_glob"])
    own = _model(dict(pr, l=base_inst[4]["l"], u=base_inst[4]["u"]), 1, 0.1)
    twin = own.solve_many([dict()], lockstep="device")
    _identical(got[1:2], dict(per_instance={0: per[1]}), twin, own.work.lockstep["rf"])
    for m_ in (mdl, own):
        m_.work.solver.close()


def test_edges_leave_the_model_and_the_engine_as_they_were():
    from miosqp_amd import _lib, bnb
    pr = _problem()
    inst = _instances(pr)
    mdl = _model(pr, 1, 0.1)
    s, data, st = mdl.work.solver, mdl.work.data, mdl.work.settings
    N, M = data.n, data.m + data.n_int
    Q, L, U, up, XI = _vectors(mdl, inst)
    B = len(inst)
    rf_on = mdl.work.rf

    def plain():
        """the model's own solve (heuristic on, as set up) and the device driver with the heuristic off"""
        mdl.update_vectors()  # (the root again, counters reset; no vector changes)
        a = mdl.solve()
        one = (a.status, mdl.work.iter_num, mdl.work.osqp_iter, a.upper_glob, np.array(a.x), dict(mdl.work.rf_stats, solve_time=0.))
        mdl.work.rf = dict(rf_on, on=0)
        try:
            many = mdl.solve_many(inst, lockstep="device")
        finally:
            mdl.work.rf = rf_on
        assert "rf" not in mdl.work.lockstep
        return one, many

    def same_plain(p, q):
        assert p[0][:4] == q[0][:4] and p[0][5] == q[0][5]
        np.testing.assert_array_equal(p[0][4], q[0][4])
        for g, w in zip(p[1], q[1]):
            assert (g["status"], g["nodes"], g["osqp_iter"], g["upper_glob"]) == (w["status"], w["nodes"], w["osqp_iter"], w["upper_glob"])
            if np.isfinite(w["upper_glob"]):  # (without an incumbent x is np.empty)
                np.testing.assert_array_equal(g["x"], w["x"])

    before = plain()
    state = _state(mdl)
    # a store that starts at 8 slots grows and gives the trees of the default capacity
    args = (Q, L, U, np.zeros((B, N)), np.zeros((B, M)), up, XI, st["tree_explor_rule"], st["max_iter_bb"],
            rf_on["K"], rf_on["max_iter"], rf_on["every"])
    x8, info8, st8, rf8 = s.solve_trees_lockstep_rf(*args, capacity=8)
    x0, info0, st0, rf0 = s.solve_trees_lockstep_rf(*args)
    assert st8.grown > 1
    for a, b in zip(info8, info0):
        assert (a.nodes, a.osqp_iter, a.found, a.upper_glob, a.leaves_left) == (b.nodes, b.osqp_iter, b.found, b.upper_glob, b.leaves_left)
    np.testing.assert_array_equal(x8, x0)
    assert (rf8.calls, rf8.candidates, rf8.feasible, rf8.improved, rf8.iters, rf8.batches, rf8.columns, rf8.iters_slowest) == \
        (rf0.calls, rf0.candidates, rf0.feasible, rf0.improved, rf0.iters, rf0.batches, rf0.columns, rf0.iters_slowest)
    assert 0.0 < rf0.device_time < st0.device_time
    want, want_rf = _reference(("seven", 1, 0.1), lambda: _model(pr, 1, 0.1), inst)
    assert [i.nodes for i in info0] == [w["nodes"] for w in want] and rf0.calls == [w["calls"] for w in want_rf]
    _assert_state(mdl, state)
    # max_iter_bb cuts the trees mid-search
    keep, cut_inst = st["max_iter_bb"], _seventy(pr)[:7]
    st["max_iter_bb"] = 12
    try:
        cut = mdl.solve_many(cut_inst, lockstep="device")
        rf_cut = mdl.work.lockstep["rf"]
    finally:
        st["max_iter_bb"] = keep
    wcut, wcut_rf = _reference(("seventy7",), lambda: _model(pr, 1, 0.1, max_iter_bb=12), cut_inst)
    capped = [g for g in cut if g["status"] in (bnb.MI_MAX_ITER_FEASIBLE, bnb.MI_MAX_ITER_UNSOLVED)]
    assert capped and all(g["nodes"] == 11 for g in capped)
    _same(cut, rf_cut, wcut, wcut_rf, pr["i_idx"])
    # bad rf_* arguments: MIOSQP_EARG with a text, nothing queued, the engine usable
    infos = (_lib.TreeInfo * B)()
    xo = np.zeros((B, N))
    zx, zy = np.zeros((B, N)), np.zeros((B, M))
    upc = np.minimum(up, 1.7e308)
    for bad, word in (((0, 250, 3), "rf_candidates"), ((33, 250, 3), "rf_candidates"), ((7, 0, 3), "rf_max_iter"),
                      ((7, 260, 3), "rf_max_iter"), ((7, 250, 0), "rf_every")):
        ls, rs = _lib.LockstepStats(), _lib.LockstepRfStats()
        rc = s._lib.miosqp_qp_solve_trees_lockstep_rf(
            s._h, B, _lib.as_d(Q), _lib.as_d(L), _lib.as_d(U), _lib.as_d(zx), _lib.as_d(zy), _lib.as_d(upc), _lib.as_d(XI),
            1, 1000, 0, bad[0], bad[1], bad[2], _lib.as_d(xo), infos, C.byref(ls), C.byref(rs))
        assert rc == -1 and word in _lib.last_error(), (bad, rc, _lib.last_error())
        with pytest.raises(ValueError, match=word):
            s.solve_trees_lockstep_rf(Q, L, U, zx, zy, up, XI, 1, 1000, *bad)
    # the engine's max_iter itself is a permitted cap, whatever check_termination is
    s.solve_trees_lockstep_rf(Q[:1], L[:1], U[:1], zx[:1], zy[:1], up[:1], None, 1, 3, 7, int(s.settings.max_iter), 1)
    _assert_state(mdl, state)
    same_plain(plain(), before)
    s.close()
