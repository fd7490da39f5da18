"""MIOSQP.solve_many(lockstep="device") with branching_rule 1 and 2 on the HIP engine (needs an MI355X): strong and
reliability branching inside the lock-step trees (miosqp_qp_solve_trees_lockstep_sb -- the strong-branching children of
all nodes with candidates in a wave as one more batch, built and solved on the device, the position chosen per tree in
C++) against the sequential path on a fresh model: `solve_many(..., lockstep=False)`, which is update_vectors + set_x0 +
solve() per instance, with `work.sb_stats` read after every solve().  Every tree must make the decisions of its
sequential solve: status, nodes and node iterations equal, strong branching's calls, children and iterations equal, the
incumbent's value within 1e-9 relative (the value is the device's sum; the sequential path recomputes it with numpy),
its integers exact.  Common setting: sb_max_iter 50."""
import ctypes as C

import numpy as np
import pytest

from miosqp_amd import problems

import test_gpu_lockstep_rf as rfm

pytestmark = pytest.mark.gpu

_CACHE = {}
SB_KEYS = ("calls", "children", "osqp_iter")
_problem, _instances, _seventy, _four, _vectors = rfm._problem, rfm._instances, rfm._seventy, rfm._four, rfm._vectors


def _model(pr, rule, rho, br, qp=None, **st):
    from miosqp_amd import bnb
    settings = dict(problems.BNB_SETTINGS, tree_explor_rule=rule, branching_rule=br, sb_max_iter=50)
    settings.update(st)
    mdl = bnb.MIOSQP()
    mdl.setup(pr["P"], pr["q"], pr["A"], pr["l"].copy(), pr["u"].copy(), pr["i_idx"], pr["i_l"], pr["i_u"], settings,
              dict(problems.QP_SETTINGS, rho=rho, **(qp or {})))
    return mdl


def _sequential(mdl, inst):
    """solve_many(lockstep=False) -- update_vectors + set_x0 + solve() per instance -- with work.sb_stats read after
    every solve(): (dicts, per-instance sb_stats)"""
    from miosqp_amd import bnb
    stats = []
    solve0 = bnb.MIOSQP.solve

    def solve(self, *a, **kw):
        res = solve0(self, *a, **kw)
        stats.append({k: int(self.work.sb_stats[k]) for k in SB_KEYS})
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


def _same(got, sb, want, want_sb, ii):
    """the device driver's dicts and work.lockstep['sb'] against the sequential path's"""
    from miosqp_amd import bnb
    assert len(got) == len(want) == len(want_sb)
    per = sb["per_instance"]
    for k, (g, w) in enumerate(zip(got, want)):
        print("instance %d: device %s %d nodes %d iterations %.12g sb %s | sequential %s %d %d %.12g sb %s"
              % (k, g["status"], g["nodes"], g["osqp_iter"], g["upper_glob"], [per[k][a] for a in SB_KEYS], w["status"],
                 w["nodes"], w["osqp_iter"], w["upper_glob"], [want_sb[k][a] for a in SB_KEYS]))
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g["status"], g["nodes"], g["osqp_iter"]) == (w["status"], w["nodes"], w["osqp_iter"]), k
        assert {a: per[k][a] for a in SB_KEYS} == want_sb[k], k
        if w["status"] in (bnb.MI_SOLVED, bnb.MI_MAX_ITER_FEASIBLE):
            assert abs(g["upper_glob"] - w["upper_glob"]) <= 1e-9 * max(1.0, abs(w["upper_glob"])), k
            np.testing.assert_array_equal(g["x"][ii], w["x"][ii])
        else:
            assert g["upper_glob"] == w["upper_glob"], k
    for a in SB_KEYS:
        assert sb[a] == sum(s[a] for s in want_sb), a


def _identical(a, sa, b, sb):
    """bit for bit: the same trees however the batches were cut"""
    assert len(a) == len(b)
    for k, (g, w) in enumerate(zip(a, b)):
        assert (g["status"], g["nodes"], g["osqp_iter"], g["upper_glob"]) == (w["status"], w["nodes"], w["osqp_iter"], w["upper_glob"]), k
        if np.isfinite(w["upper_glob"]):
            np.testing.assert_array_equal(g["x"], w["x"])
        assert sa["per_instance"][k] == sb["per_instance"][k], k


def _state(mdl):
    w = mdl.work
    return dict(q=w.data.q.copy(), l=w.data.l.copy(), u=w.data.u.copy(), leaves=list(w.leaves), iter_num=w.iter_num,
                osqp_iter=w.osqp_iter, upper_glob=w.upper_glob, lower_glob=w.lower_glob, status=w.status,
                first_run=w.first_run, sb_stats=dict(w.sb_stats), pc_sum=w.pc_sum.copy(), pc_cnt=w.pc_cnt.copy())


def _assert_state(mdl, s):
    w = mdl.work
    for key in ("q", "l", "u"):
        np.testing.assert_array_equal(getattr(w.data, key), s[key])
    assert len(w.leaves) == len(s["leaves"]) and all(a is b for a, b in zip(w.leaves, s["leaves"]))
    for key in ("iter_num", "osqp_iter", "upper_glob", "lower_glob", "status", "first_run", "sb_stats"):
        assert getattr(w, key) == s[key], key
    np.testing.assert_array_equal(w.pc_sum, s["pc_sum"])
    np.testing.assert_array_equal(w.pc_cnt, s["pc_cnt"])


@pytest.mark.parametrize("rho", [0.1, "auto"])
@pytest.mark.parametrize("rule", [1, 3])
@pytest.mark.parametrize("br", [1, 2])
def test_branching_rules_in_the_device_trees_equal_the_sequential_solve(br, rule, rho):
    from miosqp_amd import bnb
    pr = _problem()
    inst = _instances(pr)
    want, want_sb = _reference(("seven", br, rule, rho), lambda: _model(pr, rule, rho, br), inst)
    mdl = _model(pr, rule, rho, br)
    before = _state(mdl)
    got = mdl.solve_many(inst, lockstep="device")  # (ValueError before the branching rules ran in this driver)
    rec = mdl.work.lockstep
    assert rec["driver"] == "device" and rec["instances"] == len(inst) and rec["waves"] == max(g["nodes"] for g in got)
    sb = rec["sb"]
    _assert_state(mdl, before)
    _same(got, sb, want, want_sb, pr["i_idx"])
    assert got[6]["status"] == bnb.MI_PRIMAL_INFEASIBLE and got[5]["upper_glob"] < np.inf
    # the run means something: every feasible tree calls more than once, and a batch holds the children of several trees
    assert all(want_sb[k]["calls"] >= 2 for k in range(6)) and want_sb[6]["calls"] == 0
    assert sb["columns"] == sb["children"]
    assert 0 < sb["batches"] < sb["calls"]
    mdl.work.solver.close()


@pytest.mark.parametrize("K", [1, 8, 32])
@pytest.mark.parametrize("shape", [(10, 5, 2), (65, 130, 33)])
@pytest.mark.parametrize("br", [1, 2])
def test_small_and_ragged_shapes(br, shape, K):
    """tiles of 64 rows and 64 columns partly filled: n = 10 (one partial tile; two integers: the single-fractional
    shortcut of rule 1, and K larger than the fractional set), n = 65 (a tile and one row), up to 4 x 64 columns.  The
    larger shape's trees have hundreds of nodes: cut at 60"""
    pr = _problem(*shape)
    inst = _four(pr)
    st = dict(sb_candidates=K, max_iter_bb=60)
    want, want_sb = _reference(("small", br, shape, K), lambda: _model(pr, 1, 0.1, br, **st), inst)
    mdl = _model(pr, 1, 0.1, br, **st)
    got = mdl.solve_many(inst, lockstep="device")
    assert mdl.work.lockstep["driver"] == "device"
    _same(got, mdl.work.lockstep["sb"], want, want_sb, pr["i_idx"])
    if shape[0] > 10:
        assert sum(s["calls"] for s in want_sb) >= 2
    mdl.work.solver.close()


@pytest.mark.parametrize("br", [1, 2])
def test_child_groups_straddle_the_slices(br):
    """70 trees x 7 candidates: groups of 14 columns, up to 980 per batch, cut at 64 (64 = 4 * 14 + 8: a group straddles
    every boundary), at the default width and at 128 (compaction inside a slice: the judge finds a child's column
    through c_node).  A child is a pure function of its node: every tree is the same bit for bit however the batch is
    cut; the first seven are their sequential solves."""
    pr = _problem()
    inst = _seventy(pr)
    st = dict(max_iter_bb=12, sb_candidates=7)
    runs = {}
    for name, qp in (("64", dict(max_batch=64)), ("default", {}), ("128", dict(max_batch=128))):
        mdl = _model(pr, 1, 0.1, br, qp=qp, **st)
        runs[name] = (mdl.solve_many(inst, lockstep="device"), mdl.work.lockstep["sb"])
        sb = runs[name][1]
        print("max_batch %s: %d batches, %d columns, widest %d trees" % (name, sb["batches"], sb["columns"],
                                                                         mdl.work.lockstep["max_width"]))
        assert sb["columns"] > 64 * sb["batches"]  # batches wider than one slice at 64
        mdl.work.solver.close()
    _identical(*runs["64"], *runs["default"])
    _identical(*runs["64"], *runs["128"])
    want, want_sb = _reference(("seventy7", br), lambda: _model(pr, 1, 0.1, br, **st), inst[:7])
    got, sb = runs["64"]
    seven = dict(sb, per_instance={k: sb["per_instance"][k] for k in range(7)})
    for a in SB_KEYS:
        seven[a] = sum(seven["per_instance"][k][a] for k in range(7))
    _same(got[:7], seven, want, want_sb, pr["i_idx"])


def test_first_call_child_by_child():
    """What kls_sb_judge leaves per child (through c_node, in upload order) for every tree's first call, against what
    `OSQP.strong_branch` returns per child at the same node of the sequential solve: status and iterations equal, lower
    1e-9 relative, the same candidates and the same chosen one.  K = 32 and max_batch = 64: the 6 x 64 = 384 columns of
    the first batch run in six slices."""
    from miosqp_amd import bnb
    pr = _problem()
    inst = _instances(pr)
    st, K = dict(sb_candidates=32, max_iter_bb=4), 32
    seq = _model(pr, 1, 0.1, 1, **st)
    calls = []
    sb0, solve0 = bnb.Workspace.strong_branch, bnb.MIOSQP.solve

    def sb(self, leaf, cand):
        r = sb0(self, leaf, cand)
        if calls[-1] is None:
            calls[-1] = (list(cand), np.array(r.status), np.array(r.iter), np.array(r.lower), int(r.chosen))
        return r

    def solve(self, *a, **kw):
        calls.append(None)
        return solve0(self, *a, **kw)

    bnb.Workspace.strong_branch, bnb.MIOSQP.solve = sb, solve
    try:
        seq.solve_many(inst, lockstep=False)
    finally:
        bnb.Workspace.strong_branch, bnb.MIOSQP.solve = sb0, solve0
    seq.work.solver.close()
    mdl = _model(pr, 1, 0.1, 1, qp=dict(max_batch=64), **st)
    data, s = mdl.work.data, mdl.work.solver
    Q, L, U, up, XI = _vectors(mdl, inst)
    B, M = len(inst), data.m + data.n_int
    x, infos, stats, r = s.solve_trees_lockstep_sb(Q, L, U, np.zeros((B, data.n)), np.zeros((B, M)), up, XI, 1, 4, 1, K, 50, 4,
                                                   1e-6, first_call=True)
    fc = r.first_call
    assert len(calls) == B and calls[6] is None and all(c is not None for c in calls[:6])
    assert fc.k[6] == 0 and np.all(fc.status[6] == -1)  # the infeasible tree never called
    for k in range(6):
        cand, status, iters, lower, chosen = calls[k]
        kk = len(cand)
        assert fc.k[k] == kk and fc.cand[k][:kk].tolist() == [int(c) for c in cand]
        print("instance %d: K %d, worst lower difference %.3g, iterations %s, chosen %d"
              % (k, kk, np.nanmax(np.abs(fc.lower[k][:2 * kk] - lower)), fc.iter[k][:2 * kk].tolist(), fc.chosen[k]))
        np.testing.assert_array_equal(fc.status[k][:2 * kk], status)
        np.testing.assert_array_equal(fc.iter[k][:2 * kk], iters)
        has = np.isfinite(lower)
        assert np.sum(has) >= 1 and np.array_equal(has, np.isfinite(fc.lower[k][:2 * kk]))
        assert np.all(np.abs(fc.lower[k][:2 * kk][has] - lower[has]) <= 1e-9 * np.maximum(1.0, np.abs(lower[has])))
        assert fc.chosen[k] == chosen
    s.close()


def test_edges_leave_the_model_and_the_engine_as_they_were():
    from miosqp_amd import _lib, bnb
    pr = _problem()
    inst = _instances(pr)
    mdl = _model(pr, 1, 0.1, 2)
    s, data, st = mdl.work.solver, mdl.work.data, mdl.work.settings
    N, M = data.n, data.m + data.n_int
    Q, L, U, up, XI = _vectors(mdl, inst)
    B = len(inst)
    sbs = mdl.work.sb
    state = _state(mdl)
    # a store that starts at 8 slots grows and gives the trees of the default capacity
    args = (Q, L, U, np.zeros((B, N)), np.zeros((B, M)), up, XI, st["tree_explor_rule"], st["max_iter_bb"],
            2, sbs["K"], sbs["max_iter"], sbs["reliability"], sbs["eps"])
    x8, info8, st8, sb8 = s.solve_trees_lockstep_sb(*args, capacity=8)
    x0, info0, st0, sb0 = s.solve_trees_lockstep_sb(*args)
    assert st8.grown > 1
    for a, b in zip(info8, info0):
        assert (a.nodes, a.osqp_iter, a.found, a.upper_glob, a.leaves_left) == (b.nodes, b.osqp_iter, b.found, b.upper_glob, b.leaves_left)
    np.testing.assert_array_equal(x8, x0)
    assert (sb8.calls, sb8.children, sb8.iters, sb8.batches, sb8.columns, sb8.iters_slowest) == \
        (sb0.calls, sb0.children, sb0.iters, sb0.batches, sb0.columns, sb0.iters_slowest)
    assert 0.0 < sb0.device_time < st0.device_time
    want, want_sb = _reference(("seven", 2, 1, 0.1), lambda: _model(pr, 1, 0.1, 2), inst)
    assert [i.nodes for i in info0] == [w["nodes"] for w in want] and sb0.calls == [w["calls"] for w in want_sb]
    _assert_state(mdl, state)
    # max_iter_bb cuts the trees mid-search
    keep, cut_inst = st["max_iter_bb"], _seventy(pr)[:7]
    st["max_iter_bb"] = 12
    try:
        cut = mdl.solve_many(cut_inst, lockstep="device")
        sb_cut = mdl.work.lockstep["sb"]
    finally:
        st["max_iter_bb"] = keep
    wcut, wcut_sb = _reference(("cut7",), lambda: _model(pr, 1, 0.1, 2, max_iter_bb=12), cut_inst)
    capped = [g for g in cut if g["status"] in (bnb.MI_MAX_ITER_FEASIBLE, bnb.MI_MAX_ITER_UNSOLVED)]
    assert capped and all(g["nodes"] == 11 for g in capped)
    _same(cut, sb_cut, wcut, wcut_sb, pr["i_idx"])
    # bad arguments: MIOSQP_EARG with a text, nothing queued, the engine usable
    infos = (_lib.TreeInfo * B)()
    xo = np.zeros((B, N))
    zx, zy = np.zeros((B, N)), np.zeros((B, M))
    upc = np.minimum(up, 1.7e308)
    for bad, word in (((0, 8, 50, 4, 1e-6), "branching_rule"), ((3, 8, 50, 4, 1e-6), "branching_rule"),
                      ((1, 0, 50, 4, 1e-6), "sb_candidates"), ((1, 33, 50, 4, 1e-6), "sb_candidates"),
                      ((1, 8, 0, 4, 1e-6), "sb_max_iter"), ((1, 8, 60, 4, 1e-6), "sb_max_iter"),
                      ((2, 8, 50, -1, 1e-6), "sb_reliability"), ((2, 8, 50, 4, 0.0), "sb_eps")):
        ls, bs = _lib.LockstepStats(), _lib.LockstepSbStats()
        rc = s._lib.miosqp_qp_solve_trees_lockstep_sb(
            s._h, B, _lib.as_d(Q), _lib.as_d(L), _lib.as_d(U), _lib.as_d(zx), _lib.as_d(zy), _lib.as_d(upc), _lib.as_d(XI),
            1, 1000, 0, bad[0], bad[1], bad[2], bad[3], bad[4], _lib.as_d(xo), infos, C.byref(ls), C.byref(bs))
        assert rc == -1 and word in _lib.last_error(), (bad, rc, _lib.last_error())
        with pytest.raises(ValueError, match=word):
            s.solve_trees_lockstep_sb(Q, L, U, zx, zy, up, XI, 1, 1000, *bad)
    _assert_state(mdl, state)
    again = s.solve_trees_lockstep_sb(*args)
    assert [i.nodes for i in again[1]] == [i.nodes for i in info0] and again[3].calls == sb0.calls
    # the drivers that refuse the rules name them; None falls to the sequential path
    for name in (True, "refill", "ahead"):
        with pytest.raises(ValueError, match="branching_rule 2"):
            mdl.solve_many(inst[:2], lockstep=name)
    s.close()
    both = _model(pr, 1, 0.1, 1, primal_heuristic=1, rf_max_iter=250)
    with pytest.raises(ValueError, match="branching_rule 1"):
        both.solve_many(inst[:2], lockstep="device")
    both.work.solver.close()
