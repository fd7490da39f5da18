"""Round and fix in the lock-step trees: the host logic (miosqp_amd/csrc/lockstep_trees.hpp, Tree::begin / heuristic /
end) checked on the CPU.

The header is plain C++; it is compiled with g++ into a throw-away library together with tests/lockstep_rf_harness.cpp
(a test-only wrapper), nothing here touches a GPU.  The reference is the sequential solve with primal_heuristic = 1 on
the CPU oracle (`solve_many(lockstep=False)`: update_vectors + set_x0 + solve per instance) with logging wrapped around
`choose_leaf`, `bound_and_branch` and `round_and_fix`: per node the chosen list index, the record of the solved leaf
(tests/test_lockstep_trees_cpu.py::_record), whether round and fix ran there and -- from its per-candidate arrays --
the feasible count, the iterations and the lowest objective among the candidates that count (the argmin WITHOUT the
`< upper_glob` filter of Workspace.round_and_fix: the C++ tree applies that test once, to the winner).  The records are
fed to the C++ trees, which must choose the same index at every node, fire at the same nodes, hold the same list length
after every node and end with the same upper bound (equal as floats: the values are fed in), node count, iteration count
and heuristic counters -- one tree at a time, and all trees interleaved wave by wave on one shared free list.

Seeds: problems.random_miqp(40, 60, 20, seed=2) with the instances of test_lockstep_trees_cpu.py (RandomState(11)), as
named by that file; with rf_every 1 and 3 every feasible tree fires at least twice and the heuristic improves an
incumbent (asserted below on the reference's own rf_stats).

A stand-alone program over the same header (tests/lockstep_rf_fuzz.cpp) is built with -fsanitize=address,undefined and
run as a subprocess: random records and heuristic outcomes through several trees sharing one free list, growth
included."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_lockstep_trees_cpu as base
from miosqp_amd import bnb, problems

HERE = os.path.dirname(os.path.abspath(__file__))
dp = C.POINTER(C.c_double)
RF = dict(primal_heuristic=1, rf_max_iter=250)


@pytest.fixture(scope="module")
def lrh(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lrh") / "liblrh.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared",
                           os.path.join(HERE, "lockstep_rf_harness.cpp"), "-o", out])
    L = C.CDLL(out)
    L.lrh_new.restype = C.c_void_p
    L.lrh_new.argtypes = [C.c_int, C.c_int, dp, C.c_int]
    L.lrh_free.argtypes = [C.c_void_p]
    L.lrh_can_continue.argtypes = [C.c_void_p, C.c_int, C.c_int64]
    L.lrh_choose.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.lrh_begin.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_double]
    L.lrh_heuristic.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int64]
    L.lrh_end.argtypes = [C.c_void_p, C.c_int]
    L.lrh_end.restype = None
    L.lrh_open.argtypes = [C.c_void_p, C.c_int]
    L.lrh_upper.restype = C.c_double
    L.lrh_upper.argtypes = [C.c_void_p, C.c_int]
    for name in ("lrh_nodes", "lrh_iters"):
        getattr(L, name).restype = C.c_int64
        getattr(L, name).argtypes = [C.c_void_p, C.c_int]
    L.lrh_rf.restype = C.c_int64
    L.lrh_rf.argtypes = [C.c_void_p, C.c_int, C.c_int]
    for name in ("lrh_grown", "lrh_cap", "lrh_free_slots"):
        getattr(L, name).argtypes = [C.c_void_p]
    return L


def _model(oracle_mod, pr, rule, every, cap=None, **more):
    st = dict(problems.BNB_SETTINGS, tree_explor_rule=rule, rf_every=every, **RF)
    st.update(more)
    if cap is not None:
        st["max_iter_bb"] = cap
    mdl = bnb.MIOSQP(backend=oracle_mod)
    mdl.setup(pr["P"], pr["q"], pr["A"], pr["l"].copy(), pr["u"].copy(), pr["i_idx"], pr["i_l"], pr["i_u"], st,
              dict(problems.QP_SETTINGS))
    return mdl


def _call_outcome(work, r):
    """what the device's judge reports of one round_and_fix call: feasible count, the lowest objective among the
    candidates that count (ties to the lowest k) or None, and the candidates' iterations"""
    best = None
    for k in range(len(r.obj)):
        if r.status[k] not in work.ok or not r.viol[k] <= 0.0:
            continue
        if best is None or r.obj[k] < r.obj[best]:
            best = k
    return dict(feasible=int(r.feasible), obj=None if best is None else float(r.obj[best]), iters=int(r.iters),
                chosen=int(r.chosen))


def _recorded(oracle_mod, monkeypatch, pr, inst, rule, every, cap=None):
    """the sequential path on the oracle with the log: per instance the list of its nodes (chosen index, leaves before,
    record, the heuristic call's outcome or None, leaves after, upper after) and its rf_stats"""
    mdl = _model(oracle_mod, pr, rule, every, cap)
    logs, stats, cur = [], [], {}
    choose0, bb0, rf0, solve0 = bnb.Workspace.choose_leaf, bnb.Workspace.bound_and_branch, bnb.Workspace.round_and_fix, \
        bnb.MIOSQP.solve

    def choose(self, r):
        cur["idx"] = (self.leaf_index(r), len(self.leaves))
        return choose0(self, r)

    def rf(self, leaf):
        r = rf0(self, leaf)
        assert cur["call"] is None  # one call per node at the most
        cur["call"] = _call_outcome(self, r)
        return r

    def bb(self, leaf):
        rec = base._record(self, leaf)
        cur["call"] = None
        bb0(self, leaf)
        idx, before = cur["idx"]
        logs[-1].append((idx, before, rec, cur["call"], len(self.leaves), float(self.upper_glob)))

    def solve(self, *a, **kw):
        logs.append([])
        res = solve0(self, *a, **kw)
        stats.append(dict(self.work.rf_stats))
        return res

    monkeypatch.setattr(bnb.Workspace, "choose_leaf", choose)
    monkeypatch.setattr(bnb.Workspace, "bound_and_branch", bb)
    monkeypatch.setattr(bnb.Workspace, "round_and_fix", rf)
    monkeypatch.setattr(bnb.MIOSQP, "solve", solve)
    out = mdl.solve_many(inst, lockstep=False)
    monkeypatch.undo()
    assert len(logs) == len(stats) == len(inst)
    assert [len(lg) for lg in logs] == [o["nodes"] for o in out]
    return mdl, out, logs, stats


def _replay(lrh, logs, out, stats, up0, rule, every, K, max_iter_bb, trees, capacity=4):
    """the trees `trees` (indices into logs) in ONE harness, wave by wave: all choose, all begin, the heuristic for those
    that fired, all end"""
    up = np.ascontiguousarray(np.minimum(up0[trees], 1.7e308), dtype=np.float64)
    h = lrh.lrh_new(len(trees), capacity, up.ctypes.data_as(dp), every)
    try:
        for w in range(max(len(logs[k]) for k in trees)):
            live = [t for t, k in enumerate(trees) if w < len(logs[k])]
            assert live == [t for t in range(len(trees)) if lrh.lrh_can_continue(h, t, max_iter_bb)], w
            for t in live:
                idx, before, rec, call, after, upper = logs[trees[t]][w]
                assert lrh.lrh_open(h, t) == before, (w, t)
                assert lrh.lrh_choose(h, t, rule) == idx, (w, t)
            fired = []
            for t in live:
                idx, before, rec, call, after, upper = logs[trees[t]][w]
                v = lrh.lrh_begin(h, t, int(rec["ok"]), rec["iter"], rec["lower"], rec["int_inf"], rec["nextvar"],
                                  int(rec["heur_feasible"]), rec["heur_obj"])
                assert bool(v >> 3) == (call is not None), (w, t)  # fire / no fire
                if call is not None:
                    fired.append(t)
            for t in fired:
                idx, before, rec, call, after, upper = logs[trees[t]][w]
                imp = lrh.lrh_heuristic(h, t, K, int(call["obj"] is not None), 0.0 if call["obj"] is None else call["obj"],
                                        call["feasible"], call["iters"])
                assert bool(imp) == (call["chosen"] >= 0), (w, t)  # the one `< upper` test chooses what k_rf_pick's rule chooses
            for t in live:
                idx, before, rec, call, after, upper = logs[trees[t]][w]
                lrh.lrh_end(h, t)
                assert lrh.lrh_open(h, t) == after, (w, t)
                assert lrh.lrh_upper(h, t) == upper, (w, t)
        assert not any(lrh.lrh_can_continue(h, t, max_iter_bb) for t in range(len(trees)))
        for t, k in enumerate(trees):
            o, s = out[k], stats[k]
            assert (lrh.lrh_nodes(h, t), lrh.lrh_iters(h, t)) == (o["nodes"], o["osqp_iter"]), k
            assert lrh.lrh_upper(h, t) == o["upper_glob"], k
            assert [lrh.lrh_rf(h, t, j) for j in range(5)] == \
                [s["calls"], s["candidates"], s["feasible"], s["improved"], s["osqp_iter"]], k
        if all(lrh.lrh_open(h, t) == 0 for t in range(len(trees))):  # every slot came back
            assert lrh.lrh_free_slots(h) == lrh.lrh_cap(h)
        return lrh.lrh_grown(h)
    finally:
        lrh.lrh_free(h)


@pytest.fixture(scope="module")
def prob():
    return problems.random_miqp(40, 60, 20, seed=2)


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("rule", [0, 1, 2, 3])
def test_cpp_trees_replay_the_sequential_solves_with_round_and_fix(lrh, oracle_mod, monkeypatch, prob, rule, every):
    inst = base._instances(prob)
    mdl, out, logs, stats = _recorded(oracle_mod, monkeypatch, prob, inst, rule, every)
    K, cap = mdl.work.rf["K"], mdl.work.settings["max_iter_bb"]
    assert out[6]["status"] == bnb.MI_PRIMAL_INFEASIBLE and out[5]["upper_glob"] < np.inf
    # the run means something: every feasible tree fires at least twice, and the heuristic improves an incumbent somewhere
    print("rule %d every %d: calls %s improved %s" % (rule, every, [s["calls"] for s in stats], [s["improved"] for s in stats]))
    assert all(s["calls"] >= 2 for s in stats[:6]) and stats[6]["calls"] == 0
    assert sum(s["improved"] for s in stats) >= 1
    up0 = base._upper0(mdl, inst)
    for k in range(len(inst)):  # one tree at a time
        _replay(lrh, logs, out, stats, up0, rule, every, K, cap, [k], capacity=2)
    # all trees interleaved wave by wave on one shared free list: the same per-tree results
    grown = _replay(lrh, logs, out, stats, up0, rule, every, K, cap, list(range(len(inst))))
    assert grown > 1  # the store started at 4 slots for 7 roots
    _replay(lrh, logs, out, stats, up0, rule, every, K, cap, [5, 2, 4])


def test_cpp_trees_with_round_and_fix_stop_at_max_iter_bb(lrh, oracle_mod, monkeypatch, prob):
    inst = base._instances(prob)
    mdl, out, logs, stats = _recorded(oracle_mod, monkeypatch, prob, inst, 1, 3, cap=6)
    capped = [o for o in out if o["status"] in (bnb.MI_MAX_ITER_FEASIBLE, bnb.MI_MAX_ITER_UNSOLVED)]
    assert capped and all(o["nodes"] == 5 for o in capped)
    _replay(lrh, logs, out, stats, base._upper0(mdl, inst), 1, 3, mdl.work.rf["K"], 6, list(range(len(inst))))


def test_begin_heuristic_end_by_hand(lrh):
    up = np.array([1.7e308])
    h = lrh.lrh_new(1, 4, up.ctypes.data_as(dp), 2)
    try:
        lrh.lrh_choose(h, 0, 1)
        # fractional, the rounded point is feasible with value 9: incumbent by the rounding (2), branching (1), first asking node fires (8)
        assert lrh.lrh_begin(h, 0, 1, 7, 2.0, 3, 4, 1, 9.0) == (1 | 2 << 1 | 1 << 3)
        assert lrh.lrh_open(h, 0) == 0  # the children are not in the list yet
        assert lrh.lrh_heuristic(h, 0, 7, 1, 9.0, 3, 70) == 0  # equal is not better
        assert lrh.lrh_heuristic(h, 0, 7, 0, 1.0, 0, 70) == 0  # nothing counted: the objective means nothing
        assert lrh.lrh_upper(h, 0) == 9.0
        lrh.lrh_end(h, 0)
        assert lrh.lrh_open(h, 0) == 2
        # the second asking node does not fire under rf_every = 2, the third does
        lrh.lrh_choose(h, 0, 1)
        assert lrh.lrh_begin(h, 0, 1, 5, 3.0, 2, 1, 0, 0.0) == 1
        lrh.lrh_end(h, 0)
        lrh.lrh_choose(h, 0, 1)
        assert lrh.lrh_begin(h, 0, 0, 5, float("nan"), -1, -1, 0, float("nan")) == 0  # infeasible: does not ask
        lrh.lrh_end(h, 0)
        lrh.lrh_choose(h, 0, 1)
        assert lrh.lrh_begin(h, 0, 1, 5, 3.5, 0, -1, 0, 0.0) == 1 << 1  # integral: incumbent 1, no heuristic
        lrh.lrh_end(h, 0)
        assert lrh.lrh_upper(h, 0) == 3.5
        lrh.lrh_choose(h, 0, 1)
        assert lrh.lrh_begin(h, 0, 1, 5, 3.2, 2, 1, 0, 0.0) == (1 | 1 << 3)
        assert lrh.lrh_heuristic(h, 0, 7, 1, 3.25, 2, 60) == 1  # better: the incumbent
        assert lrh.lrh_upper(h, 0) == 3.25 and lrh.lrh_open(h, 0) == 0
        lrh.lrh_end(h, 0)
        assert lrh.lrh_open(h, 0) == 2  # the children enter whatever the new incumbent is (branch_children)
        assert [lrh.lrh_rf(h, 0, j) for j in range(5)] == [3, 21, 5, 1, 200]
        assert lrh.lrh_nodes(h, 0) == 5 and lrh.lrh_iters(h, 0) == 27
    finally:
        lrh.lrh_free(h)


def test_sanitized_random_records_and_heuristic_outcomes(tmp_path):
    exe = str(tmp_path / "lockstep_rf_fuzz")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(HERE, "lockstep_rf_fuzz.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "lockstep_rf_fuzz ok" in r.stdout


def test_the_other_drivers_keep_refusing_the_heuristic(oracle_mod, prob):
    inst = base._instances(prob)[:2]
    mdl = _model(oracle_mod, prob, 1, 3)
    with pytest.raises(ValueError, match="primal_heuristic 0"):
        mdl.solve_many(inst, lockstep=True)
    with pytest.raises(ValueError):  # (on the oracle: no entry; on the HIP engine: the heuristic -- tests/test_gpu_lockstep_rf.py)
        mdl.solve_many(inst, lockstep="refill")
    with pytest.raises(ValueError):  # the oracle has no device driver at all
        mdl.solve_many(inst, lockstep="device")
    other = _model(oracle_mod, prob, 1, 3, branching_rule=1)
    with pytest.raises(ValueError):
        other.solve_many(inst, lockstep="device")
    with pytest.raises(ValueError, match="branching_rule 0"):
        other.solve_many(inst, lockstep=True)
    assert not hasattr(mdl.work, "lockstep") and not hasattr(other.work, "lockstep")
    # None falls to the sequential path with the heuristic on
    got = mdl.solve_many(inst)
    assert all(g["status"] == bnb.MI_SOLVED for g in got)


def test_device_rf_supported_reads_the_settings(oracle_mod, prob):
    """`device_rf_supported` without an engine: the entry is what decides on the oracle; with a stand-in solver that has
    it, the settings decide"""
    from miosqp_amd import lockstep
    mdl = _model(oracle_mod, prob, 1, 3)
    assert not lockstep.device_rf_supported(mdl.work)  # no entry, no root on the device

    class Stub(object):
        solve_trees_lockstep_rf = None

    work = bnb.Workspace.__new__(bnb.Workspace)
    work.solver, work.root_on_device, work.data = Stub(), True, mdl.work.data
    for rule, br, want in ((0, 0, True), (3, 0, True), (1, 1, False), (1, 2, False), (4, 0, False)):
        work.settings = dict(mdl.work.settings, tree_explor_rule=rule, branching_rule=br)
        assert lockstep.device_rf_supported(work) is want, (rule, br)
    work.root_on_device = False
    work.settings = dict(mdl.work.settings)
    assert not lockstep.device_rf_supported(work)
