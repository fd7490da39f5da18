"""Strong and reliability branching in the lock-step trees: the host logic (miosqp_amd/csrc/lockstep_sb.hpp beside
lockstep_trees.hpp) checked on the CPU.

The headers are plain C++; they are compiled with g++ into a throw-away library together with
tests/lockstep_sb_harness.cpp (a test-only wrapper), nothing here touches a GPU.  The reference is the sequential solve
with branching_rule 1 and 2 on the CPU oracle (`solve_many(lockstep=False)`: update_vectors + set_x0 + solve per
instance) with logging wrapped around `choose_leaf`, `bound_and_branch`, `strong_branch` and `branch_children`: per node
the chosen list index, the record of the solved leaf (tests/test_lockstep_trees_cpu.py::_record), its x at the integer
positions, the strong-branching call's candidates and children, the position the children were made on and the open
list (depth, inherited bound) afterwards.  The children are keyed by (node, position, side): the C++ trees ask for the
children of the candidates THEY chose.  Every tree must choose the same index and the same position at every node,
hold the same open list after every node and end with the same upper bound (equal as floats: the values are fed in),
node count, iteration count, strong-branching counters and -- rule 2 -- the same pc_sum / pc_cnt bit for bit; one tree
at a time (1), three (3) and all seven (7) interleaved wave by wave on one shared free list.

Seeds: problems.random_miqp(40, 60, 20, seed=2) with the instances of test_lockstep_trees_cpu.py (RandomState(11)), as
named by that file.

`np_mean` / `pseudo_costs` of the header restate numpy's summation order (pairwise, blocks of 128, eight
accumulators); one case holds them to `Workspace.pseudo_costs` at 1, 7, 8, 9, 127, 128, 129 and 300 observed positions.

A stand-alone program over the same headers (tests/lockstep_sb_fuzz.cpp) is built with -fsanitize=address,undefined and
run as a subprocess."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import test_lockstep_trees_cpu as base
from miosqp_amd import bnb, problems

HERE = os.path.dirname(os.path.abspath(__file__))
dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int)
i64p = C.POINTER(C.c_int64)


@pytest.fixture(scope="module")
def lbh(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lbh") / "liblbh.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared",
                           os.path.join(HERE, "lockstep_sb_harness.cpp"), "-o", out])
    L = C.CDLL(out)
    L.lbh_new.restype = C.c_void_p
    L.lbh_new.argtypes = [C.c_int, C.c_int, dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double]
    L.lbh_free.argtypes = [C.c_void_p]
    L.lbh_can_continue.argtypes = [C.c_void_p, C.c_int, C.c_int64]
    L.lbh_choose.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.lbh_begin.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_double]
    L.lbh_ask.argtypes = [C.c_void_p, C.c_int, dp]
    L.lbh_ncand.argtypes = [C.c_void_p, C.c_int]
    L.lbh_cand.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.lbh_decide.argtypes = [C.c_void_p, C.c_int, ip, ip, dp, ip]
    L.lbh_end.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.lbh_end.restype = None
    L.lbh_open.argtypes = [C.c_void_p, C.c_int]
    L.lbh_open_depth.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.lbh_open_lower.restype = C.c_double
    L.lbh_open_lower.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.lbh_upper.restype = C.c_double
    L.lbh_upper.argtypes = [C.c_void_p, C.c_int]
    for name in ("lbh_nodes", "lbh_iters"):
        getattr(L, name).restype = C.c_int64
        getattr(L, name).argtypes = [C.c_void_p, C.c_int]
    L.lbh_sb.restype = C.c_int64
    L.lbh_sb.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.lbh_pc.restype = None
    L.lbh_pc.argtypes = [C.c_void_p, C.c_int, dp, i64p]
    for name in ("lbh_grown", "lbh_cap", "lbh_free_slots"):
        getattr(L, name).argtypes = [C.c_void_p]
    L.lbh_pseudo_costs.restype = None
    L.lbh_pseudo_costs.argtypes = [C.c_int, dp, i64p, dp]
    return L


def _model(oracle_mod, pr, rule, br, cap=None, **more):
    st = dict(problems.BNB_SETTINGS, tree_explor_rule=rule, branching_rule=br, sb_max_iter=50)
    st.update(more)
    if cap is not None:
        st["max_iter_bb"] = cap
    mdl = bnb.MIOSQP(backend=oracle_mod)
    mdl.setup(pr["P"], pr["q"], pr["A"], pr["l"].copy(), pr["u"].copy(), pr["i_idx"], pr["i_l"], pr["i_u"], st,
              dict(problems.QP_SETTINGS))
    return mdl


def _recorded(oracle_mod, monkeypatch, pr, inst, rule, br, cap=None, **more):
    """the sequential path on the oracle with the log: per instance the list of its nodes (chosen index, leaves before,
    record, x at the integer positions, the strong-branching call or None, the branching position or -1, the open list
    after, upper after), its sb_stats and its pseudo-cost tables; the children of all calls keyed by (instance, node,
    position, side)"""
    mdl = _model(oracle_mod, pr, rule, br, cap, **more)
    logs, stats, tables, kids, cur = [], [], [], {}, {}
    choose0, bb0, sb0, bc0, solve0 = bnb.Workspace.choose_leaf, bnb.Workspace.bound_and_branch, \
        bnb.Workspace.strong_branch, bnb.Workspace.branch_children, bnb.MIOSQP.solve

    def choose(self, r):
        cur["idx"] = (self.leaf_index(r), len(self.leaves))
        return choose0(self, r)

    def sb(self, leaf, cand):
        r = sb0(self, leaf, cand)
        assert cur["call"] is None  # one call per node at the most
        K = len(cand)
        cur["call"] = dict(cand=[int(c) for c in cand], chosen=int(r.chosen))
        for side in (0, 1):
            for j, c in enumerate(cand):
                b = side * K + j
                kids[(len(logs) - 1, len(logs[-1]), int(c), side)] = (int(r.status[b] in self.ok), int(r.iter[b]),
                                                                      float(r.lower[b]))
        return r

    def bc(self, leaf):
        cur["pos"] = int(leaf.constr_idx - self.data.m)
        return bc0(self, leaf)

    def bb(self, leaf):
        rec = base._record(self, leaf)
        cur["call"], cur["pos"] = None, -1
        bb0(self, leaf)
        idx, before = cur["idx"]
        xi = np.array(leaf.x[self.data.i_idx], dtype=float) if rec["ok"] else None
        logs[-1].append((idx, before, rec, xi, cur["call"], cur["pos"], [(int(lf.depth), float(lf.lower)) for lf in self.leaves],
                         float(self.upper_glob)))

    def solve(self, *a, **kw):
        logs.append([])
        res = solve0(self, *a, **kw)
        stats.append(dict(self.work.sb_stats))
        tables.append((self.work.pc_sum.copy(), self.work.pc_cnt.copy()))
        return res

    monkeypatch.setattr(bnb.Workspace, "choose_leaf", choose)
    monkeypatch.setattr(bnb.Workspace, "bound_and_branch", bb)
    monkeypatch.setattr(bnb.Workspace, "strong_branch", sb)
    monkeypatch.setattr(bnb.Workspace, "branch_children", bc)
    monkeypatch.setattr(bnb.MIOSQP, "solve", solve)
    out = mdl.solve_many(inst, lockstep=False)
    monkeypatch.undo()
    assert len(logs) == len(stats) == len(inst)
    assert [len(lg) for lg in logs] == [o["nodes"] for o in out]
    return types.SimpleNamespace(mdl=mdl, out=out, logs=logs, stats=stats, tables=tables, kids=kids)


def _replay(lbh, R, up0, rule, br, max_iter_bb, trees, capacity=4):
    """the trees `trees` (indices into the logs) in ONE harness, wave by wave: all choose, all begin, the branching
    step for those that branch, all end"""
    logs, out, sb = R.logs, R.out, R.mdl.work.sb
    p = R.mdl.work.data.n_int
    up = np.ascontiguousarray(np.minimum(up0[trees], 1.7e308), dtype=np.float64)
    h = lbh.lbh_new(len(trees), capacity, up.ctypes.data_as(dp), p, br, sb["K"], sb["reliability"], sb["eps"],
                    R.mdl.work.settings["eps_int_feas"])
    try:
        for w in range(max(len(logs[k]) for k in trees)):
            live = [t for t, k in enumerate(trees) if w < len(logs[k])]
            assert live == [t for t in range(len(trees)) if lbh.lbh_can_continue(h, t, max_iter_bb)], w
            for t in live:
                idx, before = logs[trees[t]][w][:2]
                assert lbh.lbh_open(h, t) == before, (w, t)
                assert lbh.lbh_choose(h, t, rule) == idx, (w, t)
            chosen = {}
            for t in live:
                k = trees[t]
                idx, before, rec, xi, call, pos, after, upper = logs[k][w]
                v = lbh.lbh_begin(h, t, int(rec["ok"]), rec["iter"], rec["lower"], rec["int_inf"], rec["nextvar"],
                                  int(rec["heur_feasible"]), rec["heur_obj"])
                assert bool(v & 1) == (pos >= 0), (w, t)
                chosen[t] = -1
                if not v & 1:
                    continue
                x = np.ascontiguousarray(xi)
                got = lbh.lbh_ask(h, t, x.ctypes.data_as(dp))
                if got == -1:
                    assert call is not None, (w, t)
                    cand = [lbh.lbh_cand(h, t, j) for j in range(lbh.lbh_ncand(h, t))]
                    assert cand == call["cand"], (w, t)
                    ch = [R.kids[(k, w, c, side)] for side in (0, 1) for c in cand]  # KeyError: a child nobody solved
                    has = (C.c_int * len(ch))(*[c[0] for c in ch])
                    it = (C.c_int * len(ch))(*[c[1] for c in ch])
                    lo = (C.c_double * len(ch))(*[c[2] for c in ch])
                    best = C.c_int(-1)
                    got = lbh.lbh_decide(h, t, has, it, lo, C.byref(best))
                    assert best.value == call["chosen"], (w, t)
                else:
                    assert call is None, (w, t)
                assert got == pos, (w, t, got, pos)
                chosen[t] = got
            for t in live:
                idx, before, rec, xi, call, pos, after, upper = logs[trees[t]][w]
                lbh.lbh_end(h, t, chosen[t])
                mine = [(lbh.lbh_open_depth(h, t, i), lbh.lbh_open_lower(h, t, i)) for i in range(lbh.lbh_open(h, t))]
                assert mine == after, (w, t)
                assert lbh.lbh_upper(h, t) == upper, (w, t)
        assert not any(lbh.lbh_can_continue(h, t, max_iter_bb) for t in range(len(trees)))
        for t, k in enumerate(trees):
            o, s = out[k], R.stats[k]
            assert (lbh.lbh_nodes(h, t), lbh.lbh_iters(h, t)) == (o["nodes"], o["osqp_iter"]), k
            assert lbh.lbh_upper(h, t) == o["upper_glob"], k
            assert [lbh.lbh_sb(h, t, j) for j in range(3)] == [s["calls"], s["children"], s["osqp_iter"]], k
            pc_sum, pc_cnt = np.zeros((2, p)), np.zeros((2, p), dtype=np.int64)
            lbh.lbh_pc(h, t, pc_sum.ctypes.data_as(dp), pc_cnt.ctypes.data_as(i64p))
            assert np.array_equal(pc_cnt, R.tables[k][1]), k
            assert pc_sum.tobytes() == np.ascontiguousarray(R.tables[k][0]).tobytes(), k  # bit for bit
        if all(lbh.lbh_open(h, t) == 0 for t in range(len(trees))):  # every slot came back
            assert lbh.lbh_free_slots(h) == lbh.lbh_cap(h)
        return lbh.lbh_grown(h)
    finally:
        lbh.lbh_free(h)


@pytest.fixture(scope="module")
def prob():
    return problems.random_miqp(40, 60, 20, seed=2)


@pytest.mark.parametrize("br", [1, 2])
@pytest.mark.parametrize("rule", [1, 3])
def test_cpp_trees_replay_the_sequential_solves_with_strong_branching(lbh, oracle_mod, monkeypatch, prob, rule, br):
    inst = base._instances(prob)
    R = _recorded(oracle_mod, monkeypatch, prob, inst, rule, br)
    cap = R.mdl.work.settings["max_iter_bb"]
    assert R.out[6]["status"] == bnb.MI_PRIMAL_INFEASIBLE and R.out[5]["upper_glob"] < np.inf
    print("rule %d branching %d: nodes %s calls %s" % (rule, br, [o["nodes"] for o in R.out], [s["calls"] for s in R.stats]))
    # the run means something: strong branching ran in every feasible tree, never in the infeasible one
    assert all(s["calls"] >= 1 for s in R.stats[:6]) and R.stats[6]["calls"] == 0
    if br == 2:  # ... and reliability branching has observations and nodes decided by pseudo-costs alone
        assert all(t[1].sum() > 0 for t in R.tables[:6])
        assert any(call is None and pos >= 0 for lg in R.logs for (_, _, _, _, call, pos, _, _) in lg)
    else:
        assert all(t[1].sum() == 0 for t in R.tables)
    up0 = base._upper0(R.mdl, inst)
    for k in range(len(inst)):  # one tree at a time
        _replay(lbh, R, up0, rule, br, cap, [k], capacity=2)
    _replay(lbh, R, up0, rule, br, cap, [5, 2, 4])  # three
    grown = _replay(lbh, R, up0, rule, br, cap, list(range(len(inst))))  # seven, on one shared free list
    assert grown > 1  # the store started at 4 slots for 7 roots


@pytest.mark.parametrize("br", [1, 2])
def test_cpp_trees_with_few_candidates_and_a_cap(lbh, oracle_mod, monkeypatch, prob, br):
    """sb_candidates below the fractional set (the most-fractional cut decides), sb_reliability 1, max_iter_bb mid-search"""
    inst = base._instances(prob)
    R = _recorded(oracle_mod, monkeypatch, prob, inst, 1, br, cap=9, sb_candidates=2, sb_reliability=1)
    capped = [o for o in R.out if o["status"] in (bnb.MI_MAX_ITER_FEASIBLE, bnb.MI_MAX_ITER_UNSOLVED)]
    assert capped and all(o["nodes"] == 8 for o in capped)
    assert any(call is not None and len(call["cand"]) == 2 and rec["int_inf"] > 2
               for lg in R.logs for (_, _, rec, _, call, _, _, _) in lg)
    _replay(lbh, R, base._upper0(R.mdl, inst), 1, br, 9, list(range(len(inst))))


@pytest.mark.parametrize("count", [1, 7, 8, 9, 127, 128, 129, 300])
def test_pseudo_costs_restate_numpys_mean(lbh, count):
    """`count` observed positions per direction among count + 5: the mean over them, which the unobserved positions
    get, follows numpy's summation order (n < 8: a plain loop; up to 128: eight accumulators; beyond: halves)"""
    rng = np.random.RandomState(count)
    p = count + 5
    work = bnb.Workspace.__new__(bnb.Workspace)
    work.data = types.SimpleNamespace(n_int=p)
    work.pc_sum = np.zeros((2, p))
    work.pc_cnt = np.zeros((2, p), dtype=np.int64)
    for side in (0, 1):
        have = rng.permutation(p)[:count]
        work.pc_cnt[side, have] = rng.randint(1, 9, size=count)
        work.pc_sum[side, have] = rng.rand(count) * 10.0 ** rng.uniform(-3, 3, size=count)
    want = work.pseudo_costs()
    got = np.zeros((2, p))
    lbh.lbh_pseudo_costs(p, work.pc_sum.ctypes.data_as(dp), work.pc_cnt.ctypes.data_as(i64p), got.ctypes.data_as(dp))
    assert got.tobytes() == np.ascontiguousarray(want).tobytes()
    none = np.zeros((2, p))
    lbh.lbh_pseudo_costs(p, none.ctypes.data_as(dp), np.zeros((2, p), dtype=np.int64).ctypes.data_as(i64p), got.ctypes.data_as(dp))
    assert np.array_equal(got, np.ones((2, p)))


def test_sanitized_random_records_candidates_and_children(tmp_path):
    exe = str(tmp_path / "lockstep_sb_fuzz")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(HERE, "lockstep_sb_fuzz.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "lockstep_sb_fuzz ok" in r.stdout


def test_the_drivers_that_refuse_the_rules_name_them(oracle_mod, prob):
    inst = base._instances(prob)[:2]
    for br in (1, 2):
        mdl = _model(oracle_mod, prob, 1, br)
        with pytest.raises(ValueError, match="branching_rule %d" % br):
            mdl.solve_many(inst, lockstep=True)
        for name in ("refill", "ahead"):
            with pytest.raises(ValueError):  # (on the oracle: no entry; on the HIP engine: the rule -- tests/test_gpu_lockstep_sb.py)
                mdl.solve_many(inst, lockstep=name)
        with pytest.raises(ValueError):  # the oracle has no device driver at all
            mdl.solve_many(inst, lockstep="device")
        assert not hasattr(mdl.work, "lockstep")
        got = mdl.solve_many(inst)  # None falls to the sequential path with the rule on
        assert all(g["status"] == bnb.MI_SOLVED for g in got)


def test_device_sb_supported_reads_the_settings(oracle_mod, prob):
    from miosqp_amd import lockstep
    mdl = _model(oracle_mod, prob, 1, 1)
    assert not lockstep.device_sb_supported(mdl.work)  # no entry, no root on the device

    class Stub(object):
        solve_trees_lockstep_sb = None

    work = bnb.Workspace.__new__(bnb.Workspace)
    work.solver, work.root_on_device, work.data = Stub(), True, mdl.work.data
    for rule, br, rf_on, want in ((0, 1, False, True), (3, 2, False, True), (1, 0, False, False), (1, 1, True, False),
                                  (4, 2, False, False)):
        work.settings = dict(mdl.work.settings, tree_explor_rule=rule, branching_rule=br)
        work.rf = dict(on=rf_on)
        assert lockstep.device_sb_supported(work) is want, (rule, br, rf_on)
    work.root_on_device = False
    work.settings = dict(mdl.work.settings)
    work.rf = dict(on=False)
    assert not lockstep.device_sb_supported(work)
