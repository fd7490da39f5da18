"""The host logic of the lock-step trees whose spare columns solve open leaves early (miosqp_amd/csrc/lockstep_ahead.hpp)
checked on the CPU.

The header is plain C++; it is compiled with g++ into a throw-away library together with tests/lockstep_ahead_harness.cpp
(a test-only wrapper), nothing here touches a GPU.  `lockstep.run` runs on the CPU oracle, on the instances and under the
rules of tests/test_lockstep_trees_cpu.py, with logging wrapped around `choose_leaf` and `bound_and_branch`: per tree the
sequence of absorbed nodes -- each known by its PATH from the root --, the chosen list index, the node's record and the
list length and incumbent value afterwards.  The harness replays the trees with ahead in {1, 2, 8} and B = 1, 3 and all
instances: a recorded node answers with its record, every node OUTSIDE the recorded set with an adversarial record
drawn from a seed (infeasible, integral with a tiny objective, crossed, huge iteration counts).  Every tree must end
with the recorded sequence of absorbed nodes, the recorded index, list length and incumbent after every absorb and the
recorded nodes, iters, upper, lower_glob, leaves_left and max_open: what is solved ahead and never reached cannot matter.

Call-off model: an ahead column is finished iff ceil(iter / check_termination) <= the wave's largest mandatory chunk
count.

A stand-alone program over the same header (tests/lockstep_ahead_fuzz.cpp) is built with -fsanitize=address,undefined
and run as a subprocess: random pure record functions against `Tree` driven one node per wave."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_lockstep_trees_cpu as base
from miosqp_amd import bnb, lockstep

HERE = os.path.dirname(os.path.abspath(__file__))
dp = C.POINTER(C.c_double)
CT = 25  # check_termination of the call-off model (the engine's default chunk)
_CACHE = {}


@pytest.fixture(scope="module")
def lah(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lah") / "liblah.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared",
                           os.path.join(HERE, "lockstep_ahead_harness.cpp"), "-o", out])
    L = C.CDLL(out)
    L.lah_new.restype = C.c_void_p
    L.lah_new.argtypes = [C.c_int, dp]
    L.lah_free.argtypes = [C.c_void_p]
    L.lah_add_node.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int,
                               C.c_double]
    L.lah_run.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_uint64]
    for name in ("lah_slots_complete", "lah_waves", "lah_grown", "lah_free_slots", "lah_cap"):
        getattr(L, name).argtypes = [C.c_void_p]
    L.lah_wave_width.argtypes = [C.c_void_p, C.c_int]
    for name in ("lah_mandatory_chunks", "lah_columns"):
        getattr(L, name).restype = C.c_int64
        getattr(L, name).argtypes = [C.c_void_p]
    L.lah_count.restype = C.c_int64
    L.lah_count.argtypes = [C.c_void_p, C.c_int]
    for name in ("lah_log_len", "lah_open", "lah_max_open", "lah_found", "lah_finished_at"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_int]
    L.lah_log.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                          C.POINTER(C.c_int), dp]
    for name in ("lah_upper", "lah_lower_glob"):
        getattr(L, name).restype = C.c_double
        getattr(L, name).argtypes = [C.c_void_p, C.c_int]
    for name in ("lah_nodes", "lah_iters"):
        getattr(L, name).restype = C.c_int64
        getattr(L, name).argtypes = [C.c_void_p, C.c_int]
    return L


def _recorded(oracle_mod, monkeypatch, pr, rule, cap=None):
    """lockstep.run on the oracle, once per (rule, cap): per tree, in the order of the instances, the absorbed nodes
    [(path, chosen index, record, leaves after, upper after)] and dict(nodes, iters, upper, lower_glob, leaves_left,
    max_open); the number of waves; the incumbent values the trees started with"""
    key = (rule, cap)
    if key in _CACHE:
        return _CACHE[key]
    inst = base._instances(pr)
    mdl = base._model(oracle_mod, pr, rule, cap)
    order, trees, logs, path, keep, chosen, max_open = {}, [], [], {}, [], {}, []
    choose0, bb0 = lockstep._Tree.choose_leaf, lockstep._Tree.bound_and_branch

    def number(tree):
        if id(tree) not in order:
            order[id(tree)] = len(order)
            trees.append(tree)
            logs.append([])
            max_open.append(1)
            path[id(tree.leaves[0])] = ""
            keep.append(tree.leaves[0])  # (a node's id is its key: it must stay alive)
        return order[id(tree)]

    def choose(self, r):
        t = number(self)
        chosen[t] = self.leaf_index(r)
        return choose0(self, r)

    def bb(self, leaf):
        t = order[id(self)]
        rec = base._record(self, leaf)
        before = set(id(lf) for lf in self.leaves)
        bb0(self, leaf)
        kids = [lf for lf in self.leaves if id(lf) not in before]
        assert len(kids) in (0, 2) and kids == self.leaves[len(self.leaves) - len(kids):]
        for c, lf in enumerate(kids):  # add_left (the lowered upper bound) first
            path[id(lf)] = path[id(leaf)] + "01"[c]
            keep.append(lf)
        max_open[t] = max(max_open[t], len(self.leaves))
        logs[t].append((path[id(leaf)], chosen[t], rec, len(self.leaves), float(self.upper_glob)))

    monkeypatch.setattr(lockstep._Tree, "choose_leaf", choose)
    monkeypatch.setattr(lockstep._Tree, "bound_and_branch", bb)
    out = mdl.solve_many(inst, lockstep=True)
    monkeypatch.undo()
    assert len(trees) == len(inst)
    ends = []
    for t, tree in enumerate(trees):
        assert (out[t]["nodes"], out[t]["osqp_iter"]) == (len(logs[t]), sum(e[2]["iter"] for e in logs[t]))
        lower = min(lf.lower for lf in tree.leaves) if tree.leaves else float(tree.upper_glob)
        ends.append(dict(nodes=out[t]["nodes"], iters=out[t]["osqp_iter"], upper=float(out[t]["upper_glob"]),
                         lower_glob=float(lower), leaves_left=len(tree.leaves), max_open=max_open[t]))
    res = (logs, ends, mdl.work.lockstep["waves"], base._upper0(mdl, inst), mdl.work.settings["max_iter_bb"])
    _CACHE[key] = res
    return res


def _replay(lah, logs, ends, up0, which, rule, max_iter_bb, ahead, capacity=8, seed=1):
    """the trees `which` through the harness; returns its counters"""
    up = np.ascontiguousarray(np.minimum(up0[which], 1.7e308), dtype=np.float64)
    h = lah.lah_new(len(which), up.ctypes.data_as(dp))
    try:
        for j, t in enumerate(which):
            for pth, idx, rec, after, upper in logs[t]:
                lah.lah_add_node(h, j, pth.encode(), int(rec["ok"]), rec["iter"], rec["lower"], rec["int_inf"],
                                 rec["nextvar"], int(rec["heur_feasible"]), rec["heur_obj"])
        rc = lah.lah_run(h, rule, max_iter_bb, ahead, capacity, CT, seed)
        assert rc == 0, "harness error %d (ahead %d, trees %s)" % (rc, ahead, which)
        buf = C.create_string_buffer(4096)
        idx_, open_, hit_, up_ = C.c_int(), C.c_int(), C.c_int(), C.c_double()
        for j, t in enumerate(which):
            assert lah.lah_log_len(h, j) == len(logs[t]), (t, ahead)
            for k, (pth, idx, rec, after, upper) in enumerate(logs[t]):
                lah.lah_log(h, j, k, buf, 4096, C.byref(idx_), C.byref(open_), C.byref(hit_), C.byref(up_))
                assert (buf.value.decode(), idx_.value, open_.value, up_.value) == (pth, idx, after, upper), (t, k, ahead)
            e = ends[t]
            assert (lah.lah_nodes(h, j), lah.lah_iters(h, j)) == (e["nodes"], e["iters"]), t
            assert lah.lah_upper(h, j) == e["upper"] and lah.lah_lower_glob(h, j) == e["lower_glob"], t
            assert (lah.lah_open(h, j), lah.lah_max_open(h, j)) == (e["leaves_left"], e["max_open"]), t
        # no slot leaked, none is in two places, nothing reserved is left -- also when max_iter_bb cut the run
        assert lah.lah_slots_complete(h) == 1
        if all(ends[t]["leaves_left"] == 0 for t in which):
            assert lah.lah_free_slots(h) == lah.lah_cap(h)
        sent, hits, disc, off = (lah.lah_count(h, w) for w in range(4))
        assert sent == hits + disc + off
        waves = lah.lah_waves(h)
        assert lah.lah_columns(h) == sum(lah.lah_wave_width(h, w) for w in range(waves))
        assert sum(ends[t]["nodes"] for t in which) == lah.lah_columns(h) - disc - off  # every node solved once, or dropped
        return dict(waves=waves, sent=sent, hits=hits, discarded=disc, called_off=off,
                    chunks=lah.lah_mandatory_chunks(h), grown=lah.lah_grown(h),
                    hit_iters=lah.lah_count(h, 5), wasted_iters=lah.lah_count(h, 6) + lah.lah_count(h, 7))
    finally:
        lah.lah_free(h)


@pytest.fixture(scope="module")
def prob():
    return base.problems.random_miqp(40, 60, 20, seed=2)


@pytest.mark.parametrize("rule", [0, 1, 2, 3])
def test_trees_that_solve_ahead_replay_the_recorded_trees(lah, oracle_mod, monkeypatch, prob, rule):
    logs, ends, waves, up0, cap = _recorded(oracle_mod, monkeypatch, prob, rule)
    B = len(logs)
    assert max(e["nodes"] for e in ends) > 10
    hits_b1 = 0
    for which in ([0], [3], [5], [0, 4, 6], list(range(B))):
        ref = None
        for ahead in (1, 2, 8):
            for seed in (1, 2):
                r = _replay(lah, logs, ends, up0, which, rule, cap, ahead, seed=seed)
                print("rule %d trees %s ahead %d seed %d: %s" % (rule, which, ahead, seed, r))
                if ahead == 1:
                    # the waves and choices of the existing harness: one node of every live tree per wave, nothing ahead
                    assert r["sent"] == 0 and r["waves"] == max(ends[t]["nodes"] for t in which)
                    ref = r
                    if len(which) == B:
                        assert r["waves"] == waves
                assert r["waves"] <= ref["waves"]
                if len(which) == 1:
                    # B = 1: a node is absorbed behind its own wave or as a hit, and every wave's mandatory node is one
                    # that ahead = 1 solves alone -- the waves' lengths add up to no more than there
                    assert ends[which[0]]["nodes"] == r["waves"] + r["hits"]
                    assert r["chunks"] <= ref["chunks"]
                    if ahead > 1:
                        hits_b1 += r["hits"]
    assert hits_b1 > 0  # (every rule has hits on these instances: no other seed was needed)


@pytest.mark.parametrize("rule", [1, 2])
def test_trees_that_solve_ahead_stop_at_max_iter_bb(lah, oracle_mod, monkeypatch, prob, rule):
    logs, ends, waves, up0, cap = _recorded(oracle_mod, monkeypatch, prob, rule, cap=6)
    assert cap == 6 and waves == 5 and any(e["leaves_left"] > 0 for e in ends)
    for which in ([0], [1, 2, 5], list(range(len(logs)))):
        for ahead in (1, 2, 8):
            r = _replay(lah, logs, ends, up0, which, rule, 6, ahead)
            if ahead == 1:
                assert r["waves"] == 5 and r["sent"] == 0
            assert r["waves"] <= 5


def test_the_store_grows_from_eight_slots(lah, oracle_mod, monkeypatch, prob):
    logs, ends, waves, up0, cap = _recorded(oracle_mod, monkeypatch, prob, 1)
    r = _replay(lah, logs, ends, up0, list(range(len(logs))), 1, cap, 8, capacity=8)
    assert r["grown"] >= 1 and r["hits"] > 0


def test_sanitized_random_trees(tmp_path):
    exe = str(tmp_path / "lockstep_ahead_fuzz")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(HERE, "lockstep_ahead_fuzz.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "lockstep_ahead_fuzz ok" in r.stdout


def test_ahead_driver_is_refused_on_the_oracle(oracle_mod, prob):
    mdl = base._model(oracle_mod, prob, 1)
    with pytest.raises(ValueError, match="solve_trees_lockstep_ahead"):
        mdl.solve_many(base._instances(prob)[:2], lockstep="ahead")
    with pytest.raises(ValueError, match='"device" or "refill"'):
        mdl.solve_many(base._instances(prob)[:2], lockstep="behind")
    assert not hasattr(mdl.work, "lockstep")
    assert bnb.MIOSQP.solve_many.__defaults__ == (False, None, 8)  # no default is flipped
