"""The host logic of the lock-step trees driven in the library (miosqp_amd/csrc/lockstep_trees.hpp) checked on the CPU.

The header is plain C++; it is compiled with g++ into a throw-away library together with tests/lockstep_harness.cpp
(a test-only wrapper), nothing here touches a GPU.  `lockstep.run` runs on the CPU oracle with logging wrapped around
`choose_leaf` and `bound_and_branch`: per wave and tree the chosen list index, the record of the solved leaf (status,
iterations, lower, int_inf, nextvar, the rounded point's feasibility and objective -- computed here from the leaf's
fields exactly as bound_and_branch computes them) and the list length afterwards.  The records are fed to the C++
trees, which must choose the same index at every wave, hold the same list length after every absorb and end with the
same status family, node count, iteration count and upper bound (equal as floats: the values are fed in).

A stand-alone program over the same header (tests/lockstep_fuzz.cpp) is built with -fsanitize=address,undefined and
run as a subprocess: random records through several trees sharing one free list, growth included."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from miosqp_amd import bnb, lockstep, problems

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
dp = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def lsh(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lsh") / "liblsh.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared",
                           os.path.join(HERE, "lockstep_harness.cpp"), "-o", out])
    L = C.CDLL(out)
    L.lsh_new.restype = C.c_void_p
    L.lsh_new.argtypes = [C.c_int, C.c_int, dp]
    L.lsh_free.argtypes = [C.c_void_p]
    L.lsh_can_continue.argtypes = [C.c_void_p, C.c_int, C.c_int64]
    L.lsh_choose.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.lsh_absorb.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_double]
    for name in ("lsh_open", "lsh_found"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_int]
    L.lsh_upper.restype = C.c_double
    L.lsh_upper.argtypes = [C.c_void_p, C.c_int]
    for name in ("lsh_nodes", "lsh_iters"):
        getattr(L, name).restype = C.c_int64
        getattr(L, name).argtypes = [C.c_void_p, C.c_int]
    for name in ("lsh_grown", "lsh_cap", "lsh_free_slots"):
        getattr(L, name).argtypes = [C.c_void_p]
    return L


def _model(oracle_mod, pr, rule, cap=None):
    st = dict(problems.BNB_SETTINGS)
    st["tree_explor_rule"] = rule
    if cap is not None:
        st["max_iter_bb"] = cap
    mdl = bnb.MIOSQP(backend=oracle_mod)
    mdl.setup(pr["P"], pr["q"], pr["A"], pr["l"].copy(), pr["u"].copy(), pr["i_idx"], pr["i_l"], pr["i_u"], st,
              dict(problems.QP_SETTINGS))
    return mdl


def _instances(pr):
    """own q (four), own l and u, an accepted x0, and bounds no x satisfies (m > n: alternating equalities)"""
    n, m = len(pr["q"]), len(pr["l"])
    rng = np.random.RandomState(11)
    inst = [dict(q=pr["q"] + 0.3 * rng.randn(n)) for _ in range(4)]
    inst.append(dict(l=pr["l"] - 0.5 * rng.rand(m), u=pr["u"] - 0.5 * rng.rand(m)))
    x0 = np.zeros(n)
    x0[pr["i_idx"][0]] = 1.0  # A has entries in [0, 1): 0 <= A x0 < 1 lies inside [l, u]
    inst.append(dict(q=pr["q"] + 0.3 * rng.randn(n), x0=x0))
    b = 50.0 * (1 - 2 * (np.arange(m) % 2))
    inst.append(dict(l=b, u=b.copy()))
    return inst


def _record(tree, leaf):
    """what the device leaves of a solved node, from the leaf's fields as bound_and_branch reads them"""
    ok = leaf.status in tree.ok
    rec = dict(ok=ok, iter=int(leaf.num_iter), lower=0.0, int_inf=-1, nextvar=-1, heur_feasible=False, heur_obj=0.0)
    if not ok:
        return rec
    data = tree.data
    xi = leaf.x[data.i_idx]
    frac = abs(xi - np.round(xi))
    rec["lower"] = float(leaf.lower)
    rec["int_inf"] = int(np.sum(frac > tree.settings["eps_int_feas"]))
    rec["nextvar"] = int(np.argmax(frac))
    x_int = tree.get_integer_solution(leaf.x)
    rec["heur_feasible"] = bool(tree.satisfies_lin_constraints(x_int, data.l, data.u))
    rec["heur_obj"] = float(data.compute_obj_val(x_int))
    return rec


def _recorded_run(oracle_mod, monkeypatch, pr, inst, rule, cap=None):
    """lockstep.run on the oracle with the log: waves = [[(tree, chosen index, leaves before, record, leaves after,
    upper after)]], trees numbered in the order of the instances"""
    mdl = _model(oracle_mod, pr, rule, cap)
    order, waves, chosen = {}, [], {}
    choose0, bb0 = lockstep._Tree.choose_leaf, lockstep._Tree.bound_and_branch

    def choose(self, r):
        t = order.setdefault(id(self), len(order))
        if t in chosen or not waves:
            waves.append([])
            chosen.clear()
        chosen[t] = (self.leaf_index(r), len(self.leaves))
        return choose0(self, r)

    def bb(self, leaf):
        t = order[id(self)]
        rec = _record(self, leaf)
        bb0(self, leaf)
        idx, before = chosen[t]
        waves[-1].append((t, idx, before, rec, len(self.leaves), float(self.upper_glob)))

    monkeypatch.setattr(lockstep._Tree, "choose_leaf", choose)
    monkeypatch.setattr(lockstep._Tree, "bound_and_branch", bb)
    out = mdl.solve_many(inst, lockstep=True)
    monkeypatch.undo()
    assert mdl.work.lockstep["waves"] == len(waves)
    return mdl, out, waves


def _replay(lsh, waves, out, up0, rule, max_iter_bb, capacity=4):
    B = len(out)
    up = np.ascontiguousarray(np.minimum(up0, 1.7e308), dtype=np.float64)
    h = lsh.lsh_new(B, capacity, up.ctypes.data_as(dp))
    try:
        for w, wave in enumerate(waves):
            live = [t for t in range(B) if lsh.lsh_can_continue(h, t, max_iter_bb)]
            assert live == [e[0] for e in wave], w
            for t, idx, before, rec, after, upper in wave:  # all choose, then all absorb: a wave
                assert lsh.lsh_open(h, t) == before, (w, t)
                assert lsh.lsh_choose(h, t, rule) == idx, (w, t)
            for t, idx, before, rec, after, upper in wave:
                lsh.lsh_absorb(h, t, int(rec["ok"]), rec["iter"], rec["lower"], rec["int_inf"], rec["nextvar"],
                               int(rec["heur_feasible"]), rec["heur_obj"])
                assert lsh.lsh_open(h, t) == after, (w, t)
                assert lsh.lsh_upper(h, t) == upper, (w, t)
        assert not any(lsh.lsh_can_continue(h, t, max_iter_bb) for t in range(B))
        for t, o in enumerate(out):
            nodes, upper = lsh.lsh_nodes(h, t), lsh.lsh_upper(h, t)
            assert (nodes, lsh.lsh_iters(h, t)) == (o["nodes"], o["osqp_iter"]), t
            assert upper == o["upper_glob"], t
            finished = nodes + 1 < max_iter_bb  # the status family, as solve_many forms it from (upper, nodes)
            status = (bnb.MI_SOLVED if finished else bnb.MI_MAX_ITER_FEASIBLE) if upper != np.inf else \
                (bnb.MI_PRIMAL_INFEASIBLE if finished else bnb.MI_MAX_ITER_UNSOLVED)
            assert status == o["status"], t
        closed = all(lsh.lsh_open(h, t) == 0 for t in range(B))
        if closed:  # every slot came back
            assert lsh.lsh_free_slots(h) == lsh.lsh_cap(h)
        return lsh.lsh_grown(h)
    finally:
        lsh.lsh_free(h)


def _upper0(mdl, inst):
    """what solve_many hands the trees: the value of an accepted x0, inf otherwise"""
    data = mdl.work.data
    up = np.full(len(inst), np.inf)
    Q, _, _ = mdl._instance_vectors(inst)
    for k, it in enumerate(inst):
        if it.get("x0") is not None:
            x0 = np.asarray(it["x0"], dtype=float)
            up[k] = .5 * np.dot(x0, data.P.dot(x0)) + np.dot(Q[k], x0)
    return up


@pytest.fixture(scope="module")
def prob():
    return problems.random_miqp(40, 60, 20, seed=2)


@pytest.mark.parametrize("rule", [0, 1, 2, 3])
def test_cpp_trees_replay_the_python_trees(lsh, oracle_mod, monkeypatch, prob, rule):
    inst = _instances(prob)
    mdl, out, waves = _recorded_run(oracle_mod, monkeypatch, prob, inst, rule)
    assert out[6]["status"] == bnb.MI_PRIMAL_INFEASIBLE and out[5]["upper_glob"] < np.inf
    assert max(o["nodes"] for o in out) > 10
    # (instance 5 starts with an incumbent: under rules 1 and 3 its second phase begins at the first node)
    grown = _replay(lsh, waves, out, _upper0(mdl, inst), rule, mdl.work.settings["max_iter_bb"])
    assert grown > 1  # the store started at 4 slots for 7 roots


@pytest.mark.parametrize("rule", [1, 2])
def test_cpp_trees_stop_at_max_iter_bb(lsh, oracle_mod, monkeypatch, prob, rule):
    inst = _instances(prob)
    mdl, out, waves = _recorded_run(oracle_mod, monkeypatch, prob, inst, rule, cap=6)
    capped = [o for o in out if o["status"] in (bnb.MI_MAX_ITER_FEASIBLE, bnb.MI_MAX_ITER_UNSOLVED)]
    assert capped and all(o["nodes"] == 5 for o in capped) and len(waves) == 5
    _replay(lsh, waves, out, _upper0(mdl, inst), rule, 6)


def test_nothing_to_do_at_max_iter_bb_one(lsh):
    up = np.array([np.inf, 3.0])
    h = lsh.lsh_new(2, 8, np.minimum(up, 1.7e308).ctypes.data_as(dp))
    try:
        assert not lsh.lsh_can_continue(h, 0, 1) and not lsh.lsh_can_continue(h, 1, 1)
        assert lsh.lsh_nodes(h, 0) == 0 and lsh.lsh_upper(h, 0) == np.inf and lsh.lsh_upper(h, 1) == 3.0
    finally:
        lsh.lsh_free(h)


def test_prune_skips_the_leaf_behind_a_removed_one(lsh):
    """Three branchings under depth first leave the list [a, b, c, d] with inherited bounds 1, 5, 5, 2 ... built here by
    hand: a root (lower 1) branches, its second child (lower 5) branches, then an integer-feasible node of value 3
    prunes: the two adjacent leaves with bound 5 > 3 -- only the first goes, the one behind it is not examined
    (workspace.py:278-280), exactly what the Python list does."""
    up = np.array([1.7e308])
    h = lsh.lsh_new(1, 16, up.ctypes.data_as(dp))
    try:
        ws = bnb.Workspace.__new__(bnb.Workspace)  # the Python mirror's prune on the same bounds

        class Leaf(object):
            def __init__(self, lower):
                self.lower = lower

        # root: lower 1, fractional -> children A, B inherit 1                      list [A, B]
        assert lsh.lsh_choose(h, 0, 0) == 0
        assert lsh.lsh_absorb(h, 0, 1, 10, 1.0, 2, 0, 0, 0.0) == 1
        # rule 0 takes the first deepest: A (index 0); lower 5 -> children C, D inherit 5   list [B, C, D]
        assert lsh.lsh_choose(h, 0, 0) == 0
        assert lsh.lsh_absorb(h, 0, 1, 10, 5.0, 2, 1, 0, 0.0) == 1
        assert lsh.lsh_open(h, 0) == 3
        # rule 2 (best bound) takes B (inherited 1, index 0): integer feasible with value 3 -> incumbent, prune [C, D]
        assert lsh.lsh_choose(h, 0, 2) == 0
        assert lsh.lsh_absorb(h, 0, 1, 10, 3.0, 0, -1, 0, 0.0) == 2
        ws.leaves, ws.upper_glob = [Leaf(5.0), Leaf(5.0)], 3.0
        ws.prune()
        assert len(ws.leaves) == 1  # the skip
        assert lsh.lsh_open(h, 0) == 1 and lsh.lsh_upper(h, 0) == 3.0
        # the survivor is solved: its bound 6 exceeds the incumbent -> the tree closes and every slot is free again
        assert lsh.lsh_choose(h, 0, 1) == 0
        assert lsh.lsh_absorb(h, 0, 1, 10, 6.0, 1, 0, 0, 0.0) == 0
        assert lsh.lsh_open(h, 0) == 0 and lsh.lsh_nodes(h, 0) == 4 and lsh.lsh_iters(h, 0) == 40
        assert lsh.lsh_free_slots(h) == lsh.lsh_cap(h)
    finally:
        lsh.lsh_free(h)


def test_heuristic_incumbent_and_infeasible_records(lsh):
    up = np.array([1.7e308])
    h = lsh.lsh_new(1, 4, up.ctypes.data_as(dp))
    try:
        lsh.lsh_choose(h, 0, 1)
        # fractional, the rounded point is feasible with value 9: incumbent by the heuristic (2) AND a branching (1)
        assert lsh.lsh_absorb(h, 0, 1, 7, 2.0, 3, 4, 1, 9.0) == (1 | 2 << 1)
        assert lsh.lsh_upper(h, 0) == 9.0 and lsh.lsh_found(h, 0) == 1
        # rule 1 with an incumbent: the LARGEST inherited bound, first one
        assert lsh.lsh_choose(h, 0, 1) == 0
        assert lsh.lsh_absorb(h, 0, 0, 5, float("nan"), -1, -1, 0, float("nan")) == 0  # infeasible: nothing happens
        assert lsh.lsh_open(h, 0) == 1
        # a rounded point that is feasible but no better than the incumbent changes nothing
        lsh.lsh_choose(h, 0, 1)
        assert lsh.lsh_absorb(h, 0, 1, 5, 4.0, 1, 0, 1, 9.0) == 1
        assert lsh.lsh_upper(h, 0) == 9.0 and lsh.lsh_nodes(h, 0) == 3 and lsh.lsh_iters(h, 0) == 17
    finally:
        lsh.lsh_free(h)


def test_sanitized_random_records(tmp_path):
    exe = str(tmp_path / "lockstep_fuzz")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(HERE, "lockstep_fuzz.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "lockstep_fuzz ok" in r.stdout


def test_device_driver_is_refused_on_the_oracle(oracle_mod, prob):
    mdl = _model(oracle_mod, prob, 1)
    with pytest.raises(ValueError):
        mdl.solve_many(_instances(prob)[:2], lockstep="device")
    with pytest.raises(ValueError):
        mdl.solve_many(_instances(prob)[:2], lockstep="somewhere")
    assert not hasattr(mdl.work, "lockstep")
