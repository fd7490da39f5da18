"""solve_many(..., large="device") (miosqp_amd/bnb.py), the parts that need no GPU:

1. the keywords: ValueError for a `large` other than None / "device" and for a `leaf_cap` that is not an int >= 2, before
   the backend or the instances are touched; no default is flipped;
2. the oracle backend ignores the keyword, bit for bit;
3. the three symbols are declared in the header and bound in `_lib`, the three methods are on `qp.OSQP`;
4. routing, with a stub solver that records calls (`tree_form` 0, `tree_form_large` 3, canned infos): which entry runs
   under which settings and keywords, an overflowed instance redone by what `lockstep` says, a None return falling through
   as a decline does;
5. the layout of the batch's arena (miosqp_amd/csrc/trees_large_plan.hpp) in the stand-alone program
   tests/trees_large_plan_fuzz.cpp, built with -fsanitize=address,undefined and run as its own executable."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import miosqp_amd
from miosqp_amd import _lib, bnb, problems, qp
from oracle import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = ("miosqp_qp_solve_trees_large", "miosqp_qp_solve_trees_large_rf", "miosqp_qp_solve_trees_large_sb")


def _model(rule=0, heuristic=0, **st):
    pr = problems.random_miqp(12, 30, 6, seed=8)
    mdl = bnb.MIOSQP(backend=oracle)
    mdl.setup(pr["P"], pr["q"], pr["A"], pr["l"].copy(), pr["u"].copy(), pr["i_idx"], pr["i_l"], pr["i_u"],
              dict(problems.BNB_SETTINGS, branching_rule=rule, primal_heuristic=heuristic, sb_max_iter=50, **st),
              dict(problems.QP_SETTINGS))
    return mdl, pr


def _instances(pr):
    rng = np.random.RandomState(5)
    return [{}, dict(q=pr["q"] + 0.1 * rng.randn(len(pr["q"]))), dict(q=pr["q"] * 1.5)]


def _same(a, b, who=""):
    assert (a["status"], a["nodes"], a["osqp_iter"], a["upper_glob"]) == (b["status"], b["nodes"], b["osqp_iter"], b["upper_glob"]), who
    np.testing.assert_array_equal(a["x"], b["x"], err_msg=str(who))


class _Untouched:  # anything that ran would have to read the instances
    def __iter__(self):
        raise AssertionError("the instances were read")

    def __len__(self):
        raise AssertionError("the instances were read")


class _NoBackend:  # ... or the workspace
    def __getattr__(self, name):
        raise AssertionError("the workspace was read: %s" % name)


@pytest.mark.parametrize("kw", [dict(large="host"), dict(large=True), dict(large="Device"), dict(leaf_cap=1), dict(leaf_cap=True),
                                dict(leaf_cap=2.0), dict(leaf_cap="256"), dict(large="device", leaf_cap=0)], ids=repr)
def test_value_errors_before_the_backend_is_touched(kw):
    mdl = bnb.MIOSQP(backend=oracle)
    mdl.work = _NoBackend()
    what = "leaf_cap must be an int of at least 2" if "leaf_cap" in kw else 'large must be None or "device"'
    with pytest.raises(ValueError, match=what):
        mdl.solve_many(_Untouched(), **kw)


def test_no_default_is_flipped_and_the_keywords_are_keyword_only():
    """the declared parameters of solve_many and their defaults are what they were (other tests pin them); `large` and
    `leaf_cap` are taken by name only, with None and 256 when they are not given"""
    assert bnb.MIOSQP.solve_many.__defaults__ == (False, None, 8)
    assert bnb.MIOSQP.solve_many.__kwdefaults__ == dict(heuristic=None, branching=None)
    assert bnb._large_options({}, "solve_many") == (None, 256)
    assert bnb._large_options(dict(large="device", leaf_cap=np.int64(4)), "solve_many") == ("device", 4)
    mdl = bnb.MIOSQP(backend=oracle)
    mdl.work = _NoBackend()
    with pytest.raises(TypeError):  # not positional: there is no seventh position
        mdl.solve_many(_Untouched(), False, None, 8, "device")
    with pytest.raises(TypeError, match="unexpected keyword argument 'leafcap'"):
        mdl.solve_many(_Untouched(), large="device", leafcap=4)
    for name in ("solve_trees_large", "solve_trees_large_rf", "solve_trees_large_sb"):
        assert inspect.signature(getattr(qp.OSQP, name)).parameters["leaf_cap"].default == 256


@pytest.mark.parametrize("rule, heuristic", [(0, 0), (1, 0), (0, 1)])
def test_on_the_oracle_backend_the_keyword_changes_nothing(rule, heuristic):
    mdl, pr = _model(rule, heuristic)
    inst = _instances(pr)
    a = mdl.solve_many(inst)
    b = mdl.solve_many(inst, large="device")
    c = mdl.solve_many(inst, large="device", leaf_cap=4, heuristic="device", branching="device")
    assert not hasattr(mdl.work, "trees_info") and not getattr(mdl.work, "_no_trees_large", False)
    for k in range(len(inst)):
        _same(a[k], b[k], k)
        _same(a[k], c[k], k)


def test_the_three_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "miosqp_amd.h")).read()
    cites = ("miosqp_qp_solve_trees_lockstep", "miosqp_qp_solve_trees_lockstep_rf", "miosqp_qp_solve_trees_lockstep_sb")
    for name, cite in zip(NAMES, cites):
        assert name in _lib.SYMBOLS
        decl = re.search(r"\nint %s\(([^;]*)\);" % name, header)
        assert decl, name
        pars = decl.group(1).split(",")
        assert len(pars) == len(_lib.SYMBOLS[name][1])  # one ctypes argument per declared parameter
        assert "int32_t leaf_cap" in pars[11]  # behind max_iter_bb, as the Python methods pass it
        assert cite in header[:decl.start()].rsplit("*/", 2)[-2]  # the comment in front says what the entry replaces
    assert len(_lib.SYMBOLS[NAMES[0]][1]) == len(_lib.SYMBOLS["miosqp_qp_solve_trees"][1]) + 1
    assert len(_lib.SYMBOLS[NAMES[1]][1]) == len(_lib.SYMBOLS["miosqp_qp_solve_trees_rf"][1]) + 1
    assert len(_lib.SYMBOLS[NAMES[2]][1]) == len(_lib.SYMBOLS["miosqp_qp_solve_trees_sb"][1]) + 1
    for name in ("solve_trees_large", "solve_trees_large_rf", "solve_trees_large_sb"):
        assert callable(getattr(qp.OSQP, name))
    # the kernels and the plan the entries drive are in the library's one translation unit
    csrc = os.path.join(ROOT, "miosqp_amd", "csrc")
    assert '#include "trees_large_plan.hpp"' in open(os.path.join(csrc, "engine.hip")).read()
    kernels = open(os.path.join(csrc, "kernels_tree.inc")).read()
    for k in ("k_tree_r", "k_tree_rf_r", "k_tree_sb_r"):
        assert re.search(r"__launch_bounds__\(RES_THREADS\) void %s\(Dev d, TreeArgs ta\)" % k, kernels), k


# ---- routing ----------------------------------------------------------------------------------------------------------
class _Stub:
    """the model's own (oracle) solver with the one-launch entries of the HIP engine in front: an engine beyond the small
    forms that the reduced form takes; every call of an entry is recorded, the answer is canned"""

    def __init__(self, real, answer, form=0, form_large=3):
        self._real, self._answer, self._form, self._form_large = real, answer, form, form_large
        self.calls = []

    def __getattr__(self, name):  # everything else: the real solver (the sequential path runs on it)
        return getattr(self._real, name)

    def tree_form(self):
        return self._form

    def tree_form_large(self, leaf_cap=256):
        self.calls.append(("tree_form_large", leaf_cap))
        return self._form_large

    def _entry(self, name, q, extra, leaf_cap):
        self.calls.append((name, len(q), tuple(extra), leaf_cap))
        return self._answer(name, q)

    def solve_trees(self, q, *a):
        return self._entry("solve_trees", q, (), None)

    def solve_trees_rf(self, q, l, u, x0, y0, up, xi, rule, mi, *rf):
        return self._entry("solve_trees_rf", q, rf, None)

    def solve_trees_sb(self, q, l, u, x0, y0, up, xi, rule, mi, *sb):
        return self._entry("solve_trees_sb", q, sb, None)

    def solve_trees_large(self, q, l, u, x0, y0, up, xi, rule, mi, leaf_cap=256):
        return self._entry("solve_trees_large", q, (), leaf_cap)

    def solve_trees_large_rf(self, q, l, u, x0, y0, up, xi, rule, mi, *rf, leaf_cap=256):
        return self._entry("solve_trees_large_rf", q, rf, leaf_cap)

    def solve_trees_large_sb(self, q, l, u, x0, y0, up, xi, rule, mi, *sb, leaf_cap=256):
        return self._entry("solve_trees_large_sb", q, sb, leaf_cap)


def _canned(overflow=()):
    """every tree found x = 0.25 everywhere with value 7 + k in 3 nodes; the instances in `overflow` overflowed"""
    def answer(name, q):
        B, n = q.shape
        infos = [_lib.TreeInfo() for _ in range(B)]
        for k, i in enumerate(infos):
            i.nodes, i.osqp_iter, i.found, i.upper_glob, i.overflow = 3, 40 + k, 1, 7.0 + k, int(k in overflow)
        if name.endswith("_rf"):
            rec = [_lib.TreeRfInfo() for _ in range(B)]
            for k, r in enumerate(rec):
                r.calls, r.candidates, r.feasible, r.improved, r.osqp_iter = 1 + k, 7, 2, 1, 90
            return np.full((B, n), 0.25), infos, rec
        if name.endswith("_sb"):
            rec = [_lib.TreeSbInfo() for _ in range(B)]
            for k, r in enumerate(rec):
                r.calls, r.children, r.osqp_iter = 2 + k, 8, 70
            return np.full((B, n), 0.25), infos, rec
        return np.full((B, n), 0.25), infos
    return answer


def _stubbed(rule=0, heuristic=0, answer=None, **kw):
    mdl, pr = _model(rule, heuristic)
    stub = _Stub(mdl.work.solver, answer or _canned(), **kw)
    mdl.work.solver = stub
    return mdl, pr, stub


def _entries(stub):
    return [c[0] for c in stub.calls if c[0] != "tree_form_large"]


@pytest.mark.parametrize("rule, heuristic, kw, entry", [
    (0, 0, {}, "solve_trees_large"),
    (0, 0, dict(heuristic="device", branching="device"), "solve_trees_large"),  # the keywords without their settings
    (0, 1, dict(heuristic="device"), "solve_trees_large_rf"),
    (1, 0, dict(branching="device"), "solve_trees_large_sb"),
    (2, 0, dict(branching="device"), "solve_trees_large_sb"),
])
def test_the_entry_that_runs(rule, heuristic, kw, entry):
    mdl, pr, stub = _stubbed(rule, heuristic)
    inst = _instances(pr)
    got = mdl.solve_many(inst, large="device", leaf_cap=64, **kw)
    assert _entries(stub) == [entry]  # one call, and the small forms' entries are not asked
    call = [c for c in stub.calls if c[0] == entry][0]
    assert call[1] == 3 and call[3] == 64 and ("tree_form_large", 64) in stub.calls
    if entry.endswith("_rf"):
        assert call[2] == (mdl.work.rf["K"], mdl.work.rf["max_iter"], mdl.work.rf["every"])
        assert mdl.work.trees_rf == [dict(calls=1 + k, candidates=7, feasible=2, improved=1, osqp_iter=90) for k in range(3)]
    if entry.endswith("_sb"):
        sb = mdl.work.sb
        assert call[2] == (rule, sb["K"], sb["max_iter"], sb["reliability"], sb["eps"])
        assert mdl.work.trees_sb == [dict(calls=2 + k, children=8, osqp_iter=70) for k in range(3)]
    assert len(mdl.work.trees_info) == 3
    for k, g in enumerate(got):  # the dicts are formed from the canned records, as the small forms' are
        assert (g["status"], g["nodes"], g["osqp_iter"], g["upper_glob"]) == (bnb.MI_SOLVED, 3, 40 + k, 7.0 + k)
        want = np.full(len(pr["q"]), 0.25)
        want[pr["i_idx"]] = 0.0
        np.testing.assert_array_equal(g["x"], want)
    assert not getattr(mdl.work, "_no_trees", False) and not getattr(mdl.work, "_no_trees_large", False)


@pytest.mark.parametrize("rule, heuristic, kw", [
    (1, 1, dict(heuristic="device", branching="device")),  # a rule together with the heuristic
    (2, 1, dict(heuristic="device", branching="device")),
    (0, 1, {}),                                              # the heuristic without its keyword
    (0, 1, dict(branching="device")),
    (1, 0, {}),                                              # a rule without its keyword
    (2, 0, dict(heuristic="device")),
])
def test_no_large_attempt(rule, heuristic, kw):
    mdl, pr, stub = _stubbed(rule, heuristic)
    plain, _ = _model(rule, heuristic)
    inst = _instances(pr)
    got = mdl.solve_many(inst, large="device", **kw)
    assert _entries(stub) == []  # as today: no one-launch attempt of either kind
    for k, w in enumerate(plain.solve_many(inst)):
        _same(got[k], w, k)


def test_no_large_attempt_for_the_engine_s_sake():
    inst = None
    for kw in (dict(form=2), dict(form_large=0)):
        # (an engine of a small form keeps its entry; an engine the reduced form does not take keeps today's path: the
        #  small entry is asked and, here, answers)
        mdl, pr, stub = _stubbed(**kw)
        inst = _instances(pr)
        mdl.solve_many(inst, large="device")
        assert _entries(stub) == ["solve_trees"], kw
    for off in (dict(device_tree=False), dict(device_digest=False)):
        mdl, pr = _model(**off)
        stub = mdl.work.solver = _Stub(mdl.work.solver, _canned())
        mdl.solve_many(inst, large="device")
        assert _entries(stub) == [], off

    class Older(_Stub):  # a backend without the entry ignores the keyword
        solve_trees_large = property()

    mdl, pr = _model()
    stub = mdl.work.solver = Older(mdl.work.solver, _canned())
    assert not hasattr(stub, "solve_trees_large")
    mdl.solve_many(inst, large="device")
    assert _entries(stub) == ["solve_trees"]


def test_without_the_keyword_the_small_entry_is_asked_as_before():
    mdl, pr, stub = _stubbed(answer=lambda name, q: None)
    mdl.solve_many(_instances(pr))
    assert _entries(stub) == ["solve_trees"] and mdl.work._no_trees is True
    # ... and that decline does not keep the large attempt from being made afterwards
    stub._answer = _canned()
    got = mdl.solve_many(_instances(pr), large="device")
    assert _entries(stub) == ["solve_trees", "solve_trees_large"] and got[2]["upper_glob"] == 9.0
    assert mdl.work._no_trees is True


def test_an_overflowed_instance_is_redone_by_what_lockstep_says(monkeypatch):
    from miosqp_amd import lockstep as ls
    plain, pr = _model()
    inst = _instances(pr)
    want = plain.solve_many(inst, lockstep=False)
    # lockstep=False: the sequential path, for the overflowed instance alone
    mdl, _, stub = _stubbed(answer=_canned(overflow=(1,)))
    got = mdl.solve_many(inst, large="device", lockstep=False)
    assert _entries(stub) == ["solve_trees_large"]
    assert [i.overflow for i in mdl.work.trees_info] == [0, 1, 0]
    _same(got[1], want[1], "the overflowed instance")
    assert [got[k]["upper_glob"] for k in (0, 2)] == [7.0, 9.0]
    # lockstep=True: the lock-step driver gets exactly that instance
    seen = []

    def run(model, todo, Q, L, U, up, XI, instances, out, batched):
        seen.append(list(todo))
        for k in todo:
            out[k] = dict(want[k], by="lockstep")

    monkeypatch.setattr(ls, "run", run)
    mdl, _, stub = _stubbed(answer=_canned(overflow=(1,)))
    got = mdl.solve_many(inst, large="device", lockstep=True)
    assert seen == [[1]] and got[1]["by"] == "lockstep" and "by" not in got[0]
    # lockstep=None: the call was not declined, so the overflowed instance goes the sequential way (as a small form's does)
    seen.clear()
    mdl, _, stub = _stubbed(answer=_canned(overflow=(0, 2)))
    got = mdl.solve_many(inst, large="device")
    assert seen == [] and got[1]["upper_glob"] == 8.0
    _same(got[0], want[0], 0)
    _same(got[2], want[2], 2)


def test_a_none_return_falls_through_as_a_decline_does():
    plain, pr = _model()
    inst = _instances(pr)
    want = plain.solve_many(inst)
    mdl, _, stub = _stubbed(answer=lambda name, q: None)
    got = mdl.solve_many(inst, large="device")
    assert _entries(stub) == ["solve_trees_large"]
    for k in range(3):
        _same(got[k], want[k], k)
    assert mdl.work._no_trees_large is True and not hasattr(mdl.work, "trees_info")
    # the engine that declined is not asked again
    mdl.solve_many(inst, large="device")
    assert _entries(stub) == ["solve_trees_large", "solve_trees"]


# ---- the planning header ----------------------------------------------------------------------------------------------
def test_sanitized_plan_of_the_batch_arena(tmp_path):
    exe = str(tmp_path / "trees_large_plan_fuzz")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(HERE, "trees_large_plan_fuzz.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "trees_large_plan ok" in r.stdout
