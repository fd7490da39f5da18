"""Strong and reliability branching inside the one-launch trees (solve_many / solve_models with branching="device"), the
parts that need no GPU:

1. the decisions of the kernel block -- miosqp_amd/csrc/tree_sb_logic.hpp, which the kernels include -- side by side with
   `lockstep::SbTree` (lockstep_sb.hpp, pinned by recorded trees) in the stand-alone program tests/tree_sb_harness.cpp
   (built with -fsanitize=address,undefined, run as its own executable): every chosen position, score, pc_sum and pc_cnt
   equal bit for bit;
2. the arena plan with the two extra table groups and the work areas (tests/models_plan_sb_fuzz.cpp, sanitized as well),
   and the plan programs of the earlier entries unchanged;
3. the keyword: ValueError for anything but None / "device" before anything runs, the oracle backend ignores it, the
   symbols are in `_lib.SYMBOLS` and in the header."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import miosqp_amd
from miosqp_amd import _lib, bnb, problems
from oracle import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FLAGS = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_sanitized_decisions_equal_the_lockstep_restatement_bit_for_bit(tmp_path):
    exe = str(tmp_path / "tree_sb_harness")
    subprocess.check_call(FLAGS + [os.path.join(HERE, "tree_sb_harness.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = re.search(r"tree_sb ok: 162 runs, (\d+) asks, (\d+) decides, (\d+) solved nodes; ties in fractions (\d+), in scores (\d+), "
                    r"children without a value (\d+), means over more than 128 positions (\d+)", r.stdout)
    assert got, r.stdout
    # 2 rules x 3 K x 3 p x 3 reliabilities x 3 repeats; and no case class is empty
    assert all(int(v) > 0 for v in got.groups())


def test_the_kernels_include_the_header_the_harness_tests():
    """the harness proves something about the kernels only while they include the header it drives (what the block does
    with it is the GPU tests' subject)"""
    csrc = os.path.join(ROOT, "miosqp_amd", "csrc")
    assert '#include "tree_sb_logic.hpp"' in open(os.path.join(csrc, "engine.hip")).read()
    assert "miosqp::tree_sb" in open(os.path.join(csrc, "kernels_tree_sb_block.inc")).read()
    assert '#include "kernels_tree_sb_block.inc"' in open(os.path.join(csrc, "kernels_tree_body.inc")).read()


@pytest.mark.parametrize("name, says", [("models_plan_sb_fuzz", "models_plan_sb ok"), ("models_plan_rf_fuzz", "models_plan_rf ok"),
                                        ("models_plan_fuzz", None), ("models_plan_large_fuzz", "models_plan_large ok")])
def test_sanitized_plan(tmp_path, name, says):
    exe = str(tmp_path / name)
    subprocess.check_call(FLAGS + [os.path.join(HERE, name + ".cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    if says:
        assert says in r.stdout


def _oracle_models(rule, heuristic=0):
    out = []
    for n, m, p, s in [(12, 30, 6, 8), (10, 5, 2, 0)]:
        pr = problems.random_miqp(n, m, p, seed=s)
        mdl = bnb.MIOSQP(backend=oracle)
        st = dict(problems.BNB_SETTINGS, branching_rule=rule, sb_max_iter=50, primal_heuristic=heuristic)
        mdl.setup(pr["P"], pr["q"], pr["A"], pr["l"], pr["u"], pr["i_idx"], pr["i_l"], pr["i_u"], st, dict(problems.QP_SETTINGS))
        out.append(mdl)
    return out


@pytest.mark.parametrize("bad", ["host", True, 1, "Device", b"device"], ids=repr)
def test_value_errors_of_the_keyword(bad):
    models = _oracle_models(1)

    class Untouched:  # anything that ran would have to read the instances
        def __iter__(self):
            raise AssertionError("the instances were read")

        def __len__(self):
            raise AssertionError("the instances were read")

    with pytest.raises(ValueError, match="branching must be None or \"device\""):
        models[0].solve_many(Untouched(), branching=bad)
    with pytest.raises(ValueError, match="branching must be None or \"device\""):
        miosqp_amd.solve_models(Untouched(), branching=bad)


@pytest.mark.parametrize("rule", [0, 1, 2])
def test_on_the_oracle_backend_the_keyword_changes_nothing(rule):
    models = _oracle_models(rule)
    for mdl in models:
        a = mdl.solve_many([{}, {"q": mdl.work.data.q * 1.5}])
        b = mdl.solve_many([{}, {"q": mdl.work.data.q * 1.5}], branching="device")
        assert not hasattr(mdl.work, "trees_sb")
        for x, y in zip(a, b):
            assert (x["status"], x["nodes"], x["osqp_iter"], x["upper_glob"]) == (y["status"], y["nodes"], y["osqp_iter"], y["upper_glob"])
            np.testing.assert_array_equal(x["x"], y["x"])
    plain_info, sb_info, both_info = {}, {}, {}
    plain = miosqp_amd.solve_models(models, info=plain_info)
    keyed = miosqp_amd.solve_models(models, info=sb_info, branching="device")
    miosqp_amd.solve_models(models, info=both_info, branching="device", heuristic="device", large="device")
    for x, y in zip(plain, keyed):
        assert (x["status"], x["nodes"], x["osqp_iter"], x["upper_glob"]) == (y["status"], y["nodes"], y["osqp_iter"], y["upper_glob"])
        np.testing.assert_array_equal(x["x"], y["x"])
    assert plain_info["forms"] == dict(wave=0, group=0) and "sb" not in plain_info  # without the keyword the dict is what it was
    assert sb_info["forms"] == dict(wave=0, group=0, group_sb=0, reduced_sb=0) and sb_info["sb"] == {} and "rf" not in sb_info
    assert both_info["forms"] == dict(wave=0, group=0, reduced=0, group_rf=0, reduced_rf=0, group_sb=0, reduced_sb=0)
    assert sb_info["launched"] == [] and sb_info["launches"] == 0 and sb_info["own"] == plain_info["own"]
    assert all("backend" in why for why in sb_info["own"].values())


def test_the_defaults_are_what_they_were_and_the_keyword_is_keyword_only():
    assert bnb.MIOSQP.solve_many.__defaults__ == (False, None, 8)
    assert bnb.MIOSQP.solve_many.__kwdefaults__ == dict(heuristic=None, branching=None)
    for f in (bnb.MIOSQP.solve_many, miosqp_amd.solve_models):
        par = inspect.signature(f).parameters
        assert par["branching"].kind is inspect.Parameter.KEYWORD_ONLY and par["branching"].default is None
        assert list(par)[-2:] == ["heuristic", "branching"]  # behind `heuristic`


class _Solver:  # the questions of one_launch_trees_ok / _models_own_reason need attributes only
    def solve_trees(self): pass
    def solve_trees_rf(self): pass
    def solve_trees_sb(self): pass
    def tree_form(self): return 2


def _work(rule, heuristic=0, solver=_Solver):
    import types
    return types.SimpleNamespace(
        solver=solver(), settings=dict(branching_rule=rule, tree_explor_rule=1, primal_heuristic=heuristic),
        rf=dict(on=heuristic), data=types.SimpleNamespace(n_int=3), qp_settings=dict(eps_abs=1e-3))


def test_the_sb_question_beside_the_rf_question():
    for rule in (1, 2):
        w = _work(rule)
        assert bnb._models_own_reason(w) == "branching_rule %d" % rule and not bnb.one_launch_trees_ok(w)
        assert bnb._models_own_reason(w, rf=True) == "branching_rule %d" % rule and not bnb.one_launch_trees_ok(w, rf=True)
        assert bnb._models_own_reason(w, sb=True) is None and bnb.one_launch_trees_ok(w, sb=True)
        # the rule and the heuristic together: its own reason, whatever `heuristic` says
        both = _work(rule, heuristic=1)
        for rf in (False, True):
            assert bnb._models_own_reason(both, rf=rf, sb=True) == "branching_rule %d together with primal_heuristic on" % rule
            assert not bnb.one_launch_trees_ok(both, rf=rf, sb=True)

    class Older:  # a backend without the entry: the keyword is ignored
        def solve_trees(self): pass
        def tree_form(self): return 2

    assert bnb._models_own_reason(_work(1, solver=Older), sb=True) == "branching_rule 1"
    w0 = _work(0)
    assert bnb._models_own_reason(w0) is None and bnb._models_own_reason(w0, sb=True) is None
    assert bnb._models_own_reason(_work(0, heuristic=1), sb=True) == "primal_heuristic on"
    assert bnb._models_own_reason(_work(0, heuristic=1), rf=True, sb=True) is None


def test_the_entries_are_declared():
    header = open(os.path.join(ROOT, "include", "miosqp_amd.h")).read()
    for name in ("miosqp_qp_solve_trees_sb", "miosqp_qp_solve_trees_models_sb"):
        assert name in _lib.SYMBOLS
        decl = re.search(r"\nint %s\(([^;]*)\);" % name, header)
        assert decl, name
        # one ctypes argument per declared parameter
        assert len(decl.group(1).split(",")) == len(_lib.SYMBOLS[name][1])
        # ... and the comment in front says which host logic the entry restates
        assert "Workspace.select_branching" in header[:decl.start()].rsplit("*/", 2)[-2]
    fields = re.search(r"typedef struct miosqp_tree_sb_info \{(.*?)\} miosqp_tree_sb_info;", header, re.S).group(1)
    names = re.findall(r"int32_t ([\w, ]+);", fields)
    assert [n.strip() for group in names for n in group.split(",")] == [f for f, _ in _lib.TreeSbInfo._fields_]
    # the existing records and signatures are what they were
    assert [f for f, _ in _lib.TreeRfInfo._fields_] == ["calls", "candidates", "feasible", "improved", "osqp_iter", "form", "pad0", "pad1"]
    assert len(_lib.SYMBOLS["miosqp_qp_solve_trees_rf"][1]) == 17 and len(_lib.SYMBOLS["miosqp_qp_solve_trees_models_rf"][1]) == 19
