"""Round and fix inside the one-launch trees (solve_many / solve_models with heuristic="device"), the parts that need no GPU:

1. the decisions of the kernel block -- miosqp_amd/csrc/tree_rf_logic.hpp, which the kernels include -- replayed by the
   stand-alone program tests/tree_rf_harness.cpp (built with -fsanitize=address,undefined, run as its own executable) on
   random cases written here together with what `bnb.rf_roundings` and the pick loop of `Workspace.round_and_fix` answer;
   fixed values and picks must be equal bit for bit;
2. the arena plan with the two extra table groups (tests/models_plan_rf_fuzz.cpp, sanitized as well), and the plan
   programs of the earlier entries unchanged;
3. the keyword: ValueError for anything but None / "device" before anything runs, the oracle backend ignores it, the
   symbols are in `_lib.SYMBOLS` and in the header."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import miosqp_amd
from miosqp_amd import _lib, bnb, problems
from oracle import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FLAGS = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _pick_loop(has_x, viol, obj, upper):
    """the pick loop of Workspace.round_and_fix (xs[k] is None: no x), as written there"""
    chosen, feasible = -1, 0
    for k in range(len(obj)):
        if not has_x[k] or not viol[k] <= 0.0:
            continue
        feasible += 1
        if obj[k] < upper and (chosen < 0 or obj[k] < obj[chosen]):
            chosen = k
    return chosen, feasible


def _cases(path):
    rng = np.random.default_rng(20240917)
    n_round = n_pick = 0
    with open(path, "wb") as f:
        for K in (1, 7, 32):
            for rep in range(40):
                p = int(rng.integers(1, 40))
                lo = np.floor(rng.uniform(-4, 2, p))
                hi = lo + rng.integers(0, 4, p)
                x = rng.uniform(lo - 0.0, hi + 0.0)
                # values exactly on a bound, exactly integral, a hair inside and outside; thetas that land on .5
                x[::5] = lo[::5]
                x[1::5] = hi[1::5]
                x[2::7] = np.round(x[2::7])
                x[3::11] = np.nextafter(hi[3::11], -np.inf)
                x[4::13] = np.nextafter(lo[4::13], np.inf)
                if rep % 8 == 0:
                    x = lo + 0.5
                    hi = np.maximum(hi, lo + 1)
                want = bnb.rf_roundings(x, lo, hi, K)
                f.write(struct.pack("=iii", 1, K, p))
                for a in (x, lo, hi, want.ravel()):
                    f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
                n_round += K * p
            for rep in range(200):
                obj = rng.normal(size=K)
                viol = rng.normal(size=K) - 0.3
                has_x = rng.random(K) < 0.8
                if K > 1 and rep % 3 == 0:  # ties in the objective: the lowest k must win
                    obj = np.round(obj)
                    viol[:] = -1.0
                if rep % 4 == 1:  # margins exactly at 0 (feasible) and just above
                    viol[::2] = 0.0
                    viol[1::2] = np.nextafter(0.0, 1.0)
                obj[~has_x] = np.nan  # candidates without an x report NaN
                viol[~has_x] = np.nan
                if rep % 7 == 2:  # a NaN margin on a candidate WITH an x is not feasible
                    viol[0] = np.nan
                upper = [np.inf, float(np.min(obj[has_x]) - 1.0) if has_x.any() else 0.0, float(np.median(obj[has_x])) if has_x.any() else 0.0,
                         float(obj[has_x][0]) if has_x.any() else 0.0][rep % 4]
                chosen, feasible = _pick_loop(has_x, viol, obj, upper)
                f.write(struct.pack("=iid", 2, K, upper))
                f.write(np.ascontiguousarray(has_x, dtype=np.int32).tobytes())
                f.write(viol.tobytes())
                f.write(obj.tobytes())
                f.write(struct.pack("=ii", chosen, feasible))
                n_pick += 1
        for every in (1, 2, 3, 10):
            # Workspace.primal_heuristic: fire = rf_nodes % every == 0, then rf_nodes += 1
            fire, rf_nodes = [], 0
            for _ in range(35):
                fire.append(int(rf_nodes % every == 0))
                rf_nodes += 1
            f.write(struct.pack("=iii", 3, every, len(fire)))
            f.write(np.array(fire, dtype=np.int32).tobytes())
        f.write(struct.pack("=i", 0))
    return n_round, n_pick


def test_sanitized_decisions_equal_the_host_logic_bit_for_bit(tmp_path):
    exe, cases = str(tmp_path / "tree_rf_harness"), str(tmp_path / "cases.bin")
    subprocess.check_call(FLAGS + [os.path.join(HERE, "tree_rf_harness.cpp"), "-o", exe])
    n_round, n_pick = _cases(cases)
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tree_rf ok: %d fixed values, %d picks, 140 firing decisions" % (n_round, n_pick) in r.stdout


def test_the_pick_cases_cover_what_they_claim():
    # (so that the harness cannot pass on cases that never tie, never lack an x or never beat `upper`)
    K = 7
    assert _pick_loop([True] * K, [-1.0] * K, [2.0, 1.0, 1.0, 3.0, 1.0, 2.0, 2.0], np.inf) == (1, 7)
    assert _pick_loop([False, True], [np.nan, -1.0], [np.nan, 5.0], 5.0) == (-1, 1)
    assert _pick_loop([True, True], [np.nan, 0.0], [0.0, 1.0], np.inf) == (1, 1)


def test_the_kernels_include_the_header_the_harness_tests():
    csrc = os.path.join(ROOT, "miosqp_amd", "csrc")
    block = open(os.path.join(csrc, "kernels_tree_rf_block.inc")).read()
    assert '#include "tree_rf_logic.hpp"' in open(os.path.join(csrc, "engine.hip")).read()
    for call in ("rf::fires(", "rf::theta(", "rf::fixed_value(", "pick.take("):
        assert call in block
    assert "floor(" not in block and "% ta.rf_every" not in block  # no second copy of the decisions


@pytest.mark.parametrize("name, says", [("models_plan_rf_fuzz", "models_plan_rf ok"), ("models_plan_fuzz", None),
                                        ("models_plan_large_fuzz", "models_plan_large ok")])
def test_sanitized_plan(tmp_path, name, says):
    exe = str(tmp_path / name)
    subprocess.check_call(FLAGS + [os.path.join(HERE, name + ".cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    if says:
        assert says in r.stdout


def _oracle_models(heuristic):
    out = []
    for n, m, p, s in [(12, 30, 6, 8), (10, 5, 2, 0)]:
        pr = problems.random_miqp(n, m, p, seed=s)
        mdl = bnb.MIOSQP(backend=oracle)
        st = dict(problems.BNB_SETTINGS, primal_heuristic=heuristic, rf_every=3, rf_max_iter=250)
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

    with pytest.raises(ValueError, match="heuristic must be None or \"device\""):
        models[0].solve_many(Untouched(), heuristic=bad)
    with pytest.raises(ValueError, match="heuristic must be None or \"device\""):
        miosqp_amd.solve_models(Untouched(), heuristic=bad)


@pytest.mark.parametrize("heuristic", [0, 1])
def test_on_the_oracle_backend_the_keyword_changes_nothing(heuristic):
    models = _oracle_models(heuristic)
    for mdl in models:
        a = mdl.solve_many([{}, {"q": mdl.work.data.q * 1.5}])
        stats = dict(mdl.work.rf_stats)
        b = mdl.solve_many([{}, {"q": mdl.work.data.q * 1.5}], heuristic="device")
        assert dict(mdl.work.rf_stats) == stats and not hasattr(mdl.work, "trees_rf")
        for x, y in zip(a, b):
            assert (x["status"], x["nodes"], x["osqp_iter"], x["upper_glob"]) == (y["status"], y["nodes"], y["osqp_iter"], y["upper_glob"])
            np.testing.assert_array_equal(x["x"], y["x"])
    plain_info, rf_info = {}, {}
    plain = miosqp_amd.solve_models(models, info=plain_info)
    keyed = miosqp_amd.solve_models(models, info=rf_info, heuristic="device")
    for x, y in zip(plain, keyed):
        assert (x["status"], x["nodes"], x["osqp_iter"], x["upper_glob"]) == (y["status"], y["nodes"], y["osqp_iter"], y["upper_glob"])
        np.testing.assert_array_equal(x["x"], y["x"])
    assert plain_info["forms"] == dict(wave=0, group=0) and "rf" not in plain_info  # without the keyword the dict is what it was
    assert rf_info["forms"] == dict(wave=0, group=0, group_rf=0, reduced_rf=0) and rf_info["rf"] == {}
    assert rf_info["launched"] == [] and rf_info["launches"] == 0 and rf_info["own"] == plain_info["own"]
    assert all("backend" in why for why in rf_info["own"].values())


def test_the_entries_are_declared():
    header = open(os.path.join(ROOT, "include", "miosqp_amd.h")).read()
    for name in ("miosqp_qp_solve_trees_rf", "miosqp_qp_solve_trees_models_rf"):
        assert name in _lib.SYMBOLS
        decl = re.search(r"\nint %s\(([^;]*)\);" % name, header)
        assert decl, name
        # one ctypes argument per declared parameter
        assert len(decl.group(1).split(",")) == len(_lib.SYMBOLS[name][1])
        # ... and the comment in front says which host logic the entry restates
        assert "Workspace.primal_heuristic" in header[:decl.start()].rsplit("*/", 2)[-2]
    assert "typedef struct miosqp_tree_rf_info" in header
    fields = re.search(r"typedef struct miosqp_tree_rf_info \{(.*?)\} miosqp_tree_rf_info;", header, re.S).group(1)
    names = re.findall(r"(\w+)(?:,\s*(\w+))?;", fields)
    assert [n for pair in names for n in pair if n] == [f for f, _ in _lib.TreeRfInfo._fields_]
    # the existing records and signatures are what they were
    assert [f for f, _ in _lib.TreeInfo._fields_] == ["nodes", "osqp_iter", "leaves_left", "overflow", "max_leaves", "found",
                                                      "upper_glob", "lower_glob", "device_time", "run_time"]
    assert len(_lib.SYMBOLS["miosqp_qp_solve_trees"][1]) == 13 and len(_lib.SYMBOLS["miosqp_qp_solve_trees_models_large"][1]) == 15
