"""The scheduling of the refilled columns (miosqp_amd/csrc/lockstep_refill.hpp) checked on the CPU.

tests/refill_fuzz.cpp is a stand-alone program over the header: the loop of the refill driver without a device, every
node lasting 1-8 chunks.  It is built with -fsanitize=address,undefined and run as a subprocess, once on random records
(1, 3 and 64 trees with a column each, 70 trees on 64, 3 and 1 columns) and once per rule on the trees
tests/test_lockstep_trees_cpu.py records from `lockstep.run` on the CPU backend.  It fails unless: no tree ever has two
nodes in flight, no column or slot is handed out twice, every tree's sequence of (chosen leaf's rank, leaves after the
absorb) equals the wave driver's -- and the recorded Python one --, every slot comes back, and with a column per tree
the chunks run equal the largest per-tree sum of durations.

The Python front: on a backend without the entry, lockstep="refill" is refused by name."""
import os
import subprocess

import numpy as np
import pytest

import test_lockstep_trees_cpu as base

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fuzz(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("refill") / "refill_fuzz")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(HERE, "refill_fuzz.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def prob():
    return base.problems.random_miqp(40, 60, 20, seed=2)


def test_sanitized_random_records(fuzz):
    r = subprocess.run([fuzz], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "refill_fuzz ok: 64 cases" in r.stdout
    print(r.stdout.strip())


def _write(path, waves, out, up0, rule, max_iter_bb):
    """the recorded run as the program reads it: per tree its records in node order with the Python tree's choice and
    list length"""
    B = len(out)
    per = [[] for _ in range(B)]
    for wave in waves:
        for t, idx, before, rec, after, upper in wave:
            per[t].append((rec, idx, after))
    with open(path, "w") as f:
        f.write("%d %d %d\n" % (B, rule, max_iter_bb))
        for t in range(B):
            f.write("%r %d\n" % (float(min(up0[t], 1.7e308)), len(per[t])))
            for rec, idx, after in per[t]:
                f.write("%d %d %r %d %d %d %r %d %d\n" % (int(rec["ok"]), rec["iter"], float(rec["lower"]), rec["int_inf"],
                                                         rec["nextvar"], int(rec["heur_feasible"]), float(rec["heur_obj"]),
                                                         idx, after))
    return sum(len(p) for p in per)


@pytest.mark.parametrize("rule,cap", [(0, None), (1, None), (2, None), (3, None), (1, 6)])
def test_recorded_trees_do_not_depend_on_the_order_of_the_columns(fuzz, oracle_mod, monkeypatch, prob, tmp_path, rule, cap):
    inst = base._instances(prob)
    mdl, out, waves = base._recorded_run(oracle_mod, monkeypatch, prob, inst, rule, cap)
    assert max(o["nodes"] for o in out) > (10 if cap is None else 4)
    path = str(tmp_path / "trees.txt")
    nodes = _write(path, waves, out, base._upper0(mdl, inst), rule, mdl.work.settings["max_iter_bb"])
    assert nodes == sum(o["nodes"] for o in out)
    r = subprocess.run([fuzz, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "refill_fuzz ok: 3 cases, %d nodes" % (3 * nodes) in r.stdout  # on 1, 3 and 7 columns


def test_refill_is_refused_by_name_without_the_entry(oracle_mod, prob):
    mdl = base._model(oracle_mod, prob, 1)
    with pytest.raises(ValueError, match="solve_trees_refill"):
        mdl.solve_many(base._instances(prob)[:2], lockstep="refill")
    with pytest.raises(ValueError, match='"device" or "refill"'):
        mdl.solve_many(base._instances(prob)[:2], lockstep="somewhere")
    assert not hasattr(mdl.work, "lockstep")
