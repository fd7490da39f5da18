"""solve_models (miosqp_amd/bnb.py) on the CPU: the list handling, the errors and the per-model fallback on the oracle
backend -- where no model has the one-launch trees, so every model is solved by its own solve_many --, the declared
symbols, and the host logic of the library's entry (miosqp_amd/csrc/models_plan.hpp) in a stand-alone program built
with -fsanitize=address,undefined and run as a subprocess.  Nothing here touches a GPU."""
import os
import subprocess

import numpy as np
import pytest

import miosqp_amd
from miosqp_amd import bnb, problems

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(12, 30, 6, 8), (10, 5, 2, 0), (20, 10, 8, 1)]


def _model(backend, pr, **settings):
    m = bnb.MIOSQP(backend=backend)
    m.setup(pr["P"], pr["q"], pr["A"], np.copy(pr["l"]), np.copy(pr["u"]), pr["i_idx"], pr["i_l"], pr["i_u"],
            dict(problems.BNB_SETTINGS, **settings), dict(problems.QP_SETTINGS))
    return m


def _instance(pr, k):
    """another q, l, u for model k (the box is widened, so l <= u stays true)"""
    rng = np.random.RandomState(100 + k)
    return dict(q=pr["q"] + 0.1 * rng.randn(len(pr["q"])), l=pr["l"] - 0.05 * rng.rand(len(pr["l"])),
                u=pr["u"] + 0.05 * rng.rand(len(pr["u"])))


@pytest.fixture(scope="module")
def three(oracle_mod):
    prs = [problems.random_miqp(n, m, p, seed=s) for n, m, p, s in SHAPES]
    return prs, [_model(oracle_mod, pr) for pr in prs]


def test_three_oracle_models_equal_their_own_solve_many(oracle_mod, three):
    prs, models = three
    insts = [_instance(pr, k) for k, pr in enumerate(prs)]
    keep = [(m.work.data.q.copy(), m.work.data.l.copy(), m.work.data.u.copy(), len(m.work.leaves)) for m in models]
    info = {}
    got = miosqp_amd.solve_models(models, insts, info=info)
    assert len(got) == 3
    assert sorted(info["own"]) == [0, 1, 2] and info["launched"] == [] and info["launches"] == 0
    assert info["overflow"] == [] and info["forms"] == dict(wave=0, group=0)
    for k, m in enumerate(models):
        want = m.solve_many([insts[k]])[0]
        g = got[k]
        assert set(g) == set(want)
        assert (g["status"], g["nodes"], g["osqp_iter"]) == (want["status"], want["nodes"], want["osqp_iter"]), k
        assert g["upper_glob"] == want["upper_glob"], k
        np.testing.assert_array_equal(g["x"], want["x"])
        q, l, u, nleaves = keep[k]
        np.testing.assert_array_equal(m.work.data.q, q)
        np.testing.assert_array_equal(m.work.data.l, l)
        np.testing.assert_array_equal(m.work.data.u, u)
        assert len(m.work.leaves) == nleaves
    # no instances: the models' own vectors
    got = miosqp_amd.solve_models(models)
    for k, m in enumerate(models):
        want = m.solve_many([{}])[0]
        assert (got[k]["status"], got[k]["nodes"], got[k]["upper_glob"]) == (want["status"], want["nodes"], want["upper_glob"])


def test_the_five_errors(oracle_mod, three):
    prs, models = three
    with pytest.raises(ValueError, match="empty"):
        miosqp_amd.solve_models([])
    with pytest.raises(ValueError, match="2 instances for 3 models"):
        miosqp_amd.solve_models(models, [{}, {}])
    with pytest.raises(ValueError, match="position 0 is listed again at position 2"):
        miosqp_amd.solve_models([models[0], models[1], models[0]])
    with pytest.raises(ValueError, match="position 1 was not set up"):
        miosqp_amd.solve_models([models[0], bnb.MIOSQP(backend=oracle_mod)])
    bad = dict(l=prs[1]["l"].copy(), u=prs[1]["u"].copy())
    bad["l"][0] = bad["u"][0] + 1.0
    with pytest.raises(ValueError, match="instance 1: Lower bound must be lower than or equal to upper bound"):
        miosqp_amd.solve_models(models, [{}, bad, {}])
    # ... and nothing was touched: the same call without the bad instance goes through
    assert len(miosqp_amd.solve_models(models, [{}, {}, {}])) == 3


def test_an_overflowed_tree_is_redone_by_its_own_solve_many(oracle_mod, three, monkeypatch):
    """the launch stubbed out (no GPU here): every model is taken, every tree reports a leaf-list overflow"""
    from miosqp_amd import _lib, qp
    prs, models = three
    calls = []

    def launch(solvers, q, l, u, x0, y0, upper0, x_inc0, rules, max_iter_bb):
        calls.append(len(solvers))
        infos = [_lib.TreeInfo() for _ in solvers]
        for i in infos:
            i.overflow = 1
        stats = _lib.ModelsStats()
        stats.launches, stats.models_wave, stats.models_group = 1, len(solvers), 0
        return [np.zeros(len(a)) for a in q], infos, stats

    monkeypatch.setattr(bnb, "_models_own_reason", lambda work: None)
    monkeypatch.setattr(qp, "solve_trees_models", launch)
    insts = [_instance(pr, k) for k, pr in enumerate(prs)]
    info = {}
    got = miosqp_amd.solve_models(models, insts, info=info)
    assert calls == [3] and info["launched"] == [0, 1, 2] and info["overflow"] == [0, 1, 2] and info["own"] == {}
    assert info["forms"] == dict(wave=3, group=0) and info["launches"] == 1
    for k, m in enumerate(models):
        assert len(m.work.trees_info) == 1 and m.work.trees_info[0].overflow == 1
        want = m.solve_many([insts[k]])[0]
        assert (got[k]["status"], got[k]["nodes"], got[k]["osqp_iter"], got[k]["upper_glob"]) == \
            (want["status"], want["nodes"], want["osqp_iter"], want["upper_glob"])
        np.testing.assert_array_equal(got[k]["x"], want["x"])


def test_the_symbols_are_declared():
    from miosqp_amd import _lib, qp
    assert "miosqp_qp_solve_trees_models" in _lib.SYMBOLS and "miosqp_qp_tree_form" in _lib.SYMBOLS
    assert [f[0] for f in _lib.ModelsStats._fields_] == ["launches", "models_wave", "models_group", "pad", "lds_bytes",
                                                         "device_time", "run_time"]
    assert callable(qp.solve_trees_models) and callable(qp.OSQP.tree_form)
    header = open(os.path.join(os.path.dirname(HERE), "include", "miosqp_amd.h")).read()
    assert "int miosqp_qp_tree_form(miosqp_qp_engine *e);" in header and "int miosqp_qp_solve_trees_models(int32_t B," in header


def test_sanitized_argument_checks_and_arena_layout(tmp_path):
    exe = str(tmp_path / "models_plan_fuzz")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(HERE, "models_plan_fuzz.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "models_plan ok" in r.stdout
