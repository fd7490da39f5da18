"""polish_models / solve_models(polish=True) (miosqp_amd/bnb.py) on the CPU: on the oracle backend no model has
`polish_models`, so every model is polished by its own polish_many and the list call must equal the per-model
solve_many(polish=True) key for key; the errors; and the host logic of the library's entry
(miosqp_amd/csrc/polish_models_plan.hpp) in a stand-alone program built with -fsanitize=address,undefined and run as a
subprocess.  Nothing here touches a GPU."""
import os
import subprocess

import numpy as np
import pytest

import miosqp_amd
from miosqp_amd import bnb, problems

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(10, 5, 2, 0), (20, 10, 5, 1), (32, 8, 16, 2)]


def _model(backend, pr, settings=None, qp_settings=None):
    m = bnb.MIOSQP(backend=backend)
    m.setup(pr["P"], pr["q"], pr["A"], np.copy(pr["l"]), np.copy(pr["u"]), pr["i_idx"], pr["i_l"], pr["i_u"],
            dict(problems.BNB_SETTINGS) if settings is None else dict(settings),
            dict(problems.QP_SETTINGS) if qp_settings is None else dict(qp_settings))
    return m


def _four(backend):
    """(models, instances): three random MIQPs of different shapes and the power converter's first MPC step"""
    prs = [problems.random_miqp(n, m, p, seed=s) for n, m, p, s in SHAPES]
    insts = []
    for k, pr in enumerate(prs):
        rng = np.random.RandomState(100 + k)
        insts.append(dict(q=pr["q"] + 0.1 * rng.randn(len(pr["q"]))))
    models = [_model(backend, pr) for pr in prs]
    pc = problems.load_power_converter()
    pcp = dict(P=pc["P"], q=pc["q"][0].copy(), A=pc["A"], l=pc["l"].copy(), u=pc["u"][0].copy(), i_idx=pc["i_idx"],
               i_l=pc["i_l"], i_u=pc["i_u"])
    models.insert(2, _model(backend, pcp, pc["settings"], pc["qp_settings"]))
    insts.insert(2, dict(q=pc["q"][1].copy(), u=pc["u"][1].copy(), x0=pc["x0"][1].copy()))
    return models, insts


def _same(got, want, k):
    assert set(got) == set(want), k
    for key in want:
        if key == "run_time":
            continue
        g, w = got[key], want[key]
        if isinstance(w, np.ndarray):
            np.testing.assert_array_equal(g, w, err_msg="%s of model %d" % (key, k))
        elif isinstance(w, float) and w != w:
            assert g != g, (key, k)
        else:
            assert g == w, (key, k, g, w)


def test_four_oracle_models_equal_their_own_polished_solve_many(oracle_mod):
    models, insts = _four(oracle_mod)
    info = {}
    got = miosqp_amd.solve_models(models, insts, info=info, polish=True)
    assert len(got) == 4
    assert info["polished"] == [] and info["polish_launches"] == 0
    copies, _ = _four(oracle_mod)
    some = 0
    for k, m in enumerate(copies):
        want = m.solve_many([insts[k]], polish=True)[0]
        assert {"polished", "polish_rounds", "pri_after", "dua_after"} <= set(got[k])
        _same(got[k], want, k)
        assert info["polish_own"].get(k) == "backend without polish_models" or \
            got[k]["status"] not in (bnb.MI_SOLVED, bnb.MI_MAX_ITER_FEASIBLE)
        some += bool(got[k]["polished"])
    assert some >= 1  # (the comparison is not one of four untouched incumbents)
    # polish=False: today's dicts, without the polish keys
    plain = miosqp_amd.solve_models(models, insts)
    assert all("polished" not in r for r in plain)
    # the list form on its own, in place, equals the keyword
    again = miosqp_amd.polish_models(models, insts, plain)
    assert again is plain
    for k in range(4):
        _same(plain[k], got[k], k)


def test_polish_must_be_a_bool(oracle_mod):
    models, insts = _four(oracle_mod)
    for bad in ("yes", "device", 1, None):
        with pytest.raises(ValueError, match="polish must be False or True"):
            miosqp_amd.solve_models(models, insts, polish=bad)
    with pytest.raises(ValueError, match='guess must be "host" or "device"'):
        miosqp_amd.solve_models(models, insts, polish=True, polish_guess="both")


def test_mismatched_list_lengths(oracle_mod):
    from miosqp_amd import qp
    models, insts = _four(oracle_mod)
    res = miosqp_amd.solve_models(models, insts)
    with pytest.raises(ValueError, match="4 models, 3 instances, 4 results"):
        miosqp_amd.polish_models(models, insts[:3], res)
    with pytest.raises(ValueError, match="4 models, 4 instances, 2 results"):
        miosqp_amd.polish_models(models, insts, res[:2])
    with pytest.raises(ValueError, match="tau must be positive"):
        miosqp_amd.polish_models(models, insts, res, tau=0.0)
    # the engine-level call: the lists are compared before the library is loaded
    v = [np.zeros(3)] * 2
    with pytest.raises(ValueError, match="one entry per model in every list"):
        qp.polish_models([object(), object()], v, v, v, v[:1], v, 1e-6, 3, 20)
    with pytest.raises(ValueError, match="delta must be a scalar or have one entry per model"):
        qp.polish_models([object(), object()], v, v, v, v, v, [1e-6] * 3, 3, 20)


def test_the_symbols_are_declared():
    from miosqp_amd import _lib, qp
    assert "miosqp_qp_polish_models" in _lib.SYMBOLS and "miosqp_qp_polish_models_fits" in _lib.SYMBOLS
    assert [f[0] for f in _lib.PolishModelsStats._fields_] == ["launches", "models", "lds_bytes", "arena_bytes", "device_time",
                                                               "run_time", "upload_time", "launch_time", "download_time"]
    assert callable(qp.polish_models) and callable(miosqp_amd.polish_models)
    header = open(os.path.join(os.path.dirname(HERE), "include", "miosqp_amd.h")).read()
    assert "int miosqp_qp_polish_models(int32_t B, miosqp_qp_engine *const *engines," in header


def test_sanitized_refusals_arena_layout_and_lds_figure(tmp_path):
    exe = str(tmp_path / "polish_models_plan_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(HERE, "polish_models_plan_harness.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "polish_models_plan ok" in r.stdout
