"""polish_models(large="device") / solve_models(polish_large="device") (miosqp_amd/bnb.py) on the CPU: the oracle
backend has no `polish_models_large`, so the keyword is ignored there and every call must equal the call without it key
for key; the values that are refused before anything runs; the two new symbols; and the host logic of the library's
entry (miosqp_amd/csrc/polish_models_large_plan.hpp) in a stand-alone program built with -fsanitize=address,undefined
and run as a subprocess.  Nothing here touches a GPU."""
import os
import subprocess

import pytest

import miosqp_amd
from test_polish_models_cpu import _four, _same

HERE = os.path.dirname(os.path.abspath(__file__))


def test_the_oracle_backend_ignores_the_keyword(oracle_mod):
    models, insts = _four(oracle_mod)
    info, plain_info = {}, {}
    got = miosqp_amd.solve_models(models, insts, info=info, polish=True, polish_large="device")
    want = miosqp_amd.solve_models(models, insts, info=plain_info, polish=True)
    assert len(got) == len(want) == 4
    for k in range(4):
        _same(got[k], want[k], k)
    assert info["polished"] == [] and info["polish_launches"] == 0 and info["polish_forms"] == dict(small=0, large=0)
    assert info["polish_own"] == plain_info["polish_own"] and plain_info["polish_forms"] == dict(small=0, large=0)
    assert any(r["polished"] for r in got)  # (the comparison is not one of four untouched incumbents)
    # the list form on its own
    raw = miosqp_amd.solve_models(models, insts)
    a = miosqp_amd.polish_models(models, insts, [dict(r) for r in raw], large="device")
    b = miosqp_amd.polish_models(models, insts, [dict(r) for r in raw])
    for k in range(4):
        _same(a[k], b[k], k)
        _same(a[k], got[k], k)
    # without polish=True the keyword is not read beyond its validation
    plain = miosqp_amd.solve_models(models, insts, polish_large="device")
    assert all("polished" not in r for r in plain)


def test_other_values_are_refused_before_anything_runs(oracle_mod, monkeypatch):
    from miosqp_amd import bnb
    models, insts = _four(oracle_mod)
    raw = miosqp_amd.solve_models(models, insts)

    def never(*a, **kw):
        raise AssertionError("something ran before the keyword was refused")

    monkeypatch.setattr(bnb.MIOSQP, "solve_many", never)
    monkeypatch.setattr(bnb.MIOSQP, "polish_many", never)
    for bad in ("gpu", True, "host", 1, "Device"):
        res = [dict(r) for r in raw]
        with pytest.raises(ValueError, match='polish_models: large must be None or "device"'):
            miosqp_amd.polish_models(models, insts, res, large=bad)
        assert all("polished" not in r for r in res)  # (not even the keys were written)
    for bad in (True, "host", "gpu", 0):
        for polish in (True, False):
            with pytest.raises(ValueError, match='solve_models: polish_large must be None or "device"'):
                miosqp_amd.solve_models(models, insts, polish=polish, polish_large=bad)
    # polish="device" stays refused: the keyword of the large polish is polish_large
    with pytest.raises(ValueError, match="polish must be False or True"):
        miosqp_amd.solve_models(models, insts, polish="device", polish_large="device")


def test_the_symbols_are_declared():
    from miosqp_amd import _lib, qp
    assert "miosqp_qp_polish_models_large" in _lib.SYMBOLS and "miosqp_qp_polish_models_large_fits" in _lib.SYMBOLS
    assert [f[0] for f in _lib.PolishModelsLargeStats._fields_] == [
        "launches", "models", "workgroups", "pad", "slab_bytes", "arena_bytes", "device_time", "run_time", "upload_time",
        "launch_time", "download_time"]
    assert len(_lib.SYMBOLS["miosqp_qp_polish_models_large"][1]) == len(_lib.SYMBOLS["miosqp_qp_polish_models"][1])
    assert callable(qp.polish_models_large) and callable(qp.OSQP.polish_models_large_fits)
    header = open(os.path.join(os.path.dirname(HERE), "include", "miosqp_amd.h")).read()
    assert "int miosqp_qp_polish_models_large(int32_t B, miosqp_qp_engine *const *engines," in header
    assert "int miosqp_qp_polish_models_large_fits(miosqp_qp_engine *e);" in header
    assert "} miosqp_polish_models_large_stats;" in header
    # the engine-level call compares its lists before the library is loaded
    import numpy as np
    v = [np.zeros(3)] * 2
    with pytest.raises(ValueError, match="polish_models_large: one entry per model in every list"):
        qp.polish_models_large([object(), object()], v, v, v, v[:1], v, 1e-6, 3, 20)
    with pytest.raises(ValueError, match="polish_models_large: delta must be a scalar or have one entry per model"):
        qp.polish_models_large([object(), object()], v, v, v, v, v, [1e-6] * 3, 3, 20)


def test_sanitized_refusals_fit_rule_workgroups_and_arena_layout(tmp_path):
    exe = str(tmp_path / "polish_models_large_plan_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(HERE, "polish_models_large_plan_harness.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "polish_models_large_plan ok" in r.stdout
