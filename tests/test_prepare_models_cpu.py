"""setup_models(..., prepare="device") without a GPU: the ARITHMETIC of k_prepare_models and the plan of such a call.

miosqp_amd/csrc/prepare_models_body.hpp is written as phases between barriers; tests/prepare_models_cpu.cpp (a program
with its own main, linked with factor.cpp, built with -fsanitize=address,undefined and run directly) runs those phases with
a loop over the thread index and compares EVERY output bit for bit with scale_problem + pack_factor_rows: the shapes
(10,5,2), n + M = 192 and 193, (50,200,10), (20,530,4) with M > 512, n = 198 with M = 2; an empty column and an empty
row of A, a zero column of P, P given as a full symmetric matrix, rows of odd and even counts, an explicit zero in A, a
column norm below kMinScaling and one above kMaxScaling, q = 0; scaling 0, 1 and 10 on every problem.  The program also
walks the plan of calls with prepared models (setup_plan.hpp): sizes, an exact cover of the arena, the pinned slab holding
the one download, small and large forms mixed.

What the CPU cannot show -- that the device's 1 / sqrt is correctly rounded as the host's is -- is tests/
test_gpu_prepare_models.py's.  Then the keyword in the package: its ValueError, and the CPU oracle ignoring it."""
import os
import subprocess

import numpy as np
import pytest

import miosqp_amd
from miosqp_amd import bnb, problems
from oracle import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "miosqp_amd", "csrc")


def test_sanitized_phases_bit_for_bit_the_hosts_and_the_plan(tmp_path):
    exe = str(tmp_path / "prepare_models_cpu")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(HERE, "prepare_models_cpu.cpp"),
                           os.path.join(CSRC, "factor.cpp"), "-pthread", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "prepare_models ok (10 problems x 3 scalings)" in r.stdout


def _problems():
    return [problems.random_miqp(n, m, p, seed=s) for n, m, p, s in [(12, 30, 6, 8), (10, 5, 2, 0)]]


@pytest.mark.parametrize("bad", ["host", True, 1, "Device", b"device"])
def test_any_other_value_is_a_value_error_before_anything_is_set_up(bad):
    with pytest.raises(ValueError, match='prepare must be None or "device"'):
        miosqp_amd.setup_models(_problems(), dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS), backend=oracle, prepare=bad)


def test_the_oracle_backend_ignores_the_keyword():
    prs = _problems()
    info, plain = {}, {}
    got = miosqp_amd.setup_models(prs, dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS), info=info, backend=oracle,
                                  prepare="device")
    ref = miosqp_amd.setup_models(prs, dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS), info=plain, backend=oracle)
    assert info["prepare"] == [] and plain["prepare"] == [] and info["batched"] == [] and info["launches"] == 0
    assert info["own"] == plain["own"]
    for a, b in zip(got, ref):
        assert isinstance(a, bnb.MIOSQP)
        ra, rb = a.solve(), b.solve()
        assert ra.status == rb.status and ra.upper_glob == rb.upper_glob
        np.testing.assert_array_equal(ra.x, rb.x)


def test_the_symbols_are_declared():
    from miosqp_amd import _lib, qp
    assert "miosqp_qp_setup_models_prepared" in _lib.SYMBOLS
    assert callable(qp.setup_models_prepared)
    header = open(os.path.join(os.path.dirname(HERE), "include", "miosqp_amd.h")).read()
    assert "int miosqp_qp_setup_models_prepared(int32_t B," in header
    for flag in ("MIOSQP_SETUP_MODELS_RHO_AUTO 1", "MIOSQP_SETUP_MODELS_LARGE 2", "MIOSQP_SETUP_MODELS_LARGE_RHO_AUTO 4"):
        assert "#define " + flag in header
