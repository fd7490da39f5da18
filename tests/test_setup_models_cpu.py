"""setup_models on the CPU: the list handling, the errors and the per-model fallback on the oracle backend (where no model
goes into the launch), Workspace(solver=...), the declared symbols, the host logic of the library's entry
(miosqp_amd/csrc/setup_plan.hpp) in a stand-alone program built with -fsanitize=address,undefined, and the ARITHMETIC of
the kernel itself: setup_models_body.hpp is written as phases between barriers, and tests/setup_models_body_cpu.cpp runs
those phases with a loop over the thread index (sanitized as well), so every product of k_setup_models is compared here
with the long-double reference under the rule of setup_cases.check.  Nothing here touches a GPU."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as spa

import miosqp_amd
import setup_cases as sc
import setup_models_cpu_body as cb
import setup_reference as sr
from miosqp_amd import bnb, problems
from oracle import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(12, 30, 6, 8), (10, 5, 2, 0), (20, 10, 8, 1)]


def _problems():
    return [problems.random_miqp(n, m, p, seed=s) for n, m, p, s in SHAPES]


def test_sanitized_argument_checks_eligibility_and_arena_layout(tmp_path):
    exe = str(tmp_path / "setup_plan_fuzz")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(HERE, "setup_plan_fuzz.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "setup_plan ok" in r.stdout


@pytest.fixture(scope="module")
def body(tmp_path_factory):
    d = tmp_path_factory.mktemp("setup_models_body")
    return cb.build(d), d


@pytest.mark.parametrize("shape", [(3, 2, 1), sc.SMALL, (65, 20, 5), (129, 30, 10), (100, 82, 10)], ids=str)
def test_kernel_arithmetic_against_the_long_double_reference(body, shape):
    """every product of the kernel's phases, run on the CPU: d2inv, Linv, W and f_rows under the rule of the set-up
    kernels' tests; LinvT the exact transpose; padding exactly zero; the dense copies, Kc, the scalings and the bounds
    bit for bit what the per-model host set-up makes; the guard below its threshold"""
    exe, d = body
    pr, P, A, l, u = sc.instance(shape)
    o = cb.run(exe, d, P, pr["q"], A, l, u, rho=sc.RHO, sigma=sc.SIGMA, passes=sc.PASSES)
    ld, f64 = sc.reference(shape)
    n, M = shape[0], A.shape[0]
    N = n + M
    assert o.bad_pivot == 0 and o.host_ok
    assert o.lds_doubles * 8 <= 160 * 1024
    sc.check("d2inv", o.d2inv, ld.d2inv, f64.d2inv, n)
    sc.check("Linv", o.Linv[:, :n], ld.Linv, f64.Linv, n)
    assert np.all(np.triu(o.Linv[:, :n]) == 0.0)
    np.testing.assert_array_equal(o.LinvT[:, :n], o.Linv[:, :n].T)
    assert np.all(o.Linv[:, n:] == 0.0) and np.all(o.LinvT[:, n:] == 0.0)
    Kinv = o.W[:, :N].astype(np.longdouble)
    Kinv[:M, :M] -= np.longdouble(sc.RHO) * np.eye(M, dtype=np.longdouble)
    sc.check("W", Kinv, ld.Kinv, f64.Kinv, n)
    assert np.all(o.W[:, N:] == 0.0) and np.all(o.Kc[:, N:] == 0.0)
    F_ld, F_64 = cb.product_form_reference(ld, sc.RHO), cb.product_form_reference(f64, sc.RHO)
    sc.check("f_rows", o.f_rows[:, :N], F_ld, F_64, n)
    sc.check("f_rows", o.h_rows[:, :N], F_ld, F_64, n)  # the host's build_folded under the same formula: anchors it
    assert np.all(o.f_rows[:, N:] == 0.0)
    np.testing.assert_array_equal(o.f_GmT[:, :n], o.f_rows[:, :M].T)
    assert np.all(o.f_GmT[:, n:] == 0.0)
    for name in ("Ad", "Atd", "Pd"):
        np.testing.assert_array_equal(getattr(o, "f_" + name), getattr(o, "h_" + name), err_msg=name)
    np.testing.assert_allclose(o.Kc[:, :N], sr.kc(ld.Pbar, ld.Abar).astype(np.float64), rtol=1e-14, atol=0.0)
    np.testing.assert_array_equal(o.Kc[:M, M:N], o.h_Ad[:, :n])
    np.testing.assert_array_equal(o.Kc[M:N, M:N], o.h_Pd[:, :n])
    np.testing.assert_array_equal(o.l, o.E * np.maximum(l, -1e30))
    np.testing.assert_array_equal(o.u, o.E * np.minimum(u, 1e30))
    assert 0.0 <= o.guard <= 1e-9  # COOP_GUARD_TOL (kernels_guard.inc)


def test_kernel_arithmetic_reports_the_first_bad_pivot(body):
    exe, d = body
    n = 40
    A = spa.identity(n, format="csc")
    for k in (0, 17, 39):
        p = np.ones(n)
        p[k] = -50.0
        o = cb.run(exe, d, spa.diags(p).tocsc(), np.zeros(n), A, -np.ones(n), np.ones(n), passes=0)
        assert o.bad_pivot == 1 and o.pivot == k and not o.host_ok
        assert sr.run(np.diag(p), np.eye(n), np.zeros(n), sc.RHO, sc.SIGMA, 0, np.longdouble, inverses=False).bad_pivot == k


def _run(models):
    return [m.solve() for m in models]


def test_on_the_oracle_backend_every_model_is_set_up_in_place_and_solves_as_the_loop_does():
    prs = _problems()
    info = {}
    got = miosqp_amd.setup_models(prs, dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS), info=info, backend=oracle)
    assert len(got) == len(prs) and all(isinstance(m, bnb.MIOSQP) for m in got)
    assert info["batched"] == [] and sorted(info["own"]) == [0, 1, 2] and info["launches"] == 0
    assert all("backend" in why for why in info["own"].values())
    assert info["device_time"] == 0.0 and info["arena_bytes"] == 0 and info["host_time"] >= 0.0
    for pr, mdl in zip(prs, got):
        ref = bnb.MIOSQP(backend=oracle)
        ref.setup(pr["P"], pr["q"], pr["A"], pr["l"], pr["u"], pr["i_idx"], pr["i_l"], pr["i_u"], dict(problems.BNB_SETTINGS),
                  dict(problems.QP_SETTINGS))
        a, b = mdl.solve(), ref.solve()
        assert a.status == b.status and a.upper_glob == b.upper_glob and a.osqp_iter_avg == b.osqp_iter_avg
        np.testing.assert_array_equal(a.x, b.x)
        assert mdl.work.iter_num == ref.work.iter_num


def test_settings_one_for_all_or_one_per_model():
    prs = _problems()
    per = [dict(problems.BNB_SETTINGS, tree_explor_rule=k % 2) for k in range(3)]
    got = miosqp_amd.setup_models(prs, per, [dict(problems.QP_SETTINGS) for _ in prs], backend=oracle)
    assert [m.work.settings["tree_explor_rule"] for m in got] == [0, 1, 0]
    assert got[0].work.settings is per[0]
    one = dict(problems.BNB_SETTINGS)
    got = miosqp_amd.setup_models(prs, one, dict(problems.QP_SETTINGS), backend=oracle)
    assert got[0].work.settings is not got[1].work.settings and got[0].work.settings is not one


def test_value_errors_before_anything_is_set_up():
    prs = _problems()
    st, qs = dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS)
    with pytest.raises(ValueError, match="empty list"):
        miosqp_amd.setup_models([], st, qs, backend=oracle)
    with pytest.raises(ValueError, match="2 settings for 3 problems"):
        miosqp_amd.setup_models(prs, [st, st], qs, backend=oracle)
    with pytest.raises(ValueError, match="4 qp_settings for 3 problems"):
        miosqp_amd.setup_models(prs, st, [qs] * 4, backend=oracle)
    crossed = [dict(p) for p in prs]
    crossed[1]["l"] = crossed[1]["u"] + 1.0
    crossed[2]["i_l"] = np.asarray(crossed[2]["i_u"]) + 1.0
    with pytest.raises(ValueError, match=r"Lower bound .* position\(s\) \[1, 2\]"):
        miosqp_amd.setup_models(crossed, st, qs, backend=oracle)
    wrong = [dict(p) for p in prs]
    wrong[0]["P"] = spa.identity(5, format="csc")
    with pytest.raises(ValueError, match=r"P must be n x n .* position\(s\) \[0\]"):
        miosqp_amd.setup_models(wrong, st, qs, backend=oracle)


def test_workspace_adopts_a_ready_solver():
    pr = _problems()[1]
    data = bnb.Data(spa.csc_matrix(pr["P"]), pr["q"], spa.csc_matrix(pr["A"]), pr["l"], pr["u"], pr["i_idx"], pr["i_l"], pr["i_u"])
    ready = oracle.OSQP()
    ready.setup(data.P, data.q, data.A, data.l, data.u, **problems.QP_SETTINGS)
    calls = []
    ready.setup = lambda *a, **k: calls.append("setup")
    work = bnb.Workspace(data, dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS), backend=oracle, solver=ready)
    assert work.solver is ready and calls == []
    mdl = bnb.MIOSQP(backend=oracle)
    mdl.work = work
    ref = bnb.MIOSQP(backend=oracle)
    ref.setup(pr["P"], pr["q"], pr["A"], pr["l"], pr["u"], pr["i_idx"], pr["i_l"], pr["i_u"], dict(problems.BNB_SETTINGS),
              dict(problems.QP_SETTINGS))
    a, b = mdl.solve(), ref.solve()
    assert a.status == b.status and a.upper_glob == b.upper_glob
    np.testing.assert_array_equal(a.x, b.x)
    # the default path is unchanged: without `solver` the workspace sets its own solver up
    assert bnb.Workspace(data, dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS), backend=oracle).solver is not ready


def test_the_symbols_are_declared():
    from miosqp_amd import _lib, qp
    for name in ("miosqp_qp_setup_models", "miosqp_qp_setup_models_eligible", "miosqp_qp_setup_groups_live", "miosqp_qp_setup_group",
                 "miosqp_qp_debug_product_form"):
        assert name in _lib.SYMBOLS
    assert [f[0] for f in _lib.SetupModelsStats._fields_] == ["models", "launches", "device_mallocs", "host_mallocs", "streams",
                                                              "reserved", "arena_bytes", "pinned_bytes", "lds_bytes",
                                                              "device_time", "run_time"]
    assert callable(qp.setup_models) and callable(qp.OSQP.debug_product_form) and callable(qp.OSQP.setup_group)
    assert callable(miosqp_amd.setup_models)
    header = open(os.path.join(os.path.dirname(HERE), "include", "miosqp_amd.h")).read()
    assert "int miosqp_qp_setup_models(int32_t B," in header and "int miosqp_qp_setup_groups_live(void);" in header
    assert "int miosqp_qp_debug_product_form(miosqp_qp_engine *e," in header
