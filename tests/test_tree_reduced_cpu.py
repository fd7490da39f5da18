"""The reduced-form relaxation of the one-launch trees (solve_models(..., large="device"); k_tree_r_m) on the CPU:

1. the ARITHMETIC of the kernel's iteration: miosqp_amd/csrc/tree_reduced_body.hpp is written as phases between barriers,
   and tests/tree_reduced_body_cpu.cpp runs those phases with a loop over the thread index (built with
   -fsanitize=address,undefined; the LDS of the workgroup is a heap block of exactly the size the launch asks for), on the
   packed rows and the factor the host's scale_problem / build_factor make.  From a warm start that is not zero (x, z, y of a
   solved root, two rows then fixed to one of their bounds) 25 and 100 iterations are compared with the long-double
   restatement of admm_step in tests/tree_reduced_reference.py, under the rule of setup_cases.check: the error against the
   long-double run may be 8 x the larger of (what the float64 run of the same restatement shows, N rounding units), N = n + M
   being the length of a row of the KKT solve.  The program also asserts the LDS rule: inside 160 KB, no two arrays that are
   live together overlap, every entry of the packed triangle in its own place.
2. the reduced iteration against a plain loop of res_admm's two product-form sweeps: both within the rule, hence at most
   two bounds apart.
3. the plan of miosqp_qp_solve_trees_models_large (models_plan.hpp) in a sanitized stand-alone fuzz program.
4. the list handling of solve_models(large=...) on the oracle backend, and the declared symbols.
Nothing here touches a GPU."""
import os
import subprocess

import numpy as np
import pytest

import miosqp_amd
import setup_reference as sr
import tree_reduced_reference as trr
from miosqp_amd import bnb, problems
from oracle import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(3, 2, 1), (60, 125, 8), (120, 60, 13), (20, 530, 4), (150, 100, 5)]
MARKS = (25, 100)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("tree_reduced_body")
    return trr.build(d), d


_RUNS = {}


def _case(exe, shape):
    """(program output, long-double run, float64 run) of one shape: computed once, shared, read-only"""
    if shape not in _RUNS:
        n, m, p = shape
        pr = problems.random_miqp(n, m, p, seed=n)
        A, l, u = problems.extended(pr)
        # fixed after the warm start: the first integer row to its lower bound, the second (a general row where the model
        # has one integer variable) to its upper bound
        tight = (m, m + 1 if p >= 2 else 0)
        o = trr.run(exe[0], exe[1], pr["P"], pr["q"], A, l, u, tight)
        ref = [trr.admm(o.Pbar, o.Abar, o.q, o.l, o.u, o.rho, o.sigma, o.alpha, o.x0, o.z0, o.y0, MARKS, T)
               for T in (np.longdouble, np.float64)]
        _RUNS[shape] = (o, ref[0], ref[1])
    return _RUNS[shape]


def _rule(name, Z, ref_ld, ref_64, N):
    floor, got = sr.err(ref_64, ref_ld), sr.err(Z, ref_ld)
    bound = sr.bound(floor, N)
    print("tree-reduced rule %-22s N=%-4d floor %.3e  measured %.3e  bound %.3e  factor taken %.2f of 8"
          % (name, N, floor, got, bound, got / max(floor, N * 2.0 ** -53)))
    assert floor < 1e-8, (name, floor)  # the instance is sane: the restatement itself resolves it
    assert got <= bound, (name, got, floor, bound)
    return bound


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_phases_against_the_long_double_restatement(exe, shape):
    o, ld, f64 = _case(exe, shape)
    N = o.n + o.M
    assert o.lds_doubles * 8 <= 160 * 1024
    assert o.tri_ld % 32 == 28 and o.tri_ld >= o.n - 1
    assert np.abs(o.x0).max() > 0 and np.abs(o.z0).max() > 0 and np.abs(o.y0).max() > 0  # the warm start is not zero
    for source in ("packed", "dense"):
        for k in MARKS:
            for name, Z, a, b in zip("xzy", o.runs[source][k], ld[k], f64[k]):
                _rule("%s %s after %d" % (name, source, k), Z, a, b, N)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_reduced_iteration_equals_the_product_form_iteration(exe, shape):
    o, ld, f64 = _case(exe, shape)
    N = o.n + o.M
    for k in MARKS:
        for name, Zp, Zr, a, b in zip("xzy", o.runs["product"][k], o.runs["packed"][k], ld[k], f64[k]):
            bound = _rule("%s product form after %d" % (name, k), Zp, a, b, N)
            apart = float(np.abs(Zp.astype(np.longdouble) - Zr).max() / np.abs(a).max())
            print("   reduced against product form: %.3e (two bounds: %.3e)" % (apart, 2 * bound))
            assert apart <= 2 * bound


def test_sanitized_plan_of_the_large_entry(tmp_path):
    exe = str(tmp_path / "models_plan_large_fuzz")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(HERE, "models_plan_large_fuzz.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "models_plan_large ok" in r.stdout


def _oracle_models():
    out = []
    for n, m, p, s in [(12, 30, 6, 8), (10, 5, 2, 0)]:
        pr = problems.random_miqp(n, m, p, seed=s)
        mdl = bnb.MIOSQP(backend=oracle)
        mdl.setup(pr["P"], pr["q"], pr["A"], pr["l"], pr["u"], pr["i_idx"], pr["i_l"], pr["i_u"], dict(problems.BNB_SETTINGS),
                  dict(problems.QP_SETTINGS))
        out.append(mdl)
    return out


def test_on_the_oracle_backend_the_keyword_changes_nothing():
    models = _oracle_models()
    plain_info, large_info = {}, {}
    plain = miosqp_amd.solve_models(models, info=plain_info)
    large = miosqp_amd.solve_models(models, info=large_info, large="device", leaf_cap=2)
    for a, b in zip(plain, large):
        assert (a["status"], a["nodes"], a["osqp_iter"], a["upper_glob"]) == (b["status"], b["nodes"], b["osqp_iter"], b["upper_glob"])
        np.testing.assert_array_equal(a["x"], b["x"])
    assert plain_info["forms"] == dict(wave=0, group=0)  # without the keyword the dict is what it was
    assert large_info["forms"] == dict(wave=0, group=0, reduced=0)
    assert large_info["launched"] == [] and large_info["launches"] == 0 and large_info["own"] == plain_info["own"]
    assert all("backend" in why for why in large_info["own"].values())


def test_value_errors_of_the_keywords():
    models = _oracle_models()
    for bad in (True, False, "host", 1, "Device"):
        with pytest.raises(ValueError, match="large must be None or"):
            miosqp_amd.solve_models(models, large=bad)
    for bad in (1, 0, -3, 2.5, True):
        with pytest.raises(ValueError, match="leaf_cap must be an integer of at least 2"):
            miosqp_amd.solve_models(models, large="device", leaf_cap=bad)
    with pytest.raises(ValueError, match="leaf_cap must be an integer of at least 2"):
        miosqp_amd.solve_models(models, leaf_cap=1)  # checked whether or not the keyword is on


def test_the_symbols_are_declared():
    from miosqp_amd import _lib, qp
    assert "miosqp_qp_tree_form_large" in _lib.SYMBOLS and "miosqp_qp_solve_trees_models_large" in _lib.SYMBOLS
    assert len(_lib.SYMBOLS["miosqp_qp_solve_trees_models_large"][1]) == len(_lib.SYMBOLS["miosqp_qp_solve_trees_models"][1]) + 1
    assert callable(qp.OSQP.tree_form_large)
    header = open(os.path.join(os.path.dirname(HERE), "include", "miosqp_amd.h")).read()
    assert "int miosqp_qp_tree_form_large(miosqp_qp_engine *e, int32_t leaf_cap);" in header
    assert "int miosqp_qp_solve_trees_models_large(int32_t B," in header
