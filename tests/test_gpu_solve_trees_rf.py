"""solve_many / solve_models with heuristic="device" on the HIP engine (needs an MI355X): round and fix INSIDE the one-launch
trees (miosqp_qp_solve_trees_rf, miosqp_qp_solve_trees_models_rf; kernels k_tree_rf, k_tree_rf_m, k_tree_rf_r_m).

The reference for a tree is the CPU oracle backend's sequential solve of the same instance with the same settings --
`bnb.MIOSQP(backend=oracle)`, `solve_many(inst, lockstep=False)`, `rf_stats` read after each solve, as
tests/test_gpu_lockstep_rf.py::_sequential reads them --, computed inside the test.  Per instance: status, nodes and
osqp_iter equal, the five counters of the heuristic equal, upper_glob within 1e-9 relative (a winner's value is the
device's sum), x exact at the integer positions.  The HIP engine's own sequential path (`solve_many`
without the keyword) must agree with the oracle in the same way: the condition is on the references, not on the new code.
Every case also asserts the reference tree's own numbers, so that no case can pass on a tree that never fires.
Settings unless said otherwise: QP_SETTINGS with rho 0.1, rf_max_iter 250, rf_candidates 7, tree_explor_rule 1."""
import copy

import numpy as np
import pytest

import miosqp_amd
from miosqp_amd import bnb, problems
from oracle import oracle

pytestmark = pytest.mark.gpu

RF_KEYS = ("calls", "candidates", "feasible", "improved", "osqp_iter")
FEASIBLE = (bnb.MI_SOLVED, bnb.MI_MAX_ITER_FEASIBLE)
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _engines_closed_at_the_end():
    """the models of the mixed list are shared by this module's tests and closed when it is done (a later module counts the
    engines of the process)"""
    yield
    for mdl in _CACHE.pop("mixed", ([],))[0]:
        mdl.work.solver.close()


def _problem(shape):
    if ("pr",) + shape not in _CACHE:
        n, m, p, seed = shape
        _CACHE[("pr",) + shape] = problems.random_miqp(n, m, p, seed=seed)
    return _CACHE[("pr",) + shape]


def _model(shape, backend=None, rho=0.1, **st):
    pr = _problem(shape)
    settings = dict(problems.BNB_SETTINGS, primal_heuristic=1, rf_max_iter=250, rf_every=3)
    settings.update(st)
    mdl = bnb.MIOSQP() if backend is None else bnb.MIOSQP(backend=backend)
    mdl.setup(pr["P"], pr["q"], pr["A"], pr["l"].copy(), pr["u"].copy(), pr["i_idx"], pr["i_l"], pr["i_u"], settings,
              dict(problems.QP_SETTINGS, rho=rho))
    return mdl


def _sequential(mdl, inst):
    """solve_many(lockstep=False) with work.rf_stats read after every solve(): (dicts, per-instance counters)"""
    stats = []
    solve0 = bnb.MIOSQP.solve

    def solve(self, *a, **kw):
        res = solve0(self, *a, **kw)
        stats.append({k: int(self.work.rf_stats[k]) for k in RF_KEYS})
        return res

    bnb.MIOSQP.solve = solve
    try:
        out = mdl.solve_many(inst, lockstep=False)
    finally:
        bnb.MIOSQP.solve = solve0
    assert len(stats) == len(inst)
    return out, stats


def _oracle_reference(key, shape, inst, rho=0.1, **st):
    """the oracle backend's sequential solve, once per session and left unchanged"""
    if ("ref",) + key not in _CACHE:
        _CACHE[("ref",) + key] = _sequential(_model(shape, backend=oracle, rho=rho, **st), inst)
    return _CACHE[("ref",) + key]


def _same_tree(g, grf, w, wrf, ii, what):
    print("%s: %s %d nodes %d iterations %.12g rf %s | oracle %s %d %d %.12g rf %s"
          % (what, g["status"], g["nodes"], g["osqp_iter"], g["upper_glob"], [grf[a] for a in RF_KEYS], w["status"], w["nodes"],
             w["osqp_iter"], w["upper_glob"], [wrf[a] for a in RF_KEYS]))
    assert (g["status"], g["nodes"], g["osqp_iter"]) == (w["status"], w["nodes"], w["osqp_iter"]), what
    assert {a: grf[a] for a in RF_KEYS} == wrf, what
    if w["status"] in FEASIBLE:
        assert abs(g["upper_glob"] - w["upper_glob"]) <= 1e-9 * max(1.0, abs(w["upper_glob"])), what
        np.testing.assert_array_equal(g["x"][ii], w["x"][ii])
    else:
        assert g["upper_glob"] == w["upper_glob"], what


def _bitwise(a, b, what=""):
    assert (a["status"], a["nodes"], a["osqp_iter"], a["upper_glob"]) == (b["status"], b["nodes"], b["osqp_iter"], b["upper_glob"]), what
    if np.isfinite(b["upper_glob"]):
        np.testing.assert_array_equal(a["x"], b["x"])


S40, S60, S12, S50, S100, S50L = (40, 60, 20, 7), (60, 80, 30, 3), (12, 30, 6, 8), (50, 100, 10, 0), (100, 200, 15, 0), (50, 200, 10, 0)

# (id, shape, bnb settings, rho, the reference tree's own numbers)
CASES = [
    ("40-rule1", S40, dict(tree_explor_rule=1, rf_every=3, rf_candidates=7), 0.1, dict(nodes=25, calls=4, feasible=8, improved=2)),
    ("60-rule0", S60, dict(tree_explor_rule=0, rf_every=3, rf_candidates=7), 0.1,
     dict(nodes=82, osqp_iter=4325, calls=14, feasible=22, improved=3)),
    ("60-rule1", S60, dict(tree_explor_rule=1, rf_every=3, rf_candidates=7), 0.1,
     dict(nodes=82, osqp_iter=4325, calls=14, feasible=22, improved=3)),
    ("60-rule2", S60, dict(tree_explor_rule=2, rf_every=3, rf_candidates=7), 0.1,
     dict(nodes=72, osqp_iter=3850, calls=13, feasible=21, improved=2)),
    ("60-rule3", S60, dict(tree_explor_rule=3, rf_every=3, rf_candidates=7), 0.1,
     dict(nodes=72, osqp_iter=3850, calls=13, feasible=21, improved=2)),
    # n + M = 48: wave-sized, runs in k_tree_rf
    ("12-rule1", S12, dict(tree_explor_rule=1, rf_every=3), 0.1, dict(nodes=25, calls=4, feasible=6, improved=1)),
    ("12-rule3", S12, dict(tree_explor_rule=3, rf_every=3), 0.1, dict(nodes=13, calls=3, feasible=0, improved=0)),
    ("12-K1", S12, dict(rf_every=1, rf_candidates=1), 0.1, dict(calls=12, candidates=12, feasible=1)),
    ("12-K32", S12, dict(rf_every=1, rf_candidates=32), 0.1, dict(candidates=384, feasible=68, improved=3)),
    # one termination test per candidate
    ("40-cap25", S40, dict(rf_every=1, rf_max_iter=25), 0.1, dict(nodes=73, calls=36, feasible=32, improved=4)),
    ("40-bb10", S40, dict(rf_every=1, max_iter_bb=10), 0.1, dict(status=bnb.MI_MAX_ITER_FEASIBLE, nodes=9, calls=5)),
    ("60-bb10", S60, dict(rf_every=1, max_iter_bb=10), 0.1, dict(status=bnb.MI_MAX_ITER_FEASIBLE, nodes=9, calls=7)),
    ("40-auto", S40, dict(rf_every=3), "auto", dict(nodes=71, calls=12, improved=4)),
]


@pytest.mark.parametrize("name, shape, st, rho, tree", CASES, ids=[c[0] for c in CASES])
def test_a_tree_with_round_and_fix_inside_equals_the_oracle(name, shape, st, rho, tree):
    ii = _problem(shape)["i_idx"]
    (w,), (wrf,) = _oracle_reference((name,), shape, [{}], rho=rho, **st)
    have = dict(wrf, **w)  # (osqp_iter: the nodes' iterations)
    assert {k: have[k] for k in tree} == tree  # the reference tree is the one this case was chosen for
    mdl = _model(shape, rho=rho, **st)
    try:
        (s,), (srf,) = _sequential(mdl, [{}])
        _same_tree(s, srf, w, wrf, ii, name + " HIP sequential")
        before = (dict(mdl.work.rf_stats), mdl.work.rf_nodes)
        mdl.work.trees_info = None
        (g,) = mdl.solve_many([{}], heuristic="device")
        assert mdl.work.trees_info is not None and not mdl.work.trees_info[0].overflow  # the launch ran and holds the tree
        assert (dict(mdl.work.rf_stats), mdl.work.rf_nodes) == before
        _same_tree(g, mdl.work.trees_rf[0], w, wrf, ii, name + " in the launch")
    finally:
        mdl.work.solver.close()


def test_without_the_heuristic_the_first_tree_is_the_long_one():
    (w,), _ = _oracle_reference(("40-off",), S40, [{}], primal_heuristic=0)
    assert w["nodes"] == 84


def _batch_instances(pr, B, ref_model):
    """the recipe of test_many_trees_in_one_launch_equal_the_sequential_calls: own q per instance, own l and u on two
    thirds, an x0 that set_x0 accepts on every fourth, and one instance infeasible by its bounds.  The x0 is a unit
    vector (A has entries in [0, 1): 0 <= A x0 < 1 lies inside [l, u]), not the optimum of a first run as in that recipe:
    with the optimum as incumbent, a candidate that finds the same point again TIES with it, and whether
    `obj < upper_glob` holds is then the rounding of two sums taken in different orders -- `improved` differed by one on
    such an instance while every other figure agreed.  That is no property of the trees."""
    n, m = len(pr["q"]), len(pr["l"])
    rng = np.random.RandomState(99)
    inst = []
    for k in range(B):
        d = dict(q=rng.randn(n), l=-2 + rng.rand(m), u=2 + rng.rand(m))
        if k % 3 == 0:
            d = dict(q=rng.randn(n))
        inst.append(d)
    b = 50.0 * (1 - 2 * (np.arange(m) % 2))  # alternating equalities, more rows than variables
    inst[B - 2] = dict(q=inst[B - 2]["q"], l=b, u=b.copy())
    x0 = np.zeros(n)
    x0[pr["i_idx"][0]] = 1.0
    for k in range(0, B, 4):
        inst[k] = dict(inst[k], x0=x0.copy())
    Q, L, U = ref_model._instance_vectors(inst)
    for k in range(0, B, 4):
        assert ref_model._instance_incumbent(inst[k], Q[k], L[k], U[k]) is not None, k  # accepted
    return inst


def test_a_batch_of_trees_each_against_its_own_reference():
    B, pr = 24, _problem(S50)
    st = dict(rf_every=2)
    ref_model = _model(S50, backend=oracle, **st)
    inst = _batch_instances(pr, B, ref_model)
    assert sum("x0" in d for d in inst) == 6
    want, want_rf = _sequential(ref_model, inst)
    mdl = _model(S50, **st)
    try:
        data = mdl.work.data
        before = (data.q.copy(), data.l.copy(), data.u.copy(), dict(mdl.work.rf_stats), mdl.work.rf_nodes, mdl.work.upper_glob)
        got = mdl.solve_many(inst, heuristic="device")
        assert np.array_equal(data.q, before[0]) and np.array_equal(data.l, before[1]) and np.array_equal(data.u, before[2])
        assert (dict(mdl.work.rf_stats), mdl.work.rf_nodes, mdl.work.upper_glob) == before[3:]
        assert len(got) == len(mdl.work.trees_rf) == B and not any(t.overflow for t in mdl.work.trees_info)
        for k in range(B):
            _same_tree(got[k], mdl.work.trees_rf[k], want[k], want_rf[k], pr["i_idx"], "instance %d" % k)
        # the per-instance record is offset per instance: the counters are not one tree's, repeated
        assert len({tuple(c[a] for a in RF_KEYS) for c in mdl.work.trees_rf}) >= 4
        assert any(c["improved"] > 0 for c in want_rf) and any(c["calls"] > 1 for c in want_rf)
        k = B - 2  # infeasible by its bounds: no node branches, nothing fires
        assert want[k]["status"] == bnb.MI_PRIMAL_INFEASIBLE and got[k]["upper_glob"] == np.inf
        assert mdl.work.trees_rf[k] == dict.fromkeys(RF_KEYS, 0)
        # the sequential path of the HIP engine agrees with the oracle on the same instances
        seq, seq_rf = _sequential(mdl, inst)
        for k in range(B):
            _same_tree(seq[k], seq_rf[k], want[k], want_rf[k], pr["i_idx"], "instance %d HIP sequential" % k)
    finally:
        mdl.work.solver.close()


# ---- solve_models on a mixed list -------------------------------------------------------------------------------------
MIXED = [(S12, dict(primal_heuristic=1)), (S12, dict(primal_heuristic=0)), (S40, dict(primal_heuristic=1)),
         ((50, 100, 10, 1), dict(primal_heuristic=0)), (S100, dict(primal_heuristic=1)), (S50L, dict(primal_heuristic=0)),
         (S12, dict(primal_heuristic=0, branching_rule=1))]
ON, OFF = (0, 2, 4), (1, 3, 5)


def _mixed():
    """the seven models, set up once, and the call under test"""
    if "mixed" not in _CACHE:
        models = [_model(shape, **st) for shape, st in MIXED]
        info = {}
        before = [(dict(m.work.rf_stats), m.work.rf_nodes, m.work.data.q.copy()) for m in models]
        out = miosqp_amd.solve_models(models, info=info, large="device", heuristic="device")
        for m, (stats, nodes, q) in zip(models[:6], before):  # the launched models are left as they were
            assert (dict(m.work.rf_stats), m.work.rf_nodes) == (stats, nodes) and np.array_equal(m.work.data.q, q)
        _CACHE["mixed"] = (models, out, info)
    return _CACHE["mixed"]


def test_solve_models_mixed_list_forms_and_reasons():
    models, out, info = _mixed()
    assert info["forms"] == dict(wave=1, group=1, reduced=1, group_rf=2, reduced_rf=1)
    assert info["launches"] == 5 and info["launched"] == [0, 1, 2, 3, 4, 5] and info["overflow"] == []
    assert info["own"] == {6: "branching_rule 1"}
    assert sorted(info["rf"]) == list(ON)
    assert all(info["rf"][k]["calls"] > 0 and info["rf"][k]["candidates"] == 7 * info["rf"][k]["calls"] for k in ON)
    assert {k: info["rf"][k]["improved"] for k in ON} == {0: 1, 2: 2, 4: 2}  # (the reference trees' figures)


def test_solve_models_heuristic_off_models_are_untouched_by_the_keyword():
    models, out, _ = _mixed()
    info = {}
    plain = miosqp_amd.solve_models(models, info=info, large="device")
    assert info["forms"] == dict(wave=1, group=1, reduced=1) and "rf" not in info
    assert {k: info["own"][k] for k in ON} == dict.fromkeys(ON, "primal_heuristic on")
    for k in OFF + (6,):
        _bitwise(out[k], plain[k], "model %d" % k)


def test_solve_models_product_form_models_equal_their_own_solve_many():
    models, out, info = _mixed()
    for k in (0, 2):
        (own,) = models[k].solve_many([{}], heuristic="device")
        _bitwise(out[k], own, "model %d" % k)
        assert models[k].work.trees_rf == [info["rf"][k]]


def test_solve_models_does_not_depend_on_the_order_of_the_list():
    models, out, info = _mixed()
    rinfo = {}
    rev = miosqp_amd.solve_models(models[::-1], info=rinfo, large="device", heuristic="device")[::-1]
    for k in range(len(models)):
        _bitwise(rev[k], out[k], "model %d" % k)
    assert rinfo["forms"] == info["forms"] and {6 - k: c for k, c in rinfo["rf"].items()} == info["rf"]


def test_solve_models_product_form_models_equal_the_oracle():
    models, out, info = _mixed()
    for k, name in ((0, "12-rule1"), (2, "40-rule1")):
        (w,), (wrf,) = _oracle_reference((name,), MIXED[k][0], [{}], rho=0.1, **CASES[[c[0] for c in CASES].index(name)][2])
        _same_tree(out[k], info["rf"][k], w, wrf, _problem(MIXED[k][0])["i_idx"], "model %d" % k)


def test_solve_models_reduced_form_with_round_and_fix_equals_the_oracle():
    models, out, info = _mixed()
    (w,), (wrf,) = _oracle_reference(("100-rule1",), S100, [{}])
    assert (w["nodes"], wrf["calls"], wrf["improved"]) == (37, 6, 2)
    _same_tree(out[4], info["rf"][4], w, wrf, _problem(S100)["i_idx"], "reduced form")
    (s,), (srf,) = _sequential(models[4], [{}])
    _same_tree(s, srf, w, wrf, _problem(S100)["i_idx"], "reduced form's model, HIP sequential")


def test_solve_models_with_the_keyword_and_polish():
    models, out, _ = _mixed()
    info = {}
    pol = miosqp_amd.solve_models(models, info=info, large="device", heuristic="device", polish=True)
    assert info["forms"] == dict(wave=1, group=1, reduced=1, group_rf=2, reduced_rf=1) and "polished" in info
    for k in range(len(models)):
        assert {"polished", "polish_rounds", "pri_after", "dua_after"} <= set(pol[k]) and "polished" not in out[k]
        own = copy.deepcopy(out[k])  # what polish_many makes of the same x
        models[k].polish_many([{}], [own])
        assert (pol[k]["polished"], pol[k]["polish_rounds"]) == (own["polished"], own["polish_rounds"]), k
        np.testing.assert_array_equal([pol[k]["pri_after"], pol[k]["dua_after"]], [own["pri_after"], own["dua_after"]])


def test_an_overflowed_tree_under_the_keyword_is_redone_by_its_own_model():
    models, out, _ = _mixed()
    info = {}
    (got,) = miosqp_amd.solve_models([models[4]], info=info, large="device", heuristic="device", leaf_cap=2)
    assert info["overflow"] == [0] and info["forms"]["reduced_rf"] == 1 and info["launched"] == [0]
    (own,) = models[4].solve_many([{}])
    _bitwise(got, own, "the overflowed model")


def test_the_library_refuses_bad_settings_before_anything_is_queued():
    from miosqp_amd import qp
    models, _, _ = _mixed()
    s, d = models[0].work.solver, models[0].work.data
    n, M = d.n, d.m + d.n_int
    args = (d.q[None], d.l[None], d.u[None], np.zeros((1, n)), np.zeros((1, M)), [np.inf], None, 1, 1000)
    for bad in ((0, 250, 3), (33, 250, 3), (7, 0, 3), (7, 250, 0)):
        with pytest.raises(RuntimeError, match="solve_trees_rf"):
            s.solve_trees_rf(*args, *bad)
    margs = ([s], [d.q], [d.l], [d.u], [np.zeros(n)], [np.zeros(M)], [np.inf], [None], [1], [1000])
    for bad in ((33, 250, 3), (-1, 250, 3), (7, 0, 3), (7, 250, 0)):
        with pytest.raises(RuntimeError, match="of model 0"):
            qp.solve_trees_models(*margs, rf=[bad])
