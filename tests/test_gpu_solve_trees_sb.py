"""solve_many / solve_models with branching="device" on the HIP engine (needs an MI355X): strong and reliability branching
INSIDE the one-launch trees (miosqp_qp_solve_trees_sb, miosqp_qp_solve_trees_models_sb; kernels k_tree_sb, k_tree_sb_m,
k_tree_sb_r_m).

The reference for a tree is the CPU oracle backend's sequential solve of the same instance with the same settings --
`bnb.MIOSQP(backend=oracle)`, `solve_many(inst, lockstep=False)`, `sb_stats` read after each solve, as
tests/test_gpu_solve_trees_rf.py::_oracle_reference does for `rf_stats` --, computed inside the test.  Per tree: status,
nodes and osqp_iter equal, the three sb counters equal, upper_glob within 1e-9 relative (the tolerance the project uses
where an incumbent's value is the device's sum), x exact at the integer positions.  The HIP engine's own
path without the keyword must agree with the oracle in the same way: the condition is on the references, not on the new
code.  Every case also asserts the reference tree's own numbers, so that no case can pass on a tree that never
strong-branches.  On the oracle the smallest relative gap between the best and the second-best score over all these
cases is 2.5e-3 and the smallest gap in fraction at the candidate cut 4.5e-3: far above what the device's summation order
can move.  Settings unless said otherwise: BNB_SETTINGS, QP_SETTINGS with rho 0.1, sb_max_iter 50, sb_candidates 8,
tree_explor_rule 1."""
import copy

import numpy as np
import pytest

import miosqp_amd
from miosqp_amd import bnb, problems
from oracle import oracle

pytestmark = pytest.mark.gpu

SB_KEYS = ("calls", "children", "osqp_iter")
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


def _model(shape, backend=None, rho=0.1, q=None, **st):
    pr = _problem(shape)
    settings = dict(problems.BNB_SETTINGS, sb_max_iter=50, sb_candidates=8, tree_explor_rule=1)
    settings.update(st)
    mdl = bnb.MIOSQP() if backend is None else bnb.MIOSQP(backend=backend)
    mdl.setup(pr["P"], pr["q"] if q is None else q, pr["A"], pr["l"].copy(), pr["u"].copy(), pr["i_idx"], pr["i_l"], pr["i_u"],
              settings, dict(problems.QP_SETTINGS, rho=rho))
    return mdl


def _sequential(mdl, inst):
    """solve_many(lockstep=False) with work.sb_stats read after every solve(): (dicts, per-instance counters)"""
    stats = []
    solve0 = bnb.MIOSQP.solve

    def solve(self, *a, **kw):
        res = solve0(self, *a, **kw)
        stats.append({k: int(self.work.sb_stats[k]) for k in SB_KEYS})
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


def _same_tree(g, gsb, w, wsb, ii, what):
    print("%s: %s %d nodes %d iterations %.12g sb %s | oracle %s %d %d %.12g sb %s"
          % (what, g["status"], g["nodes"], g["osqp_iter"], g["upper_glob"], [gsb[a] for a in SB_KEYS], w["status"], w["nodes"],
             w["osqp_iter"], w["upper_glob"], [wsb[a] for a in SB_KEYS]))
    assert (g["status"], g["nodes"], g["osqp_iter"]) == (w["status"], w["nodes"], w["osqp_iter"]), what
    assert {a: gsb[a] for a in SB_KEYS} == wsb, what
    if w["status"] in FEASIBLE:
        assert abs(g["upper_glob"] - w["upper_glob"]) <= 1e-9 * max(1.0, abs(w["upper_glob"])), what
        np.testing.assert_array_equal(g["x"][ii], w["x"][ii])
    else:
        assert g["upper_glob"] == w["upper_glob"], what


def _bitwise(a, b, what=""):
    assert (a["status"], a["nodes"], a["osqp_iter"], a["upper_glob"]) == (b["status"], b["nodes"], b["osqp_iter"], b["upper_glob"]), what
    if np.isfinite(b["upper_glob"]):
        np.testing.assert_array_equal(a["x"], b["x"])


S12, S40, S60, S50L, S100 = (12, 30, 6, 8), (40, 60, 20, 7), (60, 80, 30, 3), (50, 200, 10, 0), (100, 200, 15, 0)


def _tree(nodes, osqp_iter, calls, children, sb_iter, **more):
    return dict(nodes=nodes, osqp_iter=osqp_iter, sb=dict(calls=calls, children=children, osqp_iter=sb_iter), **more)


# (id, shape, bnb settings, rho, the reference tree's own numbers): the workgroup form, through solve_many
CASES = [
    # n + M = 48: wave-sized, runs in k_tree_sb
    ("12-rule1", S12, dict(branching_rule=1), 0.1, _tree(23, 1950, 5, 24, 1175)),
    ("12-rule2", S12, dict(branching_rule=2), 0.1, _tree(23, 1950, 7, 28, 1375)),
    ("12-rule1-K1", S12, dict(branching_rule=1, sb_candidates=1), 0.1, _tree(25, 1975, 6, 12, 600)),
    ("12-rule1-K32", S12, dict(branching_rule=1, sb_candidates=32), 0.1, _tree(23, 1950, 5, 24, 1175)),
    ("40-rule1-explor0", S40, dict(branching_rule=1, tree_explor_rule=0), 0.1, _tree(81, 3900, 35, 332, 14700)),
    ("40-rule1-explor1", S40, dict(branching_rule=1, tree_explor_rule=1), 0.1, _tree(81, 3900, 35, 332, 14700)),
    ("40-rule1-explor2", S40, dict(branching_rule=1, tree_explor_rule=2), 0.1, _tree(27, 1425, 16, 176, 7950)),
    ("40-rule2", S40, dict(branching_rule=2), 0.1, _tree(87, 4200, 13, 122, 5400)),
    ("40-rule2-explor3", S40, dict(branching_rule=2, tree_explor_rule=3), 0.1, _tree(46, 2325, 16, 132, 5875)),
    # pseudo-costs only
    ("40-rule2-rel0", S40, dict(branching_rule=2, sb_reliability=0), 0.1, _tree(83, 4100, 0, 0, 0)),
    ("40-rule2-rel1", S40, dict(branching_rule=2, sb_reliability=1), 0.1, _tree(93, 4375, 8, 38, 1650)),
    # one termination test per child
    ("40-rule1-cap25", S40, dict(branching_rule=1, sb_max_iter=25), 0.1, _tree(83, 4050, 36, 336, 8400)),
    ("40-rule1-bb10", S40, dict(branching_rule=1, max_iter_bb=10), 0.1,
     _tree(9, 450, 9, 116, 5225, status=bnb.MI_MAX_ITER_UNSOLVED)),
    ("40-rule1-auto", S40, dict(branching_rule=1), "auto", _tree(83, 4125, 40, 368, 15975)),
    ("60-rule2-K3", S60, dict(branching_rule=2, sb_candidates=3), 0.1, _tree(123, 6300, 41, 138, 6150)),
]

# the reduced form, through solve_models(large="device")
CASES_R = [
    ("50L-rule1", S50L, dict(branching_rule=1), 0.1, _tree(14, 1175, 5, 50, 2500)),
    ("50L-rule2", S50L, dict(branching_rule=2), 0.1, _tree(14, 1175, 6, 46, 2275)),
    ("100-rule2", S100, dict(branching_rule=2), 0.1, _tree(43, 7325, 12, 84, 4125)),
]


def _reference_is_the_chosen_tree(w, wsb, tree):
    have = dict(w, sb=wsb)
    assert {k: have[k] for k in tree} == tree  # the reference tree is the one this case was chosen for


@pytest.mark.parametrize("name, shape, st, rho, tree", CASES, ids=[c[0] for c in CASES])
def test_a_tree_with_the_rule_inside_equals_the_oracle(name, shape, st, rho, tree):
    ii = _problem(shape)["i_idx"]
    (w,), (wsb,) = _oracle_reference((name,), shape, [{}], rho=rho, **st)
    _reference_is_the_chosen_tree(w, wsb, tree)
    mdl = _model(shape, rho=rho, **st)
    try:
        (s,), (ssb,) = _sequential(mdl, [{}])
        _same_tree(s, ssb, w, wsb, ii, name + " HIP without the keyword")
        before = (dict(mdl.work.sb_stats), mdl.work.pc_sum.copy(), mdl.work.pc_cnt.copy())
        mdl.work.trees_info = None
        (g,) = mdl.solve_many([{}], branching="device")
        assert mdl.work.trees_info is not None and not mdl.work.trees_info[0].overflow  # the launch ran and holds the tree
        assert dict(mdl.work.sb_stats) == before[0]
        assert np.array_equal(mdl.work.pc_sum, before[1]) and np.array_equal(mdl.work.pc_cnt, before[2])
        _same_tree(g, mdl.work.trees_sb[0], w, wsb, ii, name + " in the launch")
    finally:
        mdl.work.solver.close()


@pytest.mark.parametrize("name, shape, st, rho, tree", CASES_R, ids=[c[0] for c in CASES_R])
def test_a_reduced_form_tree_with_the_rule_inside_equals_the_oracle(name, shape, st, rho, tree):
    ii = _problem(shape)["i_idx"]
    (w,), (wsb,) = _oracle_reference((name,), shape, [{}], rho=rho, **st)
    _reference_is_the_chosen_tree(w, wsb, tree)
    mdl = _model(shape, rho=rho, **st)
    try:
        (s,), (ssb,) = _sequential(mdl, [{}])
        _same_tree(s, ssb, w, wsb, ii, name + " HIP without the keyword")
        before = (dict(mdl.work.sb_stats), mdl.work.pc_sum.copy(), mdl.work.pc_cnt.copy())
        info = {}
        (g,) = miosqp_amd.solve_models([mdl], info=info, large="device", branching="device")
        assert info["forms"] == dict(wave=0, group=0, reduced=0, group_sb=0, reduced_sb=1) and info["launches"] == 1
        assert info["launched"] == [0] and info["overflow"] == [] and info["own"] == {}
        assert dict(mdl.work.sb_stats) == before[0]
        assert np.array_equal(mdl.work.pc_sum, before[1]) and np.array_equal(mdl.work.pc_cnt, before[2])
        assert mdl.work.trees_sb == [info["sb"][0]]
        _same_tree(g, info["sb"][0], w, wsb, ii, name + " in the launch")
    finally:
        mdl.work.solver.close()


@pytest.mark.parametrize("shape", [S12, S40], ids=["12", "40"])
def test_rule_1_with_one_candidate_reproduces_the_rule_0_tree_bit_for_bit(shape, monkeypatch):
    """with sb_candidates 1 rule 1 branches where rule 0 branches: the block hands the node back untouched.
    (12,30,6) is wave-sized: its plain launch would run in the one-wavefront kernel, which sums a node in another order
    than the workgroup form (upper_glob differed in the last bit, -8.814527438389687 against ...685, every other figure
    equal) -- there is no wavefront form with a rule, so the plain launch is kept in the workgroup form for this
    comparison (MIOSQP_TREE_WAVE=0, the existing switch); (40,60,20) runs in the workgroup form either way.  The plain
    launch as it runs by default, in the one-wavefront kernel, is compared as well: status, nodes and iterations equal, x
    exact at the integer positions, upper_glob to 1e-9 relative (what two orders of the same sums may differ by)."""
    wave = None
    if shape == S12:
        mw = _model(shape, branching_rule=0)
        try:
            (wave,) = mw.solve_many([{}])
            assert mw.work.solver.tree_form() == 1 and not mw.work.trees_info[0].overflow  # the default: one wavefront
        finally:
            mw.work.solver.close()
        monkeypatch.setenv("MIOSQP_TREE_WAVE", "0")
    m0, m1 = _model(shape, branching_rule=0), _model(shape, branching_rule=1, sb_candidates=1)
    try:
        (plain,) = m0.solve_many([{}])
        assert m0.work.trees_info is not None and not m0.work.trees_info[0].overflow
        assert m0.work.solver.tree_form() == 2  # the plain launch ran in the workgroup form
        (g,) = m1.solve_many([{}], branching="device")
        _bitwise(g, plain, "rule 1, K 1 against rule 0")
        if wave is not None:
            ii = _problem(shape)["i_idx"]
            assert (g["status"], g["nodes"], g["osqp_iter"]) == (wave["status"], wave["nodes"], wave["osqp_iter"])
            assert abs(g["upper_glob"] - wave["upper_glob"]) <= 1e-9 * max(1.0, abs(wave["upper_glob"]))
            np.testing.assert_array_equal(g["x"][ii], wave["x"][ii])
        sb = m1.work.trees_sb[0]
        print("K 1:", g["nodes"], g["osqp_iter"], sb)
        assert sb["calls"] > 0 and sb["children"] == 2 * sb["calls"] and sb["osqp_iter"] > 0
    finally:
        m0.work.solver.close()
        m1.work.solver.close()


def test_eight_instances_in_one_launch_each_against_its_own_reference():
    """rule 2: pseudo-costs are per tree and start empty -- every tree equals its own sequential oracle solve"""
    B, pr = 8, _problem(S40)
    rng = np.random.RandomState(5)
    inst = [{}] + [dict(q=pr["q"] + 0.3 * rng.randn(len(pr["q"]))) for _ in range(B - 1)]
    st = dict(branching_rule=2)
    want, want_sb = _oracle_reference(("40-rule2-batch",), S40, inst, **st)
    assert len({(w["nodes"], c["calls"]) for w, c in zip(want, want_sb)}) >= 4 and all(c["calls"] > 0 for c in want_sb)
    # (the first instance is the model's own: the tree of case 40-rule2, whatever stands beside it)
    assert (want[0]["nodes"], want_sb[0]) == (87, dict(calls=13, children=122, osqp_iter=5400))
    mdl = _model(S40, **st)
    try:
        before = (dict(mdl.work.sb_stats), mdl.work.pc_sum.copy(), mdl.work.pc_cnt.copy())
        got = mdl.solve_many(inst, branching="device")
        assert dict(mdl.work.sb_stats) == before[0]
        assert np.array_equal(mdl.work.pc_sum, before[1]) and np.array_equal(mdl.work.pc_cnt, before[2])
        assert len(got) == len(mdl.work.trees_sb) == B and not any(t.overflow for t in mdl.work.trees_info)
        for k in range(B):
            _same_tree(got[k], mdl.work.trees_sb[k], want[k], want_sb[k], pr["i_idx"], "instance %d" % k)
        seq, seq_sb = _sequential(mdl, inst)
        for k in range(B):
            _same_tree(seq[k], seq_sb[k], want[k], want_sb[k], pr["i_idx"], "instance %d HIP without the keyword" % k)
    finally:
        mdl.work.solver.close()


# ---- solve_models on a mixed list -------------------------------------------------------------------------------------
MIXED = [(S12, dict(branching_rule=1)), (S12, dict(branching_rule=0)), (S40, dict(branching_rule=2)),
         ((50, 100, 10, 1), dict(branching_rule=0)), (S40, dict(branching_rule=1)), (S50L, dict(branching_rule=2)),
         (S12, dict(branching_rule=1, primal_heuristic=1, rf_max_iter=250)), (S50L, dict(branching_rule=0))]
RULED, PLAIN, BOTH = (0, 2, 4, 5), (1, 3, 7), 6


def _mixed():
    """the eight models, set up once, and the call under test"""
    if "mixed" not in _CACHE:
        models = [_model(shape, **st) for shape, st in MIXED]
        info = {}
        before = [(dict(m.work.sb_stats), m.work.pc_sum.copy(), m.work.pc_cnt.copy(), m.work.data.q.copy()) for m in models]
        out = miosqp_amd.solve_models(models, info=info, large="device", branching="device")
        for k, (m, (stats, s, c, q)) in enumerate(zip(models, before)):  # the launched models are left as they were
            if k != BOTH:
                assert dict(m.work.sb_stats) == stats and np.array_equal(m.work.pc_sum, s) and np.array_equal(m.work.pc_cnt, c)
            assert np.array_equal(m.work.data.q, q)
        _CACHE["mixed"] = (models, out, info)
    return _CACHE["mixed"]


def test_solve_models_mixed_list_forms_and_reasons():
    models, out, info = _mixed()
    assert info["forms"] == dict(wave=1, group=1, reduced=1, group_sb=3, reduced_sb=1)
    assert info["launches"] == 5 and info["launched"] == [0, 1, 2, 3, 4, 5, 7] and info["overflow"] == []
    assert info["own"] == {BOTH: "branching_rule 1 together with primal_heuristic on"}
    assert sorted(info["sb"]) == list(RULED) and "rf" not in info
    assert all(info["sb"][k]["calls"] > 0 and info["sb"][k]["children"] > 0 for k in RULED)
    # (the reference trees' figures: cases 12-rule1, 40-rule2, 40-rule1-explor1, 50L-rule2)
    assert {k: info["sb"][k]["calls"] for k in RULED} == {0: 5, 2: 13, 4: 35, 5: 6}
    for k in RULED:
        assert models[k].work.trees_sb == [info["sb"][k]]
    # the heuristic's keyword does not move the combined model
    both = {}
    miosqp_amd.solve_models([models[BOTH]], info=both, branching="device", heuristic="device")
    assert both["own"] == {0: "branching_rule 1 together with primal_heuristic on"} and both["launched"] == []


def test_solve_models_rule_0_models_are_untouched_by_the_keyword():
    models, out, _ = _mixed()
    info = {}
    plain = miosqp_amd.solve_models(models, info=info, large="device")
    assert info["forms"] == dict(wave=1, group=1, reduced=1) and "sb" not in info
    assert {k: info["own"][k] for k in RULED} == {0: "branching_rule 1", 2: "branching_rule 2", 4: "branching_rule 1", 5: "branching_rule 2"}
    assert info["own"][BOTH] == "branching_rule 1"
    for k in PLAIN:
        _bitwise(out[k], plain[k], "model %d" % k)


def test_solve_models_workgroup_form_models_equal_their_own_solve_many():
    models, out, info = _mixed()
    for k in (0, 2, 4):
        (own,) = models[k].solve_many([{}], branching="device")
        _bitwise(out[k], own, "model %d" % k)
        assert models[k].work.trees_sb == [info["sb"][k]]


def test_solve_models_does_not_depend_on_the_order_of_the_list():
    models, out, info = _mixed()
    rinfo = {}
    rev = miosqp_amd.solve_models(models[::-1], info=rinfo, large="device", branching="device")[::-1]
    for k in range(len(models)):
        if k != BOTH:  # (the combined model runs on its own path, with its own rounding of the host's sums: not the subject)
            _bitwise(rev[k], out[k], "model %d" % k)
    last = len(models) - 1
    assert rinfo["forms"] == info["forms"] and {last - k: c for k, c in rinfo["sb"].items()} == info["sb"]
    perm = [3, 5, 0, 7, 2, 6, 4, 1]
    pinfo = {}
    mixed = miosqp_amd.solve_models([models[k] for k in perm], info=pinfo, large="device", branching="device")
    for j, k in enumerate(perm):
        if k != BOTH:
            _bitwise(mixed[j], out[k], "model %d" % k)
    assert {perm[j]: c for j, c in pinfo["sb"].items()} == info["sb"]


def test_solve_models_mixed_list_equals_the_oracle():
    models, out, info = _mixed()
    names = [c[0] for c in CASES + CASES_R]
    for k, name in ((0, "12-rule1"), (2, "40-rule2"), (4, "40-rule1-explor1"), (5, "50L-rule2")):
        case = (CASES + CASES_R)[names.index(name)]
        (w,), (wsb,) = _oracle_reference((name,), case[1], [{}], rho=0.1, **case[2])
        _same_tree(out[k], info["sb"][k], w, wsb, _problem(case[1])["i_idx"], "model %d" % k)


def test_solve_models_with_the_keyword_and_polish():
    models, out, _ = _mixed()
    info = {}
    keep = [k for k in range(len(models)) if k != BOTH]
    pol = miosqp_amd.solve_models([models[k] for k in keep], info=info, large="device", branching="device", polish=True)
    assert info["forms"] == dict(wave=1, group=1, reduced=1, group_sb=3, reduced_sb=1) and "polished" in info
    for j, k in enumerate(keep):
        assert {"polished", "polish_rounds", "pri_after", "dua_after"} <= set(pol[j]) and "polished" not in out[k]
        own = copy.deepcopy(out[k])  # what polish_many makes of the same x
        models[k].polish_many([{}], [own])
        assert (pol[j]["polished"], pol[j]["polish_rounds"]) == (own["polished"], own["polish_rounds"]), k
        np.testing.assert_array_equal([pol[j]["pri_after"], pol[j]["dua_after"]], [own["pri_after"], own["dua_after"]])


def test_both_keywords_in_one_call():
    """a model with the heuristic and models with a rule in one list: two calls of the library, every result its own"""
    models, out, info = _mixed()
    rf = _model(S12, primal_heuristic=1, rf_max_iter=250, rf_every=3)
    try:
        binfo = {}
        got = miosqp_amd.solve_models([models[0], rf, models[1], models[2]], info=binfo, branching="device", heuristic="device")
        assert binfo["forms"] == dict(wave=1, group=0, group_rf=1, reduced_rf=0, group_sb=2, reduced_sb=0)
        assert binfo["launched"] == [0, 1, 2, 3] and binfo["launches"] == 3 and sorted(binfo["rf"]) == [1] and sorted(binfo["sb"]) == [0, 3]
        for j, k in ((0, 0), (2, 1), (3, 2)):
            _bitwise(got[j], out[k], "model %d" % k)
        (own,) = rf.solve_many([{}], heuristic="device")
        _bitwise(got[1], own, "the model with the heuristic")
    finally:
        rf.work.solver.close()


def test_an_overflowed_tree_under_the_keyword_is_redone_by_its_own_model():
    models, out, _ = _mixed()
    info = {}
    (got,) = miosqp_amd.solve_models([models[5]], info=info, large="device", branching="device", leaf_cap=2)
    assert info["overflow"] == [0] and info["forms"]["reduced_sb"] == 1 and info["launched"] == [0]
    (own,) = models[5].solve_many([{}])
    _bitwise(got, own, "the overflowed model")


def test_the_library_refuses_bad_settings_before_anything_is_queued():
    from miosqp_amd import qp
    models, _, _ = _mixed()
    s, d = models[0].work.solver, models[0].work.data
    n, M = d.n, d.m + d.n_int
    args = (d.q[None], d.l[None], d.u[None], np.zeros((1, n)), np.zeros((1, M)), [np.inf], None, 1, 1000)
    for bad in ((0, 8, 50, 4, 1e-6), (3, 8, 50, 4, 1e-6), (1, 0, 50, 4, 1e-6), (1, 33, 50, 4, 1e-6), (1, 8, 0, 4, 1e-6),
                (2, 8, 50, -1, 1e-6), (2, 8, 50, 4, 0.0)):
        with pytest.raises(RuntimeError, match="solve_trees_sb"):
            s.solve_trees_sb(*args, *bad)
    margs = ([s], [d.q], [d.l], [d.u], [np.zeros(n)], [np.zeros(M)], [np.inf], [None], [1], [1000])
    for bad in ((3, 8, 50, 4, 1e-6), (1, 33, 50, 4, 1e-6), (1, 8, 0, 4, 1e-6), (2, 8, 50, -1, 1e-6), (2, 8, 50, 4, 0.0)):
        with pytest.raises(RuntimeError, match="of model 0"):
            qp.solve_trees_models(*margs, sb=[bad])
    with pytest.raises(ValueError, match="rf or sb"):
        qp.solve_trees_models(*margs, sb=[None], rf=[None])
