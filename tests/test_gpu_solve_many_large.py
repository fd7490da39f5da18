"""solve_many(..., large="device") on the HIP engine (needs an MI355X): B MIQPs on ONE model beyond one workgroup's
product form (`tree_form()` 0, `tree_form_large()` 3), every tree in one launch of k_tree_r / k_tree_rf_r / k_tree_sb_r --
the batch forms of k_tree_r_m, k_tree_rf_r_m, k_tree_sb_r_m (miosqp_qp_solve_trees_large, _rf, _sb).

The reference is existing code, not the code under test: for instance k it is
`solve_models([model], [instances[k]], large="device")[0]`, the _m kernel on the same engine (with `heuristic` /
`branching` the same call with that keyword); its own contract against the CPU oracle is pinned by
tests/test_gpu_solve_models_large.py.  The batch form must equal it BIT FOR BIT in status, nodes, osqp_iter, upper_glob
and every entry of x, and in the rf / sb counters.  Unless a case says otherwise a case is five instances per call: the
variants plain, qlu, x0_valid, x0_invalid and closed of that test's `_variant` (closed: an infeasible root; the two x0
variants: an incumbent handed in, an incumbent refused)."""
import numpy as np
import pytest

from miosqp_amd import problems
from test_gpu_solve_models_large import SPARSE, _build, _problem, _variant, rel

pytestmark = pytest.mark.gpu

KINDS = ["plain", "qlu", "x0_valid", "x0_invalid", "closed"]
_MODELS = {}


def _model(shape, rule=1, rho=0.1, qp=None, **st):
    """the model of (shape, rule, rho, settings), built once per module and kept open"""
    key = (shape, rule, str(rho), tuple(sorted((qp or {}).items())), tuple(sorted(st.items())))
    if key not in _MODELS:
        if qp:
            from miosqp_amd import bnb
            pr = _problem(shape)
            mdl = bnb.MIOSQP()
            mdl.setup(pr["P"], pr["q"], pr["A"], pr["l"].copy(), pr["u"].copy(), pr["i_idx"], pr["i_l"], pr["i_u"],
                      dict(problems.BNB_SETTINGS, tree_explor_rule=rule, **st), dict(problems.QP_SETTINGS, rho=rho, **qp))
            _MODELS[key] = (mdl, pr)
        else:
            _MODELS[key] = _build(shape, rule, rho, **st)
    return _MODELS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for mdl, _ in _MODELS.values():
        mdl.work.solver.close()
    _MODELS.clear()


def _bitwise(g, w, who):
    """status, nodes, osqp_iter, upper_glob and every entry of x equal.  A result without a point (Primal Infeasible,
    Max-iter unsolved without an incumbent) carries an x that `_tree_result` leaves uninitialised on every path: there the
    entries of x are nobody's, and upper_glob (inf on both sides) says so"""
    from miosqp_amd import bnb
    assert (g["status"], g["nodes"], g["osqp_iter"]) == (w["status"], w["nodes"], w["osqp_iter"]), who
    assert g["upper_glob"] == w["upper_glob"], who
    if w["status"] in (bnb.MI_SOLVED, bnb.MI_MAX_ITER_FEASIBLE):
        np.testing.assert_array_equal(g["x"], w["x"], err_msg=who)
    else:
        assert w["upper_glob"] == np.inf and g["x"].shape == w["x"].shape, who


def _five(pr):
    return [_variant(pr, kind, k) for k, kind in enumerate(KINDS)]


def _reference(mdl, inst, **kw):
    """the _m kernel on the same engine, one instance per call: results, the calls' infos"""
    import miosqp_amd
    out, infos = [], []
    for one in inst:
        info = {}
        out.append(miosqp_amd.solve_models([mdl], [one], large="device", info=info, **kw)[0])
        infos.append(info)
    return out, infos


def _spy(mdl, name):
    """counts the calls of one entry of the model's engine"""
    solver, calls = mdl.work.solver, []
    inner = getattr(solver, name)

    def entry(*a, **kw):
        calls.append(a[0].shape[0])
        return inner(*a, **kw)

    setattr(solver, name, entry)
    return calls


def _unspy(mdl, name):
    del mdl.work.solver.__dict__[name]


def _is_form_3(mdl, leaf_cap=256):
    return mdl.work.solver.tree_form() == 0 and mdl.work.solver.tree_form_large(leaf_cap) == 3


def _report(who, got, want):
    for k, (g, w) in enumerate(zip(got, want)):
        print("%s [%d]: %s %d nodes %d iterations %.17g | reference %s %d %d %.17g" % (
            who, k, g["status"], g["nodes"], g["osqp_iter"], g["upper_glob"], w["status"], w["nodes"], w["osqp_iter"], w["upper_glob"]))


# ---- 1. every shape, five instances, bit for bit ------------------------------------------------------------------------
CASES = [((120, 60, 13, 0), 1, 0.1),   # n + M = 193, the first size beyond the small forms
         ((80, 120, 20, 1), 1, 0.1),   # a general mid-size form-3 model
         ((20, 530, 4, 0), 1, 0.1),    # M > 512
         (SPARSE, 1, 0.1),             # sp_off / pv_off >= 0: the LDS copies of Abar
         ((150, 300, 20, 1), 1, 0.1),  # 149 of 160 KB of LDS; this case only
         ((80, 120, 20, 1), 0, 0.1), ((80, 120, 20, 1), 2, 0.1), ((80, 120, 20, 1), 3, 0.1), ((80, 120, 20, 1), 1, "auto")]


@pytest.mark.parametrize("shape, rule, rho", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_five_instances_equal_their_references_bit_for_bit(shape, rule, rho):
    from miosqp_amd import bnb
    mdl, pr = _model(shape, rule, rho)
    assert _is_form_3(mdl), shape
    inst = _five(pr)
    want, _ = _reference(mdl, inst)
    calls = _spy(mdl, "solve_trees_large")
    try:
        got = mdl.solve_many(inst, large="device")
    finally:
        _unspy(mdl, "solve_trees_large")
    assert calls == [5]  # ONE call of the batch entry took all five
    _report("%r rule %d rho %s" % (shape, rule, rho), got, want)
    assert len(mdl.work.trees_info) == 5 and not any(i.overflow for i in mdl.work.trees_info)
    for k, kind in enumerate(KINDS):
        _bitwise(got[k], want[k], "%r %s" % (shape, kind))
    # the variants are what they say: an infeasible root, an incumbent handed in, an incumbent refused -- asserted on the
    # shape tests/test_gpu_solve_models_large.py asserts it on (with fewer rows than variables `closed` can be feasible)
    Q, L, U = mdl._instance_vectors(inst)
    handed_in = mdl._instance_incumbent(inst[2], Q[2], L[2], U[2]) is not None
    print("x0_valid arrives as an incumbent:", handed_in, "; closed:", got[4]["status"])
    if shape[:3] == (80, 120, 20):
        assert got[4]["status"] in (bnb.MI_PRIMAL_INFEASIBLE, bnb.MI_MAX_ITER_UNSOLVED) and got[4]["upper_glob"] == np.inf
        assert handed_in
    assert mdl._instance_incumbent(inst[3], Q[3], L[3], U[3]) is None


# ---- 2. offsets beyond one wave of workgroups ---------------------------------------------------------------------------
def test_three_hundred_instances_position_k_equals_position_k_mod_5():
    mdl, pr = _model((120, 60, 13, 0), 1, 0.1, max_iter_bb=5)
    assert _is_form_3(mdl)
    five = _five(pr)
    want, _ = _reference(mdl, five)
    # not root-only trees: the feasible variants branch within the five permitted nodes
    print("reference nodes:", [w["nodes"] for w in want])
    assert all(want[k]["nodes"] > 1 for k in (0, 1)) and max(w["nodes"] for w in want) > 1
    B = 300
    got = mdl.solve_many([five[k % 5] for k in range(B)], large="device")
    assert len(got) == B and len(mdl.work.trees_info) == B
    for k in range(5):
        _bitwise(got[k], want[k], "position %d" % k)
    for k in range(5, B):
        _bitwise(got[k], got[k % 5], "position %d against %d" % (k, k % 5))


# ---- 3. overflow --------------------------------------------------------------------------------------------------------
OVERFLOW_CAP = 4


@pytest.mark.parametrize("lockstep", [False, "device"], ids=["sequential", "lockstep_device"])
def test_overflowed_trees_go_on_as_lockstep_says(lockstep):
    """(80,120,20) under rule 2 (best bound: the longest lists) with leaf_cap = 4: confirmed on the reference calls that
    some of the five instances overflow at that capacity and some do not -- measured: plain, qlu, x0_valid and x0_invalid
    overflow (their lists reach 34-36 leaves), closed does not (its root is infeasible)."""
    mdl, pr = _model((80, 120, 20, 1), 2, 0.1)
    inst = _five(pr)
    want, infos = _reference(mdl, inst, leaf_cap=OVERFLOW_CAP)
    over = [k for k in range(5) if infos[k]["overflow"] == [0]]
    print("leaf_cap %d: overflowed on the reference calls: %r" % (OVERFLOW_CAP, over))
    assert 0 < len(over) < 5
    got = mdl.solve_many(inst, large="device", leaf_cap=OVERFLOW_CAP, lockstep=lockstep)
    assert [k for k in range(5) if mdl.work.trees_info[k].overflow] == over  # set only on the overflowed ones
    own = mdl.solve_many(inst, lockstep=lockstep)  # the same call without the keyword
    _report("overflow, lockstep=%r" % (lockstep,), got, own)
    for k in range(5):
        if k not in over:
            _bitwise(got[k], want[k], "instance %d (no overflow)" % k)
        elif lockstep is False:  # the sequential path: one instance after the other, bit for bit
            _bitwise(got[k], own[k], "instance %d (overflowed, sequential)" % k)
        else:  # the lock-step driver's contract (its batch differs): decisions equal, values to rounding
            g, w = got[k], own[k]
            assert (g["status"], g["nodes"], g["osqp_iter"]) == (w["status"], w["nodes"], w["osqp_iter"]), k
            if np.isfinite(w["upper_glob"]):
                assert abs(g["upper_glob"] - w["upper_glob"]) <= 1e-8 * max(1.0, abs(w["upper_glob"])), k
                assert rel(g["x"], w["x"]) <= 1e-6, k
            else:
                assert g["upper_glob"] == w["upper_glob"], k


# ---- 4. round and fix inside the trees ----------------------------------------------------------------------------------
RF_SB_SHAPE = (50, 200, 10, 0)


def test_heuristic_device_results_and_counters_equal_the_reference():
    mdl, pr = _model(RF_SB_SHAPE, 1, 0.1, primal_heuristic=1, rf_every=3, rf_candidates=7)
    assert _is_form_3(mdl)
    inst = _five(pr)
    want, infos = _reference(mdl, inst, heuristic="device")
    assert all(i["forms"]["reduced_rf"] == 1 for i in infos)
    ref = [i["rf"][0] for i in infos]
    print("rf counters of the references:", ref)
    assert ref[0]["calls"] > 0 and sum(r["calls"] for r in ref) > 0
    calls = _spy(mdl, "solve_trees_large_rf")
    try:
        got = mdl.solve_many(inst, large="device", heuristic="device")
    finally:
        _unspy(mdl, "solve_trees_large_rf")
    assert calls == [5]
    _report("rf", got, want)
    for k in range(5):
        _bitwise(got[k], want[k], "rf %s" % KINDS[k])
        assert mdl.work.trees_rf[k] == ref[k], k  # calls, candidates, feasible, improved, osqp_iter
        assert set(ref[k]) == {"calls", "candidates", "feasible", "improved", "osqp_iter"}


# ---- 5. strong / reliability branching inside the trees -----------------------------------------------------------------
@pytest.mark.parametrize("rule", [1, 2])
def test_branching_device_results_and_counters_equal_the_reference(rule):
    mdl, pr = _model(RF_SB_SHAPE, 1, 0.1, branching_rule=rule)
    assert _is_form_3(mdl)
    inst = _five(pr)
    want, infos = _reference(mdl, inst, branching="device")
    assert all(i["forms"]["reduced_sb"] == 1 for i in infos)
    ref = [i["sb"][0] for i in infos]
    print("sb counters of the references, rule %d:" % rule, ref)
    assert ref[0]["calls"] > 0
    if rule == 2:
        assert ref[0]["children"] > 0
    calls = _spy(mdl, "solve_trees_large_sb")
    try:
        got = mdl.solve_many(inst, large="device", branching="device")
    finally:
        _unspy(mdl, "solve_trees_large_sb")
    assert calls == [5]
    _report("sb rule %d" % rule, got, want)
    for k in range(5):
        _bitwise(got[k], want[k], "sb rule %d %s" % (rule, KINDS[k]))
        assert mdl.work.trees_sb[k] == ref[k], k  # calls, children, osqp_iter
        assert set(ref[k]) == {"calls", "children", "osqp_iter"}


# ---- 6. a model of form 2 -----------------------------------------------------------------------------------------------
def test_with_a_small_form_the_keyword_changes_nothing():
    mdl, pr = _model((50, 100, 10, 0), 1, 0.1)
    assert mdl.work.solver.tree_form() == 2 and mdl.work.solver.tree_form_large() == 0
    inst = _five(pr)
    calls = _spy(mdl, "solve_trees_large")
    try:
        got = mdl.solve_many(inst, large="device")
    finally:
        _unspy(mdl, "solve_trees_large")
    assert calls == []
    want = mdl.solve_many(inst)
    for k in range(5):
        _bitwise(got[k], want[k], "form 2 %s" % KINDS[k])


# ---- 7. polish on top ---------------------------------------------------------------------------------------------------
def test_polish_device_composes():
    mdl, pr = _model((80, 120, 20, 1), 1, 0.1)
    inst = _five(pr)
    raw = mdl.solve_many(inst, large="device")
    want = [dict(r, x=r["x"].copy()) for r in raw]
    mdl.polish_many(inst, want, large=True)
    got = mdl.solve_many(inst, large="device", polish="device")
    assert any(w.get("polished") for w in want)
    for k in range(5):
        assert set(got[k]) == set(want[k]), k
        for key in set(want[k]) - {"x", "run_time"}:
            a, b = got[k][key], want[k][key]
            assert a == b or (isinstance(a, float) and np.isnan(a) and np.isnan(b)), (k, key)
        _bitwise(got[k], want[k], "polished %s" % KINDS[k])


# ---- 8. a decline of the LDS copies -------------------------------------------------------------------------------------
def test_with_the_lds_copies_switched_off_abar_comes_from_l2(monkeypatch):
    mdl, pr = _model(SPARSE, 1, 0.1)
    inst = _five(pr)
    with_copies = mdl.solve_many(inst, large="device")
    monkeypatch.setenv("MIOSQP_RES_SP", "0")
    assert _is_form_3(mdl)
    want, _ = _reference(mdl, inst)  # under the same switch
    got = mdl.solve_many(inst, large="device")
    for k in range(5):
        _bitwise(got[k], want[k], "MIOSQP_RES_SP=0 %s" % KINDS[k])
        # the same rows from another place: the decisions cannot move
        assert (got[k]["status"], got[k]["nodes"]) == (with_copies[k]["status"], with_copies[k]["nodes"]), k


# ---- 9. a refusal -------------------------------------------------------------------------------------------------------
def test_an_engine_the_reduced_form_does_not_take_keeps_today_s_path():
    """Measured on the device: an engine set up with coop=1 still has its product-form rows and `tree_form_large()`
    answers 3 for it (the cooperative grid is what `MIOSQP.setup` builds by default at these sizes; the test below runs
    it).  The engine the reduced form refuses is the one without those rows, fold=0: `tree_form_large()` 0."""
    mdl, pr = _model((120, 60, 13, 0), 1, 0.1, qp=dict(fold=0))
    assert mdl.work.solver.tree_form() == 0 and mdl.work.solver.tree_form_large() == 0
    inst = _five(pr)
    calls = _spy(mdl, "solve_trees_large")
    try:
        got = mdl.solve_many(inst, large="device")
    finally:
        _unspy(mdl, "solve_trees_large")
    assert calls == [] and not getattr(mdl.work, "_no_trees_large", False)
    want = mdl.solve_many(inst)
    for k in range(5):
        _bitwise(got[k], want[k], "refused %s" % KINDS[k])


def test_an_engine_set_up_with_coop_1_is_taken_like_the_default_one():
    mdl, pr = _model((120, 60, 13, 0), 1, 0.1, qp=dict(coop=1))
    assert _is_form_3(mdl)
    inst = _five(pr)
    want, _ = _reference(mdl, inst)
    got = mdl.solve_many(inst, large="device")
    assert len(mdl.work.trees_info) == 5
    for k in range(5):
        _bitwise(got[k], want[k], "coop=1 %s" % KINDS[k])
