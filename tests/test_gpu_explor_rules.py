"""The best-bound exploration rules (settings["tree_explor_rule"] = 2, 3) in every search form of the HIP engine.

The yardstick is MIOSQP.solve's Python loop on the SAME engine (device_tree=False, device_search=False: solve_node per
node, Workspace.leaf_index choosing): the one-launch trees (k_tree_w for n + M <= 64, k_tree up to 192; the choice is a
parallel first-minimum over the leaf list there), solve_many and the hosted search must visit the same nodes -- status,
node count and ADMM iteration count EQUAL, incumbent within the tolerances of the form-against-form tests of
tests/test_gpu_parity.py (one-launch trees: value 1e-8, x 1e-7; hosted search: value 1e-9, x 1e-8, integers equal).
Two siblings share their parent's bound, so nearly every choice under best bound is a tie: a form that broke ties
differently would visit another tree and miss the counts.  Both settings of rho (0.1 and "auto") throughout.
"""
import numpy as np
import pytest

from miosqp_amd import problems

pytestmark = pytest.mark.gpu

RHOS = [0.1, "auto"]
# n + M <= 64: k_tree_w.  The four (10,5,2) trees close at their root and the power converter's list never exceeds 3
# leaves (measured), so two more with real lists: under rule 2 at rho 0.1 (32,8,16,0) keeps up to 67 leaves open -- more
# than one per lane of the one wavefront -- and (32,8,16,6) up to 31 (counted by the Python loop on the CPU oracle)
WAVE = [(10, 5, 2, 0), (10, 5, 2, 1), (10, 5, 2, 2), (10, 5, 2, 3), "pc", (32, 8, 16, 0), (32, 8, 16, 6)]
GROUP = [(50, 100, 10, 0), (50, 100, 10, 1), (40, 60, 20, 2), (60, 80, 30, 3), (50, 25, 25, 1)]  # 65 .. 192: k_tree


def rel(a, b):
    return np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b)))


def _problem(inst):
    """(problem dict, B&B settings, QP settings, x0 or None)"""
    if inst == "pc":  # the power-converter model's first MIQP, with the initial solution its MPC loop hands in
        pc = problems.load_power_converter()
        pr = dict(P=pc["P"], q=pc["q"][0].copy(), A=pc["A"], l=pc["l"].copy(), u=pc["u"][0].copy(), i_idx=pc["i_idx"],
                  i_l=pc["i_l"], i_u=pc["i_u"])
        return pr, dict(pc["settings"]), dict(pc["qp_settings"]), pc["x0"][0].copy()
    n, m, p, seed = inst
    return problems.random_miqp(n, m, p, seed=seed), dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS), None


def _solve(inst, rule, rho, x0=None, **st):
    from miosqp_amd import bnb
    pr, settings, qs, x0_own = _problem(inst)
    x0 = x0_own if x0 is None else x0
    mdl = bnb.MIOSQP()
    mdl.setup(pr["P"], pr["q"], pr["A"], pr["l"].copy(), pr["u"].copy(), pr["i_idx"], pr["i_l"], pr["i_u"],
              dict(settings, tree_explor_rule=rule, **st), dict(qs, rho=rho))
    w = mdl.work
    if x0 is not None:
        mdl.set_x0(np.array(x0, dtype=float))
    had_inc = bool(np.isfinite(w.upper_glob))
    r = mdl.solve()
    info = getattr(w, "tree_info", None)
    out = dict(status=r.status, nodes=w.iter_num - 1, iters=w.osqp_iter, upper=float(r.upper_glob),
               x=np.array(r.x, dtype=float), ii=pr["i_idx"], no_tree=getattr(w, "_no_tree", False),
               hosted=getattr(w, "_hosted", None) is not None, had_inc=had_inc,
               tree=None if info is None else (int(info.overflow), int(info.max_leaves), int(info.nodes)))
    w.solver.close()
    return out


_cache = {}


def _cached(inst, rule, rho, **st):
    """every (instance, rule, rho, form) is solved once per session and shared by the tests below"""
    key = (inst, rule, rho, tuple(sorted(st.items())))
    if key not in _cache:
        _cache[key] = _solve(inst, rule, rho, **st)
    return _cache[key]


def _loop(inst, rule, rho):
    return _cached(inst, rule, rho, device_tree=False, device_search=False)


def _same_tree(a, b, val_tol, x_tol):
    assert (a["status"], a["nodes"], a["iters"]) == (b["status"], b["nodes"], b["iters"])
    if np.isfinite(b["upper"]):
        assert abs(a["upper"] - b["upper"]) <= val_tol * max(1.0, abs(b["upper"]))
        assert rel(a["x"], b["x"]) <= x_tol
        np.testing.assert_array_equal(np.round(a["x"][a["ii"]]), np.round(b["x"][b["ii"]]))
    else:
        assert not np.isfinite(a["upper"])


@pytest.mark.parametrize("rho", RHOS)
@pytest.mark.parametrize("rule", [2, 3])
@pytest.mark.parametrize("inst", WAVE + GROUP, ids=str)
def test_one_launch_tree_equals_the_python_loop(inst, rule, rho):
    a, b = _cached(inst, rule, rho), _loop(inst, rule, rho)
    print("%r rule %d rho %s: launch %d nodes / %d iterations, leaf list overflow / longest / nodes %r; loop %d / %d"
          % (inst, rule, rho, a["nodes"], a["iters"], a["tree"], b["nodes"], b["iters"]))
    # the launch ran, held the tree, and is what solve() returned (no fall-back to the loop under test)
    assert not a["no_tree"] and not a["hosted"] and a["tree"] is not None and a["tree"][0] == 0
    assert a["tree"][2] == a["nodes"]
    assert b["tree"] is None and not b["hosted"]
    _same_tree(a, b, 1e-8, 1e-7)


def test_the_group_reduction_sees_more_than_one_wavefront_of_leaves():
    """k_tree's first-minimum runs across the wavefront and then, through LDS, across the eight wavefronts: only a list
    longer than 64 puts candidates into more than one of them.  Longest list per GROUP instance under rule 2 at rho 0.1,
    measured: 10, 11, 14, 66, 40 -- (60,80,30,3) is the one (the Python loop on the CPU oracle counts the same 66)."""
    longest = {inst: _cached(inst, 2, 0.1)["tree"][1] for inst in GROUP}
    print("longest leaf list under rule 2, rho 0.1: %r" % longest)
    assert max(longest.values()) > 64
    assert _cached((60, 80, 30, 3), 2, 0.1)["nodes"] == _loop((60, 80, 30, 3), 2, 0.1)["nodes"]


def test_the_wavefront_reduction_sees_more_than_one_leaf_per_lane():
    """k_tree_w: lane r takes the positions r, r + 64, ...; only a list longer than 64 gives a lane two of them and moves
    the tail in more than one round.  Longest list under rule 2 at rho 0.1, measured: (32,8,16,0) 67, (32,8,16,6) 31."""
    a = _cached((32, 8, 16, 0), 2, 0.1)
    print("longest leaf list of (32,8,16,0) under rule 2, rho 0.1: %d" % a["tree"][1])
    assert a["tree"][1] > 64 and a["nodes"] == _loop((32, 8, 16, 0), 2, 0.1)["nodes"]


@pytest.mark.parametrize("rho", RHOS)
@pytest.mark.parametrize("n,m,p,seed,B", [(50, 100, 10, 0, 16), (10, 5, 2, 0, 8), (32, 8, 16, 0, 8)])
def test_solve_many_under_rule_3_equals_the_sequential_calls(n, m, p, seed, B, rho):
    from miosqp_amd import bnb
    pr = problems.random_miqp(n, m, p, seed=seed)
    seq, bat = bnb.MIOSQP(), bnb.MIOSQP()
    for mdl in (seq, bat):
        mdl.setup(pr["P"], pr["q"], pr["A"], pr["l"].copy(), pr["u"].copy(), pr["i_idx"], pr["i_l"], pr["i_u"],
                  dict(problems.BNB_SETTINGS, tree_explor_rule=3), dict(problems.QP_SETTINGS, rho=rho))
    rng = np.random.RandomState(seed + 17)
    inst = [dict(q=rng.randn(n)) for _ in range(B)]
    want = []
    for d in inst:
        seq.update_vectors(q=d["q"].copy())
        r = seq.solve()
        want.append(dict(x=np.array(r.x, dtype=float), upper=r.upper_glob, status=r.status, nodes=seq.work.iter_num - 1,
                         osqp_iter=seq.work.osqp_iter))
    got = bat.solve_many(inst)
    infos = bat.work.trees_info
    assert len(got) == len(infos) == B and all(int(i.overflow) == 0 for i in infos)  # the one-launch path held every tree
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g["status"], g["nodes"], g["osqp_iter"]) == (w["status"], w["nodes"], w["osqp_iter"]), k
        assert int(infos[k].nodes) == w["nodes"], k
        if w["status"] == bnb.MI_SOLVED:
            assert g["upper_glob"] == w["upper"], k
            np.testing.assert_array_equal(g["x"], w["x"])
    seq.work.solver.close()
    bat.work.solver.close()


@pytest.mark.parametrize("rho", RHOS)
def test_an_incumbent_handed_in_makes_rule_3_best_bound_from_the_first_node(rho):
    """x0 = the x of the closed tree: under rule 3 nothing is left of the dive, so the tree is rule 2's with that x0 --
    on the one-launch path, in the Python loop and through the x0 key of solve_many."""
    from miosqp_amd import bnb
    inst = (50, 100, 10, 1)
    # (the tree closed at rho 0.1 for both: set_x0 holds x0 to eps_abs on the constraints, which the x of the tree
    #  closed at rho "auto" misses -- "Invalid initial solution!" --, and a refused x0 is no incumbent)
    x0 = _cached(inst, 3, 0.1)["x"]
    r2, r3 = _solve(inst, 2, rho, x0=x0), _solve(inst, 3, rho, x0=x0)
    l2, l3 = (_solve(inst, rule, rho, x0=x0, device_tree=False, device_search=False) for rule in (2, 3))
    assert r2["had_inc"] and r3["had_inc"] and l2["had_inc"] and l3["had_inc"]
    assert r3["tree"] is not None and r3["tree"][0] == 0 and r2["tree"][0] == 0 and l3["tree"] is None
    _same_tree(r3, r2, 0.0, 0.0)
    _same_tree(l3, l2, 0.0, 0.0)
    _same_tree(r3, l3, 1e-8, 1e-7)
    # without the x0, rule 3 dives first: another tree (measured at rho 0.1: 28 nodes with the dive, 25 with the x0)
    print("rule 3 with x0: %d nodes; without: %d" % (r3["nodes"], _cached(inst, 3, rho)["nodes"]))
    pr = problems.random_miqp(*inst[:3], seed=inst[3])
    many = {}
    for rule in (2, 3):
        mdl = bnb.MIOSQP()
        mdl.setup(pr["P"], pr["q"], pr["A"], pr["l"].copy(), pr["u"].copy(), pr["i_idx"], pr["i_l"], pr["i_u"],
                  dict(problems.BNB_SETTINGS, tree_explor_rule=rule), dict(problems.QP_SETTINGS, rho=rho))
        many[rule] = mdl.solve_many([dict(x0=x0.copy()), dict()])
        assert all(int(i.overflow) == 0 for i in mdl.work.trees_info)
        mdl.work.solver.close()
    for rule in (2, 3):
        g = many[rule][0]
        assert (g["status"], g["nodes"], g["osqp_iter"]) == (r3["status"], r3["nodes"], r3["iters"])
    g = many[3][1]  # the instance without x0 beside it dives
    w = _cached(inst, 3, rho)
    assert (g["status"], g["nodes"], g["osqp_iter"]) == (w["status"], w["nodes"], w["iters"])


@pytest.mark.parametrize("rho", RHOS)
@pytest.mark.parametrize("rule", [2, 3])
@pytest.mark.parametrize("inst,st", [((100, 200, 50, 0), {}), ((60, 80, 30, 3), dict(device_tree=False))], ids=str)
def test_hosted_search_equals_the_python_loop(inst, st, rule, rho):
    """bnb.MIOSQP._solve_hosted (the loop in the C++ host library, search_choose) against the Python loop: n + M = 350 runs
    on the cooperative grid kept resident over the search, (60,80,30,3) on the one-workgroup solver."""
    a, b = _cached(inst, rule, rho, **st), _loop(inst, rule, rho)
    print("%r rule %d rho %s: hosted %d nodes / %d iterations; loop %d / %d"
          % (inst, rule, rho, a["nodes"], a["iters"], b["nodes"], b["iters"]))
    assert a["hosted"] and a["tree"] is None and not b["hosted"]
    _same_tree(a, b, 1e-9, 1e-8)
    np.testing.assert_array_equal(a["x"][a["ii"]], b["x"][b["ii"]])


@pytest.mark.parametrize("rule", [2, 3])
def test_streams_and_sharded_searches_refuse_the_best_bound_rules(rule):
    from miosqp_amd import bnb, dist, stream
    pr = problems.random_miqp(30, 60, 12, seed=5)
    mdl = bnb.MIOSQP()
    mdl.setup(pr["P"], pr["q"], pr["A"], pr["l"], pr["u"], pr["i_idx"], pr["i_l"], pr["i_u"],
              dict(problems.BNB_SETTINGS, tree_explor_rule=rule), dict(problems.QP_SETTINGS, max_batch=64))
    eng = mdl.work.solver
    for make in (lambda: stream.StreamSearch(mdl, columns=64), lambda: stream.NativeStreamSearch(mdl, columns=64),
                 lambda: dist.ShardedSearch(mdl), lambda: dist.ShardedStream(mdl, columns=64)):
        with pytest.raises(ValueError, match="tree_explor_rule 0 / 1 only \\(rule %d" % rule):
            make()
    # refused before anything was created on the device
    assert not getattr(eng, "_pool_made", False) and not getattr(eng, "_sdriver_made", False)
    eng.close()


@pytest.mark.parametrize("rule", [0, 1])
@pytest.mark.parametrize("inst", [(50, 100, 10, 0), (100, 200, 50, 0)], ids=str)
def test_rules_0_and_1_are_what_they_were(inst, rule):
    """the serial choice of the one-launch tree and the hosted search's, untouched: the Python loop's counts"""
    a, b = _cached(inst, rule, 0.1), _loop(inst, rule, 0.1)
    assert (a["tree"] is not None) == (inst[0] == 50) and a["hosted"] == (inst[0] == 100)
    _same_tree(a, b, 1e-8, 1e-7)
