"""Round and fix (settings["primal_heuristic"] = 1) on the CPU oracle backend.

Without an engine that has `round_and_fix`, Workspace solves the K candidates of a node with the reference's four calls
on a second solver instance (max_iter = rf_max_iter) and judges them in numpy: the restatement the device entry point
miosqp_qp_round_and_fix is checked against on the GPU (tests/test_gpu_round_and_fix.py).
"""
import types

import numpy as np
import pytest

from golden_cases import load_case, run_case
from miosqp_amd import problems

SOLVED, MAX_ITER = 1, -2
# random_miqp n, m, p, seed (density 0.7), rho = 0.1: nodes without / with the heuristic measured at 12 / 12, 30 / 30,
# 25 / 24, 38 / 38, 122 / 85, 83 / 78
INSTANCES = [(50, 100, 10, 0), (50, 100, 10, 1), (30, 150, 15, 4), (40, 60, 20, 2), (60, 80, 30, 3), (100, 200, 50, 0)]


def _model(pr, backend, qp_extra=None, **settings):
    from miosqp_amd import bnb
    model = bnb.MIOSQP(backend=backend)
    model.setup(pr["P"], pr["q"], pr["A"], np.copy(pr["l"]), np.copy(pr["u"]), pr["i_idx"], pr["i_l"], pr["i_u"],
                dict(problems.BNB_SETTINGS, **settings), dict(problems.QP_SETTINGS, **(qp_extra or {})))
    return model


# -- 1. settings ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [dict(primal_heuristic=2), dict(rf_candidates=0), dict(rf_candidates=33),
                                 dict(rf_candidates=2.5), dict(rf_max_iter=30), dict(rf_max_iter=0),
                                 dict(rf_max_iter=-25), dict(rf_every=0), dict(rf_every=1.5)])
def test_bad_settings_are_refused_at_setup(oracle_mod, bad):
    pr = problems.random_miqp(50, 100, 10, seed=0)
    assert problems.QP_SETTINGS.get("check_termination", 25) == 25
    with pytest.raises(ValueError):
        _model(pr, oracle_mod, **dict(dict(primal_heuristic=1), **bad))


def test_defaults(oracle_mod):
    from miosqp_amd import bnb
    assert bnb.heuristic_settings({}, {}) == dict(on=0, K=7, max_iter=4000, every=10)
    # the QP's max_iter when it is a multiple of check_termination, otherwise rounded down to one
    assert bnb.heuristic_settings({}, dict(max_iter=1000))["max_iter"] == 1000
    assert bnb.heuristic_settings({}, dict(max_iter=1010))["max_iter"] == 1000
    assert bnb.heuristic_settings({}, dict(max_iter=1010, check_termination=10))["max_iter"] == 1010
    # given: a multiple, or the QP's own cap (the engine then runs the tail)
    assert bnb.heuristic_settings(dict(rf_max_iter=250), {})["max_iter"] == 250
    assert bnb.heuristic_settings(dict(rf_max_iter=1010), dict(max_iter=1010))["max_iter"] == 1010


def test_without_the_setting_the_recorded_trace_is_replayed(oracle_mod):
    for extra in (dict(), dict(primal_heuristic=0)):
        case = load_case("cfg1_n50m100p10_s0")
        case["settings"] = dict(case["settings"], **extra)
        assert "primal_heuristic" not in load_case("cfg1_n50m100p10_s0")["settings"]
        got = run_case(case, oracle_mod)
        for g, e in zip(got, case["solves"]):
            assert g["iter_num"] == e["iter_num"] and g["osqp_iter"] == e["osqp_iter"]
            np.testing.assert_array_equal(g["trace"], e["trace"])
            assert g["upper_glob"] == e["upper_glob"]


# -- 2. whole trees ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trees(oracle_mod):
    out = {}
    for inst in INSTANCES:
        n, m, p, seed = inst
        pr = problems.random_miqp(n, m, p, seed=seed)
        for on in (0, 1):
            model = _model(pr, oracle_mod, qp_extra=dict(rho=0.1), primal_heuristic=on)
            uppers, node_iters = [], []

            def obs(w, leaf):
                uppers.append(w.upper_glob)
                node_iters.append(leaf.num_iter)

            res = model.solve(observer=obs)
            out[inst, on] = types.SimpleNamespace(res=res, iter_num=model.work.iter_num, uppers=uppers,
                                                  rf=dict(model.work.rf_stats), osqp_iter=model.work.osqp_iter,
                                                  node_iters=node_iters)
    return out


@pytest.mark.parametrize("inst", INSTANCES)
def test_effect_on_trees(trees, inst):
    off, on = trees[inst, 0], trees[inst, 1]
    print("%r: %d nodes without, %d with; rf_stats %r" % (inst, off.iter_num, on.iter_num, on.rf))
    assert off.res.status == "Solved" and on.res.status == "Solved"
    assert abs(on.res.upper_glob - off.res.upper_glob) <= 1e-3 * max(1.0, abs(off.res.upper_glob))
    # an incumbent after the first node; none there without the heuristic
    assert np.isfinite(on.uppers[0]) and np.isinf(off.uppers[0])
    assert on.iter_num <= off.iter_num
    rf = on.rf
    assert rf["calls"] > 0 and rf["improved"] >= 1 and rf["feasible"] <= rf["candidates"] == 7 * rf["calls"]
    assert rf["osqp_iter"] > 0
    assert off.rf == dict(calls=0, candidates=0, feasible=0, improved=0, osqp_iter=0, solve_time=0.)


def test_fires_on_every_rf_every_th_fractional_node(oracle_mod):
    pr = problems.random_miqp(60, 80, 30, seed=3)
    calls = {}
    for every in (1, 10):
        model = _model(pr, oracle_mod, primal_heuristic=1, rf_every=every)
        model.solve()
        w = model.work
        assert w.rf_stats["calls"] == (w.rf_nodes + every - 1) // every
        calls[every] = w.rf_stats["calls"]
    assert calls[1] > calls[10] > 1


# -- 3. the candidates --------------------------------------------------------------------------------------------
def _recording_backend(oracle_mod, seen):
    class OSQP(oracle_mod.OSQP):
        def update(self, q=None, l=None, u=None):
            if l is not None:
                seen.append((np.array(l), np.array(u)))
            return oracle_mod.OSQP.update(self, q=q, l=l, u=u)

    return types.SimpleNamespace(OSQP=OSQP, constant=oracle_mod.constant)


def test_candidate_construction(oracle_mod):
    from miosqp_amd import bnb
    K = 7
    # integer entry j sits at e8/8 + s * 1e-12 inside node bounds lo, hi
    spec = [(0, +1, 0, 1), (1, -1, 0, 1), (1, +1, 0, 1), (3, -1, 0, 1), (4, +1, 0, 1), (4, -1, 0, 1), (7, +1, 0, 1),
            (8, -1, 0, 1), (5, +1, 0, 0), (2, -1, 1, 1), (12, -1, 0, 3), (12, +1, 2, 3), (-3, +1, -1, 1), (6, -1, 0, 1),
            (7, -1, 0, 1)]
    p = len(spec)
    xi = np.array([e8 / 8.0 + s * 1e-12 for e8, s, _, _ in spec])
    lo = np.array([float(a) for _, _, a, _ in spec])
    hi = np.array([float(b) for _, _, _, b in spec])
    # floor(e8/8 + s 1e-12 + (k+1)/8) in integers: (e8 + k + 1) // 8 just above a multiple of 1/8, (e8 + k) // 8 just below
    want = np.empty((K, p))
    for k in range(K):
        for j, (e8, s, a, b) in enumerate(spec):
            r = (e8 + k + 1) // 8 if s > 0 else (e8 + k) // 8
            want[k, j] = min(max(r, a), b)
    np.testing.assert_array_equal(bnb.rf_roundings(xi, lo, hi, K), want)
    assert len({tuple(row) for row in want}) == K  # no two candidates alike here
    np.testing.assert_array_equal(want[3], np.minimum(np.maximum(np.round(xi), lo), hi))  # k = 3 rounds to nearest

    # and what Workspace.round_and_fix hands to the solver: those values on the integer rows (l = u), every other row
    # the node's
    seen = []
    pr = problems.random_miqp(30, 150, p, seed=4)
    model = _model(pr, _recording_backend(oracle_mod, seen), primal_heuristic=1)
    w = model.work
    leaf = w.leaves[0]
    leaf.solve()
    leaf.l, leaf.u = leaf.l.copy(), leaf.u.copy()
    leaf.l[-p:], leaf.u[-p:] = lo, hi
    leaf.x[w.data.i_idx] = xi
    del seen[:]
    r = w.round_and_fix(leaf)
    assert len(seen) == K and len(r.status) == K
    for k, (l, u) in enumerate(seen):
        np.testing.assert_array_equal(l[-p:], want[k])
        np.testing.assert_array_equal(u[-p:], want[k])
        np.testing.assert_array_equal(l[:-p], leaf.l[:-p])
        np.testing.assert_array_equal(u[:-p], leaf.u[:-p])
    if r.chosen >= 0:
        np.testing.assert_array_equal(r.x[w.data.i_idx], want[r.chosen])


def test_acceptance_rule_by_hand(oracle_mod):
    """Per candidate: the reference's own test (satisfies_lin_constraints on the root's bounds) and objective of the
    rounded point; chosen = lowest objective among the feasible ones below upper_glob, ties to the lowest k."""
    pr = problems.random_miqp(40, 60, 20, seed=2)
    model = _model(pr, oracle_mod, primal_heuristic=1)
    w = model.work
    leaf = w.leaves[0]
    leaf.solve()
    assert not w.is_int_feas(leaf.x, leaf)
    r = w.round_and_fix(leaf)
    ii, d = w.data.i_idx, w.data
    feas = []
    for k in range(7):
        assert r.status[k] in (SOLVED, MAX_ITER)
        feas.append(bool(r.viol[k] <= 0.0))
    assert 0 < sum(feas) < 7 and r.feasible == sum(feas)  # this root has candidates of both kinds
    best = min((r.obj[k], k) for k in range(7) if feas[k])[1]
    assert r.chosen == best
    x = r.x
    np.testing.assert_array_equal(x[ii], np.round(x[ii]))
    assert w.satisfies_lin_constraints(x, d.l, d.u)
    assert d.compute_obj_val(x) == r.obj[best]
    # a caller's upper below every objective: nothing counts, the flags stay
    w.upper_glob = float(np.min(r.obj)) - 1.0
    r2 = w.round_and_fix(leaf)
    assert r2.chosen == -1 and r2.x is None and r2.feasible == r.feasible
    np.testing.assert_array_equal(r2.obj, r.obj)
    assert w.rf_stats["calls"] == 2 and w.rf_stats["candidates"] == 14 and w.rf_stats["feasible"] == 2 * r.feasible


def test_statistics_stay_apart_from_the_node_relaxations(trees):
    for inst in INSTANCES:
        on = trees[inst, 1]
        assert on.rf["osqp_iter"] > 0 and on.osqp_iter == sum(on.node_iters)


# -- 4. a new linear cost ------------------------------------------------------------------------------------------
def test_update_vectors_reaches_the_second_solver(oracle_mod):
    from miosqp_amd import bnb
    pr = problems.random_miqp(40, 60, 20, seed=2)
    q2 = pr["q"] + 0.5 * np.cos(np.arange(len(pr["q"])))
    model = _model(pr, oracle_mod, primal_heuristic=1)
    model.solve()
    w = model.work
    assert w._second  # the heuristic's solver exists, set up with the old q
    model.update_vectors(q=q2)
    assert w.rf_stats["calls"] == 0 and w.rf_nodes == 0
    leaf = w._make_root()
    leaf.solve()
    r = w.round_and_fix(leaf)
    w._reset_counters()
    # by hand: a solver set up like the second one and told the new cost the same way, the four calls per candidate
    d = w.data
    o = oracle_mod.OSQP()
    o.setup(d.P, pr["q"], d.A, d.l, d.u, **dict(problems.QP_SETTINGS, max_iter=w.rf["max_iter"]))
    o.update(q=q2)
    ii, p = d.i_idx, d.n_int
    fix = bnb.rf_roundings(leaf.x[ii], leaf.l[-p:], leaf.u[-p:], 7)
    for k in range(7):
        l, u = leaf.l.copy(), leaf.u.copy()
        l[-p:] = u[-p:] = fix[k]
        o.update(l=l, u=u)
        o.warm_start(x=leaf.x, y=leaf.y)
        res = o.solve()
        assert (res.info.status_val, res.info.iter) == (r.status[k], r.iter[k])
        x = res.x.copy()
        x[ii] = fix[k]
        assert .5 * x.dot(d.P.dot(x)) + q2.dot(x) == r.obj[k]
    # the old cost gives other candidates
    old = _model(pr, oracle_mod, primal_heuristic=1)
    root = old.work._make_root()
    root.solve()
    assert np.max(np.abs(old.work.round_and_fix(root).obj - r.obj)) > 1e-3
    # and the tree closes where a model set up with the new cost closes
    fresh = _model(dict(pr, q=q2), oracle_mod, primal_heuristic=1)
    ra, rb = model.solve(), fresh.solve()
    assert ra.status == rb.status == "Solved"
    assert abs(ra.upper_glob - rb.upper_glob) <= 1e-3 * max(1.0, abs(rb.upper_glob))
    assert w.rf_stats["calls"] > 0 and w.rf_stats["improved"] >= 1


# -- 5. searches that do not run it say so --------------------------------------------------------------------------
def test_sharded_searches_refuse_the_heuristic(oracle_mod):
    from miosqp_amd import dist
    model = _model(problems.random_miqp(50, 100, 10, seed=0), oracle_mod, primal_heuristic=1)
    with pytest.raises(ValueError):
        dist.ShardedSearch(model)
    with pytest.raises(ValueError):
        dist.ShardedStream(model)
