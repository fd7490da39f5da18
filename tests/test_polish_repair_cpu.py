"""The repair loop of the polish (repair_iter, settings["polish_repair_iter"]) on the CPU backend: bnb.polish_restatement,
the dense numpy statement the device entry miosqp_qp_polish_repair is checked against (tests/test_gpu_polish_repair.py),
and Workspace.polish_incumbent on top of it.

The expected rounds, adds and drops were measured with the restatement itself before the device code existed; the
residual bound 1e-9 is the one the polish tests use for a point that solves its KKT system in fp64.
"""
import numpy as np
import pytest

from golden_cases import load_case, run_case
from miosqp_amd import problems
import polish_repair_inputs as inputs

TOL = 1e-10
CRUDE_NAMES = [inputs.crude_name(shape, seed) for shape, seed in inputs.CRUDE]
SHARED = ("accepted", "reason", "n_lower", "n_upper", "pri_before", "dua_before", "pri_after", "dua_after", "obj")


@pytest.fixture(scope="module")
def cases(oracle_mod):
    """name -> (problem, qp_extra, Data, l, u, x, y), solved once"""
    return inputs.named_inputs(oracle_mod, ["cfg2_root_rho0.1", "cfg2_root_auto", "cfg1_s1_root_rho0.1",
                                            "cfg1_s1_incumbent_auto", "crude_n64m20p5_s0"] + CRUDE_NAMES)


def _polish(case, **kw):
    from miosqp_amd import bnb
    _, _, d, l, u, x, y = case
    return bnb.polish_restatement(d.P, d.q, d.A, l, u, x, y, 1e-6, 3, **kw)


def _same_bits(a, b):
    np.testing.assert_array_equal(a.x, b.x)
    np.testing.assert_array_equal(a.y, b.y)
    np.testing.assert_array_equal(a.xh, b.xh)
    np.testing.assert_array_equal(a.yh, b.yh)
    np.testing.assert_array_equal(a.active, b.active)
    for f in SHARED:
        assert getattr(a, f) == getattr(b, f), f


# -- 1, 2. one missing row, one round ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name, before, after", [("cfg2_root_rho0.1", 167, 168), ("cfg2_root_auto", 167, 168),
                                                 ("cfg1_s1_root_rho0.1", 18, 19)])
def test_a_root_rejected_today_is_repaired_in_one_round(cases, name, before, after):
    r0 = _polish(cases[name])
    assert (r0.accepted, r0.reason, r0.n_lower + r0.n_upper) == (False, 2, before)
    r = _polish(cases[name], repair_iter=5)
    print("%s: %d -> %d rows, rounds %d, pri %.1e dua %.1e" % (name, before, r.n_lower + r.n_upper, r.rounds,
                                                                r.pri_after, r.dua_after))
    assert (r.accepted0, r.reason0) == (False, 2)
    assert (r.accepted, r.reason, r.stop, r.rounds) == (True, 0, 0, 1)
    assert (r.n_added, r.n_dropped) == (1, 0)
    assert r.n_lower + r.n_upper == after == int(np.sum(r.active != 0))
    assert r.pri_after <= 1e-9 and r.dua_after <= 1e-9
    np.testing.assert_array_equal(r.x, r.xh)
    np.testing.assert_array_equal(r.y, r.yh)


# -- 3. accepted today, yet not the node's optimum ---------------------------------------------------------------------
def test_an_accepted_incumbent_with_a_wrong_sign_multiplier_loses_that_row(cases):
    _, _, d, l, u, x, y = cases["cfg1_s1_incumbent_auto"]
    r0 = _polish(cases["cfg1_s1_incumbent_auto"])
    assert r0.accepted
    ineq = l != u
    wrong0 = np.sum(ineq & (((r0.active < 0) & (r0.yh > TOL)) | ((r0.active > 0) & (r0.yh < -TOL))))
    assert wrong0 == 1  # a KKT point of the wrong set
    r = _polish(cases["cfg1_s1_incumbent_auto"], repair_iter=5)
    assert (r.accepted0, r.reason0, r.accepted, r.reason, r.stop) == (True, 0, True, 0, 0)
    assert (r.n_added, r.n_dropped, r.rounds) == (0, 1, 1)
    assert r.obj <= r0.obj
    # a direct solve of the UNregularised KKT system on the final set
    rows = np.where(r.active != 0)[0]
    A, P = d.A.toarray(), d.P.toarray()
    Aa, k = A[rows], len(rows)
    b = np.where(r.active[rows] < 0, l[rows], u[rows])
    sol = np.linalg.solve(np.block([[P, Aa.T], [Aa, np.zeros((k, k))]]), np.concatenate([-d.q, b]))
    assert np.max(np.abs(r.x - sol[:d.n])) <= 1e-9 * max(1.0, np.max(np.abs(sol[:d.n])))
    # the node's optimum: inactive rows satisfied, no inequality multiplier of the wrong sign
    z = A.dot(r.x)
    off = r.active == 0
    assert np.all(l[off] - z[off] <= TOL) and np.all(z[off] - u[off] <= TOL)
    assert np.all(r.y[ineq & (r.active < 0)] <= TOL) and np.all(r.y[ineq & (r.active > 0)] >= -TOL)
    assert np.all(r.y[off] == 0.0)


# -- 4. crude inputs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, moves", list(zip(CRUDE_NAMES, inputs.CRUDE_ADDS_DROPS)))
def test_crude_roots_reach_a_fixed_point_in_two_rounds(cases, name, moves):
    r = _polish(cases[name], repair_iter=5)
    print("%s: rounds %d, +%d -%d, pri %.1e dua %.1e, min margin %.1e" % (name, r.rounds, r.n_added, r.n_dropped,
                                                                         r.pri_after, r.dua_after, r.margin.min()))
    assert (r.stop, r.rounds, r.accepted, r.reason) == (0, 2, True, 0)
    assert (r.n_added, r.n_dropped) == moves
    assert r.pri_after <= 1e-9 and r.dua_after <= 1e-9
    # the round limit: one round, a changed set behind it, and the answer is that of round 1's point
    r1 = _polish(cases[name], repair_iter=1)
    assert (r1.stop, r1.rounds) == (1, 1)
    _, _, d, l, u, x, y = cases[name]
    z = d.A.dot(r1.xh)
    pri = max(np.max(l - z), np.max(z - u), 0.0)
    dua = np.max(np.abs(d.P.dot(r1.xh) + d.q + d.A.T.dot(r1.yh)))
    # (sparse products here, dense ones there: the same numbers up to rounding)
    assert abs(r1.pri_after - pri) <= 1e-12 + 1e-6 * pri and abs(r1.dua_after - dua) <= 1e-12 + 1e-6 * dua
    reason = 2 if not r1.pri_after <= max(r1.pri_before, 1e-10) else \
        3 if not r1.dua_after <= max(r1.dua_before, 1e-10) else 0
    assert (r1.reason, r1.accepted) == (reason, reason == 0)
    assert np.sum(r1.active != 0) == r1.n_lower + r1.n_upper
    assert not np.array_equal(r1.active, r.active)


# -- 5, 6. nothing to repair -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cfg2_root_rho0.1", "cfg1_s1_incumbent_auto", "crude_n65m40p12_s0"])
def test_zero_rounds_is_the_plain_polish_bit_for_bit(cases, name):
    a, b = _polish(cases[name]), _polish(cases[name], repair_iter=0)
    _same_bits(a, b)
    np.testing.assert_array_equal(a.margin >= b.margin, True)  # (the revision's comparisons can only lower a margin)
    assert (b.rounds, b.stop, b.accepted0, b.reason0) == (0, 1, a.accepted, a.reason)
    assert b.n_added + b.n_dropped > 0


def test_a_fixed_point_runs_no_round(cases):
    a, b = _polish(cases["crude_n64m20p5_s0"]), _polish(cases["crude_n64m20p5_s0"], repair_iter=5)
    _same_bits(a, b)
    assert (b.rounds, b.stop, b.n_added, b.n_dropped, b.accepted0, b.reason0) == (0, 0, 0, 0, True, 0)
    # ... and so does the repaired point of another input, fed back in
    _, _, d, l, u, x, y = cases["cfg1_s1_root_rho0.1"]
    from miosqp_amd import bnb
    r = _polish(cases["cfg1_s1_root_rho0.1"], repair_iter=5)
    again = bnb.polish_restatement(d.P, d.q, d.A, l, u, r.x, r.y, 1e-6, 3, repair_iter=5)
    assert (again.rounds, again.stop, again.accepted) == (0, 0, True)
    np.testing.assert_array_equal(again.active, r.active)


def test_a_bad_pivot_in_a_repair_round_keeps_the_round_before():
    """P is indefinite along x2; the row x2 >= 0 holds it in round 0 (S is positive definite through the row's 1 / delta),
    its multiplier comes out positive, the revision drops it and round 1 cannot be factorised"""
    from miosqp_amd import bnb
    P, q = np.diag([1.0, -1.0]), np.array([-2.0, -1.0])
    A, l, u = np.array([[0.0, 1.0]]), np.array([0.0]), np.array([5.0])
    x, y = np.array([2.0, 0.0]), np.array([-0.5])
    r0 = bnb.polish_restatement(P, q, A, l, u, x, y)
    assert r0.accepted and abs(r0.yh[0] - 1.0) <= 1e-9
    r = bnb.polish_restatement(P, q, A, l, u, x, y, repair_iter=3)
    assert (r.stop, r.rounds, r.n_added, r.n_dropped) == (2, 1, 0, 1)
    assert (r.accepted0, r.reason0, r.accepted, r.reason) == (True, 0, True, 0)
    np.testing.assert_array_equal(r.active, [-1])
    assert (r.n_lower, r.n_upper) == (1, 0)
    np.testing.assert_array_equal(r.x, r0.x)
    np.testing.assert_array_equal(r.y, r0.y)
    assert r.obj == r0.obj
    # round 0's own bad pivot stays reason 1: nothing is revised
    r = bnb.polish_restatement(-np.eye(2), q, A, l, u, x, y, repair_iter=3)
    assert (r.accepted, r.reason, r.accepted0, r.reason0, r.rounds, r.stop) == (False, 1, False, 1, 0, 0)
    assert r.xh is None


def test_the_revision_rule_by_hand():
    """every row starts inactive (y = 0, x inside): the polished point is the unconstrained minimiser (1, 1), which
    violates row 0's upper and row 1's lower bound; infinite bounds never join"""
    from miosqp_amd import bnb
    P, q = np.eye(2), np.array([-1.0, -1.0])
    A = np.array([[1.0, 0.0], [0.0, -1.0], [1.0, 1.0], [1.0, -1.0], [1.0, 0.0], [1.0, 1.0]])
    l = np.array([-1e30, -0.75, -5.0, -5.0, 0.0, -1e30])
    u = np.array([0.5, np.inf, 1e30, 5.0, 5.0, np.inf])
    x, y = np.array([0.4, 0.1]), np.zeros(6)
    r = bnb.polish_restatement(P, q, A, l, u, x, y, repair_iter=0)
    np.testing.assert_array_equal(r.active, [0, 0, 0, 0, 0, 0])
    assert (r.stop, r.rounds, r.n_added, r.n_dropped, r.accepted0, r.reason0) == (1, 0, 2, 0, False, 2)
    # margins: row 0 round 0's u - z = .1 (the revision's (1 - .5) - tol is larger); row 1 the revision's
    # (-.75 + 1) - tol; rows 2-4 round 0's comparisons 5.5, 4.7, .4; row 5 has no finite bound
    np.testing.assert_allclose(r.margin[:5], [0.1, 0.25 - TOL, 5.5, 4.7, 0.4], rtol=1e-9)
    assert r.margin[5] == np.inf
    r = bnb.polish_restatement(P, q, A, l, u, x, y, repair_iter=5)
    assert (r.stop, r.rounds, r.n_added, r.n_dropped, r.accepted, r.n_lower, r.n_upper) == (0, 1, 2, 0, True, 1, 1)
    np.testing.assert_array_equal(r.active, [1, -1, 0, 0, 0, 0])
    np.testing.assert_allclose(r.x, [0.5, 0.75], rtol=1e-9)
    np.testing.assert_allclose(r.y, [0.5, -0.25, 0, 0, 0, 0], rtol=1e-9)
    # a multiplier of the wrong sign: the same rows started active with q pulling inside leave again
    r = bnb.polish_restatement(P, np.array([-0.2, -0.2]), A, l, u, np.array([0.5, 0.75]), np.array([0.5, -0.25, 0, 0, 0, 0]),
                               repair_iter=5)
    assert (r.stop, r.rounds, r.n_added, r.n_dropped) == (0, 1, 0, 2)
    np.testing.assert_array_equal(r.active, [0, 0, 0, 0, 0, 0])
    np.testing.assert_allclose(r.x, [0.2, 0.2], rtol=1e-9)
    for bad in (-1, 21, 2.5, True):
        with pytest.raises(ValueError):
            bnb.polish_restatement(P, q, A, l, u, x, y, repair_iter=bad)


# -- 7. settings -------------------------------------------------------------------------------------------------------
def test_setting_defaults_and_refusals(oracle_mod):
    from miosqp_amd import bnb
    assert bnb.polish_repair_setting({}) == 0
    assert bnb.polish_repair_setting(dict(polish_repair_iter=20)) == 20
    pr = problems.random_miqp(10, 5, 2, seed=0)
    w = inputs.model(oracle_mod, pr, polish_incumbent=1).work
    assert w.pol_repair_iter == 0
    assert w.polish_repair_stats == dict(calls=0, rounds=0, added=0, dropped=0, fixed_points=0)
    assert inputs.model(oracle_mod, pr, polish_incumbent=1, polish_repair_iter=7).work.pol_repair_iter == 7
    for bad in (-1, 21, 2.5, "two", True, float("nan")):
        with pytest.raises(ValueError, match="polish_repair_iter"):
            bnb.polish_settings(dict(polish_repair_iter=bad))
        with pytest.raises(ValueError, match="polish_repair_iter"):
            inputs.model(oracle_mod, pr, polish_incumbent=1, polish_repair_iter=bad)


# -- 8, 9. whole trees -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n10m5p2_s0", "cfg1_n50m100p10_s0", "n30m150p15_s4", "mpc_n12m30p6_s8",
                                  "infeasible_n10"])
def test_golden_trees_with_the_key_at_zero(oracle_mod, name):
    from miosqp_amd import bnb
    got = []
    calls = []
    real = bnb.polish_restatement

    def spy(*a, **kw):
        calls.append(kw)
        return real(*a, **kw)

    bnb.polish_restatement = spy
    try:
        for extra in (dict(), dict(polish_repair_iter=0)):
            case = load_case(name)
            case["settings"] = dict(case["settings"], polish_incumbent=1, **extra)
            got.append(run_case(case, oracle_mod))
    finally:
        bnb.polish_restatement = real
    assert all("repair_iter" not in kw for kw in calls)  # exactly the call of today
    assert len(got[0]) == len(got[1])
    for a, b in zip(*got):
        np.testing.assert_array_equal(a["trace"], b["trace"])
        assert a["status"] == b["status"] and a["iter_num"] == b["iter_num"]
        assert a["upper_glob"] == b["upper_glob"]
        if a["status"] in (bnb.MI_SOLVED, bnb.MI_MAX_ITER_FEASIBLE):  # (without an incumbent x is never written)
            np.testing.assert_array_equal(a["x"], b["x"])


def test_a_whole_solve_with_repair(oracle_mod):
    from miosqp_amd import bnb
    pr = problems.random_miqp(50, 100, 10, seed=1)
    plain = inputs.model(oracle_mod, pr, qp_extra=dict(rho="auto"), polish_incumbent=1)
    rep = inputs.model(oracle_mod, pr, qp_extra=dict(rho="auto"), polish_incumbent=1, polish_repair_iter=5)
    a, b = plain.solve(), rep.solve()
    assert a.status == b.status == bnb.MI_SOLVED
    st = rep.work.polish_repair_stats
    print("upper_glob %.12f -> %.12f, repair %r" % (a.upper_glob, b.upper_glob, st))
    assert st == dict(calls=1, rounds=1, added=0, dropped=1, fixed_points=1)
    assert plain.work.polish_repair_stats["calls"] == 0
    assert b.upper_glob <= a.upper_glob
    assert sorted(rep.work.polish_stats) == sorted(plain.work.polish_stats)
    assert rep.work.polish_stats["accepted"] == 1
    np.testing.assert_array_equal(a.x[pr["i_idx"]], b.x[pr["i_idx"]])
