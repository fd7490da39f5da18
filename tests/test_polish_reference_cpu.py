"""The long-double restatement of the polish (tests/polish_reference.py) and the edge inputs of k_pol_many
(polish_many_inputs.EDGES, the bad-pivot problems), checked on the CPU so that a failure of
test_gpu_polish_many_edges.py can only mean the kernel.

1. the reference at T = np.float64 against bnb.polish_restatement on every edge input: integer fields and `active`
   equal, x and y within the floor (polish_reference.bound: the two differ in LAPACK's blocked Cholesky and BLAS sums
   against the textbook loops, as the kernel does);
2. the input conditions, from the long-double reference alone: accepted or rejected, rounds, stops and reasons as the
   table states them, the long-double and float64 runs agree on every integer field, and no row sits on a tie -- its
   margin is at least max(1e-9 max(1, |bound|), 100 x (the row's 1-norm of A) x e_floor) with
   e_floor = max |x_float64 - x_longdouble| of that instance and setting.  An input that fails is not a valid input."""
import numpy as np
import pytest

import polish_many_inputs as inputs
import polish_reference as ref


def _ids(cases):
    return [c.name for c in cases]


def test_substitutions_and_the_factorisation_solve_a_system():
    import setup_reference as sr
    rng = np.random.RandomState(0)
    G = rng.standard_normal((37, 37))
    S = (G @ G.T + 37 * np.eye(37)).astype(np.longdouble)
    r = rng.standard_normal(37).astype(np.longdouble)
    L, d, bad = sr.ldl(S)
    assert bad is None
    v = ref.backward(L, ref.forward(L, r) / d)
    assert float(np.max(np.abs(S @ v - r))) <= 37 * 64 * np.finfo(np.longdouble).eps * float(np.max(np.abs(r)))
    assert v.dtype == np.longdouble


@pytest.mark.parametrize("case", inputs.EDGES, ids=_ids(inputs.EDGES))
def test_float64_reference_is_the_restatement(oracle_mod, case):
    from miosqp_amd import bnb
    data = d, Q, L, U, X, Y = inputs.edge_inputs(oracle_mod, case)
    for b, (rl, r6) in enumerate(inputs.edge_references(case, data)):
        ro = bnb.polish_restatement(d.P, Q[b], d.A, L[b], U[b], X[b], Y[b], case.delta, case.refine_iter,
                                    repair_iter=case.repair_iter)
        for f in ref.COUNTS:
            assert getattr(r6, f) == getattr(ro, f), (case.name, b, f, getattr(r6, f), getattr(ro, f))
        np.testing.assert_array_equal(r6.active, ro.active)
        assert r6.x.dtype == np.float64 and rl.x.dtype == np.longdouble
        for f in ("xh", "yh", "x", "y"):
            e, floor = ref.err(getattr(ro, f), getattr(rl, f)), ref.err(getattr(r6, f), getattr(rl, f))
            assert e <= ref.bound(floor, getattr(rl, f)), (case.name, b, f, e, floor)
        assert ro.pri_before == r6.pri_before or abs(ro.pri_before - r6.pri_before) <= 1e-12 * abs(r6.pri_before)
        assert abs(ro.dua_before - r6.dua_before) <= 1e-12 * max(1.0, abs(r6.dua_before))


@pytest.mark.parametrize("case", inputs.EDGES, ids=_ids(inputs.EDGES))
def test_input_conditions(oracle_mod, case):
    data = d, Q, L, U, X, Y = inputs.edge_inputs(oracle_mod, case)
    refs = inputs.edge_references(case, data)
    assert len(refs) == (len(case.pick) if case.pick is not None else case.B) and d.n <= 192
    ex = case.expect
    for b, (rl, r6) in enumerate(refs):
        what = (case.name, b)
        for f in ref.COUNTS:
            assert getattr(rl, f) == getattr(r6, f), what + (f,)
        np.testing.assert_array_equal(rl.active, r6.active)
        ok, row, margin, need = ref.tie_free(rl, r6, d.A, L[b], U[b])
        print("%s[%d]: accepted %d reason %d (round 0: %d), rounds %d stop %d, +%d -%d, active %d + %d, e_floor %.1e, "
              "tightest row %d: margin %.1e, needs %.1e" % (case.name, b, rl.accepted, rl.reason, rl.reason0, rl.rounds,
                                                            rl.stop, rl.n_added, rl.n_dropped, rl.n_lower, rl.n_upper,
                                                            ref.x_floor(r6, rl), row, margin, need))
        assert ok, what + (row, margin, need)
        assert rl.reason != 1 and rl.stop != 2, what
        assert bool(rl.accepted) == ex["accepted"], what
        if ex["accepted"]:
            assert rl.reason == 0 and rl.stop == 0, what
        for f in ("reason0", "reason", "stop"):
            if f in ex:
                assert getattr(rl, f) == ex[f], what + (f,)
        if "rounds" in ex:
            assert ex["rounds"][0] <= rl.rounds <= ex["rounds"][1], what + (rl.rounds,)
        if "added" in ex:
            assert ex["added"][0] <= rl.n_added <= ex["added"][1], what + (rl.n_added,)
        if case.kind == "empty":  # nothing is active going into round 0: y = 0 and every row strictly inside
            z = d.A.dot(X[b])
            assert np.all(Y[b] == 0.0) and np.all(z > L[b]) and np.all(z < U[b]), what
            r0 = ref.polish(d.P, Q[b], d.A, L[b], U[b], X[b], Y[b], case.delta, case.refine_iter, 0, np.longdouble)
            assert (r0.n_lower, r0.n_upper) == (0, 0) and not np.any(r0.active), what
            if case.repair_iter == 0:
                np.testing.assert_array_equal(rl.x, X[b].astype(np.longdouble))
                np.testing.assert_array_equal(rl.y, Y[b].astype(np.longdouble))
    if ex.get("moves"):
        assert sum(r.n_added for r, _ in refs) > 0 and sum(r.n_dropped for r, _ in refs) > 0, case.name


def test_the_inputs_reach_what_they_are_there_for(oracle_mod):
    """the third register segment needs n >= 129, the third ballot chunk M > 128 with active rows at and beyond row 128,
    the refinement settings their two values"""
    for case in inputs.EDGES:
        d = inputs.edge_inputs(oracle_mod, case)[0]
        if case.group == "segment3":
            assert 129 <= d.n <= 192
        if case.group == "chunk3":
            data = inputs.edge_inputs(oracle_mod, case)
            assert d.m + d.n_int > 128
            assert any(np.any(rl.active[128:] != 0) for rl, _ in inputs.edge_references(case, data)), case.name
    sizes = {inputs.edge_inputs(oracle_mod, inputs.EDGE[n])[0].n: inputs.edge_inputs(oracle_mod, inputs.EDGE[n])[0].m +
             inputs.edge_inputs(oracle_mod, inputs.EDGE[n])[0].n_int for n in ("r191_s0", "r192_s0")}
    assert sizes == {191: 1, 192: 3}
    seen = {(c.delta, c.refine_iter) for c in inputs.EDGES if c.group == "settings"}
    assert seen == {(1e-6, 0), (1e-6, 10), (1e-4, 3), (1e-8, 3)}


def test_structured_inputs_contain_their_structure():
    counts = inputs.structure_counts()
    print(counts)
    assert counts["one_sided"]["l_inf"] == 12 and counts["one_sided"]["u_inf"] == 14 and counts["one_sided"]["free"] >= 1
    assert counts["equality"]["eq_general"] == 8
    assert counts["sparse5"]["empty_rows"] >= 1 and counts["sparse5"]["empty_cols"] >= 1
    assert counts["low_rank"]["rank_P"] == 15 and counts["low_rank"]["n"] == 60
    assert counts["milp"]["nnz_P"] == 0
    for name in ("one_sided", "equality", "sparse5", "low_rank"):
        assert (counts[name]["n"], counts[name]["M"]) == (60, 90)
    assert (counts["milp"]["n"], counts["milp"]["M"]) == (40, 90)


# ---- the bad pivots ----------------------------------------------------------------------------------------------------
def _records(P, A, Q, L, U, X, Y, repair_iter, T):
    return [ref.polish(P, Q[b], A, L[b], U[b], X[b], Y[b], 1e-6, 3, repair_iter, T) for b in range(len(Q))]


def test_the_indefinite_problem_reaches_both_bad_pivot_exits():
    from miosqp_amd import bnb, problems
    pr = inputs.indefinite_problem()
    A, _, _ = problems.extended(pr)
    P, A, k = np.asarray(pr["P"].todense()), np.asarray(A.todense()), pr["k"]
    assert P.shape == (70, 70) and k == 66 and A.shape == (2, 70) and A[0, k] == 1.0 and A[1, 0] == 1.0
    # what set-up factorises (rho 2, sigma 1e-6, no scaling) is positive definite, P is not
    assert np.linalg.eigvalsh(P + 1e-6 * np.eye(70) + 2.0 * A.T.dot(A)).min() >= 1.0
    assert np.linalg.eigvalsh(P).min() == pytest.approx(-1.0)
    Q, L, U, X, Y = inputs.indefinite_batch(pr)
    for T in (np.longdouble, np.float64):
        r = _records(P, A, Q, L, U, X, Y, 3, T)
        for b in (0, 3):  # healthy: the row is active with a negative multiplier, a fixed point
            assert (r[b].accepted, r[b].reason, r[b].rounds, r[b].stop, r[b].n_lower, r[b].n_upper) == (True, 0, 0, 0, 2, 0)
            assert r[b].yh[0] < -0.5
        s2 = r[1]
        assert (s2.stop, s2.rounds, s2.n_added, s2.n_dropped, s2.accepted, s2.reason) == (2, 1, 0, 1, True, 0)
        assert (s2.accepted0, s2.reason0, s2.n_lower, s2.n_upper) == (True, 0, 2, 0)
        np.testing.assert_array_equal(s2.active, [-1, -1])
        assert abs(float(s2.yh[0]) - 1.0) <= 1e-9
        r1 = r[2]
        assert (r1.accepted, r1.reason, r1.accepted0, r1.reason0, r1.rounds, r1.stop) == (False, 1, False, 1, 0, 0)
        assert np.isnan(float(r1.pri_after)) and np.isnan(float(r1.dua_after)) and np.isnan(float(r1.obj))
        assert np.isfinite(float(r1.pri_before)) and np.isfinite(float(r1.dua_before))
        np.testing.assert_array_equal(r1.active, [0, -1])
        np.testing.assert_array_equal(r1.x, X[2].astype(T))
        # repair_iter 0 is the round stop 2 goes back to
        z = ref.polish(P, Q[1], A, L[1], U[1], X[1], Y[1], 1e-6, 3, 0, T)
        assert (z.stop, z.rounds, z.accepted) == (1, 0, True)
        np.testing.assert_array_equal(z.x, s2.x)
        np.testing.assert_array_equal(z.y, s2.y)
        assert z.obj == s2.obj
        # the failing pivot is pivot k, late in the factorisation, and decisively negative
        import setup_reference as sr
        S = P.astype(T) + T(1e-6) * np.eye(70, dtype=T) + (A[1:].T @ A[1:]).astype(T) / T(1e-6)
        assert sr.ldl(S)[2] == k and S[k, k] < -0.5
        # no tie: every margin is of order one
        for b in range(4):
            assert r[b].margin.min() >= 0.1, (b, r[b].margin)
    # ... and the float64 restatement says the same
    for b in range(4):
        ro = bnb.polish_restatement(P, Q[b], A, L[b], U[b], X[b], Y[b], 1e-6, 3, repair_iter=3)
        for f in ref.COUNTS:
            assert getattr(ro, f) == getattr(r[b], f), (b, f)
        np.testing.assert_array_equal(ro.active, r[b].active)


def test_the_two_variable_problem_stops_at_2():
    pr = inputs.two_variable_problem()
    P, A = np.asarray(pr["P"].todense()), np.asarray(pr["A"].todense())
    assert np.linalg.eigvalsh(P + 1e-6 * np.eye(2) + 2.0 * A.T.dot(A)).min() >= 1.0
    for T in (np.longdouble, np.float64):
        r = ref.polish(P, pr["q"], A, pr["l"], pr["u"], pr["x"], pr["y"], 1e-6, 3, 3, T)
        assert (r.stop, r.rounds, r.n_added, r.n_dropped, r.accepted, r.reason) == (2, 1, 0, 1, True, 0)
        np.testing.assert_array_equal(r.active, [-1])
        assert r.margin.min() >= 0.1
