"""The inputs of test_gpu_polish_many_large.py (polish_many_large_inputs.CASES, the indefinite problems) checked on the CPU
against the long-double restatement, so that a failure on the GPU can only mean k_pol_many_g -- the two checks of
test_polish_reference_cpu.py without its n <= 192 --, what the table reaches, and MIOSQP's new keyword values on the
CPU backend, which has no batched entry: there `large=True` and `polish="device"` are the restatement."""
import numpy as np
import pytest

from miosqp_amd import bnb, problems

import polish_many_inputs as inputs
import polish_many_large_inputs as large
import polish_reference as ref
import polish_repair_inputs as single


def _ids(cases):
    return [c.name for c in cases]


@pytest.mark.parametrize("case", large.CASES, ids=_ids(large.CASES))
def test_float64_reference_is_the_restatement(oracle_mod, case):
    data = d, Q, L, U, X, Y = large.case_inputs(oracle_mod, case)
    for b, (rl, r6) in enumerate(large.case_references(case, data)):
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


@pytest.mark.parametrize("case", large.CASES, ids=_ids(large.CASES))
def test_input_conditions(oracle_mod, case):
    data = d, Q, L, U, X, Y = large.case_inputs(oracle_mod, case)
    refs = large.case_references(case, data)
    assert len(refs) == case.B
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
        if not ex["accepted"]:  # a rejected instance returns its input
            np.testing.assert_array_equal(rl.x, X[b].astype(np.longdouble))
            np.testing.assert_array_equal(rl.y, Y[b].astype(np.longdouble))
    if ex.get("moves"):
        assert sum(r.n_added for r, _ in refs) > 0 and sum(r.n_dropped for r, _ in refs) > 0, case.name


def test_the_inputs_reach_what_they_are_there_for(oracle_mod):
    """M > 256 with active rows at index >= 256, n on both sides of 256, the first n k_pol_many refuses, the edges of the
    kernel's 32-wide panel (k 32 - 1, k 32, k 32 + 1), one batch whose instances run different numbers of rounds"""
    sizes = {}
    for case in large.CASES:
        d = large.case_inputs(oracle_mod, case)[0]
        sizes[case.name] = (d.n, d.m + d.n_int)
    assert {193, 255, 256, 257} <= {n for n, _ in sizes.values()}
    assert all(n > 192 or M > 256 for name, (n, M) in sizes.items() if name != "r50_s1")
    assert sizes["r50_s1"] == (50, 110)
    for name in ("r224x300_s0_limit", "r224x300_s0", "r200x300_s1"):
        case = large.CASE[name]
        data = large.case_inputs(oracle_mod, case)
        assert sizes[name][1] > 256
        assert all(np.any(rl.active[256:] != 0) for rl, _ in large.case_references(case, data)), name
    case = large.CASE["r224x300_s0"]
    rounds = [rl.rounds for rl, _ in large.case_references(case, large.case_inputs(oracle_mod, case))]
    assert len(set(rounds)) == 2, rounds


@pytest.mark.parametrize("n,k", large.INDEFINITE)
def test_the_indefinite_problems_reach_both_bad_pivot_exits(n, k):
    """instances 0 and 3 accepted at 0 rounds, 1 stops at 2 after one round (-1 row, judged on round 0's point), 2 is
    reason 1; the failing pivot is pivot k: in the last panel of 32 for (200, 196), in a middle one for (257, 130)"""
    import setup_reference as sr
    pr = inputs.indefinite_problem(n=n, k=k)
    A, _, _ = problems.extended(pr)
    P, A = np.asarray(pr["P"].todense()), np.asarray(A.todense())
    assert P.shape == (n, n) and A.shape == (2, n) and k // 32 == {196: (n - 1) // 32, 130: 4}[k]
    assert 0 < k // 32 and (k == 196 or k // 32 < (n - 1) // 32)
    assert np.linalg.eigvalsh(P + 1e-6 * np.eye(n) + 2.0 * A.T.dot(A)).min() >= 1.0
    Q, L, U, X, Y = inputs.indefinite_batch(pr)
    for T in (np.longdouble, np.float64):
        r = [ref.polish(P, Q[b], A, L[b], U[b], X[b], Y[b], 1e-6, 3, 5, T) for b in range(4)]
        for b in (0, 3):
            assert (r[b].accepted, r[b].reason, r[b].rounds, r[b].stop, r[b].n_lower, r[b].n_upper) == (True, 0, 0, 0, 2, 0)
        s2 = r[1]
        assert (s2.stop, s2.rounds, s2.n_added, s2.n_dropped, s2.accepted, s2.reason) == (2, 1, 0, 1, True, 0)
        assert (s2.accepted0, s2.reason0) == (True, 0)
        np.testing.assert_array_equal(s2.active, [-1, -1])
        r1 = r[2]
        assert (r1.accepted, r1.reason, r1.accepted0, r1.reason0, r1.rounds, r1.stop) == (False, 1, False, 1, 0, 0)
        assert np.isnan(float(r1.pri_after)) and np.isnan(float(r1.dua_after)) and np.isnan(float(r1.obj))
        np.testing.assert_array_equal(r1.x, X[2].astype(T))
        S = P.astype(T) + T(1e-6) * np.eye(n, dtype=T) + (A[1:].T @ A[1:]).astype(T) / T(1e-6)
        assert sr.ldl(S)[2] == k and S[k, k] < -0.5
        for b in range(4):
            assert r[b].margin.min() >= 0.1, (b, r[b].margin)


# ---- MIOSQP on a backend without the batched entries ---------------------------------------------------------------------
def test_device_polish_on_the_cpu_backend_is_the_restatement(oracle_mod):
    pr = problems.random_miqp(100, 200, 50, seed=0)
    m = single.model(oracle_mod, pr)
    assert not hasattr(m.work.solver, "polish_many_large")
    inst = inputs.instances(pr, 4)
    d = m.work.data
    q0, l0, u0 = d.q.copy(), d.l.copy(), d.u.copy()
    host = m.solve_many(inst, polish=True)
    dev = m.solve_many(inst, polish="device")
    for a, b in zip(host, dev):
        assert sorted(a) == sorted(b)
        for key in a:
            if key == "run_time":
                continue
            np.testing.assert_array_equal(np.asarray(a[key]), np.asarray(b[key]), err_msg=key)
    for bad in ("gpu", "host", 1, 2, None):
        with pytest.raises(ValueError):
            m.solve_many(inst, polish=bad)
    plain = m.solve_many(inst)
    m.polish_many(inst, plain, large=True)
    for a, b in zip(host, plain):
        np.testing.assert_array_equal(a["x"], b["x"])
        assert a["polished"] == b["polished"] and a["polish_rounds"] == b["polish_rounds"]
    assert np.array_equal(d.q, q0) and np.array_equal(d.l, l0) and np.array_equal(d.u, u0)


def test_the_symbols_are_declared():
    from miosqp_amd import _lib
    assert "miosqp_qp_polish_many_large" in _lib.SYMBOLS and "miosqp_qp_get_polish_many_large_classes" in _lib.SYMBOLS
