"""B polishes in one launch (miosqp_qp_polish_many, k_pol_many in csrc/polish_many.hip) against the dense numpy
restatement (bnb.polish_restatement with repair_iter) per instance, and against the single entry on the same engine.

As in test_gpu_polish_repair.py both sides get the SAME (l, u, x, y), made by the CPU backend, so the sets can only differ
on a row whose comparison sits on a tie; every case first asserts that the restatement's margin is at least
1e-9 max(1, |bound|) on every row.  Tolerances are that file's: integer fields and `active` equal, x, y, obj within 1e-9
relative, its `_close` for the residuals.

Shapes: n = 10 .. 128 with n on both sides of a wavefront (63, 64, 65) and at the top of what one workgroup holds
(127, 128 with 40 rows); config 1 (n 50, M 110) is the widest A."""
import numpy as np
import pytest

from miosqp_amd import problems

import polish_many_inputs as inputs
import polish_repair_inputs as single

pytestmark = pytest.mark.gpu

B = 6
CRUDE = [((10, 5, 2), 0), ((20, 10, 5), 0), ((50, 100, 10), 1), ((63, 20, 5), 2), ((64, 20, 5), 1), ((65, 20, 5), 2),
         ((127, 30, 10), 0), ((128, 30, 10), 0)]
GUESS = [((10, 5, 2), 0), ((20, 10, 5), 0), ((50, 100, 10), 0), ((50, 100, 10), 1), ((64, 20, 5), 1)]
COUNTS = ("rounds", "stop", "n_added", "n_dropped", "accepted0", "reason0", "accepted", "reason", "n_lower", "n_upper")
BITS = COUNTS + ("pri_before", "dua_before", "pri_after", "dua_after", "obj")


def _id(case):
    return "n%dm%dp%d_s%d" % (case[0] + (case[1],))


@pytest.fixture(scope="module")
def made(oracle_mod):
    """(kind, shape, seed) -> (Data, Q, L, U, X, Y) by the CPU backend, made once"""
    cache = {}

    def get(kind, shape, seed):
        key = (kind, shape, seed)
        if key not in cache:
            make = inputs.crude_inputs if kind == "crude" else inputs.guess_inputs
            cache[key] = make(oracle_mod, shape, seed, B)
        return cache[key]
    return get


@pytest.fixture(scope="module")
def refs():
    """the restatement's answers, computed once per (case, repair_iter)"""
    from miosqp_amd import bnb
    cache = {}

    def get(key, case, repair_iter):
        if (key, repair_iter) not in cache:
            d, Q, L, U, X, Y = case
            cache[(key, repair_iter)] = [bnb.polish_restatement(d.P, Q[b], d.A, L[b], U[b], X[b], Y[b], 1e-6, 3,
                                                                repair_iter=repair_iter) for b in range(len(Q))]
        return cache[(key, repair_iter)]
    return get


@pytest.fixture(scope="module")
def engines():
    """one HIP engine per problem, shared by the tests (a polish_many call leaves nothing behind)"""
    from miosqp_amd import qp
    cache = {}

    def get(shape, seed):
        if (shape, seed) not in cache:
            cache[(shape, seed)] = single.model(qp, problems.random_miqp(*shape, seed=seed)).work.solver
        return cache[(shape, seed)]
    return get


def _close(a, b):
    return abs(a - b) <= 1e-12 or abs(a - b) <= 1e-6 * abs(b)


def _no_tie(ro, l, u, what):
    # no row on a tie, in any round: an input on one is not a valid test input
    bound = np.where(ro.active < 0, l, u)
    bound = np.where(np.isfinite(bound), bound, 0.0)
    assert np.all(ro.margin >= 1e-9 * np.maximum(1.0, np.abs(bound))), (what, ro.margin.min())


def _against_restatement(rg, ro, l, u, x, y, what):
    _no_tie(ro, l, u, what)
    print("%s: rounds %d stop %d, +%d -%d, accepted %d (round 0: %d reason %d), active %d + %d, pri %.2e -> %.2e, "
          "dua %.2e -> %.2e, min margin %.2e" % (what, rg.rounds, rg.stop, rg.n_added, rg.n_dropped, rg.accepted,
                                                 rg.accepted0, rg.reason0, rg.n_lower, rg.n_upper, rg.pri_before,
                                                 rg.pri_after, rg.dua_before, rg.dua_after, ro.margin.min()))
    for f in COUNTS:
        assert getattr(rg, f) == getattr(ro, f), (what, f, getattr(rg, f), getattr(ro, f))
    np.testing.assert_array_equal(rg.active, ro.active)
    assert ro.reason != 1
    if ro.accepted:
        assert np.max(np.abs(rg.x - ro.x)) <= 1e-9 * max(1.0, np.max(np.abs(ro.x))), what
        assert np.max(np.abs(rg.y - ro.y)) <= 1e-9 * max(1.0, np.max(np.abs(ro.y))), what
        np.testing.assert_array_equal(rg.y != 0.0, ro.active != 0)
    else:
        np.testing.assert_array_equal(rg.x, x)
        np.testing.assert_array_equal(rg.y, y)
    assert _close(rg.pri_before, ro.pri_before) and _close(rg.dua_before, ro.dua_before), what
    assert _close(rg.pri_after, ro.pri_after) and _close(rg.dua_after, ro.dua_after), \
        (what, rg.pri_after, ro.pri_after, rg.dua_after, ro.dua_after)
    assert abs(rg.obj - ro.obj) <= 1e-9 * abs(ro.obj), (what, rg.obj, ro.obj)


def _same_bits(a, b):
    np.testing.assert_array_equal(a.x, b.x)
    np.testing.assert_array_equal(a.y, b.y)
    np.testing.assert_array_equal(a.active, b.active)
    for f in BITS:
        assert getattr(a, f) == getattr(b, f) or (np.isnan(getattr(a, f)) and np.isnan(getattr(b, f))), f


@pytest.mark.parametrize("case", CRUDE, ids=_id)
def test_crude_inputs_against_the_restatement(made, refs, engines, case):
    shape, seed = case
    d, Q, L, U, X, Y = data = made("crude", shape, seed)
    ref = refs(("crude",) + case, data, 5)
    got = engines(shape, seed).polish_many(Q, L, U, X, Y, 1e-6, 3, 5)
    assert len(got) == B
    for b in range(B):
        assert ref[b].accepted
        _against_restatement(got[b], ref[b], L[b], U[b], X[b], Y[b], "%s[%d]" % (_id(case), b))
    assert all(r.device_time > 0 and r.device_time == got[0].device_time for r in got)


@pytest.mark.parametrize("case", GUESS, ids=_id)
def test_primal_guess_inputs_against_the_restatement(made, refs, engines, case):
    shape, seed = case
    d, Q, L, U, X, Y = data = made("guess", shape, seed)
    ref = refs(("guess",) + case, data, 20)
    got = engines(shape, seed).polish_many(Q, L, U, X, Y, 1e-6, 3, 20)
    for b in range(B):
        assert ref[b].accepted and ref[b].stop == 0 and ref[b].rounds <= 1
        _against_restatement(got[b], ref[b], L[b], U[b], X[b], Y[b], "%s[%d]" % (_id(case), b))


@pytest.mark.parametrize("kind,case,repair_iter", [("crude", ((50, 100, 10), 1), 5), ("crude", ((65, 20, 5), 2), 5),
                                                   ("guess", ((50, 100, 10), 0), 20)])
def test_against_the_single_entry_on_the_same_engine(made, refs, engines, kind, case, repair_iter):
    shape, seed = case
    d, Q, L, U, X, Y = data = made(kind, shape, seed)
    for b, ro in enumerate(refs((kind,) + case, data, repair_iter)):
        _no_tie(ro, L[b], U[b], (kind, case, b))
    eng = engines(shape, seed)
    q0 = np.array(problems.random_miqp(*shape, seed=seed)["q"], dtype=float)
    got = eng.polish_many(Q, L, U, X, Y, 1e-6, 3, repair_iter)
    try:
        for b in range(B):
            eng.update(q=Q[b])
            one = eng.polish(L[b], U[b], X[b], Y[b], 1e-6, 3, repair_iter=repair_iter)
            for f in COUNTS:
                assert getattr(got[b], f) == getattr(one, f), (b, f)
            np.testing.assert_array_equal(got[b].active, one.active)
            assert np.max(np.abs(got[b].x - one.x)) <= 1e-9 * max(1.0, np.max(np.abs(one.x)))
            assert np.max(np.abs(got[b].y - one.y)) <= 1e-9 * max(1.0, np.max(np.abs(one.y)))
            assert abs(got[b].obj - one.obj) <= 1e-9 * abs(one.obj)
    finally:
        eng.update(q=q0)
    # q None: the engine's own linear cost, which is instance 0's
    own = eng.polish_many(None, L[:1], U[:1], X[:1], Y[:1], 1e-6, 3, repair_iter)
    _same_bits(own[0], got[0])


def test_bits(made, engines):
    shape, seed = (50, 100, 10), 1
    d, Q, L, U, X, Y = made("crude", shape, seed)
    eng = engines(shape, seed)
    x0, y0 = np.zeros(d.n), np.zeros(d.m + d.n_int)
    a = eng.solve_node(d.l, d.u, x0, y0)
    p0 = eng.polish(L[0], U[0], X[0], Y[0], 1e-6, 3, repair_iter=5)
    idx = np.arange(70) % B
    big = eng.polish_many(Q[idx], L[idx], U[idx], X[idx], Y[idx], 1e-6, 3, 5)
    again = eng.polish_many(Q[idx], L[idx], U[idx], X[idx], Y[idx], 1e-6, 3, 5)
    assert len(big) == 70
    for r, s in zip(big, again):
        _same_bits(r, s)
    for b in (0, 1, 37, 64, 69):
        k = idx[b]
        one = eng.polish_many(Q[k:k + 1], L[k:k + 1], U[k:k + 1], X[k:k + 1], Y[k:k + 1], 1e-6, 3, 5)
        _same_bits(big[b], one[0])
    assert max(r.rounds for r in big) > 0
    # the node solver and the single polish answer the same bits before and after
    c = eng.solve_node(d.l, d.u, x0, y0)
    np.testing.assert_array_equal(a.x, c.x)
    np.testing.assert_array_equal(a.y, c.y)
    assert (a.status_val, a.iter, a.lower) == (c.status_val, c.iter, c.lower)
    for f in ("pri_res", "dua_res", "obj_val", "int_inf", "nextvar", "heur_viol", "heur_obj"):
        assert getattr(a.info, f) == getattr(c.info, f), f
    p1 = eng.polish(L[0], U[0], X[0], Y[0], 1e-6, 3, repair_iter=5)
    np.testing.assert_array_equal(p0.x, p1.x)
    np.testing.assert_array_equal(p0.y, p1.y)
    for f in COUNTS + ("pri_after", "dua_after", "obj"):
        assert getattr(p0, f) == getattr(p1, f), f
    # repair_iter 0: the plain polish plus one revision
    for r in eng.polish_many(Q, L, U, X, Y, 1e-6, 3, 0):
        assert (r.rounds, r.accepted0, r.reason0) == (0, r.accepted, r.reason)
        assert r.stop in (0, 1) and (r.n_lower, r.n_upper) == (int(np.sum(r.active < 0)), int(np.sum(r.active > 0)))


def test_a_rejected_instance_returns_its_input_and_leaves_its_neighbours_alone(made, engines):
    """one instance gets a y that classifies wrongly (zeros: no inequality row is active): without repair rounds its
    polished point violates the rows it left out and is rejected (reason 2)"""
    from miosqp_amd import bnb
    shape, seed, bad = (50, 100, 10), 0, 2
    d, Q, L, U, X, Y = made("guess", shape, seed)
    Y2 = Y.copy()
    Y2[bad] = 0.0
    ref = [bnb.polish_restatement(d.P, Q[b], d.A, L[b], U[b], X[b], Y2[b], 1e-6, 3, repair_iter=0) for b in range(B)]
    assert [r.accepted for r in ref] == [b != bad for b in range(B)]  # (a condition on the inputs)
    eng = engines(shape, seed)
    got = eng.polish_many(Q, L, U, X, Y2, 1e-6, 3, 0)
    clean = eng.polish_many(Q, L, U, X, Y, 1e-6, 3, 0)
    for b in range(B):
        _against_restatement(got[b], ref[b], L[b], U[b], X[b], Y2[b], "repair_iter 0 [%d]" % b)
        if b == bad:
            assert not got[b].accepted and got[b].reason == 2 and got[b].stop == 1
            np.testing.assert_array_equal(got[b].x, X[b])
            np.testing.assert_array_equal(got[b].y, Y2[b])
        else:
            _same_bits(got[b], clean[b])


def test_argument_checks_leave_the_engine_answering(made, engines):
    shape, seed = (20, 10, 5), 0
    d, Q, L, U, X, Y = made("crude", shape, seed)
    eng = engines(shape, seed)
    want = eng.polish_many(Q, L, U, X, Y, 1e-6, 3, 5)

    def still_answers():
        for r, s in zip(eng.polish_many(Q, L, U, X, Y, 1e-6, 3, 5), want):
            _same_bits(r, s)

    bad_calls = [lambda: eng.polish_many(Q[:0], L[:0], U[:0], X[:0], Y[:0]),
                 lambda: eng.polish_many(Q, L, U, X, Y, delta=0.0),
                 lambda: eng.polish_many(Q, L, U, X, Y, delta=-1.0),
                 lambda: eng.polish_many(Q, L, U, X, Y, refine_iter=-1),
                 lambda: eng.polish_many(Q, L, U, X, Y, refine_iter=11),
                 lambda: eng.polish_many(Q, L, U, X, Y, repair_iter=-1),
                 lambda: eng.polish_many(Q, L, U, X, Y, repair_iter=21)]
    for which in range(5):
        arrs = [Q.copy(), L.copy(), U.copy(), X.copy(), Y.copy()]
        arrs[which][B - 1, 3] = np.nan
        bad_calls.append(lambda arrs=arrs: eng.polish_many(*arrs))
    for call in bad_calls:
        with pytest.raises(RuntimeError):
            call()
        still_answers()
    lo = L.copy()
    lo[B - 2, 0] = U[B - 2, 0] + 1.0
    with pytest.raises(ValueError):
        eng.polish_many(Q, lo, U, X, Y)
    still_answers()


def test_a_problem_beyond_one_workgroup_falls_back(oracle_mod):
    from miosqp_amd import bnb, qp
    shape, seed = (200, 20, 3), 0  # n + M = 223, n beyond the three entries per lane of the substitutions
    pr = problems.random_miqp(*shape, seed=seed)
    m = single.model(qp, pr)
    d = m.work.data
    res = m.solve()
    assert res.status == bnb.MI_SOLVED
    M = d.m + d.n_int
    assert m.work.solver.polish_many(None, d.l[None], d.u[None], np.zeros((1, d.n)), np.zeros((1, M))) is None
    result = dict(x=np.array(res.x, dtype=float), upper_glob=res.upper_glob, status=res.status)
    got = m.polish_many([dict()], [dict(result)], repair_iter=20)[0]
    x = result["x"].copy()
    xi = np.round(x[d.i_idx])
    x[d.i_idx] = xi
    l, u = d.l.copy(), d.u.copy()
    l[d.m:] = xi
    u[d.m:] = xi
    y = bnb.primal_guess_multipliers(l, u, d.A.dot(x), 10 * problems.QP_SETTINGS["eps_abs"])
    r = bnb.polish_restatement(d.P, d.q, d.A, l, u, x, y, 1e-6, 3, repair_iter=20)
    assert got["polished"] == bool(r.accepted and r.stop == 0)
    assert (got["polish_rounds"], got["pri_after"], got["dua_after"]) == (r.rounds, r.pri_after, r.dua_after)
    if got["polished"]:
        want = r.x.copy()
        want[d.i_idx] = xi
        np.testing.assert_array_equal(got["x"], want)


def test_solve_many_with_polish_end_to_end(oracle_mod):
    from miosqp_amd import bnb, qp
    shape, seed, nb = (50, 100, 10), 0, 8
    pr = problems.random_miqp(*shape, seed=seed)
    inst = inputs.instances(pr, nb)
    calls = []
    real = qp.OSQP.polish_many

    def spy(self, *args, **kw):
        recs = real(self, *args, **kw)
        calls.append(recs)
        return recs

    qp.OSQP.polish_many = spy
    try:
        gm = single.model(qp, pr)
        gpu = gm.solve_many(inst, polish=True)
    finally:
        qp.OSQP.polish_many = real
    cpu = single.model(oracle_mod, pr).solve_many(inst, polish=True)
    assert len(calls) == 1 and calls[0] is not None and len(calls[0]) == nb  # the device entry ran, once
    d = gm.work.data
    for b in range(nb):
        g, c, rec = gpu[b], cpu[b], calls[0][b]
        assert rec.device_time > 0
        assert g["status"] == c["status"] == bnb.MI_SOLVED
        assert g["polished"] is True and c["polished"] is True
        assert abs(g["upper_glob"] - c["upper_glob"]) <= 1e-9 * max(1.0, abs(c["upper_glob"]))
        x = g["x"]
        np.testing.assert_array_equal(x[d.i_idx], np.round(x[d.i_idx]))
        l, u = d.l.copy(), d.u.copy()
        l[d.m:] = x[d.i_idx]
        u[d.m:] = x[d.i_idx]
        pri, dua = inputs.residuals(d, inst[b]["q"], l, u, x, rec.y)
        print("instance %d: rounds %d, pri %.2e, dua %.2e" % (b, g["polish_rounds"], pri, dua))
        assert pri <= 1e-9 and dua <= 1e-9, (b, pri, dua)
        assert g["upper_glob"] == .5 * x.dot(d.P.dot(x)) + inst[b]["q"].dot(x)
