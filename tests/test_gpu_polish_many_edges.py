"""k_pol_many (csrc/polish_many.hip) at the edges test_gpu_polish_many.py does not reach, through the public entry
OSQP.polish_many, against the long-double restatement of tests/polish_reference.py:

    the third register segment of the substitutions (n 129 .. 192), the third ballot chunk of the compaction (M > 128),
    the capacity boundary (n 192 with M 3 and 4), refine_iter 0 and 10, delta 1e-4 and 1e-8, infinite bounds, equality
    rows, empty rows, a rank-deficient P and P = 0, an empty first active set and long repair sequences, both bad-pivot
    exits (reason 1 and stop 2), and more workgroups than the chip has compute units.

The inputs and what the reference says about them (accepted, rounds, stops, no row on a tie) are checked on the CPU by
test_polish_reference_cpu.py, so a failure here can only mean the kernel.

For an accepted instance, in this order: integer fields and `active` equal to the long-double reference; x, y, obj,
pri_after, dua_after within the floor tolerance; y != 0 exactly on the active rows.  For a rejected one x and y are the
input bit for bit.  The floor tolerance (polish_reference.bound) has no constant fixed in advance: with
e_dev = max |x_dev - x_ld| and e_floor = max |x_f64 - x_ld|, e_dev <= max(16 e_floor, 64 eps max(1, max |x_ld|)), the same
for y.  The kernel and the float64 restatement are the same algorithm in the same format and differ in the order of
their sums and in fused multiply-adds: one order of magnitude over the floor is the margin for that; a wrong index in a
substitution misses it by many orders.  For the three scalars the floor is |v_f64 - v_ld| at its largest over the case's
instances: one instance's scalar is a single sample of the rounding error (pri_after of the float64 restatement ranges
over 1.8e-15 .. 1.5e-13 between the four instances of one problem), the instances of a case share P, A and the
conditioning of S.  Every case prints e_dev / e_floor before it asserts."""
import numpy as np
import pytest

from miosqp_amd import problems

import polish_many_inputs as inputs
import polish_reference as ref
import polish_repair_inputs as single
from test_gpu_polish_many import BITS, _same_bits

pytestmark = pytest.mark.gpu

SCALARS = ("obj", "pri_after", "dua_after")


@pytest.fixture(scope="module")
def engines():
    """one HIP engine per problem, shared by the tests (a polish_many call leaves nothing behind)"""
    from miosqp_amd import qp
    cache = {}

    def get(prob):
        if prob not in cache:
            cache[prob] = single.model(qp, inputs.PROBLEMS[prob]()).work.solver
        return cache[prob]
    return get


def _ratio(e, floor):
    return e / floor if floor > 0.0 else (0.0 if e == 0.0 else np.inf)


def _against_reference(case_name, group, got, refs, X, Y):
    """every instance of one call against its (long double, float64) records; prints, then asserts"""
    floors = {f: max(abs(float(r6.__dict__[f]) - float(rl.__dict__[f])) for rl, r6 in refs if rl.accepted)
              for f in SCALARS if any(rl.accepted for rl, _ in refs)}
    bad = []
    for b, (rg, (rl, r6)) in enumerate(zip(got, refs)):
        what = "%s[%d]" % (case_name, b)
        for f in ref.COUNTS:
            if getattr(rg, f) != getattr(rl, f):
                bad.append((what, f, getattr(rg, f), getattr(rl, f)))
        if not np.array_equal(rg.active, rl.active):
            bad.append((what, "active", np.where(rg.active != rl.active)[0]))
        line = "%s %s: rounds %d stop %d +%d -%d accepted %d reason %d (round 0: %d) active %d + %d" % (
            group, what, rg.rounds, rg.stop, rg.n_added, rg.n_dropped, rg.accepted, rg.reason, rg.reason0, rg.n_lower,
            rg.n_upper)
        if rl.accepted:
            for f, dev in (("x", rg.x), ("y", rg.y)):
                e, floor = ref.err(dev, getattr(rl, f)), ref.err(getattr(r6, f), getattr(rl, f))
                line += ", %s e_dev %.2e e_floor %.2e ratio %.2f" % (f, e, floor, _ratio(e, floor))
                if not e <= ref.bound(floor, getattr(rl, f)):
                    bad.append((what, f, e, floor))
            for f in SCALARS:
                e = abs(float(getattr(rg, f)) - float(getattr(rl, f)))
                line += ", %s %.3e e_dev %.2e e_floor %.2e" % (f, getattr(rg, f), e, floors[f])
                if not e <= ref.bound(floors[f], getattr(rl, f)):
                    bad.append((what, f, e, floors[f]))
            if not np.array_equal(rg.y != 0.0, rl.active != 0):
                bad.append((what, "y != 0 off the active rows"))
        else:
            line += ", rejected"
            if not (np.array_equal(rg.x, X[b]) and np.array_equal(rg.y, Y[b])):
                bad.append((what, "a rejected instance must return its input"))
        print(line)
    assert not bad, bad


def _run(oracle_mod, engines, name):
    case = inputs.EDGE[name]
    data = d, Q, L, U, X, Y = inputs.edge_inputs(oracle_mod, case)
    refs = inputs.edge_references(case, data)
    got = engines(case.prob).polish_many(Q, L, U, X, Y, case.delta, case.refine_iter, case.repair_iter)
    assert got is not None and len(got) == len(Q)
    _against_reference(name, case.group, got, refs, X, Y)
    return case, data, refs, got


def _names(group):
    return [c.name for c in inputs.EDGES if c.group == group]


@pytest.mark.parametrize("name", _names("segment3"))
def test_third_register_segment(oracle_mod, engines, name):
    """n >= 129: entries lane + 128 of the forward sweep, the pivot division and the backward sweep"""
    case, data, refs, got = _run(oracle_mod, engines, name)
    assert data[0].n >= 129 and all(rl.accepted for rl, _ in refs)


@pytest.mark.parametrize("name", _names("chunk3"))
def test_third_ballot_chunk(oracle_mod, engines, name):
    """M > 128: the compaction of the active rows runs its chunk at row 128, with active rows in it"""
    case, data, refs, got = _run(oracle_mod, engines, name)
    assert data[0].m + data[0].n_int > 128 and any(np.any(r.active[128:] != 0) for r in got)


@pytest.mark.parametrize("name", _names("settings"))
def test_refine_iter_and_delta_off_their_defaults(oracle_mod, engines, name):
    case, data, refs, got = _run(oracle_mod, engines, name)
    assert (case.delta, case.refine_iter) != (1e-6, 3)


@pytest.mark.parametrize("name", _names("structured"))
def test_structured_rows(oracle_mod, engines, name):
    """infinite bounds on one or both sides, general equality rows, empty rows and columns of A, a rank-deficient P; an
    infinite bound given as +-1e30 returns the bits of +-inf"""
    case, (d, Q, L, U, X, Y), refs, got = _run(oracle_mod, engines, name)
    counts = inputs.structure_counts()[case.prob]
    gen_l, gen_u = L[0][:d.m], U[0][:d.m]
    if case.prob == "one_sided":
        assert int(np.sum(gen_l == -np.inf)) == 12 and int(np.sum(gen_u == np.inf)) == 14
        assert int(np.sum((gen_l == -np.inf) & (gen_u == np.inf))) >= 1
        big = engines(case.prob).polish_many(Q, np.maximum(L, -1e30), np.minimum(U, 1e30), X, Y, case.delta,
                                             case.refine_iter, case.repair_iter)
        for r, s in zip(got, big):
            _same_bits(r, s)
    if case.prob == "equality":
        assert int(np.sum(gen_l == gen_u)) == 8
        for r in got:
            assert np.all(r.active[:d.m][gen_l == gen_u] == -1)
    if case.prob == "sparse5":
        assert counts["empty_rows"] >= 1 and counts["empty_cols"] >= 1
        assert int(np.sum(np.diff(d.A.tocsr().indptr)[:d.m] == 0)) == counts["empty_rows"]
    if case.prob == "low_rank":
        assert counts["rank_P"] == 15 and d.n == 60


def test_no_quadratic_term(oracle_mod, engines):
    """P = 0: the rows of P are empty, S is delta I + A_act' A_act / delta"""
    case, (d, Q, L, U, X, Y), refs, got = _run(oracle_mod, engines, "milp_guess")
    assert d.P.nnz == 0 and len(got) == 2


@pytest.mark.parametrize("name", _names("empty"))
def test_empty_first_set(oracle_mod, engines, name):
    """no row is active going into round 0 (na == 0: S = P + delta I); with repair rounds 5 to 9 of them follow, without
    the violated point is rejected and the input comes back"""
    case, (d, Q, L, U, X, Y), refs, got = _run(oracle_mod, engines, name)
    first = engines(case.prob).polish_many(Q, L, U, X, Y, case.delta, case.refine_iter, 0)
    for r, g in zip(first, got):
        assert (r.n_lower, r.n_upper, r.rounds, r.stop, r.reason) == (0, 0, 0, 1, 2) and not np.any(r.active)
        if case.repair_iter == 0:
            _same_bits(r, g)
        else:
            assert g.reason0 == 2 and g.accepted and 5 <= g.rounds <= 9


def test_capacity_boundary(oracle_mod, engines):
    """n = 192 fits with M = 3 and not with M = 4.  The LDS image in doubles (polm_layout): the triangle 192 x 193 / 2 =
    18528, A's rows M x 193, six vectors of n = 1152, five of M, 8 for the reductions, (M + 1) / 2 for the active list
    and (2 M + 7) / 8 for the classes: 18528 + 579 + 1152 + 15 + 8 + 2 + 1 = 20285 for M = 3 and
    18528 + 772 + 1152 + 20 + 8 + 2 + 1 = 20483 for M = 4, against 160 KB = 20480 doubles."""
    from miosqp_amd import qp
    _run(oracle_mod, engines, "r192_s0")  # (192, 2, 1), M = 3: answered
    pr = problems.random_miqp(192, 3, 1, seed=0)
    w = single.model(qp, pr).work
    d, eng = w.data, w.solver
    M = d.m + d.n_int
    assert (d.n, M) == (192, 4)
    x0, y0 = np.zeros(d.n), np.zeros(M)
    a = eng.solve_node(d.l, d.u, x0, y0)
    assert eng.polish_many(None, d.l[None], d.u[None], a.x[None], a.y[None], 1e-6, 3, 5) is None
    c = eng.solve_node(d.l, d.u, x0, y0)
    assert a.status_val == c.status_val and a.iter == c.iter
    np.testing.assert_array_equal(a.x, c.x)
    np.testing.assert_array_equal(a.y, c.y)


# ---- the bad pivots ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def indefinite():
    """(engine, P, A, batch) of polish_many_inputs.indefinite_problem; set-up at rho 2 without scaling factorises
    P + sigma I + 2 A'A, whose smallest eigenvalue is 1"""
    from miosqp_amd import qp
    pr = inputs.indefinite_problem()
    w = single.model(qp, pr, qp_extra=dict(rho=2.0, scaling=0)).work
    return w.solver, np.asarray(w.data.P.todense()), np.asarray(w.data.A.todense()), inputs.indefinite_batch(pr)


def _ind_refs(indefinite, b, repair_iter):
    eng, P, A, (Q, L, U, X, Y) = indefinite
    return ref.both(("indefinite", b), P, Q[b], A, L[b], U[b], X[b], Y[b], 1e-6, 3, repair_iter)


def test_bad_pivot_in_a_repair_round_keeps_the_round_before(indefinite):
    """stop 2: round 0 holds the row x_k >= 0, its multiplier comes out positive, the revision drops it and pivot 66 of
    round 1 is -1 + delta: round 0's point and set are judged and returned"""
    eng, P, A, (Q, L, U, X, Y) = indefinite
    s = slice(1, 2)
    got = eng.polish_many(Q[s], L[s], U[s], X[s], Y[s], 1e-6, 3, 3)
    refs = [_ind_refs(indefinite, 1, 3)]
    assert (refs[0][0].stop, refs[0][0].rounds) == (2, 1)
    _against_reference("indefinite_stop2", "badpivot", got, refs, X[s], Y[s])
    g = got[0]
    assert (g.stop, g.rounds, g.n_added, g.n_dropped, g.accepted, g.reason) == (2, 1, 0, 1, True, 0)
    np.testing.assert_array_equal(g.active, [-1, -1])
    assert (g.n_lower, g.n_upper) == (2, 0)
    zero = eng.polish_many(Q[s], L[s], U[s], X[s], Y[s], 1e-6, 3, 0)[0]
    assert (zero.stop, zero.rounds, zero.accepted) == (1, 0, True)
    np.testing.assert_array_equal(g.x, zero.x)
    np.testing.assert_array_equal(g.y, zero.y)
    assert g.obj == zero.obj and g.pri_after == zero.pri_after and g.dua_after == zero.dua_after


def test_bad_pivot_in_round_0_returns_the_input(indefinite):
    """reason 1: x_k = 1 and y = 0 leave the row inactive, round 0's own factorisation fails"""
    eng, P, A, (Q, L, U, X, Y) = indefinite
    s = slice(2, 3)
    g = eng.polish_many(Q[s], L[s], U[s], X[s], Y[s], 1e-6, 3, 3)[0]
    rl, r6 = _ind_refs(indefinite, 2, 3)
    print("reason 1: accepted %d reason %d reason0 %d rounds %d stop %d pri %r -> %r dua %r -> %r obj %r" % (
        g.accepted, g.reason, g.reason0, g.rounds, g.stop, g.pri_before, g.pri_after, g.dua_before, g.dua_after, g.obj))
    assert rl.reason == 1
    for f in ref.COUNTS:
        assert getattr(g, f) == getattr(rl, f), f
    assert (g.accepted, g.reason, g.accepted0, g.reason0, g.rounds, g.stop) == (False, 1, False, 1, 0, 0)
    assert np.isnan(g.pri_after) and np.isnan(g.dua_after) and np.isnan(g.obj)
    for f in ("pri_before", "dua_before"):
        e, floor = abs(getattr(g, f) - float(getattr(rl, f))), abs(float(getattr(r6, f)) - float(getattr(rl, f)))
        assert np.isfinite(getattr(g, f)) and e <= ref.bound(floor, getattr(rl, f)), (f, e, floor)
    np.testing.assert_array_equal(g.x, X[2])
    np.testing.assert_array_equal(g.y, Y[2])
    np.testing.assert_array_equal(g.active, rl.active)
    np.testing.assert_array_equal(g.active, [0, -1])


def test_bad_pivots_leave_their_neighbours_alone(indefinite):
    """both exits in one batch between two healthy instances (the row active with a negative multiplier: a fixed point
    of round 0); the batch has one repair_iter, 3.  Every instance has the bits of its own call."""
    eng, P, A, (Q, L, U, X, Y) = indefinite
    got = eng.polish_many(Q, L, U, X, Y, 1e-6, 3, 3)
    assert [(r.stop, r.reason, r.rounds) for r in got] == [(0, 0, 0), (2, 0, 1), (0, 1, 0), (0, 0, 0)]
    h = [0, 3]
    healthy = eng.polish_many(Q[h], L[h], U[h], X[h], Y[h], 1e-6, 3, 3)
    refs = [_ind_refs(indefinite, b, 3) for b in h]
    _against_reference("indefinite_healthy", "badpivot", healthy, refs, X[h], Y[h])
    for b, r in zip(h, healthy):
        assert r.accepted and r.rounds == 0
        _same_bits(got[b], r)
    for b in (1, 2):
        s = slice(b, b + 1)
        _same_bits(got[b], eng.polish_many(Q[s], L[s], U[s], X[s], Y[s], 1e-6, 3, 3)[0])


def test_the_two_variable_problem_stops_at_2():
    """the smallest model of stop 2 (tests/test_polish_repair_cpu.py), on an engine without integer rows"""
    from miosqp_amd import qp
    pr = inputs.two_variable_problem()
    eng = qp.OSQP()
    eng.setup(pr["P"], pr["q"], pr["A"], pr["l"], pr["u"], rho=2.0, scaling=0, **problems.QP_SETTINGS)
    P, A = np.asarray(pr["P"].todense()), np.asarray(pr["A"].todense())
    args = [a[None] for a in (pr["q"], pr["l"], pr["u"], pr["x"], pr["y"])]
    got = eng.polish_many(*args, 1e-6, 3, 3)
    refs = [ref.both("two_variable", P, pr["q"], A, pr["l"], pr["u"], pr["x"], pr["y"], 1e-6, 3, 3)]
    _against_reference("two_variable_stop2", "badpivot", got, refs, args[3], args[4])
    assert (got[0].stop, got[0].rounds, got[0].n_dropped, got[0].accepted) == (2, 1, 1, True)
    zero = eng.polish_many(*args, 1e-6, 3, 0)[0]
    np.testing.assert_array_equal(got[0].x, zero.x)
    np.testing.assert_array_equal(got[0].y, zero.y)


def test_more_workgroups_than_compute_units(oracle_mod, engines):
    """B = 600 workgroups, each with a whole compute unit's LDS, on a chip of 256: every record has the bits of its
    instance's B = 1 call, and a second call those of the first"""
    d, Q, L, U, X, Y = inputs.crude_inputs(oracle_mod, (20, 10, 5), 0, 6)
    eng = engines("r20_s0")
    ones = [eng.polish_many(Q[k:k + 1], L[k:k + 1], U[k:k + 1], X[k:k + 1], Y[k:k + 1], 1e-6, 3, 5)[0] for k in range(6)]
    idx = np.arange(600) % 6
    big = eng.polish_many(Q[idx], L[idx], U[idx], X[idx], Y[idx], 1e-6, 3, 5)
    again = eng.polish_many(Q[idx], L[idx], U[idx], X[idx], Y[idx], 1e-6, 3, 5)
    assert len(big) == len(again) == 600 and len(BITS) == 15
    for b in range(600):
        _same_bits(big[b], ones[idx[b]])
        _same_bits(again[b], big[b])
    assert all(r.accepted for r in ones)
