"""k_pol_many_g (csrc/polish_many_large.hip) through the public entry OSQP.polish_many_large, against the long-double
restatement of tests/polish_reference.py on the cases of polish_many_large_inputs (n 193 .. 320, M up to 310, both edges
of the kernel's 32-wide panel, sparse rows, the bad pivots in a last and in a middle panel), against k_pol_many on a
size both take, against the float64 restatement at n 500 / M 1250, and end to end through solve_many(polish="device").

The inputs and what the reference says about them are checked on the CPU by test_polish_many_large_cpu.py, so a failure
here can only mean the kernel.  The tolerance is test_gpu_polish_many_edges.py's floor rule (polish_reference.bound):
e_dev <= max(16 e_floor, 64 eps max(1, max |v_ld|)) for x and y, the same for obj, pri_after and dua_after with the
floor at its largest over the case; no constant fixed in advance; every case prints e_dev / e_floor before it asserts."""
import numpy as np
import pytest

from miosqp_amd import problems

import polish_many_inputs as inputs
import polish_many_large_inputs as large
import polish_reference as ref
import polish_repair_inputs as single
from test_gpu_polish_many import _same_bits
from test_gpu_polish_many_edges import _against_reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines():
    """one HIP engine per problem, shared by the tests (a polish_many_large call leaves nothing behind)"""
    from miosqp_amd import qp
    cache = {}

    def get(prob):
        if prob not in cache:
            cache[prob] = single.model(qp, large.PROBLEMS[prob]()).work.solver
        return cache[prob]
    return get


def _run(oracle_mod, engines, name):
    case = large.CASE[name]
    data = d, Q, L, U, X, Y = large.case_inputs(oracle_mod, case)
    refs = large.case_references(case, data)
    got = engines(case.prob).polish_many_large(Q, L, U, X, Y, case.delta, case.refine_iter, case.repair_iter)
    assert got is not None and len(got) == len(Q)
    _against_reference(name, case.group, got, refs, X, Y)
    return case, data, refs, got


@pytest.mark.parametrize("name", [c.name for c in large.CASES if c.name != "r50_s1"])
def test_table_case_against_the_reference(oracle_mod, engines, name):
    case, (d, Q, L, U, X, Y), refs, got = _run(oracle_mod, engines, name)
    if name == "r224x300_s0_limit":  # rejected at the round limit: the input bit for bit
        for b, g in enumerate(got):
            assert (g.accepted, g.reason, g.stop, g.rounds, g.accepted0) == (False, 2, 1, 5, False)
            np.testing.assert_array_equal(g.x, X[b])
            np.testing.assert_array_equal(g.y, Y[b])
            assert 15 <= int(np.sum(g.active[256:] != 0)) <= 17
    else:
        assert all(g.accepted for g in got)
    if case.kind == "empty":
        first = engines(case.prob).polish_many_large(Q, L, U, X, Y, case.delta, case.refine_iter, 0)
        for r in first:
            assert (r.n_lower, r.n_upper, r.rounds, r.stop, r.reason) == (0, 0, 0, 1, 2) and not np.any(r.active)


def test_both_kernels_on_a_size_both_take(oracle_mod, engines):
    case, (d, Q, L, U, X, Y), refs, got = _run(oracle_mod, engines, "r50_s1")
    small = engines("r50_s1").polish_many(Q, L, U, X, Y, case.delta, case.refine_iter, case.repair_iter)
    _against_reference("r50_s1 (k_pol_many)", "both", small, refs, X, Y)
    for g, s in zip(got, small):
        for f in ref.COUNTS:
            assert getattr(g, f) == getattr(s, f), f
        np.testing.assert_array_equal(g.active, s.active)


# ---- the bad pivots ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", large.INDEFINITE)
def test_bad_pivots_in_a_last_and_in_a_middle_panel(n, k):
    """the engine is set up as test_gpu_polish_many_edges.py sets up its indefinite problem (rho 2, no scaling)"""
    from miosqp_amd import qp
    pr = inputs.indefinite_problem(n=n, k=k)
    w = single.model(qp, pr, qp_extra=dict(rho=2.0, scaling=0)).work
    eng, P, A = w.solver, np.asarray(w.data.P.todense()), np.asarray(w.data.A.todense())
    Q, L, U, X, Y = inputs.indefinite_batch(pr)
    got = eng.polish_many_large(Q, L, U, X, Y, 1e-6, 3, 5)
    refs = [ref.both(("indefinite", n, k, b), P, Q[b], A, L[b], U[b], X[b], Y[b], 1e-6, 3, 5) for b in range(4)]
    assert [(r.stop, r.reason, r.rounds) for r in got] == [(0, 0, 0), (2, 0, 1), (0, 1, 0), (0, 0, 0)]
    keep = [0, 1, 3]
    _against_reference("indefinite_n%d" % n, "badpivot", [got[b] for b in keep], [refs[b] for b in keep], X[keep], Y[keep])
    for b in (0, 3):
        assert got[b].accepted and got[b].rounds == 0
    # instance 1: judged on round 0's point with round 0's set
    g = got[1]
    assert (g.stop, g.rounds, g.n_added, g.n_dropped, g.accepted, g.reason) == (2, 1, 0, 1, True, 0)
    np.testing.assert_array_equal(g.active, [-1, -1])
    zero = eng.polish_many_large(Q[1:2], L[1:2], U[1:2], X[1:2], Y[1:2], 1e-6, 3, 0)[0]
    assert (zero.stop, zero.rounds, zero.accepted) == (1, 0, True)
    np.testing.assert_array_equal(g.x, zero.x)
    np.testing.assert_array_equal(g.y, zero.y)
    assert g.obj == zero.obj and g.pri_after == zero.pri_after and g.dua_after == zero.dua_after
    # instance 2: reason 1, NaN in the record, the input back
    g, (rl, r6) = got[2], refs[2]
    for f in ref.COUNTS:
        assert getattr(g, f) == getattr(rl, f), f
    assert (g.accepted, g.reason, g.accepted0, g.reason0, g.rounds, g.stop) == (False, 1, False, 1, 0, 0)
    assert np.isnan(g.pri_after) and np.isnan(g.dua_after) and np.isnan(g.obj)
    np.testing.assert_array_equal(g.x, X[2])
    np.testing.assert_array_equal(g.y, Y[2])
    np.testing.assert_array_equal(g.active, [0, -1])
    eng.close()


# ---- batch independence and slab reuse -----------------------------------------------------------------------------------
def test_more_instances_than_slabs(oracle_mod, engines):
    """B = 600 exceeds any W (at most two workgroups per compute unit): the two crude and the two empty-set instances of
    (257, 40, 5), tiled; one launch mixes 3, 7 and 8 rounds; every copy has the bits of its instance's B = 1 call"""
    crude, empty = large.CASE["r257_s0"], large.CASE["r257_s0_empty"]
    arrs = [np.concatenate([a, b]) for a, b in zip(large.case_inputs(oracle_mod, crude)[1:],
                                                   large.case_inputs(oracle_mod, empty)[1:])]
    eng = engines("r257_s0")
    ones = [eng.polish_many_large(*[a[k:k + 1] for a in arrs], 1e-6, 3, 20)[0] for k in range(4)]
    assert all(r.accepted for r in ones) and len({r.rounds for r in ones}) >= 2
    # (the references of the four distinct inputs: repair_iter 20 here, and no other reference run)
    Q, L, U, X, Y = arrs
    d = large.case_inputs(oracle_mod, crude)[0]
    keys = [(c.prob, c.kind, c.B, i) for c in (crude, empty) for i in range(2)]  # (polish_many_inputs.edge_references')
    refs = [ref.both(keys[k], d.P, Q[k], d.A, L[k], U[k], X[k], Y[k], 1e-6, 3, 20) for k in range(4)]
    _against_reference("r257_s0_mixed", "slabs", ones, refs, X, Y)
    idx = np.arange(600) % 4
    big = eng.polish_many_large(*[a[idx] for a in arrs], 1e-6, 3, 20)
    assert len(big) == 600
    for b in range(600):
        _same_bits(big[b], ones[idx[b]])


# ---- config 2's size -------------------------------------------------------------------------------------------------------
def test_config_2_size_against_the_restatement(oracle_mod):
    """(500, 1000, 250) seed 0, three crude roots, repair_iter 20, against the float64 restatement (the long-double
    reference is not run at this size): integer fields and `active` equal -- every margin of the restatement is >= 1e-7,
    asserted --, pri and dua recomputed from the original matrices <= 1e-9, obj within 1e-9 max(1, |obj|)"""
    from miosqp_amd import bnb, qp
    pr = problems.random_miqp(500, 1000, 250, seed=0)
    d, Q, L, U, X, Y = inputs.crude_inputs_of(oracle_mod, pr, 3)
    eng = single.model(qp, pr).work.solver
    got = eng.polish_many_large(Q, L, U, X, Y, 1e-6, 3, 20)
    assert got is not None
    for b, g in enumerate(got):
        ro = bnb.polish_restatement(d.P, Q[b], d.A, L[b], U[b], X[b], Y[b], 1e-6, 3, repair_iter=20)
        margin = float(np.min(ro.margin))
        pri, dua = inputs.residuals(d, Q[b], L[b], U[b], g.x, g.y)
        print("config 2 [%d]: rounds %d +%d -%d active %d, restatement rounds %d +%d -%d active %d margin %.1e; pri %.2e "
              "dua %.2e obj %.12g (restatement %.12g)" % (b, g.rounds, g.n_added, g.n_dropped, g.n_lower + g.n_upper,
                                                         ro.rounds, ro.n_added, ro.n_dropped, ro.n_lower + ro.n_upper,
                                                         margin, pri, dua, g.obj, ro.obj))
        assert margin >= 1e-7, (b, margin)
        assert ro.accepted and ro.stop == 0
        for f in ref.COUNTS:
            assert getattr(g, f) == getattr(ro, f), (b, f, getattr(g, f), getattr(ro, f))
        np.testing.assert_array_equal(g.active, ro.active)
        assert pri <= 1e-9 and dua <= 1e-9, (b, pri, dua)
        assert abs(g.obj - ro.obj) <= 1e-9 * max(1.0, abs(ro.obj)), (b, g.obj, ro.obj)
    eng.close()


# ---- arguments and isolation -------------------------------------------------------------------------------------------------
def test_argument_checks_and_isolation(oracle_mod, engines):
    case = large.CASE["r193_s0"]
    d, Q, L, U, X, Y = large.case_inputs(oracle_mod, case)
    eng = engines("r193_s0")
    B = len(Q)
    x0, y0 = np.zeros(d.n), np.zeros(d.m + d.n_int)
    a = eng.solve_node(d.l, d.u, x0, y0)
    want = eng.polish_many_large(Q, L, U, X, Y, 1e-6, 3, 5)
    assert eng.polish_many_large_slab_bytes() >= B * 8 * d.n * d.n  # W = B slabs, each holds S

    def still_answers():
        for r, s in zip(eng.polish_many_large(Q, L, U, X, Y, 1e-6, 3, 5), want):
            _same_bits(r, s)

    bad_calls = [lambda: eng.polish_many_large(Q[:0], L[:0], U[:0], X[:0], Y[:0]),
                 lambda: eng.polish_many_large(Q, L, U, X, Y, delta=0.0),
                 lambda: eng.polish_many_large(Q, L, U, X, Y, delta=-1.0),
                 lambda: eng.polish_many_large(Q, L, U, X, Y, refine_iter=-1),
                 lambda: eng.polish_many_large(Q, L, U, X, Y, refine_iter=11),
                 lambda: eng.polish_many_large(Q, L, U, X, Y, repair_iter=-1),
                 lambda: eng.polish_many_large(Q, L, U, X, Y, repair_iter=21)]
    for which in range(5):
        arrs = [Q.copy(), L.copy(), U.copy(), X.copy(), Y.copy()]
        arrs[which][B - 1, 3] = np.nan
        bad_calls.append(lambda arrs=arrs: eng.polish_many_large(*arrs))
    for call in bad_calls:
        with pytest.raises(RuntimeError):
            call()
        still_answers()
    lo = L.copy()
    lo[B - 1, 0] = U[B - 1, 0] + 1.0
    with pytest.raises(ValueError):
        eng.polish_many_large(Q, lo, U, X, Y)
    still_answers()
    # q None: the engine's linear cost (instance 0's) for every instance
    none = eng.polish_many_large(None, L[:1], U[:1], X[:1], Y[:1], 1e-6, 3, 5)
    _same_bits(none[0], want[0])
    c = eng.solve_node(d.l, d.u, x0, y0)
    assert a.status_val == c.status_val and a.iter == c.iter
    np.testing.assert_array_equal(a.x, c.x)
    np.testing.assert_array_equal(a.y, c.y)


def test_declines_above_the_limit_without_allocating():
    """n = 513 is beyond the limit: None, no slab on the engine, and solve_node's bits unchanged"""
    from miosqp_amd import qp
    pr = problems.random_miqp(513, 4, 2, seed=0)
    w = single.model(qp, pr).work
    d, eng = w.data, w.solver
    M = d.m + d.n_int
    x0, y0 = np.zeros(d.n), np.zeros(M)
    a = eng.solve_node(d.l, d.u, x0, y0)
    assert eng.polish_many_large(None, d.l[None], d.u[None], a.x[None], a.y[None], 1e-6, 3, 5) is None
    assert eng.polish_many_large_slab_bytes() == 0
    c = eng.solve_node(d.l, d.u, x0, y0)
    assert a.status_val == c.status_val and a.iter == c.iter
    np.testing.assert_array_equal(a.x, c.x)
    np.testing.assert_array_equal(a.y, c.y)
    eng.close()


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def test_solve_many_with_device_polish_end_to_end():
    """the shape of test_gpu_lockstep_many.py: the lock-step trees, then ONE polish_many_large call and no restatement;
    against polish=True (the host's restatement) on a second model"""
    from miosqp_amd import bnb, qp
    pr = problems.random_miqp(100, 200, 50, seed=0)
    inst = inputs.instances(pr, 4)
    calls, host_calls = [], []
    real, real_host = qp.OSQP.polish_many_large, bnb.polish_restatement

    def spy(self, *args, **kw):
        recs = real(self, *args, **kw)
        calls.append(recs)
        return recs

    def spy_host(*args, **kw):
        host_calls.append(1)
        return real_host(*args, **kw)

    dev_model, host_model = single.model(qp, pr), single.model(qp, pr)
    qp.OSQP.polish_many_large, bnb.polish_restatement = spy, spy_host
    try:
        dev = dev_model.solve_many(inst, polish="device")
    finally:
        qp.OSQP.polish_many_large, bnb.polish_restatement = real, real_host
    host = host_model.solve_many(inst, polish=True)
    assert len(calls) == 1 and calls[0] is not None and len(calls[0]) == 4 and not host_calls
    assert getattr(dev_model.work, "_no_polish_many", False) and not getattr(dev_model.work, "_no_polish_many_large", False)
    with pytest.raises(ValueError):
        dev_model.solve_many(inst, polish="gpu")
    for b, (g, h) in enumerate(zip(dev, host)):
        print("instance %d: %s nodes %d rounds %d polished %s upper %.12g | host rounds %d polished %s upper %.12g"
              % (b, g["status"], g["nodes"], g["polish_rounds"], g["polished"], g["upper_glob"], h["polish_rounds"],
                 h["polished"], h["upper_glob"]))
        assert g["status"] == h["status"] == bnb.MI_SOLVED
        for key in ("nodes", "osqp_iter", "polished", "polish_rounds"):
            assert g[key] == h[key], (b, key)
        assert g["polished"] is True
        assert abs(g["upper_glob"] - h["upper_glob"]) <= 1e-9 * max(1.0, abs(h["upper_glob"]))
        np.testing.assert_array_equal(g["x"][pr["i_idx"]], h["x"][pr["i_idx"]])
    for m_ in (dev_model, host_model):
        m_.work.solver.close()
