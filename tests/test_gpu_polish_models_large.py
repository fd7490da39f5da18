"""polish_models_large on the HIP engine (needs an MI355X): one polish on each of several DIFFERENT models beyond one
workgroup's LDS -- own P, A, shapes, delta, refine and repair limits --, all in one call of miosqp_qp_polish_models_large
(k_pol_many_gm: workgroup w runs entries w, w + W, .. of a table in device memory, each in slab w).  The yardstick is the
engine's own one-instance `OSQP.polish_many_large`, which test_gpu_polish_many_large.py pins to the long-double
reference: every record must have its 15 fields, x, y and `active` bit for bit (`_same_bits`) -- on a separately set-up
copy of the model, or on the engine itself where the test says so.  No tolerance anywhere, except where an accepted
point of the tree shapes is additionally held against the long-double restatement under the floor rule of
tests/polish_reference.py.

Inputs are what `bnb.polish_models` hands over (test_gpu_polish_models._polish_input).  What is computed once per
session (the nine models' trees, their host-guess records) is shared and not written to."""
import ctypes as C

import numpy as np
import pytest

from miosqp_amd import problems

import polish_many_inputs as inputs
import polish_many_large_inputs as large
import polish_reference as ref
import polish_repair_inputs as single
from test_gpu_polish_many import BITS, _same_bits
from test_gpu_polish_models import _polish_input
from test_gpu_solve_models_large import _build, _close

pytestmark = pytest.mark.gpu

REPAIR = 20
RHO = 0.1
NINE = [(60, 125, 8, 0), (120, 60, 13, 0), (80, 120, 20, 1), (20, 530, 4, 0), (50, 200, 10, 0), (100, 100, 10, 0),
        (150, 100, 5, 3), (100, 200, 15, 2), (150, 300, 20, 1)]  # (n, m, p, seed); n + M = n + m + p > 192 for every one


def _call(solvers, inp, order=None, delta=None, refine=None, repair=REPAIR, y=True, tau=None):
    """ONE qp.polish_models_large over `order` (positions into solvers / inp); returns (records in that order, stats)"""
    from miosqp_amd import qp
    order = list(range(len(solvers))) if order is None else list(order)
    pick = lambda j: [inp[k][j] for k in order]  # noqa: E731
    per = lambda v, k: v[k] if isinstance(v, (list, tuple)) else v  # noqa: E731
    r = qp.polish_models_large([solvers[k] for k in order], pick(0), pick(1), pick(2), pick(3),
                               pick(4) if y else [None] * len(order), [per(1e-6 if delta is None else delta, k) for k in order],
                               [per(3 if refine is None else refine, k) for k in order], [per(repair, k) for k in order], tau=tau)
    assert r is not None
    return r


def _own(solver, v, delta=1e-6, refine=3, repair=REPAIR):
    """the engine's own polish_many_large of that one instance"""
    r = solver.polish_many_large(v[0][None], v[1][None], v[2][None], v[3][None], v[4][None], delta, refine, repair)
    assert r is not None and len(r) == 1
    return r[0]


@pytest.fixture(scope="module")
def nine():
    """the nine models solved by ONE solve_models(large="device"), their polish inputs, the records of one
    polish_models_large call with the host's guess, and those of polish_many_large on separately set-up copies"""
    import miosqp_amd
    from miosqp_amd import bnb
    built = [_build(s, 1, RHO) for s in NINE]
    models, insts = [b[0] for b in built], [{} for _ in built]
    assert all(s[0] + s[1] + s[2] > 192 for s in NINE) and [s[0] + s[1] + s[2] for s in NINE[:2]] == [193, 193]
    results = miosqp_amd.solve_models(models, insts, large="device")
    for k, r in enumerate(results):  # every one of the nine trees closes with an incumbent: nine polishes
        assert r["status"] in (bnb.MI_SOLVED, bnb.MI_MAX_ITER_FEASIBLE), (k, NINE[k], r["status"])
    inp = [_polish_input(m, i, r) for m, i, r in zip(models, insts, results)]
    solvers = [m.work.solver for m in models]
    pol = [m.work.pol for m in models]
    # k_pol_many_m ends at 160 KB of LDS and M = 256, not at n + M = 192: five of the nine fit it as well (the large
    # entry takes every size), four are beyond it
    assert [s.polish_models_fits() for s in solvers] == [True, True, True, False, True, True, False, False, False]
    assert all(s.polish_models_large_fits() for s in solvers)
    recs, stats = _call(solvers, inp, delta=[p["delta"] for p in pol], refine=[p["refine_iter"] for p in pol])
    want = []
    for k, s in enumerate(NINE):
        copy = _build(s, 1, RHO)[0]
        want.append(_own(copy.work.solver, inp[k], pol[k]["delta"], pol[k]["refine_iter"]))
        copy.work.solver.close()
    yield dict(models=models, insts=insts, results=results, inp=inp, solvers=solvers, pol=pol, recs=recs, stats=stats,
               want=want)
    _close(models)


def test_nine_tree_shapes_one_call(nine):
    t = nine
    assert len(BITS) == 15
    st = t["stats"]
    assert st.launches == 1 and st.models == 9 and st.workgroups == 9
    assert st.slab_bytes > 0 and st.arena_bytes >= 9 * st.slab_bytes and st.device_time > 0
    for k in range(9):
        g, w = t["recs"][k], t["want"][k]
        print("model %d %r: accepted %d rounds %d stop %d pri_after %.3e dua_after %.3e" % (
            k, NINE[k], g.accepted, g.rounds, g.stop, g.pri_after, g.dua_after))
        _same_bits(g, w)
    delta, refine = [p["delta"] for p in t["pol"]], [p["refine_iter"] for p in t["pol"]]
    for order in (list(range(8, -1, -1)), [(k + 4) % 9 for k in range(9)]):
        recs, stats = _call(t["solvers"], t["inp"], order, delta=delta, refine=refine)
        assert stats.launches == 1 and stats.workgroups == 9
        for j, k in enumerate(order):
            _same_bits(recs[j], t["recs"][k])
    # the accepted points against the long-double restatement, under the floor rule (M = 534 and 470 at small n is
    # ground the cases of polish_many_large_inputs do not cover)
    bad = []
    for k, g in enumerate(t["recs"]):
        if not g.accepted:
            continue
        d, v = t["models"][k].work.data, t["inp"][k]
        rl, r6 = ref.both(("nine", NINE[k]), d.P, v[0], d.A, v[1], v[2], v[3], v[4], delta[k], refine[k], REPAIR)
        for f in ref.COUNTS:
            if getattr(g, f) != getattr(rl, f):
                bad.append((k, f, getattr(g, f), getattr(rl, f)))
        if not rl.accepted:
            continue
        for f, dev in (("x", g.x), ("y", g.y)):
            e, floor = ref.err(dev, getattr(rl, f)), ref.err(getattr(r6, f), getattr(rl, f))
            print("model %d %r %s: e_dev %.2e e_floor %.2e" % (k, NINE[k], f, e, floor))
            if not e <= ref.bound(floor, getattr(rl, f)):
                bad.append((k, f, e, floor))
    assert not bad, bad
    assert sum(r.accepted and r.stop == 0 for r in t["recs"]) >= 7  # (the comparison is not one of rejected inputs)


def _expected(case, g, who):
    """the integer fields polish_many_large_inputs.CASES states for a case (test_polish_many_large_cpu.py's reading)"""
    ex = case.expect
    assert bool(g.accepted) == ex["accepted"], who
    if ex["accepted"]:
        assert g.reason == 0 and g.stop == 0, who
    for f in ("reason0", "reason", "stop"):
        if f in ex:
            assert getattr(g, f) == ex[f], (who, f)
    if "rounds" in ex:
        assert ex["rounds"][0] <= g.rounds <= ex["rounds"][1], (who, g.rounds)
    if "added" in ex:
        assert ex["added"][0] <= g.n_added <= ex["added"][1], (who, g.n_added)


def test_crude_edges_side_by_side(oracle_mod):
    from miosqp_amd import qp
    names = ["r193_s0", "r255_s0", "r256_s1", "r257_s0", "r257_s0_empty", "r224x300_s0_limit", "r224x300_s0", "sparse5_n300",
             "r50_s1"]
    cases = [large.CASE[n] for n in names]
    assert [c.repair_iter for c in cases] == [5, 5, 5, 5, 20, 5, 20, 5, 5] and cases[4].kind == "empty"
    solvers, inp, delta, refine, repair, case_of = [], [], [], [], [], []

    def small(seed):
        d, Q, L, U, X, Y = inputs.crude_inputs(oracle_mod, (10, 5, 2), seed, 1)
        solvers.append(single.model(qp, problems.random_miqp(10, 5, 2, seed=seed)).work.solver)
        inp.append((Q[0], L[0], U[0], X[0], Y[0]))
        delta.append(1e-6); refine.append(3); repair.append(5); case_of.append(None)

    small(0)
    for c in cases:
        d, Q, L, U, X, Y = large.case_inputs(oracle_mod, c)
        solvers.append(single.model(qp, large.PROBLEMS[c.prob]()).work.solver)  # (an engine each: r257 and r224x300 twice)
        inp.append((Q[0], L[0], U[0], X[0], Y[0]))
        # the crude r257_s0 runs at repair 20 here, beside the empty one
        delta.append(c.delta); refine.append(c.refine_iter); repair.append(20 if c.name == "r257_s0" else c.repair_iter)
        case_of.append(c)
        small(len(solvers) % 4)
    assert len(solvers) == 19 and (solvers[1].n, solvers[1].m) == (193, 6) and solvers[11].m == 310
    recs, stats = _call(solvers, inp, delta=delta, refine=refine, repair=repair)  # the rows of A travel in the arena
    assert stats.launches == 1 and stats.models == 19 and stats.workgroups == 19
    own = [_own(s, v, delta[k], refine[k], repair[k]) for k, (s, v) in enumerate(zip(solvers, inp))]
    again, _ = _call(solvers, inp, delta=delta, refine=refine, repair=repair)  # ... now every engine lends its own copies
    for k, (g, w) in enumerate(zip(recs, own)):
        _same_bits(g, w)
        _same_bits(again[k], w)
        c = case_of[k]
        if c is None:
            continue
        print("%s: accepted %d reason %d rounds %d stop %d +%d -%d" % (c.name, g.accepted, g.reason, g.rounds, g.stop,
                                                                      g.n_added, g.n_dropped))
        if c.name == "r257_s0":  # (at repair 20 instead of the table's 5: the fixed point of its three rounds either way)
            assert g.accepted and g.stop == 0 and c.expect["rounds"][0] <= g.rounds <= c.expect["rounds"][1]
            continue
        _expected(c, g, c.name)
        if c.name == "r224x300_s0_limit":  # rejected at the round limit: the input bit for bit
            assert (g.accepted, g.reason, g.stop, g.rounds, g.accepted0) == (False, 2, 1, 5, False)
            np.testing.assert_array_equal(g.x, inp[k][3])
            np.testing.assert_array_equal(g.y, inp[k][4])
    for s in solvers:
        s.close()


def test_bad_pivots_between_neighbours(oracle_mod):
    from miosqp_amd import qp
    n, kk = large.INDEFINITE[0]
    assert (n, kk) == (200, 196)
    pr = inputs.indefinite_problem(n=n, k=kk)
    Q, L, U, X, Y = inputs.indefinite_batch(pr)
    solvers, inp, repair = [], [], []

    def healthy(shape, seed):
        d, q, l, u, x, y = inputs.crude_inputs(oracle_mod, shape, seed, 1)
        solvers.append(single.model(qp, problems.random_miqp(*shape, seed=seed)).work.solver)
        inp.append((q[0], l[0], u[0], x[0], y[0]))
        repair.append(5)

    healthy((10, 5, 2), 0)
    for b in (1, 2):  # stop 2 (bad pivot in repair round 1), reason 1 (bad pivot in round 0): an engine each
        solvers.append(single.model(qp, pr, qp_extra=dict(rho=2.0, scaling=0)).work.solver)
        inp.append((Q[b], L[b], U[b], X[b], Y[b]))
        repair.append(5)
        healthy((60, 125, 8), b)
    recs, stats = _call(solvers, inp, repair=repair)
    assert stats.launches == 1 and stats.workgroups == 5
    g = recs[1]
    assert (g.stop, g.rounds, g.n_added, g.n_dropped, g.accepted, g.reason) == (2, 1, 0, 1, True, 0)
    np.testing.assert_array_equal(g.active, [-1, -1])
    g = recs[3]
    assert (g.accepted, g.reason, g.accepted0, g.reason0, g.rounds, g.stop) == (False, 1, False, 1, 0, 0)
    assert np.isnan(g.pri_after) and np.isnan(g.dua_after) and np.isnan(g.obj)
    np.testing.assert_array_equal(g.x, X[2])
    np.testing.assert_array_equal(g.y, Y[2])
    np.testing.assert_array_equal(g.active, [0, -1])
    for k, (s, v) in enumerate(zip(solvers, inp)):
        _same_bits(recs[k], _own(s, v, repair=repair[k]))
    assert all(recs[k].accepted for k in (0, 2, 4))
    # the reason-1 model without a y: z = (1, 0) between (0, 0) and (5, 0) -- the first row is nearer to its lower bound,
    # the second is an equality --, so the guess is (-tau, 0), the row stays inactive (1 < tau is false), round 0's own
    # factorisation fails again, and the guess is the y that comes back
    from miosqp_amd import bnb
    v, tau = inp[3], 1e-2
    guess = bnb.primal_guess_multipliers(v[1], v[2], np.array([v[3][pr["k"]], v[3][0]]), tau)
    np.testing.assert_array_equal(guess, [-tau, 0.0])
    host = _call([solvers[3]], [v[:4] + (guess,)], repair=3)[0][0]
    dev = _call([solvers[3]], [v], repair=3, y=False, tau=tau)[0][0]
    _same_bits(dev, host)
    assert (dev.accepted, dev.reason, dev.rounds, dev.stop) == (False, 1, 0, 0)
    np.testing.assert_array_equal(dev.y, guess)
    np.testing.assert_array_equal(dev.x, v[3])
    for s in solvers:
        s.close()


def test_device_guess(nine):
    """y None: the workgroup guesses the multipliers from its own z.  The host's z (scipy) and the device's differ in
    their last bits, so the two guesses agree wherever no row sits within rounding of the middle between its bounds:
    asserted first, on the host in long double, for every model whose bits are then compared.  That a rejected record
    returns the guess is shown where a rejection is certain: test_bad_pivots_between_neighbours."""
    t = nine
    delta, refine = [p["delta"] for p in t["pol"]], [p["refine_iter"] for p in t["pol"]]
    for k, (m, v) in enumerate(zip(t["models"], t["inp"])):
        A = np.asarray(m.work.data.A.todense()).astype(np.longdouble)
        z = A.dot(v[3].astype(np.longdouble))
        l, u = v[1].astype(np.longdouble), v[2].astype(np.longdouble)
        two = (v[1] > -1e30) & (v[2] < 1e30) & (v[1] != v[2])
        gap = np.abs((z - l) - (u - z))[two]
        margin = (1e-9 * (1 + np.abs(l) + np.abs(u)))[two]
        print("model %d: %d two-sided rows, smallest gap / margin %.3g" % (k, int(two.sum()), float(np.min(gap / margin)) if two.any() else np.inf))
        assert np.all(gap >= margin), (k, float(np.min(gap - margin)))
    groups = {}
    for k, v in enumerate(t["inp"]):
        groups.setdefault(v[5], []).append(k)
    for tau, ks in groups.items():
        recs, stats = _call(t["solvers"], t["inp"], ks, delta=delta, refine=refine, y=False, tau=tau)
        assert stats.launches == 1
        for j, k in enumerate(ks):
            _same_bits(recs[j], t["recs"][k])
    # tau 0 with y None is refused, naming model 0
    with pytest.raises(RuntimeError, match="model 0"):
        _call(t["solvers"], t["inp"], [2, 5], delta=delta, refine=refine, y=False, tau=0.0)


def test_more_models_than_workgroups(nine):
    import miosqp_amd
    from miosqp_amd import bnb
    t = nine
    shapes = [(10, 5, 2), (12, 6, 3), (8, 10, 2), (16, 8, 4), (20, 10, 5), (14, 20, 3)]
    prs = [problems.random_miqp(*shapes[k % 6], seed=k // 6) for k in range(640)]
    models = miosqp_amd.setup_models(prs, dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS))
    insts = [{} for _ in prs]
    results = miosqp_amd.solve_models(models, insts)
    keep = [k for k, r in enumerate(results) if r["status"] in (bnb.MI_SOLVED, bnb.MI_MAX_ITER_FEASIBLE)][:596]
    assert len(keep) == 596
    solvers = [models[k].work.solver for k in keep]
    inp = [_polish_input(models[k], insts[k], results[k]) for k in keep]
    delta = [models[k].work.pol["delta"] for k in keep]
    refine = [models[k].work.pol["refine_iter"] for k in keep]
    # four large engines: two in front (their slabs serve a large model, then a small one) and two at the end (a small
    # model, then a large one)
    big_of = {0: 8, 1: 4, 598: 6, 599: 3}  # position -> model of the nine
    for p in sorted(big_of):
        solvers.insert(p, t["solvers"][big_of[p]])
        inp.insert(p, t["inp"][big_of[p]])
        delta.insert(p, t["pol"][big_of[p]]["delta"])
        refine.insert(p, t["pol"][big_of[p]]["refine_iter"])
    assert len(solvers) == 600
    one = lambda p: _call(solvers, inp, [p], delta=delta, refine=refine)[0][0]  # noqa: E731
    big, stats = _call(solvers, inp, delta=delta, refine=refine)
    W = stats.workgroups
    assert stats.launches == 1 and stats.models == 600 and 2 < W < 598 and W < stats.models
    size = lambda p: (solvers[p].n, solvers[p].m)  # noqa: E731
    assert size(0) != size(W) and size(1) != size(1 + W) and size(598) != size(598 - W) and size(599) != size(599 - W)
    again, _ = _call(solvers, inp, delta=delta, refine=refine)
    for k in range(600):
        _same_bits(again[k], big[k])
    for p, k9 in big_of.items():
        _same_bits(big[p], t["recs"][k9])
        _same_bits(big[p], one(p))
    smalls = [p for p in range(600) if p not in big_of]
    for p in smalls[::7]:
        _same_bits(big[p], one(p))
    assert sum(r.accepted for r in big) >= 500
    _close(models)


def test_declines_and_refusals(nine):
    from miosqp_amd import _lib, qp
    lib = _lib.load()
    # n = 513: beyond the slabs
    pr = problems.random_miqp(513, 4, 2, seed=0)
    w = single.model(qp, pr).work
    d, eng = w.data, w.solver
    M = d.m + d.n_int
    x0, y0 = np.zeros(d.n), np.zeros(M)
    a = eng.solve_node(d.l, d.u, x0, y0)
    assert not eng.polish_models_large_fits()
    t = nine
    s2, v2 = t["solvers"][1], t["inp"][1]
    r = qp.polish_models_large([s2, eng], [v2[0], None], [v2[1], d.l], [v2[2], d.u], [v2[3], a.x], [v2[4], a.y], 1e-6, 3, 5)
    assert r is None and "model 1" in _lib.last_error()
    assert eng.polish_many_large_slab_bytes() == 0
    c = eng.solve_node(d.l, d.u, x0, y0)
    assert a.status_val == c.status_val and a.iter == c.iter
    np.testing.assert_array_equal(a.x, c.x)
    np.testing.assert_array_equal(a.y, c.y)
    eng.close()
    # through the C entry
    solvers = [t["solvers"][k] for k in (0, 1, 2)]
    good = [t["inp"][k] for k in (0, 1, 2)]
    roots = [(m.work.data.l, m.work.data.u, np.zeros(s.n), np.zeros(s.m)) for m, s in zip(t["models"][:3], solvers)]
    before = [s.solve_node(*r) for s, r in zip(solvers, roots)]

    def run(order, inp, tau=1e-2, repair=(20, 20, 20), y=True):
        B = len(order)
        arr = lambda j: [np.ascontiguousarray(inp[k][j], dtype=np.float64) for k in order]  # noqa: E731
        q, l, u, x, yv = arr(0), arr(1), arr(2), arr(3), arr(4)
        ptrs = lambda a: (_lib.dp * B)(*[None if v is None else _lib.as_d(v) for v in a])  # noqa: E731
        xo = [np.full(solvers[k].n, 7.0) for k in order]
        yo = [np.full(solvers[k].m, 7.0) for k in order]
        hs = (C.c_void_p * B)(*[solvers[k]._h.value for k in order])
        dl, ri = np.full(B, 1e-6), np.full(B, 3, dtype=np.int32)
        pi = np.array(repair[:B], dtype=np.int32)
        infos, stats = (_lib.PolishRepairInfo * B)(), _lib.PolishModelsLargeStats()
        rc = lib.miosqp_qp_polish_models_large(B, hs, ptrs(q), ptrs(l), ptrs(u), ptrs(x), ptrs(yv if y else [None] * B), tau,
                                               _lib.as_d(dl), _lib.as_i(ri), _lib.as_i(pi), ptrs(xo), ptrs(yo), None, infos,
                                               C.byref(stats))
        if rc != 0:  # outputs untouched
            assert all(np.all(v == 7.0) for v in xo + yo)
        return rc, _lib.last_error()

    rc, err = run([0, 1, 0], good)
    assert rc == -1 and "model 0 is listed again as model 2" in err and "polish_models_large" in err
    rc, err = run([0, 1, 2], good, repair=(20, 21, 20))
    assert rc == -1 and "model 1" in err and "0..20" in err
    bad = [tuple(np.array(a, dtype=float) if not np.isscalar(a) else a for a in v) for v in good]
    bad[2][3][-1] = np.nan
    rc, err = run([0, 1, 2], bad)
    assert rc == -1 and "model 2" in err and "NaN" in err
    bad = [tuple(np.array(a, dtype=float) if not np.isscalar(a) else a for a in v) for v in good]
    bad[1][1][0] = bad[1][2][0] + 1.0
    rc, err = run([0, 1, 2], bad)
    assert rc == 1 and "model 1" in err
    for s, r, b in zip(solvers, roots, before):  # nothing was queued: the engines answer as before, bit for bit
        g = s.solve_node(*r)
        assert (g.status_val, g.iter) == (b.status_val, b.iter)
        np.testing.assert_array_equal(g.x, b.x)
        np.testing.assert_array_equal(g.y, b.y)
    rc, err = run([0, 1, 2], good)  # ... and the same call without a fault goes through
    assert rc == 0


def _end_to_end(shapes, beyond):
    """solve_models(large="device", polish=True, polish_large="device") on `shapes`; beyond: the positions whose models
    are beyond one workgroup of polish_models (the others go into its launch)"""
    import miosqp_amd
    models = [_build(s, 1, RHO)[0] for s in shapes]
    assert [k for k, m in enumerate(models) if not m.work.solver.polish_models_fits()] == beyond
    raw = miosqp_amd.solve_models(models, large="device")
    info = {}
    got = miosqp_amd.solve_models(models, large="device", polish=True, polish_large="device", info=info)
    assert info["polished"] == [0, 1, 2] and info["polish_own"] == {}
    assert info["polish_forms"] == {'small': 3 - len(beyond), 'large': len(beyond)}
    assert info["polish_launches"] == (2 if beyond else 1)
    plain_info = {}
    plain = miosqp_amd.solve_models(models, large="device", polish=True, info=plain_info)
    assert sorted(plain_info["polish_own"]) == beyond  # without the keyword: as before it existed
    assert plain_info["polished"] == [k for k in range(3) if k not in beyond]
    assert plain_info["polish_forms"] == {'small': 3 - len(beyond), 'large': 0}
    assert plain_info["polish_launches"] == 1
    for k in (0, 2):
        w = dict(raw[k], x=raw[k]["x"].copy())
        models[k].polish_many([{}], [w], large=True)
        assert not getattr(models[k].work, "_no_polish_many_large", False)
        for key in ("polished", "polish_rounds", "pri_after", "dua_after", "upper_glob"):
            assert got[k][key] == w[key] or (np.isnan(got[k][key]) and np.isnan(w[key])), (k, key)
        np.testing.assert_array_equal(got[k]["x"], w["x"])
        print("model %d %r: polished %s rounds %d, the host's restatement: polished %s rounds %d" % (
            k, shapes[k], got[k]["polished"], got[k]["polish_rounds"], plain[k]["polished"], plain[k]["polish_rounds"]))
    assert got[0]["polished"] or got[2]["polished"]
    # a second call with the keyword, after the models' own polish_many has remembered its decline: the same groups
    info2 = {}
    again = miosqp_amd.solve_models(models, large="device", polish=True, polish_large="device", info=info2)
    assert info2["polish_forms"] == info["polish_forms"] and info2["polish_own"] == {}
    for k in range(3):
        np.testing.assert_array_equal(again[k]["x"], got[k]["x"])
    _close(models)


def test_end_to_end():
    """two form-3 models beyond one workgroup of polish_models around one it takes: the second launch polishes them"""
    _end_to_end([(150, 100, 5, 3), (50, 100, 10, 0), (100, 200, 15, 2)], [0, 2])


def test_end_to_end_where_the_small_launch_takes_every_model():
    """(80,120,20) and (120,60,13) run their trees in reduced form (n + M > 192) but fit the 160 KB of k_pol_many_m (127 KB
    and 138 KB): polish_models has taken them in its one launch since it exists, so the keyword changes nothing for them
    -- no second launch, polish_own empty with and without it"""
    _end_to_end([(80, 120, 20, 1), (50, 100, 10, 0), (120, 60, 13, 0)], [])
