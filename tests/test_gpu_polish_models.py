"""polish_models on the HIP engine (needs an MI355X): one polish on each of several DIFFERENT models -- own P, A, shapes,
delta, refine and repair limits --, all in one call of miosqp_qp_polish_models (k_pol_many_m: workgroup b runs entry b
of a table in device memory).  The yardstick is the existing path: every record must have, bit for bit, the 15 fields,
x, y and `active` of `OSQP.polish_many` with that one instance -- on a separately set-up copy of the model, or on the
engine itself where the test says so.  No tolerance anywhere, except where an accepted point of an edge shape is
additionally held against the long-double restatement under the floor rule of tests/polish_reference.py.

Inputs are what `bnb.polish_models` hands over: the incumbent of a closed tree with its integers rounded, l and u with
the integer rows fixed to them, and the multipliers `bnb.primal_guess_multipliers` guesses (or none: the device's guess).
What is computed once per session (the twelve models' trees, their host-guess records) is shared and not written to."""
import ctypes as C

import numpy as np
import pytest

from miosqp_amd import problems

import polish_many_inputs as inputs
import polish_reference as ref
import polish_repair_inputs as single
from test_gpu_polish_many import BITS, _same_bits
from test_gpu_solve_models import RHOS, TWELVE, _build, _close, _rule

pytestmark = pytest.mark.gpu

REPAIR = 20


def _polish_input(mdl, inst, res, tau=None):
    """(q, l, u, x, y, tau) of one solved model, as bnb.polish_models prepares them with guess="host" """
    from miosqp_amd import bnb
    assert res["status"] in (bnb.MI_SOLVED, bnb.MI_MAX_ITER_FEASIBLE)
    work, d = mdl.work, mdl.work.data
    tau = 10. * work.qp_settings.get("eps_abs", 1e-3) if tau is None else tau
    Q, L, U = mdl._instance_vectors([inst])
    x = np.array(res["x"], dtype=float)
    xi = np.round(x[d.i_idx])
    x[d.i_idx] = xi
    L[0, d.m:] = xi
    U[0, d.m:] = xi
    return Q[0], L[0], U[0], x, bnb.primal_guess_multipliers(L[0], U[0], d.A.dot(x), tau), tau


def _call(solvers, inp, order=None, delta=None, refine=None, repair=REPAIR, y=True, tau=None):
    """ONE qp.polish_models over `order` (positions into solvers / inp); returns (records in that order, stats)"""
    from miosqp_amd import qp
    order = list(range(len(solvers))) if order is None else list(order)
    pick = lambda j: [inp[k][j] for k in order]  # noqa: E731
    per = lambda v, k: v[k] if isinstance(v, (list, tuple)) else v  # noqa: E731
    r = qp.polish_models([solvers[k] for k in order], pick(0), pick(1), pick(2), pick(3), pick(4) if y else [None] * len(order),
                         [per(1e-6 if delta is None else delta, k) for k in order],
                         [per(3 if refine is None else refine, k) for k in order], [per(repair, k) for k in order], tau=tau)
    assert r is not None
    return r


def _own(solver, v, delta=1e-6, refine=3, repair=REPAIR):
    """the engine's own polish_many of that one instance"""
    r = solver.polish_many(v[0][None], v[1][None], v[2][None], v[3][None], v[4][None], delta, refine, repair)
    assert r is not None and len(r) == 1
    return r[0]


@pytest.fixture(scope="module", params=RHOS, ids=["rho0.1", "rho_auto"])
def twelve(request):
    """the twelve models of test_gpu_solve_models.py solved by ONE solve_models, their polish inputs, the records of one
    polish_models call with the host's guess, and those of polish_many on separately set-up copies"""
    import miosqp_amd
    rho = request.param
    built = [_build(s, _rule(k), rho) for k, s in enumerate(TWELVE)]
    models, insts = [b[0] for b in built], [b[1] for b in built]
    results = miosqp_amd.solve_models(models, insts)
    from miosqp_amd import bnb
    for k, r in enumerate(results):  # every one of the twelve trees closes with an incumbent: twelve polishes
        assert r["status"] in (bnb.MI_SOLVED, bnb.MI_MAX_ITER_FEASIBLE), (k, TWELVE[k], r["status"])
    inp = [_polish_input(m, i, r) for m, i, r in zip(models, insts, results)]
    solvers = [m.work.solver for m in models]
    pol = [m.work.pol for m in models]
    recs, stats = _call(solvers, inp, delta=[p["delta"] for p in pol], refine=[p["refine_iter"] for p in pol])
    want = []
    for k, s in enumerate(TWELVE):
        copy = _build(s, _rule(k), rho)[0]
        want.append(_own(copy.work.solver, inp[k], pol[k]["delta"], pol[k]["refine_iter"]))
        copy.work.solver.close()
    yield dict(rho=rho, models=models, insts=insts, results=results, inp=inp, solvers=solvers, pol=pol, recs=recs,
               stats=stats, want=want)
    _close(models)


def test_twelve_models_twelve_shapes_one_call(twelve):
    t = twelve
    assert len({(s.n, s.m) for s in t["solvers"]}) == 7 and len(BITS) == 15  # (twelve P and A of seven sizes)
    assert t["stats"].launches == 1 and t["stats"].models == 12
    assert 0 < t["stats"].lds_bytes <= 160 * 1024 and t["stats"].arena_bytes > 0 and t["stats"].device_time > 0
    for k in range(12):
        g, w = t["recs"][k], t["want"][k]
        print("model %d %r: accepted %d rounds %d stop %d pri_after %.3e dua_after %.3e" % (
            k, TWELVE[k], g.accepted, g.rounds, g.stop, g.pri_after, g.dua_after))
        _same_bits(g, w)
    assert sum(r.accepted and r.stop == 0 for r in t["recs"]) >= 8  # (the comparison is not one of rejected inputs)
    delta, refine = [p["delta"] for p in t["pol"]], [p["refine_iter"] for p in t["pol"]]
    for order in (list(range(11, -1, -1)), [(k + 5) % 12 for k in range(12)]):
        recs, stats = _call(t["solvers"], t["inp"], order, delta=delta, refine=refine)
        assert stats.launches == 1
        for j, k in enumerate(order):
            _same_bits(recs[j], t["recs"][k])


def test_edge_shapes_side_by_side(oracle_mod):
    from miosqp_amd import qp
    names = ["r192_s0", "r160_s0", "r20x150_s0", "milp_guess", "one_sided_guess", "equality_crude"]
    cases = [inputs.EDGE[n] for n in names]
    assert cases[1].group == "segment3" and cases[2].group == "chunk3" and len({c.prob for c in cases}) == 6
    solvers, inp, delta, refine, repair, refs = [], [], [], [], [], []

    def small(seed):
        d, Q, L, U, X, Y = inputs.crude_inputs(oracle_mod, (10, 5, 2), seed, 1)
        solvers.append(single.model(qp, problems.random_miqp(10, 5, 2, seed=seed)).work.solver)
        inp.append((Q[0], L[0], U[0], X[0], Y[0]))
        delta.append(1e-6); refine.append(3); repair.append(5); refs.append(None)

    small(0)
    for c in cases:
        data = d, Q, L, U, X, Y = inputs.edge_inputs(oracle_mod, c)
        solvers.append(single.model(qp, inputs.PROBLEMS[c.prob]()).work.solver)
        inp.append((Q[0], L[0], U[0], X[0], Y[0]))
        delta.append(c.delta); refine.append(c.refine_iter); repair.append(c.repair_iter)
        refs.append(inputs.edge_references(c, data)[0])
        small(len(solvers) % 4)
    assert (solvers[1].n, solvers[1].m) == (192, 3) and solvers[3].n >= 129 and solvers[5].m > 128
    recs, stats = _call(solvers, inp, delta=delta, refine=refine, repair=repair)  # the rows of A travel in the arena
    assert stats.launches == 1 and stats.models == 13
    assert stats.lds_bytes == 20285 * 8  # the launch's LDS is that of (192, 3), the largest need (test_capacity_boundary)
    own = [_own(s, v, delta[k], refine[k], repair[k]) for k, (s, v) in enumerate(zip(solvers, inp))]
    again, _ = _call(solvers, inp, delta=delta, refine=refine, repair=repair)  # ... now every engine lends its own copy
    bad = []
    for k, (g, w) in enumerate(zip(recs, own)):
        _same_bits(g, w)
        _same_bits(again[k], w)
        if refs[k] is None or not g.accepted:
            continue
        rl, r6 = refs[k]
        for f, dev in (("x", g.x), ("y", g.y)):
            e, floor = ref.err(dev, getattr(rl, f)), ref.err(getattr(r6, f), getattr(rl, f))
            print("%s %s: e_dev %.2e e_floor %.2e" % (names[(k - 1) // 2], f, e, floor))
            if not e <= ref.bound(floor, getattr(rl, f)):
                bad.append((k, f, e, floor))
    assert not bad, bad
    assert all(recs[k].accepted for k in range(1, 13, 2))
    for s in solvers:
        s.close()


def test_bad_pivots_between_neighbours(oracle_mod):
    from miosqp_amd import qp
    pr = inputs.indefinite_problem()
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
        repair.append(3)
        healthy((20, 10, 5), b)
    recs, stats = _call(solvers, inp, repair=repair)
    assert stats.launches == 1
    g = recs[1]
    assert (g.stop, g.rounds, g.n_added, g.n_dropped, g.accepted, g.reason) == (2, 1, 0, 1, True, 0)
    np.testing.assert_array_equal(g.active, [-1, -1])
    assert (g.n_lower, g.n_upper) == (2, 0)
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


def test_a_model_that_does_not_fit():
    import miosqp_amd
    from miosqp_amd import qp
    shapes = [(10, 5, 2, 0), (192, 3, 1, 0), (20, 10, 5, 1)]

    def build():
        return [single.model(qp, problems.random_miqp(n, m, p, seed=s)) for n, m, p, s in shapes]

    models = build()
    insts = [{}, {}, {}]
    results = miosqp_amd.solve_models(models, insts)
    solvers = [m.work.solver for m in models]
    assert (solvers[1].n, solvers[1].m) == (192, 4)
    assert [s.polish_models_fits() for s in solvers] == [True, False, True]
    inp = [_polish_input(m, i, r) for m, i, r in zip(models, insts, results)]
    d = models[0].work.data
    before = solvers[0].solve_node(d.l, d.u, np.zeros(d.n), np.zeros(len(d.l)))
    pick = lambda j: [v[j] for v in inp]  # noqa: E731
    assert qp.polish_models(solvers, pick(0), pick(1), pick(2), pick(3), pick(4), 1e-6, 3, REPAIR) is None
    after = solvers[0].solve_node(d.l, d.u, np.zeros(d.n), np.zeros(len(d.l)))
    assert before.iter == after.iter
    np.testing.assert_array_equal(before.x, after.x)
    np.testing.assert_array_equal(before.y, after.y)
    info = {}
    got = miosqp_amd.polish_models(models, insts, [dict(r) for r in results], info=info)
    assert info["polished"] == [0, 2] and info["polish_launches"] == 1 and list(info["polish_own"]) == [1]
    assert "beyond one workgroup" in info["polish_own"][1] and info["polish_device_time"] > 0
    copies = build()
    for k, m in enumerate(copies):
        want = m.polish_many([insts[k]], [dict(results[k])])[0]
        for key in want:
            if isinstance(want[key], np.ndarray):
                np.testing.assert_array_equal(got[k][key], want[key])
            else:
                assert got[k][key] == want[key] or (want[key] != want[key] and got[k][key] != got[k][key]), (k, key)
    assert got[0]["polished"] or got[2]["polished"]
    _close(models + copies)


PC_STAND_IN = (18, 27, 6, 0)  # a seeded model of the power converter's n and general rows (see test_device_guess)


def test_device_guess(twelve):
    """y None: the workgroup guesses the multipliers from its own z.  The host's z (scipy) and the device's (one fused
    multiply-add per entry) differ in their last bits, so the two guesses agree wherever no row sits within rounding of
    the middle between its bounds: asserted first, on the host in long double, for every model whose bits are then
    compared.  The power converter cannot pass that assertion with any of its MPC steps: its rows 18..26 are differences
    of integer inputs in [-1, 1], and z = 0, the exact middle, is what most of them take (gap 0 in every format).  In
    the margin-checked list a seeded model of its n and general rows stands in for it.  The power converter itself
    still goes through the launch: such a z is a sum of exactly representable integers in either order, so both sides
    compare the same two numbers; that its bits agree as well is asserted apart, after its ties were shown to be exact."""
    import miosqp_amd
    t = twelve
    pc = TWELVE.index("pc")
    extra, own, _ = _build(PC_STAND_IN, 1, t["rho"])
    res = miosqp_amd.solve_models([extra], [own])
    models, solvers = t["models"] + [extra], t["solvers"] + [extra.work.solver]
    inp = t["inp"] + [_polish_input(extra, own, res[0])]
    delta = [p["delta"] for p in t["pol"]] + [extra.work.pol["delta"]]
    refine = [p["refine_iter"] for p in t["pol"]] + [extra.work.pol["refine_iter"]]
    host_recs = list(t["recs"]) + [_call(solvers, inp, [12], delta=delta, refine=refine)[0][0]]
    for k, (m, v) in enumerate(zip(models, inp)):
        A = np.asarray(m.work.data.A.todense()).astype(np.longdouble)
        z = A.dot(v[3].astype(np.longdouble))
        l, u = v[1].astype(np.longdouble), v[2].astype(np.longdouble)
        two = (v[1] > -1e30) & (v[2] < 1e30) & (v[1] != v[2])
        gap = np.abs((z - l) - (u - z))[two]
        margin = (1e-9 * (1 + np.abs(l) + np.abs(u)))[two]
        print("model %d: %d two-sided rows, smallest gap / margin %.3g" % (k, int(two.sum()), float(np.min(gap / margin)) if two.any() else np.inf))
        if k == pc:  # exact ties or clear of the middle, and every z an integer: nothing for rounding to decide
            assert np.all((gap == 0) | (gap >= margin)) and np.all(z[two] == np.round(z[two]))
            continue
        assert np.all(gap >= margin), (k, float(np.min(gap - margin)))
    groups = {}
    for k, v in enumerate(inp):
        groups.setdefault(v[5], []).append(k)
    rejected = 0
    for tau, ks in groups.items():
        recs, stats = _call(solvers, inp, ks, delta=delta, refine=refine, y=False, tau=tau)
        assert stats.launches == 1
        for j, k in enumerate(ks):
            _same_bits(recs[j], host_recs[k])
            if not recs[j].accepted:
                rejected += 1
                np.testing.assert_array_equal(recs[j].y, inp[k][4])
    print("device guess: %d tau groups, %d rejected models" % (len(groups), rejected))
    # ... and through the package: the results of guess="device" are those of guess="host"
    insts, results = t["insts"] + [own], t["results"] + res
    host = miosqp_amd.polish_models(models, insts, [dict(r) for r in results])
    info = {}
    dev = miosqp_amd.polish_models(models, insts, [dict(r) for r in results], guess="device", info=info)
    assert info["polished"] == list(range(13)) and info["polish_own"] == {} and info["polish_launches"] == len(groups)
    for k in range(13):
        assert set(dev[k]) == set(host[k])
        for key in ("polished", "polish_rounds", "pri_after", "dua_after", "upper_glob"):
            assert dev[k][key] == host[k][key] or (host[k][key] != host[k][key] and dev[k][key] != dev[k][key]), (k, key)
        np.testing.assert_array_equal(dev[k]["x"], host[k]["x"])
    extra.work.solver.close()


def test_more_workgroups_than_compute_units():
    import miosqp_amd
    shapes = [(10, 5, 2), (12, 6, 3), (8, 10, 2), (16, 8, 4), (20, 10, 5), (14, 20, 3)]
    prs = [problems.random_miqp(*shapes[k % 6], seed=k // 6) for k in range(300)]
    models = miosqp_amd.setup_models(prs, dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS))
    insts = [{} for _ in prs]
    results = miosqp_amd.solve_models(models, insts)
    from miosqp_amd import bnb
    keep = [k for k, r in enumerate(results) if r["status"] in (bnb.MI_SOLVED, bnb.MI_MAX_ITER_FEASIBLE)]
    assert len(keep) >= 290
    solvers = [models[k].work.solver for k in keep]
    inp = [_polish_input(models[k], insts[k], results[k]) for k in keep]
    big, stats = _call(solvers, inp)
    assert stats.launches == 1 and stats.models == len(keep) > 256
    again, _ = _call(solvers, inp)
    for k in range(len(keep)):
        one, _ = _call(solvers, inp, [k])
        _same_bits(big[k], one[0])
        _same_bits(again[k], big[k])
    assert sum(r.accepted for r in big) >= 250
    _close(models)


def test_ownership_of_the_arena():
    import miosqp_amd
    from miosqp_amd import qp
    live = qp.setup_groups_live()
    shapes = [(10, 5, 2, 0), (20, 10, 5, 1), (32, 8, 16, 0), (12, 6, 3, 2)]

    def group(batched):
        prs = [problems.random_miqp(n, m, p, seed=s) for n, m, p, s in shapes]
        if batched:
            models = miosqp_amd.setup_models(prs, dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS))
        else:
            models = [single.model(qp, pr) for pr in prs]
        insts = [{} for _ in prs]
        results = miosqp_amd.solve_models(models, insts)
        return models, [m.work.solver for m in models], [_polish_input(m, i, r) for m, i, r in zip(models, insts, results)]

    models, solvers, inp = group(True)
    assert qp.setup_groups_live() == live + 1
    first, _ = _call(solvers, inp)
    for s in reversed(solvers):  # engines[0], the arena's owner, last
        s.close()
    assert qp.setup_groups_live() == live
    models, solvers, inp = group(True)
    second, _ = _call(solvers, inp)
    for k in range(4):
        _same_bits(second[k], first[k])
    for s in solvers:  # the owner first
        s.close()
    assert qp.setup_groups_live() == live
    models, solvers, inp = group(False)
    third, _ = _call(solvers, inp)
    other, _ = _call(solvers, inp, [2, 0, 3, 1])  # a previously non-first engine comes first: it gets an arena of its own
    for j, k in enumerate([2, 0, 3, 1]):
        _same_bits(other[j], third[k])
    solvers[0].close()  # the first owner goes; the second owner's arena serves on
    last, _ = _call(solvers, inp, [2, 3, 1])
    for j, k in enumerate([2, 3, 1]):
        _same_bits(last[j], third[k])
    for s in solvers[1:]:
        s.close()
    assert qp.setup_groups_live() == live


def test_the_c_entry_refuses_before_anything_is_queued():
    from miosqp_amd import _lib, qp
    lib = _lib.load()
    shapes = [(10, 5, 2, 0), (20, 10, 5, 1), (12, 6, 3, 2)]
    models = [single.model(qp, problems.random_miqp(n, m, p, seed=s)) for n, m, p, s in shapes]
    solvers = [m.work.solver for m in models]
    roots = [(m.work.data.l, m.work.data.u, np.zeros(s.n), np.zeros(s.m)) for m, s in zip(models, solvers)]
    before = [s.solve_node(*r) for s, r in zip(solvers, roots)]
    from miosqp_amd import bnb
    good = [_polish_input(m, {}, dict(x=b.x, status=bnb.MI_SOLVED)) for m, b in zip(models, before)]

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
        infos, stats = (_lib.PolishRepairInfo * B)(), _lib.PolishModelsStats()
        rc = lib.miosqp_qp_polish_models(B, hs, ptrs(q), ptrs(l), ptrs(u), ptrs(x), ptrs(yv if y else [None] * B), tau,
                                         _lib.as_d(dl), _lib.as_i(ri), _lib.as_i(pi), ptrs(xo), ptrs(yo), None, infos,
                                         C.byref(stats))
        assert all(np.all(v == 7.0) for v in xo + yo) or rc == 0
        return rc, _lib.last_error()

    rc, err = run([0, 1, 0], good)
    assert rc == -1 and "model 0 is listed again as model 2" in err
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
    rc, err = run([0, 1, 2], good, tau=0.0, y=False)
    assert rc == -1 and "model 0" in err and "tau" in err
    for s, r, b in zip(solvers, roots, before):  # nothing was queued: the engines answer as before, bit for bit
        a = s.solve_node(*r)
        assert (a.status_val, a.iter) == (b.status_val, b.iter)
        np.testing.assert_array_equal(a.x, b.x)
        np.testing.assert_array_equal(a.y, b.y)
    rc, err = run([0, 1, 2], good)  # ... and the same call without a fault goes through
    assert rc == 0
    _close(models)


def test_end_to_end(twelve):
    import miosqp_amd
    t = twelve
    info = {}
    got = miosqp_amd.solve_models(t["models"], t["insts"], info=info, polish=True)
    assert info["polished"] == list(range(12)) and info["polish_own"] == {} and info["polish_launches"] == 1
    polished = 0
    for k, s in enumerate(TWELVE):
        copy = _build(s, _rule(k), t["rho"])[0]
        want = copy.solve_many([t["insts"][k]], polish=True)[0]
        copy.work.solver.close()
        assert set(got[k]) == set(want), k
        for key in want:
            if key == "run_time":  # (a wall-clock time)
                continue
            if isinstance(want[key], np.ndarray):
                np.testing.assert_array_equal(got[k][key], want[key], err_msg="%s of model %d" % (key, k))
            else:
                assert got[k][key] == want[key] or (want[key] != want[key] and got[k][key] != got[k][key]), (k, key)
        polished += bool(got[k]["polished"])
    assert polished >= 8
