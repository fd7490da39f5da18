"""MIOSQP.solve_many(lockstep="refill") on the HIP engine (needs an MI355X): the lock-step trees on columns that are
refilled between chunks (miosqp_qp_solve_trees_refill) against the sequential calls (lockstep=False) and the wave driver
in the library (lockstep="device").  random_miqp(100, 200, 50, seed 0) has n + M = 350 and about 80 nodes per tree; the
seven instances are those of tests/test_gpu_lockstep_device.py, restated.  A tree has one node in flight at the most,
so every tree must make the decisions of its sequential solve -- status, nodes and ADMM iterations equal, the
incumbent's value within 1e-9 relative (the heuristic's value is the device's sum), its integers exact -- and, the sums
being the wave driver's device sums, upper_glob and x must equal those of lockstep="device" bit for bit."""
import numpy as np
import pytest

from miosqp_amd import problems

pytestmark = pytest.mark.gpu

N, M_, P_ = 100, 200, 50
_CACHE = {}


def _problem():
    if "pr" not in _CACHE:
        _CACHE["pr"] = problems.random_miqp(N, M_, P_, seed=0)
    return _CACHE["pr"]


def _model(pr, rule, rho, qp=None, **st):
    from miosqp_amd import bnb
    mdl = bnb.MIOSQP()
    mdl.setup(pr["P"], pr["q"], pr["A"], pr["l"].copy(), pr["u"].copy(), pr["i_idx"], pr["i_l"], pr["i_u"],
              dict(problems.BNB_SETTINGS, tree_explor_rule=rule, **st), dict(problems.QP_SETTINGS, rho=rho, **(qp or {})))
    return mdl


def _instances(pr):
    """four with their own q, one with its own l, u, one with an x0 that passes set_x0, one infeasible by its bounds
    (200 alternating equalities on 100 variables)"""
    rng = np.random.RandomState(3)
    inst = [dict(q=pr["q"] + 0.3 * rng.randn(N)) for _ in range(4)]
    inst.append(dict(l=pr["l"] - 0.5 * rng.rand(M_), u=pr["u"] - 0.5 * rng.rand(M_)))
    x0 = np.zeros(N)
    x0[pr["i_idx"][0]] = 1.0  # A has entries in [0, 1): 0 <= A x0 < 1 lies inside [l, u]
    inst.append(dict(x0=x0))
    b = 50.0 * (1 - 2 * (np.arange(M_) % 2))
    inst.append(dict(l=b, u=b.copy()))
    return inst


def _seventy(pr):
    """the seven recipes x 10 cost perturbations from a fixed seed"""
    rng = np.random.RandomState(17)
    out = []
    for _ in range(10):
        for rec in _instances(pr):
            it = dict(rec)
            it["q"] = np.asarray(rec.get("q", pr["q"]), dtype=float) + 0.05 * rng.randn(N)
            out.append(it)
    return out


def _reference(rule, rho, lockstep, which="seven", qp=None, **st):
    """solve_many of the seven (or the seventy) instances on a fresh model, once per session; with the run's record"""
    key = (rule, rho, lockstep, which, tuple(sorted((qp or {}).items())), tuple(sorted(st.items())))
    if key not in _CACHE:
        pr = _problem()
        mdl = _model(pr, rule, rho, qp=qp, **st)
        inst = _instances(pr) if which == "seven" else _seventy(pr)
        got = mdl.solve_many(inst, lockstep=lockstep)
        _CACHE[key] = (got, dict(getattr(mdl.work, "lockstep", {})) if lockstep else {})
        mdl.work.solver.close()
    return _CACHE[key]


def _same(got, want, ii, exact=False):
    from miosqp_amd import bnb
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        print("instance %d: refill %s %d nodes %d iterations %.17g | reference %s %d %d %.17g"
              % (k, g["status"], g["nodes"], g["osqp_iter"], g["upper_glob"], w["status"], w["nodes"], w["osqp_iter"],
                 w["upper_glob"]))
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g["status"], g["nodes"], g["osqp_iter"]) == (w["status"], w["nodes"], w["osqp_iter"]), k
        if w["status"] in (bnb.MI_SOLVED, bnb.MI_MAX_ITER_FEASIBLE):
            if exact:
                assert g["upper_glob"] == w["upper_glob"], k
                np.testing.assert_array_equal(g["x"], w["x"])
            else:
                assert abs(g["upper_glob"] - w["upper_glob"]) <= 1e-9 * max(1.0, abs(w["upper_glob"])), k
                np.testing.assert_array_equal(g["x"][ii], w["x"][ii])
        else:
            assert g["upper_glob"] == w["upper_glob"], k


def _state(mdl):
    w = mdl.work
    return dict(q=w.data.q.copy(), l=w.data.l.copy(), u=w.data.u.copy(), leaves=list(w.leaves), iter_num=w.iter_num,
                osqp_iter=w.osqp_iter, upper_glob=w.upper_glob, lower_glob=w.lower_glob, status=w.status,
                first_run=w.first_run)


def _assert_state(mdl, s):
    w = mdl.work
    for key in ("q", "l", "u"):
        np.testing.assert_array_equal(getattr(w.data, key), s[key])
    assert len(w.leaves) == len(s["leaves"]) and all(a is b for a, b in zip(w.leaves, s["leaves"]))
    for key in ("iter_num", "osqp_iter", "upper_glob", "lower_glob", "status", "first_run"):
        assert getattr(w, key) == s[key], key


def _vectors(mdl, inst):
    """what solve_many hands the drivers: Q, L, U instance-major, the value and point of an accepted x0"""
    data = mdl.work.data
    Q, L, U = mdl._instance_vectors(inst)
    up, XI = np.full(len(inst), np.inf), np.zeros((len(inst), data.n))
    for k, it in enumerate(inst):
        if it.get("x0") is not None:
            x0 = np.asarray(it["x0"], dtype=float)
            up[k] = .5 * np.dot(x0, data.P.dot(x0)) + np.dot(Q[k], x0)
            XI[k] = x0
    return Q, L, U, up, XI


def _call(mdl, inst, entry="solve_trees_refill", **kw):
    """the solver method itself on the instances' vectors"""
    data, st = mdl.work.data, mdl.work.settings
    Q, L, U, up, XI = _vectors(mdl, inst)
    B, M = len(inst), data.m + data.n_int
    return getattr(mdl.work.solver, entry)(Q, L, U, np.zeros((B, data.n)), np.zeros((B, M)), up, XI,
                                           st["tree_explor_rule"], st["max_iter_bb"], **kw)


def _check_of(mdl):
    return int(mdl.work.solver.settings.check_termination)


@pytest.mark.parametrize("rho", [0.1, "auto"])
@pytest.mark.parametrize("rule", [1, 3])
def test_refill_equals_the_sequential_path_and_the_wave_driver(rule, rho):
    from miosqp_amd import bnb
    pr = _problem()
    inst = _instances(pr)
    seq, mdl = _model(pr, rule, rho), _model(pr, rule, rho)
    want = seq.solve_many(inst, lockstep=False)
    before = _state(mdl)
    got = mdl.solve_many(inst, lockstep="refill")
    rec = mdl.work.lockstep
    assert rec["driver"] == "refill" and rec["batched"] and rec["instances"] == len(inst) and rec["columns"] == len(inst)
    assert rec["nodes"] == sum(g["nodes"] for g in got) and rec["iters_all"] == sum(g["osqp_iter"] for g in got)
    assert 0.0 < rec["occupancy"] <= 1.0 and len(rec["chunk_busy"]) == rec["chunks"]
    _assert_state(mdl, before)
    _same(got, want, pr["i_idx"])
    _same(got, _reference(rule, rho, "device")[0], pr["i_idx"], exact=True)
    assert got[6]["status"] == bnb.MI_PRIMAL_INFEASIBLE and got[5]["upper_glob"] < np.inf
    assert got[5]["upper_glob"] <= _vectors(mdl, inst)[3][5]  # instance 5 keeps its x0's bound
    assert sum(g["status"] == bnb.MI_SOLVED for g in got) >= 5
    # polish= keeps working on the result
    pol = mdl.solve_many(inst, lockstep="refill", polish=True)
    assert all("polished" in p_ for p_ in pol)
    assert [(p_["status"], p_["nodes"], p_["osqp_iter"]) for p_ in pol] == [(g["status"], g["nodes"], g["osqp_iter"]) for g in got]
    _assert_state(mdl, before)
    # the model's own solve afterwards is what it is after the sequential path: the engine's q and root are the model's
    a, b = mdl.solve(), seq.solve()
    assert (a.status, mdl.work.iter_num, mdl.work.osqp_iter) == (b.status, seq.work.iter_num, seq.work.osqp_iter)
    assert abs(a.upper_glob - b.upper_glob) <= 1e-9 * max(1.0, abs(b.upper_glob))  # (the file's tolerance for device sums)
    for m_ in (seq, mdl):
        m_.work.solver.close()


@pytest.mark.parametrize("rule,rho", [(1, 0.1), (3, "auto")])
def test_no_chunk_is_idle_while_every_tree_has_a_column(rule, rho):
    """B <= columns: every node's iteration count is a multiple of check_termination and a tree's nodes run back to
    back in its column, so the call takes exactly as many chunks as its longest tree has iterations / check_termination.
    A driver that waits for waves takes iters_slowest / check_termination, which is more (the trees differ in length)."""
    pr = _problem()
    inst = _instances(pr)
    mdl = _model(pr, rule, rho)
    got = mdl.solve_many(inst, lockstep="refill")
    rec = mdl.work.lockstep
    ct = _check_of(mdl)
    mdl.work.solver.close()
    assert all(g["osqp_iter"] % ct == 0 for g in got)
    longest = max(g["osqp_iter"] for g in got) // ct
    dev = _reference(rule, rho, "device")[1]
    print("chunks %d, longest tree %d chunks, the wave driver %d chunks, occupancy %.3f"
          % (rec["chunks"], longest, dev["iters_slowest"] // ct, rec["occupancy"]))
    assert rec["chunks"] == longest
    assert rec["chunks"] < dev["iters_slowest"] // ct
    assert rec["finished_at"] == {k: g["osqp_iter"] // ct for k, g in enumerate(got)}
    assert rec["chunk_busy"][0] == len(inst) and rec["chunk_busy"][-1] >= 1


def test_more_trees_than_columns():
    """70 trees on 64 columns (max_batch=64 and the default width) and on two tiles, the second partly filled
    (max_batch=128): a node is a pure function of (q, l, u, x0, y0), every tree is the same bit for bit wherever and
    whenever its nodes ran"""
    pr = _problem()
    inst = _seventy(pr)
    runs = {}
    for name, qp, cols in (("64", dict(max_batch=64), 64), ("default", {}, 64), ("128", dict(max_batch=128), 70)):
        mdl = _model(pr, 1, 0.1, qp=qp)
        runs[name] = mdl.solve_many(inst, lockstep="refill")
        rec = mdl.work.lockstep
        print("max_batch %s: %d columns, %d chunks, occupancy %.3f" % (name, rec["columns"], rec["chunks"], rec["occupancy"]))
        assert rec["columns"] == cols and rec["instances"] == 70
        assert 0.0 < rec["occupancy"] <= 1.0
        assert all(0 < f <= rec["chunks"] for f in rec["finished_at"].values())
        assert max(rec["chunk_busy"]) == cols and rec["nodes"] == sum(g["nodes"] for g in runs[name])
        mdl.work.solver.close()
    _same(runs["64"], runs["default"], pr["i_idx"], exact=True)
    _same(runs["64"], runs["128"], pr["i_idx"], exact=True)
    _same(runs["64"], _reference(1, 0.1, "device", which="seventy")[0], pr["i_idx"], exact=True)


@pytest.mark.parametrize("B", [1, 2])
def test_one_and_two_trees(B):
    """the same column is refilled by the same tree every time"""
    pr = _problem()
    inst = _instances(pr)[:B]
    mdl, dev = _model(pr, 1, 0.1), _model(pr, 1, 0.1)
    got = mdl.solve_many(inst, lockstep="refill")
    rec = mdl.work.lockstep
    assert rec["columns"] == B and rec["chunks"] == max(g["osqp_iter"] for g in got) // _check_of(mdl)
    _same(got, dev.solve_many(inst, lockstep="device"), pr["i_idx"], exact=True)
    for m_ in (mdl, dev):
        m_.work.solver.close()


def test_a_column_reaches_max_iter_on_its_own():
    from miosqp_amd import bnb
    pr = _problem()
    inst = _instances(pr)
    qp = dict(max_iter=50, check_termination=25)
    mdl = _model(pr, 1, 0.1, qp=qp)
    x, infos, st = _call(mdl, inst)
    got = mdl.solve_many(inst, lockstep="refill")
    # nodes that stop at the limit stop at exactly 50 iterations whatever chunk they were loaded in: every node ran 25 or 50
    for i, g in zip(infos, got):
        assert (i.nodes, i.osqp_iter) == (g["nodes"], g["osqp_iter"])
        assert 25 * i.nodes <= i.osqp_iter <= 50 * i.nodes
    at_limit = sum((i.osqp_iter - 25 * i.nodes) // 25 for i in infos)
    print("nodes that ran to max_iter = 50: %d of %d" % (at_limit, sum(i.nodes for i in infos)))
    assert at_limit > 20
    # ... and the columns' own statuses: many nodes ended MAX_ITER_REACHED, each of them at exactly max_iter = 50 (no column
    # can count more than 50, so the sum says it of every one); a node that ran 50 iterations either hit the limit or was
    # decided by its second test
    print("nodes that ended MAX_ITER_REACHED: %d, their iterations: %d" % (st.nodes_max_iter, st.iters_max_iter))
    assert 20 < st.nodes_max_iter <= at_limit and st.iters_max_iter == 50 * st.nodes_max_iter
    _same(got, _reference(1, 0.1, False, qp=qp)[0], pr["i_idx"])
    _same(got, _reference(1, 0.1, "device", qp=qp)[0], pr["i_idx"], exact=True)
    mdl.work.solver.close()
    bad = _model(pr, 1, 0.1, qp=dict(max_iter=60, check_termination=25))
    with pytest.raises(ValueError, match="multiple of check_termination"):
        bad.solve_many(inst, lockstep="refill")
    with pytest.raises(ValueError, match="multiple of check_termination"):
        _call(bad, inst)
    assert bad.solve_many(inst[:1], lockstep=False)[0]["status"] in (bnb.MI_SOLVED, bnb.MI_MAX_ITER_FEASIBLE,
                                                                     bnb.MI_MAX_ITER_UNSOLVED, bnb.MI_PRIMAL_INFEASIBLE)
    bad.work.solver.close()


def test_trees_stop_at_max_iter_bb():
    from miosqp_amd import bnb
    pr = _problem()
    inst = _instances(pr)
    mdl = _model(pr, 1, 0.1, max_iter_bb=12)
    got = mdl.solve_many(inst, lockstep="refill")
    assert mdl.work.lockstep["driver"] == "refill"
    want = _reference(1, 0.1, False, max_iter_bb=12)[0]
    capped = [g for g in got if g["status"] in (bnb.MI_MAX_ITER_FEASIBLE, bnb.MI_MAX_ITER_UNSOLVED)]
    assert capped and all(g["nodes"] == 11 for g in capped)
    assert [g["nodes"] for g in got] == [w["nodes"] for w in want] and 11 in [w["nodes"] for w in want]
    _same(got, want, pr["i_idx"])
    _same(got, _reference(1, 0.1, "device", max_iter_bb=12)[0], pr["i_idx"], exact=True)
    mdl.work.solver.close()


@pytest.mark.parametrize("rule", [0, 2])
def test_slot_store_grows_from_eight_slots(rule):
    pr = _problem()
    inst = _instances(pr)
    mdl = _model(pr, rule, 0.1)
    x8, info8, st8 = _call(mdl, inst, capacity=8)
    print("rule %d: the store grew %d times from 8 slots, %d chunks" % (rule, st8.grown, st8.chunks))
    assert st8.grown > 0
    xd, infod, std_ = _call(mdl, inst, entry="solve_trees_lockstep")
    for a, b in zip(info8, infod):
        assert (a.nodes, a.osqp_iter, a.found, a.upper_glob, a.leaves_left) == (b.nodes, b.osqp_iter, b.found, b.upper_glob, b.leaves_left)
        assert a.overflow == 0
    np.testing.assert_array_equal(x8, xd)
    got = mdl.solve_many(inst, lockstep="refill")
    _same(got, _reference(rule, 0.1, "device")[0], pr["i_idx"], exact=True)
    _same(got, _reference(rule, 0.1, False)[0], pr["i_idx"])
    mdl.work.solver.close()


def test_the_engine_is_left_as_it_was():
    pr = _problem()
    inst = _instances(pr)
    mdl = _model(pr, 1, 0.1)
    s, data = mdl.work.solver, mdl.work.data
    Q, L, U, up, XI = _vectors(mdl, inst)
    M = data.m + data.n_int
    rng = np.random.RandomState(5)
    xw, yw = 0.1 * rng.randn(3, N), 0.1 * rng.randn(3, M)

    def probe():
        a = s.solve_batch(L[:3], U[:3], xw, yw)
        b = s.solve_batch_q(Q[:3], L[:3], U[:3], xw, yw)
        c = _call(mdl, inst[:3], entry="solve_trees_lockstep")
        d = s.solve_node(L[0], U[0], xw[0], yw[0]) if hasattr(s, "solve_node") else None
        return a, b, c, d

    def same_probe(p, q):
        for r0, r1 in zip(p[:2], q[:2]):
            for key in ("x", "y", "status_val", "iter", "lower"):
                np.testing.assert_array_equal(getattr(r0, key), getattr(r1, key))
        np.testing.assert_array_equal(p[2][0], q[2][0])
        for a, b in zip(p[2][1], q[2][1]):
            assert (a.nodes, a.osqp_iter, a.found, a.upper_glob, a.leaves_left) == (b.nodes, b.osqp_iter, b.found, b.upper_glob, b.leaves_left)
        if p[3] is not None:
            for key in ("x", "y"):
                np.testing.assert_array_equal(getattr(p[3], key), getattr(q[3], key))
            assert (p[3].info.status_val, p[3].info.iter) == (q[3].info.status_val, q[3].info.iter)

    probe()
    before = probe()
    state = _state(mdl)
    got = mdl.solve_many(inst, lockstep="refill")
    assert len(got) == len(inst)
    same_probe(probe(), before)
    # B = 0 never reaches the library
    assert mdl.solve_many([], lockstep="refill") == []
    with pytest.raises(ValueError):
        s.solve_trees_refill(Q[:0], L[:0], U[:0], np.zeros((0, N)), np.zeros((0, M)), up[:0], None, 1, 100)
    same_probe(probe(), before)
    # a root with l > u in one instance: refused before anything is queued
    Lb = L.copy()
    Lb[2, 7] = U[2, 7] + 1.0
    with pytest.raises(ValueError):
        s.solve_trees_refill(Q, Lb, U, np.zeros((len(inst), N)), np.zeros((len(inst), M)), up, XI, 1, 100)
    same_probe(probe(), before)
    # max_iter_bb = 1: nothing to do, no chunk runs
    x, infos, st = s.solve_trees_refill(Q, L, U, np.zeros((len(inst), N)), np.zeros((len(inst), M)), up, XI, 1, 1)
    assert st.chunks == 0 and st.nodes == 0 and st.finished_at == [0] * len(inst)
    assert all(i.nodes == 0 and i.osqp_iter == 0 and i.leaves_left == 1 for i in infos)
    same_probe(probe(), before)
    _assert_state(mdl, state)
    s.close()


def test_chunks_as_one_persistent_launch_at_config_2(monkeypatch):
    """n = 500: the chunk's iterations as the persistent whole-chip launch (MIOSQP_KBP_MIN_COLS=1 takes it below its
    automatic range of 192 columns), held by this driver's own chunk graph.  Eight trees cut at eleven nodes: refill equals
    the wave driver bit for bit and the sequential path in its counts.  Then with a workgroup that never shows up (the
    fault injection of test_batched_persistent_chunks_equal_the_launches; the flag is read when the batch arrays are
    made, at the first batched call): the first chunk's launch is called off within 100 ms, nothing was modified and
    nothing harvested, the engine goes on with the launches and the chunk is run again -- the same trees, the same bits."""
    from miosqp_amd import bnb
    cfg = problems.CONFIGS["cfg2"]
    pr = problems.random_miqp(**cfg, seed=0)
    rng = np.random.RandomState(12345)
    inst = [dict(q=rng.randn(cfg["n"]), l=-2 + rng.rand(cfg["m"]), u=2 + rng.rand(cfg["m"])) for _ in range(8)]
    monkeypatch.setenv("MIOSQP_KBP_MIN_COLS", "1")
    mdl = _model(pr, 1, 0.1, max_iter_bb=12)
    eng = mdl.work.solver
    got = mdl.solve_many(inst, lockstep="refill")
    rec = mdl.work.lockstep
    assert eng.factor_stats()["batch_pers"] and eng.batch_pers_fallbacks() == 0
    assert rec["driver"] == "refill" and rec["columns"] == 8 and rec["nodes"] == 88
    assert rec["chunks"] == max(g["osqp_iter"] for g in got) // _check_of(mdl)
    _same(got, mdl.solve_many(inst, lockstep="device"), pr["i_idx"], exact=True)
    _same(got[:2], mdl.solve_many(inst[:2], lockstep=False), pr["i_idx"])
    assert all(g["status"] in (bnb.MI_MAX_ITER_FEASIBLE, bnb.MI_MAX_ITER_UNSOLVED) for g in got)
    eng.close()
    # one workgroup missing in the first chunk
    bad = _model(pr, 1, 0.1, max_iter_bb=12)
    monkeypatch.setenv("MIOSQP_COOP_DBG", "64")
    off = bad.solve_many(inst, lockstep="refill")
    monkeypatch.delenv("MIOSQP_COOP_DBG")
    # (exactly one call-off, in the batched chunk: the switch was read after setup() and before the first batched call --
    #  set earlier it would call off the set-up's cooperative launch instead, set later it is never read, and both show here)
    assert bad.work.solver.batch_pers_fallbacks() == 1 and not bad.work.solver.factor_stats()["batch_pers"]
    assert bad.work.solver.factor_stats()["coop_fallbacks"] == 0
    assert bad.work.lockstep["chunks"] == rec["chunks"]  # (the called-off chunk is not counted: it iterated nothing)
    _same(off, got, pr["i_idx"], exact=True)
    bad.work.solver.close()
