"""MIOSQP.solve_many(lockstep="device") on the HIP engine (needs an MI355X): the lock-step trees driven inside the
library on device-resident leaves (miosqp_qp_solve_trees_lockstep) against the sequential calls (lockstep=False) and
the Python driver (lockstep=True).  random_miqp(100, 200, 50, seed 0) has n + M = 350 -- beyond the one-launch trees --
and about 80 nodes per tree; the seven instances are those of tests/test_gpu_lockstep_many.py, restated.  Every tree
must make the decisions of its sequential solve: status, nodes and ADMM iterations equal, the incumbent's value within
1e-9 relative (the heuristic's value is the device's sum), its integers exact."""
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


def _reference(rule, rho, lockstep, **st):
    """solve_many of the seven instances on a fresh model, once per session"""
    key = (rule, rho, lockstep, tuple(sorted(st.items())))
    if key not in _CACHE:
        pr = _problem()
        mdl = _model(pr, rule, rho, **st)
        _CACHE[key] = mdl.solve_many(_instances(pr), lockstep=lockstep)
        mdl.work.solver.close()
    return _CACHE[key]


def _same(got, want, ii, exact=False):
    from miosqp_amd import bnb
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        print("instance %d: device %s %d nodes %d iterations %.12g | reference %s %d %d %.12g"
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


def _call(mdl, inst, **kw):
    """the solver method itself on the instances' vectors"""
    data, st = mdl.work.data, mdl.work.settings
    Q, L, U, up, XI = _vectors(mdl, inst)
    B, M = len(inst), data.m + data.n_int
    return mdl.work.solver.solve_trees_lockstep(Q, L, U, np.zeros((B, data.n)), np.zeros((B, M)), up, XI,
                                                st["tree_explor_rule"], st["max_iter_bb"], **kw)


@pytest.mark.parametrize("rho", [0.1, "auto"])
@pytest.mark.parametrize("rule", [1, 3])
def test_device_driver_equals_the_sequential_and_the_python_driver(rule, rho):
    from miosqp_amd import bnb
    pr = _problem()
    inst = _instances(pr)
    seq, mdl = _model(pr, rule, rho), _model(pr, rule, rho)
    want = seq.solve_many(inst, lockstep=False)
    before = _state(mdl)
    got = mdl.solve_many(inst, lockstep="device")
    rec = mdl.work.lockstep
    assert rec["driver"] == "device" and rec["batched"] and rec["instances"] == len(inst)
    assert rec["nodes"] == sum(g["nodes"] for g in got) and rec["waves"] == max(g["nodes"] for g in got)
    assert len(rec["iters_max"]) == rec["waves"] and rec["max_width"] == len(inst)
    assert rec["finished_at"] == {k: g["nodes"] for k, g in enumerate(got)}  # one node per wave from the first wave on
    _assert_state(mdl, before)
    _same(got, want, pr["i_idx"])
    _same(got, _reference(rule, rho, True), pr["i_idx"])
    assert got[6]["status"] == bnb.MI_PRIMAL_INFEASIBLE and got[5]["upper_glob"] < np.inf
    assert sum(g["status"] == bnb.MI_SOLVED for g in got) >= 5
    # polish= keeps working on the result
    pol = mdl.solve_many(inst, lockstep="device", polish=True)
    assert all("polished" in p_ for p_ in pol)
    assert [(p_["status"], p_["nodes"], p_["osqp_iter"]) for p_ in pol] == [(g["status"], g["nodes"], g["osqp_iter"]) for g in got]
    _assert_state(mdl, before)
    # the model's own solve afterwards is what it is after the sequential path: the engine's q and root are the model's
    a, b = mdl.solve(), seq.solve()
    assert (a.status, mdl.work.iter_num, mdl.work.osqp_iter) == (b.status, seq.work.iter_num, seq.work.osqp_iter)
    assert abs(a.upper_glob - b.upper_glob) <= 1e-9 * max(1.0, abs(b.upper_glob))  # (the file's tolerance for device sums)
    for m_ in (seq, mdl):
        m_.work.solver.close()


@pytest.mark.parametrize("rule", [0, 2])
def test_slot_store_grows_from_eight_slots(rule):
    pr = _problem()
    inst = _instances(pr)
    mdl = _model(pr, rule, 0.1)
    x8, info8, st8 = _call(mdl, inst, capacity=8)
    print("rule %d: the store grew %d times from 8 slots, %d waves" % (rule, st8.grown, st8.waves))
    assert st8.grown > 1
    x0, info0, st0 = _call(mdl, inst)  # the default capacity
    for a, b in zip(info8, info0):
        assert (a.nodes, a.osqp_iter, a.found, a.upper_glob, a.leaves_left) == (b.nodes, b.osqp_iter, b.found, b.upper_glob, b.leaves_left)
        assert a.overflow == 0
    np.testing.assert_array_equal(x8, x0)
    assert (st8.waves, st8.nodes, st8.iters_all, st8.iters_slowest) == (st0.waves, st0.nodes, st0.iters_all, st0.iters_slowest)
    # ... and they are the sequential trees
    got = mdl.solve_many(inst, lockstep="device")
    assert [g["nodes"] for g in got] == [i.nodes for i in info0]
    _same(got, _reference(rule, 0.1, False), pr["i_idx"])
    mdl.work.solver.close()


def test_trees_stop_at_max_iter_bb():
    from miosqp_amd import bnb
    pr = _problem()
    inst = _instances(pr)
    mdl = _model(pr, 1, 0.1, max_iter_bb=12)
    got = mdl.solve_many(inst, lockstep="device")
    assert mdl.work.lockstep["driver"] == "device" and mdl.work.lockstep["waves"] == 11
    capped = [g for g in got if g["status"] in (bnb.MI_MAX_ITER_FEASIBLE, bnb.MI_MAX_ITER_UNSOLVED)]
    assert capped and all(g["nodes"] == 11 for g in capped)
    _same(got, _reference(1, 0.1, False, max_iter_bb=12), pr["i_idx"])
    mdl.work.solver.close()


def test_a_wave_wider_than_max_batch_runs_in_slices():
    """70 instances: 64 + 6 columns per wave under max_batch=64 (the default width is 64 as well), 70 columns in two
    tiles under max_batch=128.  A node is a pure function of (q, l, u, x0, y0): every tree is the same bit for bit
    however the wave is cut.  A slice of one tile is never compacted, so the compaction counter is read on the
    128-wide engine, where finished columns are swapped out of the first tile and the scatter finds its slots through
    c_node."""
    pr = _problem()
    inst = _seventy(pr)
    runs = {}
    for name, qp in (("64", dict(max_batch=64)), ("default", {}), ("128", dict(max_batch=128))):
        mdl = _model(pr, 1, 0.1, qp=qp)
        s = mdl.work.solver
        c0 = s._lib.miosqp_qp_debug_counter(s._h, 0)
        runs[name] = mdl.solve_many(inst, lockstep="device")
        rec = mdl.work.lockstep
        assert rec["max_width"] == 70 and rec["waves"] == max(g["nodes"] for g in runs[name])
        if name == "128":
            compactions = s._lib.miosqp_qp_debug_counter(s._h, 0) - c0
            print("compactions on the 128-wide engine: %d" % compactions)
            assert compactions > 0
        if name == "default":
            py = _model(pr, 1, 0.1)
            _same(runs[name], py.solve_many(inst, lockstep=True), pr["i_idx"])
            py.work.solver.close()
        s.close()
    _same(runs["64"], runs["default"], pr["i_idx"], exact=True)
    _same(runs["64"], runs["128"], pr["i_idx"], exact=True)


def test_rounded_point_is_judged_against_the_instances_root(monkeypatch):
    """c_hviol per node: for an instance whose root is the model's, kls_heur_rows must leave the bits kb_heur_rows
    leaves -- the Python driver's solve_batch_q goes through kb_heur_rows and its trees are the same node for node.  The
    instance with l, u of its own is judged by the host there (one product with A): its tree must be the same."""
    from miosqp_amd import lockstep
    pr = _problem()
    inst = _instances(pr)
    py, mdl = _model(pr, 1, 0.1), _model(pr, 1, 0.1)
    log = {k: [] for k in range(len(inst))}
    wave0 = lockstep._wave_batched

    def wave(solver, trees, live, leaves):
        r = wave0(solver, trees, live, leaves)
        for k, lf in zip(live, leaves):
            log[k].append(np.nan if lf.digest is None else lf.digest.info_viol)
        return r

    monkeypatch.setattr(lockstep, "_wave_batched", wave)
    want = py.solve_many(inst, lockstep=True)
    monkeypatch.undo()
    cap = max(len(v) for v in log.values())
    x, infos, st = _call(mdl, inst, node_hviol=cap)
    for k in (0, 1, 2, 3, 5):
        assert infos[k].nodes == len(log[k]) == want[k]["nodes"]
        np.testing.assert_array_equal(st.node_hviol[k, :len(log[k])], np.array(log[k]))
        assert np.sum(np.isfinite(st.node_hviol[k])) > 5
    assert (infos[4].nodes, infos[4].osqp_iter) == (want[4]["nodes"], want[4]["osqp_iter"]) and want[4]["nodes"] > 5
    assert abs(infos[4].upper_glob - want[4]["upper_glob"]) <= 1e-9 * max(1.0, abs(want[4]["upper_glob"]))
    # its violations are measured against other rows than the model root's: the values differ
    a4, b4 = st.node_hviol[4, :len(log[4])], np.array(log[4])
    both = np.isfinite(a4) & np.isfinite(b4)
    assert np.sum(both) > 5 and np.all(a4[both] != b4[both])
    for m_ in (py, mdl):
        m_.work.solver.close()


def _entry_call(s, entry, Q, L, U, up, XI, rule, max_iter_bb):
    """one of the five tree drivers on B x n / B x M vectors, each with settings under which its own step runs"""
    ct = int(s.settings.check_termination)
    zx, zy = np.zeros((len(Q), Q.shape[1])), np.zeros((len(Q), L.shape[1]))
    args = (Q, L, U, zx, zy, up, XI, rule, max_iter_bb)
    if entry == "lockstep":
        return s.solve_trees_lockstep(*args)
    if entry == "rf":  # K = 4 candidates at every fractional node
        return s.solve_trees_lockstep_rf(*args, 4, ct, 1)
    if entry == "sb":  # strong branching, K = 4
        return s.solve_trees_lockstep_sb(*args, 1, 4, ct, 4, 1e-6)
    if entry == "ahead":
        return s.solve_trees_lockstep_ahead(*args, 4)
    assert int(s.settings.max_iter) % ct == 0
    return s.solve_trees_refill(*args)


@pytest.mark.parametrize("entry", ["lockstep", "rf", "sb", "ahead", "refill"])
def test_a_branching_that_crosses_is_refused_and_leaves_no_trace(entry):
    """The error exit in the middle of a call.  Instance 1 gets [0.25, 0.75] at every integer position: its root
    relaxation is fractional wherever it branches and both children have l > u.  The call is refused from inside the
    first wave (chunk), after trees, slots and the driver's own lists have been written; the next call on the same
    engine must be the call of an engine that never saw the refusal, bit for bit."""
    pr = _problem()
    inst = _instances(pr)[:3]
    mdl, fresh = _model(pr, 1, 0.1), _model(pr, 1, 0.1)
    m = mdl.work.data.m
    Q, L, U, up, XI = _vectors(mdl, inst)
    Lb, Ub = L.copy(), U.copy()
    Lb[1, m:], Ub[1, m:] = 0.25, 0.75
    with pytest.raises(RuntimeError, match="branching produced l > u"):
        _entry_call(mdl.work.solver, entry, Q, Lb, Ub, up, XI, 1, 1000)
    got = _entry_call(mdl.work.solver, entry, Q, L, U, up, XI, 1, 1000)
    want = _entry_call(fresh.work.solver, entry, Q, L, U, up, XI, 1, 1000)
    for k, (g, w) in enumerate(zip(got[1], want[1])):
        print("%s, instance %d: %d nodes %d iterations %.12g, %d leaves left | fresh engine %d %d %.12g %d"
              % (entry, k, g.nodes, g.osqp_iter, g.upper_glob, g.leaves_left, w.nodes, w.osqp_iter, w.upper_glob, w.leaves_left))
    for k, (g, w) in enumerate(zip(got[1], want[1])):  # (found and leaves_left are what the status is made of)
        assert (g.found, g.leaves_left, g.nodes, g.osqp_iter, g.upper_glob) == (w.found, w.leaves_left, w.nodes, w.osqp_iter, w.upper_glob), k
        assert g.nodes > 5
    np.testing.assert_array_equal(got[0], want[0])
    for m_ in (mdl, fresh):
        m_.work.solver.close()


def test_edges_leave_the_engine_as_it_was():
    from miosqp_amd import bnb
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
        c = mdl.solve_many(inst[:3], lockstep=False)
        return a, b, c

    def same_probe(p, q):
        for r0, r1 in zip(p[:2], q[:2]):
            for key in ("x", "y", "status_val", "iter", "lower"):
                np.testing.assert_array_equal(getattr(r0, key), getattr(r1, key))
        for g, w in zip(p[2], q[2]):
            assert (g["status"], g["nodes"], g["osqp_iter"], g["upper_glob"]) == (w["status"], w["nodes"], w["osqp_iter"], w["upper_glob"])
            np.testing.assert_array_equal(g["x"], w["x"])

    # (the first sequential solve_many puts the model's q back through update_lin_cost, whose scaled q differs in the last
    #  bit from the one the set-up left: solve_batch reads it, so the engine is brought to that state before the reference)
    probe()
    before = probe()
    state = _state(mdl)
    # B = 1
    one = mdl.solve_many(inst[:1], lockstep="device")
    assert mdl.work.lockstep["max_width"] == 1 and mdl.work.lockstep["waves"] == one[0]["nodes"]
    _same(one, before[2][:1], pr["i_idx"])
    same_probe(probe(), before)
    # max_iter_bb = 1: nothing to do
    keep = mdl.work.settings["max_iter_bb"]
    mdl.work.settings["max_iter_bb"] = 1
    x, infos, st = _call(mdl, inst)
    got = mdl.solve_many(inst, lockstep="device")
    mdl.work.settings["max_iter_bb"] = keep
    assert st.waves == 0 and st.nodes == 0 and st.finished_at == [0] * len(inst)
    assert all(i.nodes == 0 and i.osqp_iter == 0 and i.leaves_left == 1 for i in infos)
    assert all(g["nodes"] == 0 for g in got) and set(mdl.work.lockstep["finished_at"].values()) == {0}
    assert got[5]["status"] == bnb.MI_MAX_ITER_FEASIBLE and got[0]["status"] == bnb.MI_MAX_ITER_UNSOLVED
    same_probe(probe(), before)
    # a root with l > u in one instance: refused before anything is queued
    Lb = L.copy()
    Lb[2, 7] = U[2, 7] + 1.0
    with pytest.raises(ValueError):
        s.solve_trees_lockstep(Q, Lb, U, np.zeros((len(inst), N)), np.zeros((len(inst), M)), up, XI, 1, keep)
    same_probe(probe(), before)
    _assert_state(mdl, state)
    s.close()
