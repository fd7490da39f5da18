"""MIOSQP.solve_many(lockstep="ahead") on the HIP engine (needs an MI355X): the lock-step trees whose spare columns solve
open leaves early (miosqp_qp_solve_trees_lockstep_ahead) against lockstep="device" and the sequential calls.  The
workload is that of tests/test_gpu_lockstep_device.py -- random_miqp(100, 200, 50, seed 0), n + M = 350, its seven
instances (own q, own l / u, an accepted x0, an infeasible one) and an eighth with its own q.  "ahead" runs the kernels
of "device" on the same inputs, so every field of every result must be EQUAL, floats bit for bit; only the number of
waves may differ."""
import numpy as np
import pytest

import test_gpu_lockstep_device as dev

pytestmark = pytest.mark.gpu

N = dev.N
FIELDS = ("nodes", "osqp_iter", "upper_glob", "lower_glob", "leaves_left", "max_leaves", "found", "overflow")
_CACHE = {}


def _eight(pr):
    rng = np.random.RandomState(29)
    return dev._instances(pr) + [dict(q=pr["q"] + 0.3 * rng.randn(N))]


def _seventy(pr):
    """the seventy instances of the device driver's file with ONE infeasible instance instead of ten (the other nine keep
    their cost and lose their bounds): an infeasible tree closes at its root, and the second slice of a wave under
    max_batch = 64 has mandatory columns only while more than 64 trees are alive"""
    out = dev._seventy(pr)
    for k in range(13, 70, 7):
        out[k] = dict(q=out[k]["q"])
    return out


def _pick(inst, B):
    """B = 1: an instance with its own q; B = 3: own l / u, the accepted x0, the infeasible one; B = 8: all"""
    return {1: inst[:1], 3: inst[4:7], 8: inst}[B]


def _device(mdl, inst, **kw):
    return dev._call(mdl, inst, **kw)


def _ahead(mdl, inst, ahead, **kw):
    data, st = mdl.work.data, mdl.work.settings
    Q, L, U, up, XI = dev._vectors(mdl, inst)
    B, M = len(inst), data.m + data.n_int
    return mdl.work.solver.solve_trees_lockstep_ahead(Q, L, U, np.zeros((B, data.n)), np.zeros((B, M)), up, XI,
                                                      st["tree_explor_rule"], st["max_iter_bb"], ahead, **kw)


def _equal(got, want):
    """(x, infos) of two drivers: every field equal, floats bit for bit"""
    (xg, ig), (xw, iw) = got, want
    assert len(ig) == len(iw)
    for k, (a, b) in enumerate(zip(ig, iw)):
        for f in FIELDS:
            va, vb = getattr(a, f), getattr(b, f)
            assert va == vb or (isinstance(va, float) and np.isnan(va) and np.isnan(vb)), (k, f, va, vb)
    np.testing.assert_array_equal(xg, xw)


def _sequential(rule, rho):
    key = (rule, rho)
    if key not in _CACHE:
        pr = dev._problem()
        mdl = dev._model(pr, rule, rho)
        _CACHE[key] = mdl.solve_many(_eight(pr), lockstep=False)
        mdl.work.solver.close()
    return _CACHE[key]


@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("rule,rho", [(1, 0.1), (1, "auto"), (3, 0.1), (3, "auto"), (0, 0.1), (2, 0.1)])
def test_ahead_equals_the_device_driver(rule, rho, B):
    pr = dev._problem()
    inst = _pick(_eight(pr), B)
    mdl = dev._model(pr, rule, rho)
    xd, infd, sd = _device(mdl, inst)
    for ahead in (2, 8):
        xa, infa, sa, a = _ahead(mdl, inst, ahead)
        print("rule %s rho %s B %d ahead %d: %d waves (device %d), sent %d hits %d discarded %d called off %d"
              % (rule, rho, B, ahead, sa.waves, sd.waves, a.sent, a.hits, a.discarded, a.called_off))
        _equal((xa, infa), (xd, infd))
        assert sa.waves <= sd.waves and sa.nodes == sd.nodes and sa.iters_all == sd.iters_all
        assert a.sent == a.hits + a.discarded + a.called_off and a.columns == sd.nodes + a.discarded + a.called_off
        assert all(w <= 64 for w in a.width)  # never a tile "device" would not launch
        if all(i.leaves_left == 0 for i in infa):
            assert a.free_slots == a.slot_cap  # every slot came back
    if B == 8:
        # ... and through solve_many: the dicts of "device" bit for bit, status, nodes and iterations of the sequential path
        got = mdl.solve_many(inst, lockstep="ahead", ahead=8)
        rec = mdl.work.lockstep
        assert rec["driver"] == "ahead" and rec["ahead"]["ahead"] == 8 and rec["instances"] == 8
        assert rec["nodes"] == sum(g["nodes"] for g in got)
        dev._same(got, mdl.solve_many(inst, lockstep="device"), pr["i_idx"], exact=True)
        want = _sequential(rule, rho)
        assert [(g["status"], g["nodes"], g["osqp_iter"]) for g in got] == [(w["status"], w["nodes"], w["osqp_iter"]) for w in want]
    mdl.work.solver.close()


def test_ahead_one_is_the_device_driver():
    pr = dev._problem()
    inst = _pick(_eight(pr), 3)
    mdl = dev._model(pr, 1, 0.1)
    xd, infd, sd = _device(mdl, inst)
    xa, infa, sa, a = _ahead(mdl, inst, 1)
    _equal((xa, infa), (xd, infd))
    assert (sa.waves, sa.nodes, sa.iters_all, sa.iters_slowest, sa.width, sa.iters_max) == \
        (sd.waves, sd.nodes, sd.iters_all, sd.iters_slowest, sd.width, sd.iters_max)
    assert (a.sent, a.hits, a.discarded, a.called_off) == (0, 0, 0, 0) and a.columns == sd.nodes and a.width == sd.width
    mdl.work.solver.close()


@pytest.mark.parametrize("rho", [0.1, "auto"])
def test_a_wave_ends_with_its_mandatory_columns(rho):
    """B = 1: every node is absorbed behind its own wave or as a hit.  Every wave runs exactly the chunks its mandatory
    columns need, ceil(largest mandatory iteration count / check_termination).  The tail at max_iter (max_iter %
    check_termination iterations behind the last full chunk) is counted as one chunk, so a mandatory column that reaches
    max_iter gives ceil(max_iter / check_termination) on both sides and the equality holds there too."""
    pr = dev._problem()
    mdl = dev._model(pr, 1, rho)
    ct = int(mdl.work.solver.settings.check_termination)
    for B in (1, 8):
        inst = _pick(_eight(pr), B)
        x, infos, s, a = _ahead(mdl, inst, 8)
        print("rho %s B %d: %d nodes in %d waves, %d hits; chunks %s" % (rho, B, s.nodes, s.waves, a.hits, a.chunks[:12]))
        if B == 1:
            assert infos[0].nodes == s.waves + a.hits and a.hits > 0
        assert len(a.chunks) == s.waves == len(a.iter_mandatory)
        assert a.chunks == [-(-it // ct) for it in a.iter_mandatory]
        assert a.iter_mandatory == s.iters_max
    mdl.work.solver.close()


def test_ahead_columns_in_a_sliced_wave():
    """70 instances, 69 of them alive after the first wave: under max_batch = 64 (the default width as well) the mandatory
    columns are cut 64 + 5 and the second slice's tile has 59 free columns; under max_batch = 128 one slice of two tiles
    has them.  The same bits however the wave is cut, and those of "device"."""
    pr = dev._problem()
    inst = _seventy(pr)
    runs = {}
    for name, qp in (("64", dict(max_batch=64)), ("default", {}), ("128", dict(max_batch=128))):
        mdl = dev._model(pr, 1, 0.1, qp=qp)
        runs[name] = _ahead(mdl, inst, 8)
        a = runs[name][3]
        print("max_batch %s: %d waves, widest %d, sent %d hits %d" % (name, a.waves, max(a.width), a.sent, a.hits))
        # the second wave: at most 70 mandatory columns and every tree's other child to send -- two full tiles, so at
        # least 58 ahead columns, which under max_batch = 64 sit in the second slice behind its mandatory columns
        assert a.width[0] == 70 and a.width[1] == 128 and max(a.width) == 128 and a.sent > 0 and a.hits > 0
        if name == "default":
            runs["device"] = _device(mdl, inst)
        mdl.work.solver.close()
    for name in ("64", "default", "128"):
        _equal(runs[name][:2], runs["device"][:2])
    # (the widths need not agree: under max_batch = 64 the second slice ends with ITS six mandatory columns, so other ahead
    #  columns are called off than under 128, where one slice waits for all seventy)
    assert runs["64"][3].width == runs["default"][3].width


@pytest.mark.parametrize("rule", [0, 2])
def test_slot_store_grows_from_eight_slots(rule):
    pr = dev._problem()
    inst = _eight(pr)
    mdl = dev._model(pr, rule, 0.1)
    xd, infd, sd = _device(mdl, inst)
    xa, infa, sa, a = _ahead(mdl, inst, 8, capacity=8)
    print("rule %d: the store grew %d times from 8 slots, %d waves, %d hits" % (rule, sa.grown, sa.waves, a.hits))
    assert sa.grown > 1 and a.hits > 0
    _equal((xa, infa), (xd, infd))
    assert a.free_slots == a.slot_cap or any(i.leaves_left for i in infa)
    mdl.work.solver.close()


def test_trees_stop_at_max_iter_bb():
    pr = dev._problem()
    inst = _eight(pr)
    mdl = dev._model(pr, 1, 0.1, max_iter_bb=12)
    xd, infd, sd = _device(mdl, inst)
    assert sd.waves == 11 and any(i.leaves_left > 0 for i in infd)
    for ahead in (2, 8):
        xa, infa, sa, a = _ahead(mdl, inst, ahead)
        _equal((xa, infa), (xd, infd))
        assert sa.waves <= 11 and max(i.nodes for i in infa) == 11
        # the open leaves and the parents their warm starts need are all that is not free: nothing reserved is left
        assert a.slot_cap - a.free_slots >= sum(i.leaves_left for i in infa)
    mdl.work.solver.close()


def test_refusals_leave_the_engine_as_it_was():
    from miosqp_amd import bnb
    pr = dev._problem()
    inst = _eight(pr)[:3]
    mdl = dev._model(pr, 1, 0.1)
    s, data = mdl.work.solver, mdl.work.data
    Q, L, U, up, XI = dev._vectors(mdl, inst)
    M = data.m + data.n_int
    rng = np.random.RandomState(5)
    xw, yw = 0.1 * rng.randn(3, N), 0.1 * rng.randn(3, M)

    def probe():
        a = s.solve_batch(L, U, xw, yw)
        b = mdl.solve_many(inst, lockstep="device")
        return a, b

    def same_probe(p, q):
        for key in ("x", "y", "status_val", "iter", "lower"):
            np.testing.assert_array_equal(getattr(p[0], key), getattr(q[0], key))
        dev._same(p[1], q[1], pr["i_idx"], exact=True)

    mdl.solve_many(inst, lockstep=False)  # (brings the engine's q to what update_lin_cost leaves: see the device driver's test)
    before = probe()
    state = dev._state(mdl)
    for bad in (0, -3, 2.5, True, None, "8"):
        with pytest.raises(ValueError, match="ahead"):
            mdl.solve_many(inst, lockstep="ahead", ahead=bad)
    with pytest.raises(ValueError, match="ahead must be at least 1"):
        _ahead(mdl, inst, 0)
    assert not hasattr(mdl.work, "lockstep") or mdl.work.lockstep["driver"] == "device"
    for more in (dict(primal_heuristic=1), dict(branching_rule=1)):
        other = dev._model(pr, 1, 0.1, **more)
        with pytest.raises(ValueError, match='lockstep="ahead"'):
            other.solve_many(inst, lockstep="ahead")
        assert not hasattr(other.work, "lockstep")
        other.work.solver.close()
    dev._assert_state(mdl, state)
    same_probe(probe(), before)
    got = mdl.solve_many(inst, lockstep="ahead")  # the default ahead
    assert mdl.work.lockstep["driver"] == "ahead" and mdl.work.lockstep["ahead"]["ahead"] == 8
    dev._same(got, before[1], pr["i_idx"], exact=True)
    dev._assert_state(mdl, state)
    same_probe(probe(), before)
    # a root with l > u in one instance: refused before anything is queued
    Lb = L.copy()
    Lb[2, 7] = U[2, 7] + 1.0
    with pytest.raises(ValueError):
        s.solve_trees_lockstep_ahead(Q, Lb, U, np.zeros((3, N)), np.zeros((3, M)), up, XI, 1, 100, 8)
    same_probe(probe(), before)
    dev._assert_state(mdl, state)
    assert bnb.MIOSQP.solve_many.__defaults__ == (False, None, 8)
    s.close()
