"""The repair loop of the polish on the device (miosqp_qp_polish_repair, k_pol_revise in csrc/kernels_polish.inc) against
its dense numpy restatement (bnb.polish_restatement with repair_iter).

As in test_gpu_polish.py both sides get the SAME (l, u, x, y), solved by the CPU backend, so the sets can only differ on
a row whose comparison sits on a tie, in round 0 or in a revision; the restatement reports every row's margin over all
the comparisons that classified it and each case asserts that none is below 1e-9 max(1, |bound|) (measured: 1.8e-4 or
more).  Tolerances are those of test_gpu_polish.py: 1e-9 relative for x, y and obj, its `_close` for the residuals.

Shapes: the inputs of test_polish_repair_cpu.py (n = 50 .. 500: one partial 64-block of the factorisation up to seven
full ones and a remainder), and n = 63, 64, 65 on the edges of the 64-wide tile."""
import numpy as np
import pytest

from golden_cases import load_case, run_case
import polish_repair_inputs as inputs

pytestmark = pytest.mark.gpu

NAMES = ["cfg2_root_rho0.1", "cfg2_root_auto", "cfg1_s1_root_rho0.1", "cfg1_s1_incumbent_auto"] + \
    [inputs.crude_name(shape, seed) for shape, seed in inputs.CRUDE + inputs.TILE_EDGES]
COUNTS = ("rounds", "stop", "n_added", "n_dropped", "accepted0", "reason0", "accepted", "reason", "n_lower", "n_upper")
BITS = ("accepted", "reason", "n_lower", "n_upper", "pri_before", "dua_before", "pri_after", "dua_after", "obj")


@pytest.fixture(scope="module")
def cases(oracle_mod):
    """name -> (problem, qp_extra, Data, l, u, x, y) solved once by the CPU backend, and the restatement's answers"""
    from miosqp_amd import bnb
    out = {}
    for name, case in inputs.named_inputs(oracle_mod, NAMES).items():
        _, _, d, l, u, x, y = case
        ref = {it: bnb.polish_restatement(d.P, d.q, d.A, l, u, x, y, 1e-6, 3, repair_iter=it) for it in (5, 1)}
        out[name] = case + (ref,)
    return out


@pytest.fixture(scope="module")
def engines():
    """one engine per problem and rho, shared by the tests (a polish call leaves nothing behind)"""
    from miosqp_amd import qp
    made = {}

    def get(cases, name):
        pr, extra = cases[name][:2]
        if name not in made:
            made[name] = inputs.model(qp, pr, qp_extra=extra).work.solver
        return made[name]
    return get


def _close(a, b):
    return abs(a - b) <= 1e-12 or abs(a - b) <= 1e-6 * abs(b)


def _same_bits(a, b):
    np.testing.assert_array_equal(a.x, b.x)
    np.testing.assert_array_equal(a.y, b.y)
    for f in BITS:
        assert getattr(a, f) == getattr(b, f) or (np.isnan(getattr(a, f)) and np.isnan(getattr(b, f))), f


@pytest.mark.parametrize("repair_iter", [5, 1])
@pytest.mark.parametrize("name", NAMES)
def test_device_against_restatement(cases, engines, name, repair_iter):
    _, _, d, l, u, x, y, ref = cases[name]
    ro = ref[repair_iter]
    # no row on a tie, in any round: an input on one is not a valid test input
    bound = np.where(ro.active < 0, l, u)
    bound = np.where(np.isfinite(bound), bound, 0.0)
    assert np.all(ro.margin >= 1e-9 * np.maximum(1.0, np.abs(bound))), (name, ro.margin.min())
    rg = engines(cases, name).polish(l, u, x, y, 1e-6, 3, repair_iter=repair_iter)
    print("%s repair_iter %d: rounds %d stop %d, +%d -%d, accepted %d (round 0: %d reason %d), active %d + %d, "
          "pri %.2e -> %.2e, dua %.2e -> %.2e, min margin %.2e, device %.0f us"
          % (name, repair_iter, rg.rounds, rg.stop, rg.n_added, rg.n_dropped, rg.accepted, rg.accepted0, rg.reason0,
             rg.n_lower, rg.n_upper, rg.pri_before, rg.pri_after, rg.dua_before, rg.dua_after, ro.margin.min(),
             1e6 * rg.device_time))
    for f in COUNTS:
        assert getattr(rg, f) == getattr(ro, f), (name, f, getattr(rg, f), getattr(ro, f))
    np.testing.assert_array_equal(rg.active, ro.active)
    assert ro.reason != 1
    if ro.accepted:
        assert np.max(np.abs(rg.x - ro.x)) <= 1e-9 * max(1.0, np.max(np.abs(ro.x))), name
        assert np.max(np.abs(rg.y - ro.y)) <= 1e-9 * max(1.0, np.max(np.abs(ro.y))), name
        np.testing.assert_array_equal(rg.y != 0.0, ro.active != 0)
    else:
        np.testing.assert_array_equal(rg.x, x)
        np.testing.assert_array_equal(rg.y, y)
    assert _close(rg.pri_before, ro.pri_before) and _close(rg.dua_before, ro.dua_before)
    assert _close(rg.pri_after, ro.pri_after) and _close(rg.dua_after, ro.dua_after), \
        (name, rg.pri_after, ro.pri_after, rg.dua_after, ro.dua_after)
    assert abs(rg.obj - ro.obj) <= 1e-9 * abs(ro.obj), (name, rg.obj, ro.obj)


@pytest.mark.parametrize("name", ["cfg2_root_rho0.1", "cfg1_s1_incumbent_auto", "crude_n65m40p12_s0",
                                  "crude_n64m20p5_s0"])
def test_zero_rounds_is_the_plain_polish_bit_for_bit(cases, engines, name):
    _, _, d, l, u, x, y, ref = cases[name]
    eng = engines(cases, name)
    a = eng.polish(l, u, x, y)
    b = eng.polish(l, u, x, y, repair_iter=0)
    c = eng.polish(l, u, x, y)  # ... and the plain entry answers the same after a repair call
    _same_bits(a, b)
    _same_bits(a, c)
    assert (b.rounds, b.accepted0, b.reason0) == (0, a.accepted, a.reason)
    assert b.stop == (0 if ref[5].rounds == 0 else 1)
    assert (b.n_lower, b.n_upper) == (int(np.sum(b.active < 0)), int(np.sum(b.active > 0)))


def test_two_repair_calls_give_identical_bits_and_leave_the_node_solver_alone(cases, engines):
    name = "crude_n129m30p10_s1"
    _, _, d, l, u, x, y, ref = cases[name]
    eng = engines(cases, name)
    x0, y0 = np.zeros(d.n), np.zeros(d.m + d.n_int)
    a = eng.solve_node(l, u, x0, y0)
    p1 = eng.polish(l, u, x, y, repair_iter=5)
    b = eng.solve_node(l, u, x0, y0)
    p2 = eng.polish(l, u, x, y, repair_iter=5)
    assert p1.rounds == 2
    np.testing.assert_array_equal(a.x, b.x)
    np.testing.assert_array_equal(a.y, b.y)
    assert (a.status_val, a.iter, a.lower) == (b.status_val, b.iter, b.lower)
    for f in ("pri_res", "dua_res", "obj_val", "int_inf", "nextvar", "heur_viol", "heur_obj"):
        assert getattr(a.info, f) == getattr(b.info, f), f
    _same_bits(p1, p2)
    np.testing.assert_array_equal(p1.active, p2.active)
    for f in COUNTS:
        assert getattr(p1, f) == getattr(p2, f), f
    # identical sets give identical bits whatever path led to them: the repaired point fed back in is a fixed point of
    # the same set, and round 0 on that set computes what round 2 computed
    p3 = eng.polish(l, u, p1.x, p1.y, repair_iter=5)
    assert (p3.rounds, p3.stop) == (0, 0)
    np.testing.assert_array_equal(p3.active, p1.active)
    np.testing.assert_array_equal(p3.x, p1.x)
    np.testing.assert_array_equal(p3.y, p1.y)
    dev, wait = eng.polish_rounds()
    assert dev[0] > 0 and np.all(dev[1:] == 0) and np.all(wait[1:] == 0)


def test_argument_checks(cases, engines):
    name = "crude_n64m20p5_s0"
    _, _, d, l, u, x, y, ref = cases[name]
    eng = engines(cases, name)
    for it in (-1, 21):
        with pytest.raises(RuntimeError):
            eng.polish(l, u, x, y, repair_iter=it)
    with pytest.raises(RuntimeError):
        eng.polish(l, u, x, y, delta=0.0, repair_iter=2)
    with pytest.raises(RuntimeError):
        eng.polish(l, u, x, y, refine_iter=11, repair_iter=2)
    bad = x.copy()
    bad[3] = np.nan
    with pytest.raises(RuntimeError):
        eng.polish(l, u, bad, y, repair_iter=2)
    lo = l.copy()
    lo[0] = u[0] + 1.0
    with pytest.raises(ValueError):
        eng.polish(lo, u, x, y, repair_iter=2)
    assert eng.polish(l, u, x, y, repair_iter=20).stop == 0  # ... and the engine still answers


def test_a_whole_tree_with_repair(oracle_mod):
    """the tolerances of test_whole_trees_with_a_polished_incumbent"""
    from miosqp_amd import bnb, qp
    got, stats = {}, {}
    real = bnb.Workspace.polish_incumbent

    def spy(self):
        real(self)
        stats.setdefault(key, []).append(dict(self.polish_repair_stats))

    bnb.Workspace.polish_incumbent = spy
    try:
        for key, backend in (("gpu", qp), ("cpu", oracle_mod)):
            case = load_case("cfg1_n50m100p10_s0")
            case["settings"] = dict(case["settings"], polish_incumbent=1, polish_repair_iter=5)
            got[key] = run_case(case, backend)
    finally:
        bnb.Workspace.polish_incumbent = real
    case = load_case("cfg1_n50m100p10_s0")
    ii = case["prob"]["i_idx"]
    assert stats["gpu"] == stats["cpu"] and len(stats["gpu"]) > 0
    assert all(s["calls"] == 1 and s["fixed_points"] == 1 for s in stats["gpu"]), stats["gpu"]
    for g, c, e in zip(got["gpu"], got["cpu"], case["solves"]):
        assert g["status"] == c["status"] == e["status"]
        assert g["iter_num"] == c["iter_num"] == e["iter_num"]
        np.testing.assert_array_equal(g["trace"][:, :4], c["trace"][:, :4])
        np.testing.assert_array_equal(g["trace"][:, 7:], c["trace"][:, 7:])
        np.testing.assert_allclose(g["trace"][:, 4:7], c["trace"][:, 4:7], rtol=1e-6, atol=1e-9)
        np.testing.assert_array_equal(g["x"][ii], c["x"][ii])
        np.testing.assert_array_equal(g["x"][ii], np.round(g["x"][ii]))
        assert np.max(np.abs(g["x"] - c["x"])) <= 1e-9, np.max(np.abs(g["x"] - c["x"]))
        assert abs(g["upper_glob"] - c["upper_glob"]) <= 1e-9 * max(1.0, abs(c["upper_glob"]))
