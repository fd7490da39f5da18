"""Polishing (settings["polish_incumbent"] = 1) on the CPU backend.

Without an engine that has `polish`, Workspace polishes with bnb.polish_restatement: the dense numpy statement of the
operation the device entry point miosqp_qp_polish is checked against on the GPU (tests/test_gpu_polish.py).
"""
import numpy as np
import pytest

from golden_cases import load_case, run_case
from miosqp_amd import problems

SOLVED, MAX_ITER = 1, -2


def _model(pr, backend, qp_extra=None, **settings):
    from miosqp_amd import bnb
    model = bnb.MIOSQP(backend=backend)
    model.setup(pr["P"], pr["q"], pr["A"], np.copy(pr["l"]), np.copy(pr["u"]), pr["i_idx"], pr["i_l"], pr["i_u"],
                dict(problems.BNB_SETTINGS, **settings), dict(problems.QP_SETTINGS, **(qp_extra or {})))
    return model


def _residuals(d, l, u, x, y):
    """pri, dua of (x, y) from the original P, q, A over all rows"""
    z = d.A.dot(x)
    return max(np.max(l - z), np.max(z - u), 0.0), np.max(np.abs(d.P.dot(x) + d.q + d.A.T.dot(y)))


# -- 1. the incumbent with its integers fixed ------------------------------------------------------------------------
@pytest.mark.parametrize("rho", [0.1, "auto"])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_incumbent_is_polished_to_the_optimum_of_its_active_set(oracle_mod, seed, rho):
    from miosqp_amd import bnb
    pr = problems.random_miqp(50, 100, 10, seed=seed)
    model = _model(pr, oracle_mod, qp_extra=dict(rho=rho))
    res = model.solve()
    assert res.status == bnb.MI_SOLVED
    w, d = model.work, model.work.data
    xi = np.round(res.x[d.i_idx])
    l, u = d.l.copy(), d.u.copy()
    l[d.m:] = xi
    u[d.m:] = xi
    node = bnb.Node(d, l, u, w.solver, x0=np.array(res.x), y0=np.zeros(d.m + d.n_int), constant=w.constant)
    node.solve()
    assert node.status in (SOLVED, MAX_ITER)
    r = bnb.polish_restatement(d.P, d.q, d.A, l, u, node.x, node.y, 1e-6, 3)
    pri, dua = _residuals(d, l, u, r.x, r.y)
    print("seed %d rho %r: %d + %d active, pri %.1e -> %.1e, dua %.1e -> %.1e, objective %.6f -> %.6f (search %.6f)"
          % (seed, rho, r.n_lower, r.n_upper, r.pri_before, pri, r.dua_before, dua, node.lower, r.obj, res.upper_glob))
    assert r.accepted and r.reason == 0
    assert pri <= 1e-9 and dua <= 1e-9
    assert np.all(r.y[r.active == 0] == 0.0)
    # a direct solve of the UNregularised KKT system on the same active set
    rows = np.where(r.active != 0)[0]
    assert len(rows) == r.n_lower + r.n_upper and np.all(r.active[d.m:] == -1)  # (the fixed rows are equalities)
    A, P = d.A.toarray(), d.P.toarray()
    Aa, k = A[rows], len(rows)
    b = np.where(r.active[rows] < 0, l[rows], u[rows])
    sol = np.linalg.solve(np.block([[P, Aa.T], [Aa, np.zeros((k, k))]]), np.concatenate([-d.q, b]))
    assert np.max(np.abs(r.x - sol[:d.n])) <= 1e-9 * max(1.0, np.max(np.abs(sol[:d.n])))


# -- 2. a wrong active set is caught -----------------------------------------------------------------------------------
@pytest.mark.parametrize("rho", [0.1, "auto"])
def test_config2_root_is_rejected_for_its_primal_residual(oracle_mod, rho):
    """The set guessed from the 1e-3 iterate of the config-2 root leaves out rows the polished point then violates
    (4.9e-4 at rho 0.1, 2.2e-4 at "auto", against 0 before): reason 2, and the input comes back bit for bit."""
    from miosqp_amd import bnb
    pr = problems.random_miqp(500, 1000, 250, seed=0)
    w = _model(pr, oracle_mod, qp_extra=dict(rho=rho)).work
    root = w.leaves[0]
    root.solve()
    x, y = root.x.copy(), root.y.copy()
    r = bnb.polish_restatement(w.data.P, w.data.q, w.data.A, root.l, root.u, x, y)
    assert (r.accepted, r.reason) == (False, 2)
    assert r.pri_after > max(r.pri_before, 1e-10) and r.pri_after > 1e-4
    np.testing.assert_array_equal(r.x, x)
    np.testing.assert_array_equal(r.y, y)
    assert r.x is not x and r.xh is not None


def test_the_classification_rule_by_hand():
    """an equality row is always active, an infinite bound never is, the others follow OSQP's two comparisons; margins
    are the distances of the comparisons that decided"""
    from miosqp_amd import bnb
    P, q = np.eye(2), np.array([-1.0, -1.0])
    A = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [1.0, -1.0], [1.0, 0.0]])
    l = np.array([0.25, -np.inf, -1e30, -5.0, 0.0])
    u = np.array([0.25, 0.5, 1.0, 1e30, 5.0])
    x, y = np.array([0.25, 0.5]), np.array([0.75, 0.5, 0.0, 0.0, 0.0])
    r = bnb.polish_restatement(P, q, A, l, u, x, y)
    np.testing.assert_array_equal(r.active, [-1, 1, 0, 0, 0])
    assert (r.n_lower, r.n_upper) == (1, 1)
    # row 0: equality; row 1: u - z = 0 < y = .5, margin .5; row 2: u - z = .25 vs 0; row 3: z - l = 4.75 vs 0;
    # row 4: both sides finite and inactive: min(z - l + y, u - z - y) = .25
    np.testing.assert_allclose(r.margin, [np.inf, 0.5, 0.25, 4.75, 0.25])
    assert r.accepted and np.max(np.abs(r.x - x)) <= 1e-12 and np.max(np.abs(r.y - y)) <= 1e-9
    # a matrix that is not positive definite on the null space of the set: factorisation
    r = bnb.polish_restatement(-np.eye(2), q, A[:1], l[:1], u[:1], x, y[:1])
    assert (r.accepted, r.reason) == (False, 1) and np.isnan(r.obj) and r.xh is None


# -- 3. whole trees --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n10m5p2_s0", "cfg1_n50m100p10_s0", "n30m150p15_s4", "mpc_n12m30p6_s8",
                                  "infeasible_n10"])
def test_golden_trees_with_a_polished_incumbent(oracle_mod, name):
    from miosqp_amd import bnb
    case = load_case(name)
    case["settings"] = dict(case["settings"], polish_incumbent=1)
    stats = []
    real_polish = bnb.Workspace.polish_incumbent

    def spy(self):
        real_polish(self)
        stats.append(dict(self.polish_stats))

    bnb.Workspace.polish_incumbent = spy
    try:
        got = run_case(case, oracle_mod)
    finally:
        bnb.Workspace.polish_incumbent = real_polish
    pr = case["prob"]
    A, l, u = problems.extended(pr)
    ii = pr["i_idx"]
    assert len(got) == len(case["solves"])
    k = 0
    for s, (g, e) in enumerate(zip(got, case["solves"])):
        np.testing.assert_array_equal(g["trace"], e["trace"])
        assert g["iter_num"] == e["iter_num"] and g["osqp_iter"] == e["osqp_iter"]
        assert g["status"] == e["status"]
        if e["status"] not in (bnb.MI_SOLVED, bnb.MI_MAX_ITER_FEASIBLE):
            continue
        assert stats[k]["calls"] == 1 and stats[k]["accepted"] == 1, stats[k]
        k += 1
        np.testing.assert_array_equal(g["x"][ii], np.round(g["x"][ii]))
        np.testing.assert_array_equal(g["x"][ii], e["x"][ii])
        # this solve's root bounds: the updates before it replace l, u of A proper
        ls, us = l.copy(), u.copy()
        if s > 0:
            ls[:len(pr["l"])], us[:len(pr["u"])] = case["updates"][s - 1][1], case["updates"][s - 1][2]
        z = A.dot(g["x"])
        viol = max(np.max(ls - z), np.max(z - us), 0.0)
        print("%s solve %d: violation %.1e, upper %.9f (recorded %.9f)" % (name, s, viol, g["upper_glob"], e["upper_glob"]))
        assert viol <= 1e-9
        assert abs(g["upper_glob"] - e["upper_glob"]) <= 2e-3 * max(1.0, abs(e["upper_glob"]))
    assert k == len(stats)
    if name == "infeasible_n10":
        assert stats == []  # no incumbent, no polish call


def test_off_is_the_code_path_of_today(oracle_mod):
    from miosqp_amd import bnb
    calls = []
    real = bnb.Workspace.polish_incumbent
    bnb.Workspace.polish_incumbent = lambda self: calls.append(1)
    try:
        for extra in (dict(), dict(polish_incumbent=0)):
            case = load_case("cfg1_n50m100p10_s0")
            case["settings"] = dict(case["settings"], **extra)
            got = run_case(case, oracle_mod)
            for g, e in zip(got, case["solves"]):
                np.testing.assert_array_equal(g["trace"], e["trace"])
                np.testing.assert_array_equal(g["x"], e["x"])
                assert g["upper_glob"] == e["upper_glob"]
    finally:
        bnb.Workspace.polish_incumbent = real
    assert calls == []


def test_statistics(oracle_mod):
    pr = problems.random_miqp(50, 100, 10, seed=0)
    model = _model(pr, oracle_mod, polish_incumbent=1)
    assert model.work.polish_stats == dict(calls=0, accepted=0, n_active=0, pri_after=model.work.polish_stats["pri_after"],
                                           dua_after=model.work.polish_stats["dua_after"], time=0.)
    res = model.solve()
    st = model.work.polish_stats
    assert st["calls"] == 1 and st["accepted"] == 1 and st["n_active"] == 20 and st["time"] > 0
    assert st["pri_after"] <= 1e-9 and st["dua_after"] <= 1e-9
    assert res.upper_glob == model.work.data.compute_obj_val(res.x)
    assert abs(res.upper_glob - (-9.51003)) <= 1e-5  # the search alone reports -9.50991
    model.update_vectors(q=pr["q"])
    assert model.work.polish_stats["calls"] == 0


# -- 4. settings and refusals ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [dict(polish_incumbent=2), dict(polish_incumbent=-1), dict(polish_delta=0),
                                 dict(polish_delta=-1e-6), dict(polish_delta="small"), dict(polish_delta=float("nan")),
                                 dict(polish_refine_iter=11), dict(polish_refine_iter=-1), dict(polish_refine_iter=2.5)])
def test_bad_settings_are_refused_at_setup(oracle_mod, bad):
    pr = problems.random_miqp(10, 5, 2, seed=0)
    with pytest.raises(ValueError):
        _model(pr, oracle_mod, **dict(dict(polish_incumbent=1), **bad))


def test_defaults():
    from miosqp_amd import bnb
    assert bnb.polish_settings({}) == dict(on=0, delta=1e-6, refine_iter=3)
    assert bnb.polish_settings(dict(polish_incumbent=1, polish_delta=1e-5, polish_refine_iter=0)) == \
        dict(on=1, delta=1e-5, refine_iter=0)


def test_the_other_searches_refuse_the_setting(oracle_mod):
    from miosqp_amd import bnb, dist, stream
    model = _model(problems.random_miqp(50, 100, 10, seed=0), oracle_mod, polish_incumbent=1)
    with pytest.raises(ValueError, match="polish_incumbent"):
        model.solve_many([dict()])
    with pytest.raises(ValueError, match="polish_incumbent"):
        dist.ShardedSearch(model)
    with pytest.raises(ValueError, match="polish_incumbent"):
        dist.ShardedStream(model)
    with pytest.raises(ValueError, match="polish_incumbent"):
        bnb.require_plain_search(model.work.settings, "streaming search")
    # the stream's own constructors reach that call only on the HIP engine: without it they refuse the backend first
    for cls in (stream.StreamSearch, stream.NativeStreamSearch):
        with pytest.raises((ValueError, TypeError)):
            cls(model)
    # MIOSQP.solve's own hosted loop is not one of them
    bnb.require_plain_search(model.work.settings, "hosted search", rule=False, polish=False)
