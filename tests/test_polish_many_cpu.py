"""Polishing the answers of solve_many (bnb.primal_guess_multipliers, MIOSQP.polish_many, solve_many(polish=True)) on a
backend without the batched device entry (the CPU oracle): the per-instance restatement is the fallback."""
import numpy as np

from miosqp_amd import bnb, problems

import polish_many_inputs as inputs
import polish_repair_inputs as single


def test_primal_guess_multipliers_row_by_row():
    inf = np.inf
    #             equality  both inf  both 1e30  nearer l  nearer u  tie -> u  only u   only l   l at -1e30
    l = np.array([1.0,      -inf,     -1e30,     0.0,      0.0,      0.0,      -inf,    -3.0,    -1e30])
    u = np.array([1.0,      inf,      1e30,      1.0,      1.0,      1.0,      2.0,     inf,     5.0])
    z = np.array([0.7,      0.3,      0.0,       0.2,      0.9,      0.5,      -40.0,   50.0,    0.0])
    tau = 0.01
    y = bnb.primal_guess_multipliers(l, u, z, tau)
    np.testing.assert_array_equal(y, [0.0, 0.0, 0.0, -tau, tau, tau, tau, -tau, tau])
    # the rule, row by row, on random rows
    rng = np.random.RandomState(3)
    l = rng.standard_normal(200)
    u = l + rng.rand(200)
    u[::7] = l[::7]
    z = l + (u - l) * rng.rand(200)
    l[1::11] = -inf
    u[2::13] = inf
    y = bnb.primal_guess_multipliers(l, u, z, tau)
    for j in range(200):
        if l[j] == u[j] or (l[j] == -inf and u[j] == inf):
            want = 0.0
        else:
            want = -tau if z[j] - l[j] < u[j] - z[j] else tau
        assert y[j] == want, j
    # ... and what OSQP's rule makes of it: lower-active iff z - l < tau, otherwise upper-active iff u - z < tau
    for j in range(200):
        if l[j] == u[j] or not (np.isfinite(l[j]) or np.isfinite(u[j])):
            continue
        lower = np.isfinite(l[j]) and z[j] - l[j] < -y[j]
        upper = not lower and np.isfinite(u[j]) and u[j] - z[j] < y[j]
        assert lower == bool(np.isfinite(l[j]) and y[j] < 0 and z[j] - l[j] < tau), j
        assert upper == bool(not lower and np.isfinite(u[j]) and y[j] > 0 and u[j] - z[j] < tau), j


def _model(oracle_mod, shape=(50, 100, 10), seed=0):
    pr = problems.random_miqp(*shape, seed=seed)
    return pr, single.model(oracle_mod, pr)


def test_polish_many_on_the_fallback_is_the_restatement_per_instance(oracle_mod):
    pr, m = _model(oracle_mod, (20, 10, 5), 0)
    inst = inputs.instances(pr, 4)
    res = m.solve_many(inst)
    plain = [dict(r, x=r["x"].copy()) for r in res]
    d = m.work.data
    assert not hasattr(m.work.solver, "polish_many")
    got = m.polish_many(inst, res, tau=1e-2, repair_iter=20)
    assert got is res
    for i, p, g in zip(inst, plain, got):
        assert p["status"] == bnb.MI_SOLVED
        x = p["x"].copy()
        xi = np.round(x[d.i_idx])
        x[d.i_idx] = xi
        l, u = d.l.copy(), d.u.copy()
        l[d.m:] = xi
        u[d.m:] = xi
        y = bnb.primal_guess_multipliers(l, u, d.A.dot(x), 1e-2)
        r = bnb.polish_restatement(d.P, i["q"], d.A, l, u, x, y, 1e-6, 3, repair_iter=20)
        assert g["polished"] == bool(r.accepted and r.stop == 0)
        assert (g["polish_rounds"], g["pri_after"], g["dua_after"]) == (r.rounds, r.pri_after, r.dua_after)
        want = r.x.copy()
        want[d.i_idx] = xi
        np.testing.assert_array_equal(g["x"], want if g["polished"] else p["x"])
        if g["polished"]:
            assert g["upper_glob"] == .5 * want.dot(d.P.dot(want)) + i["q"].dot(want)
        for key in ("status", "nodes", "osqp_iter"):
            assert g[key] == p[key]


def test_solve_many_with_polish(oracle_mod):
    pr, m = _model(oracle_mod)
    inst = inputs.instances(pr, 6)
    assert np.array_equal(inst[0]["q"], pr["q"])
    d = m.work.data
    q0, l0, u0 = d.q.copy(), d.l.copy(), d.u.copy()
    plain = m.solve_many(inst)
    again = m.solve_many(inst, polish=False)
    for a, b in zip(plain, again):
        assert sorted(a) == sorted(b) == ["nodes", "osqp_iter", "run_time", "status", "upper_glob", "x"]
        assert (a["status"], a["nodes"], a["osqp_iter"], a["upper_glob"]) == (b["status"], b["nodes"], b["osqp_iter"], b["upper_glob"])
        np.testing.assert_array_equal(a["x"], b["x"])
    got = m.solve_many(inst, polish=True)
    assert np.array_equal(d.q, q0) and np.array_equal(d.l, l0) and np.array_equal(d.u, u0)
    ii = d.i_idx
    for i, p, g in zip(inst, plain, got):
        assert g["status"] == p["status"] == bnb.MI_SOLVED
        assert g["polished"] is True and g["polish_rounds"] <= 1
        x = g["x"]
        np.testing.assert_array_equal(x[ii], np.round(p["x"][ii]))
        l, u = d.l.copy(), d.u.copy()
        l[d.m:] = x[ii]
        u[d.m:] = x[ii]
        # the residuals of the adopted x from the original matrices, with the multipliers the fallback computed
        xin = p["x"].copy()
        xin[ii] = x[ii]
        y0 = bnb.primal_guess_multipliers(l, u, d.A.dot(xin), 10 * problems.QP_SETTINGS["eps_abs"])
        r = bnb.polish_restatement(d.P, i["q"], d.A, l, u, xin, y0, 1e-6, 3, repair_iter=20)
        assert r.accepted and r.stop == 0
        pri, dua = inputs.residuals(d, i["q"], l, u, x, r.y)
        assert pri <= 1e-9 and dua <= 1e-9, (pri, dua)
        assert g["pri_after"] <= 1e-9 and g["dua_after"] <= 1e-9, (g["pri_after"], g["dua_after"])
        assert g["upper_glob"] == .5 * x.dot(d.P.dot(x)) + i["q"].dot(x)


def test_the_setting_stays_refused_and_the_symbols_are_declared(oracle_mod):
    import pytest
    from miosqp_amd import _lib
    pr = problems.random_miqp(10, 5, 2, seed=0)
    m = single.model(oracle_mod, pr, polish_incumbent=1)
    with pytest.raises(ValueError):
        m.solve_many([dict()], polish=True)
    assert "miosqp_qp_polish_many" in _lib.SYMBOLS and "miosqp_qp_get_polish_many_classes" in _lib.SYMBOLS
