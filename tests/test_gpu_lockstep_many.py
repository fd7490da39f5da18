"""MIOSQP.solve_many beyond the one-launch trees on the HIP engine (needs an MI355X): B trees in lock step, one node of
every unfinished tree per wave, the wave ONE solve_batch_q.  random_miqp(100, 200, 50, seed 0) has n + M = 350 -- beyond
miosqp_qp_solve_trees, which declines -- and about 80 nodes per tree.  Every tree must make the decisions of its
sequential solve (lockstep=False: update_vectors + set_x0 + solve per instance, the hosted search): status, nodes and
ADMM iterations equal, the incumbent's value within 1e-9 relative, its integers exact."""
import numpy as np
import pytest

from miosqp_amd import problems

pytestmark = pytest.mark.gpu

N, M_, P_ = 100, 200, 50
POLISH_KEYS = ("polished", "polish_rounds", "pri_after", "dua_after")


def _problem():
    return problems.random_miqp(N, M_, P_, seed=0)


def _model(pr, rule, rho, **st):
    from miosqp_amd import bnb
    mdl = bnb.MIOSQP()
    mdl.setup(pr["P"], pr["q"], pr["A"], pr["l"].copy(), pr["u"].copy(), pr["i_idx"], pr["i_l"], pr["i_u"],
              dict(problems.BNB_SETTINGS, tree_explor_rule=rule, **st), dict(problems.QP_SETTINGS, rho=rho))
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


def _same(got, want, ii):
    from miosqp_amd import bnb
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        print("instance %d: lock-step %s %d nodes %d iterations %.12g | sequential %s %d %d %.12g"
              % (k, g["status"], g["nodes"], g["osqp_iter"], g["upper_glob"], w["status"], w["nodes"], w["osqp_iter"],
                 w["upper_glob"]))
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g["status"], g["nodes"], g["osqp_iter"]) == (w["status"], w["nodes"], w["osqp_iter"]), k
        if w["status"] in (bnb.MI_SOLVED, bnb.MI_MAX_ITER_FEASIBLE):
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


@pytest.mark.parametrize("rho", [0.1, "auto"])
@pytest.mark.parametrize("rule", [1, 3])
def test_lockstep_trees_equal_the_sequential_calls(rule, rho):
    from miosqp_amd import bnb
    pr = _problem()
    inst = _instances(pr)
    seq, mdl = _model(pr, rule, rho), _model(pr, rule, rho)
    want = seq.solve_many(inst, lockstep=False)
    assert not hasattr(seq.work, "lockstep")
    before = _state(mdl)
    got = mdl.solve_many(inst)  # the default: the one-launch path declines, the lock-step driver takes over
    rec = mdl.work.lockstep
    assert getattr(mdl.work, "_no_trees", False) and rec["batched"] and rec["instances"] == len(inst)
    assert rec["nodes"] == sum(g["nodes"] for g in got) and rec["waves"] == max(g["nodes"] for g in got)
    assert len(set(rec["finished_at"].values())) > 1
    _assert_state(mdl, before)
    _same(got, want, pr["i_idx"])
    assert got[6]["status"] == bnb.MI_PRIMAL_INFEASIBLE and got[5]["upper_glob"] < np.inf
    assert sum(g["status"] == bnb.MI_SOLVED for g in got) >= 5
    # the model's own solve afterwards is what it is after the sequential path: the engine's q and root are the model's
    a, b = mdl.solve(), seq.solve()
    assert (a.status, mdl.work.iter_num, mdl.work.osqp_iter) == (b.status, seq.work.iter_num, seq.work.osqp_iter)
    for m_ in (seq, mdl):
        m_.work.solver.close()


@pytest.mark.parametrize("rule", [1, 3])
def test_lockstep_trees_at_the_node_cap_and_with_polish(rule):
    from miosqp_amd import bnb
    pr = _problem()
    inst = _instances(pr)
    seq, mdl = _model(pr, rule, 0.1, max_iter_bb=12), _model(pr, rule, 0.1, max_iter_bb=12)
    want = seq.solve_many(inst, lockstep=False)
    got = mdl.solve_many(inst)
    assert mdl.work.lockstep["batched"] and mdl.work.lockstep["waves"] == 11
    capped = [g for g in got if g["status"] in (bnb.MI_MAX_ITER_FEASIBLE, bnb.MI_MAX_ITER_UNSOLVED)]
    assert capped and all(g["nodes"] == 11 for g in capped)
    _same(got, want, pr["i_idx"])
    # polish=True goes on to polish_many: the same trees, every dict gains the polish keys
    pol = mdl.solve_many(inst, polish=True)
    for g, p_ in zip(got, pol):
        assert all(key in p_ for key in POLISH_KEYS) and not any(key in g for key in POLISH_KEYS)
        assert (p_["status"], p_["nodes"], p_["osqp_iter"]) == (g["status"], g["nodes"], g["osqp_iter"])
    for m_ in (seq, mdl):
        m_.work.solver.close()
