"""MIOSQP.solve_many(lockstep=True) on the CPU oracle: the lock-step driver with its generic wave (update(q=) +
Node.solve per column on the model's solver) against the sequential path (lockstep=False).  Both run the same solver
on the same (q, l, u, x0, y0) per node, so every count is equal and every x is equal bit for bit."""
import numpy as np
import pytest

from miosqp_amd import bnb, problems

SHAPES = {"n50": (50, 25, 25, 1), "n40": (40, 60, 20, 2)}
CAP = 6  # max_iter_bb of the capped runs: five nodes per tree


def _problem(key):
    n, m, p, seed = SHAPES[key]
    return problems.random_miqp(n, m, p, seed=seed)


def _model(oracle_mod, pr, rule, cap=None):
    st = dict(problems.BNB_SETTINGS)
    st["tree_explor_rule"] = rule
    if cap is not None:
        st["max_iter_bb"] = cap
    mdl = bnb.MIOSQP(backend=oracle_mod)
    mdl.setup(pr["P"], pr["q"], pr["A"], pr["l"].copy(), pr["u"].copy(), pr["i_idx"], pr["i_l"], pr["i_u"], st,
              dict(problems.QP_SETTINGS))
    return mdl


def _instances(pr):
    """four with their own q, one with its own l, u, one with an x0 that passes set_x0, one that its bounds make
    infeasible where the shape allows it (m > n: alternating equalities no x satisfies; for m < n the same rows are merely
    far away)"""
    n, m = len(pr["q"]), len(pr["l"])
    rng = np.random.RandomState(11)
    inst = [dict(q=pr["q"] + 0.3 * rng.randn(n)) for _ in range(4)]
    inst.append(dict(l=pr["l"] - 0.5 * rng.rand(m), u=pr["u"] - 0.5 * rng.rand(m)))
    x0 = np.zeros(n)
    x0[pr["i_idx"][0]] = 1.0  # A has entries in [0, 1): 0 <= A x0 < 1 lies inside [l, u]
    inst.append(dict(q=pr["q"] + 0.3 * rng.randn(n), x0=x0))
    b = 50.0 * (1 - 2 * (np.arange(m) % 2))
    inst.append(dict(l=b, u=b.copy()))
    return inst


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert set(g) == set(w)
        for key in ("status", "nodes", "osqp_iter", "upper_glob"):
            assert g[key] == w[key], key
        if w["status"] in (bnb.MI_SOLVED, bnb.MI_MAX_ITER_FEASIBLE):  # (x is uninitialised memory without an incumbent)
            np.testing.assert_array_equal(g["x"], w["x"])


@pytest.fixture(scope="module")
def probs():
    return {k: _problem(k) for k in SHAPES}


@pytest.mark.parametrize("rule", [0, 1, 2, 3])
@pytest.mark.parametrize("key", list(SHAPES))
def test_lockstep_equals_sequential(oracle_mod, probs, key, rule):
    pr = probs[key]
    inst = _instances(pr)
    want = _model(oracle_mod, pr, rule).solve_many(inst, lockstep=False)
    mdl = _model(oracle_mod, pr, rule)
    got = mdl.solve_many(inst, lockstep=True)
    _same(got, want)
    rec = mdl.work.lockstep
    assert rec["instances"] == len(inst) and not rec["batched"]
    assert rec["nodes"] == sum(g["nodes"] for g in got)
    assert rec["waves"] == max(g["nodes"] for g in got)
    assert len(set(rec["finished_at"].values())) > 1  # trees finish at different waves
    assert got[5]["upper_glob"] < np.inf  # the accepted x0 is an incumbent at the least
    if key == "n40":
        assert got[6]["status"] == bnb.MI_PRIMAL_INFEASIBLE


@pytest.mark.parametrize("rule", [0, 1, 2, 3])
@pytest.mark.parametrize("key", list(SHAPES))
def test_lockstep_equals_sequential_at_the_node_cap(oracle_mod, probs, key, rule):
    pr = probs[key]
    inst = _instances(pr)
    want = _model(oracle_mod, pr, rule, CAP).solve_many(inst, lockstep=False)
    got = _model(oracle_mod, pr, rule, CAP).solve_many(inst, lockstep=True)
    _same(got, want)
    capped = [g for g in got if g["status"] in (bnb.MI_MAX_ITER_FEASIBLE, bnb.MI_MAX_ITER_UNSOLVED)]
    assert capped and all(g["nodes"] == CAP - 1 for g in capped)


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


def test_model_is_restored_also_when_an_instance_raises(oracle_mod, probs):
    pr = probs["n40"]
    ref = _model(oracle_mod, pr, 1)
    ref.solve_many(_instances(pr)[:3], lockstep=False)
    want = ref.solve()
    mdl = _model(oracle_mod, pr, 1)
    before = _state(mdl)
    mdl.solve_many(_instances(pr)[:3], lockstep=True)
    _assert_state(mdl, before)
    bad = _instances(pr)[:2] + [dict(l=pr["u"].copy(), u=pr["l"].copy())]
    with pytest.raises(ValueError):
        mdl.solve_many(bad, lockstep=True)
    _assert_state(mdl, before)
    # ... and the solver holds the model's q again: the model's own solve is what it is after the sequential path
    # (the oracle's second solve of one problem differs from its first in the last bit, hence not a fresh model's)
    res = mdl.solve()
    assert (res.status, res.upper_glob, mdl.work.iter_num) == (want.status, want.upper_glob, ref.work.iter_num)
    np.testing.assert_array_equal(res.x, want.x)


def test_default_on_the_oracle_is_the_sequential_path(oracle_mod, probs):
    pr = probs["n50"]
    inst = _instances(pr)[:3]
    mdl = _model(oracle_mod, pr, 1)
    got = mdl.solve_many(inst)
    assert not hasattr(mdl.work, "lockstep")
    _same(got, _model(oracle_mod, pr, 1).solve_many(inst, lockstep=False))


def test_lockstep_refuses_what_it_does_not_cover(oracle_mod, probs):
    pr = probs["n50"]
    mdl = _model(oracle_mod, pr, 1)
    mdl.work.settings["branching_rule"] = 1
    with pytest.raises(ValueError):
        mdl.solve_many(_instances(pr)[:2], lockstep=True)
