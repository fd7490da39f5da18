"""The best-bound exploration rules (settings["tree_explor_rule"] = 2, 3) in the Python loop, on the CPU oracle backend.

Rule 2 takes the open leaf with the SMALLEST inherited bound, the first one in list order on ties; rule 3 dives like rule
0 until there is an incumbent and takes the best bound from then on.  The reference has neither, so the yardstick is
this restatement itself: the choice on hand-made leaf lists, and whole trees whose node and iteration counts were
measured once with it (rho = 0.1, problems.BNB_SETTINGS) and are keyed by `problems.instance_digest`.
"""
import types

import numpy as np
import pytest

from miosqp_amd import bnb, problems

# random_miqp (n, m, p, seed) -> digest, then (nodes, ADMM iterations) to close the tree under rule 1 (= rule 0), 2, 3
# without the heuristic and under rules 1, 3 with round and fix (primal_heuristic 1)
TABLE = {
    (50, 100, 10, 0): ("a1ac4300f664952b", (11, 675), (15, 1000), (11, 675), (11, 675), (11, 675)),
    (50, 100, 10, 1): ("d05885fa20f7d51b", (29, 1675), (28, 1625), (28, 1625), (29, 1675), (28, 1625)),
    (30, 150, 15, 4): ("c997c2a6fa991549", (24, 1650), (22, 1575), (22, 1575), (23, 1625), (19, 1325)),
    (40, 60, 20, 2): ("938595c9b3cd83c5", (37, 1775), (21, 1050), (26, 1275), (37, 1775), (21, 1050)),
    (60, 80, 30, 3): ("06e161c80da162fb", (121, 6325), (98, 5200), (103, 5425), (84, 4400), (70, 3750)),
    (100, 200, 50, 0): ("0430b8ccbeffab2f", (82, 8625), (121, 12475), (82, 8625), (77, 8350), (77, 8350)),
    (50, 25, 25, 1): ("e744151a0f1f590c", (107, 3825), (60, 2200), (63, 2300), (41, 1575), (41, 1575)),
    (80, 40, 40, 2): ("9e946d94f491930e", (266, 11800), (236, 11000), (245, 10900), (191, 8650), (157, 7175)),
}
INSTANCES = list(TABLE)
# scipy's sampling decides the instances: one whose digest is not in the table cannot be compared with it and is skipped,
# but no more of them than this (the table was measured where all eight digests are these)
MAX_UNKNOWN = 0


def _model(pr, backend, qp_extra=None, **settings):
    model = bnb.MIOSQP(backend=backend)
    model.setup(pr["P"], pr["q"], pr["A"], np.copy(pr["l"]), np.copy(pr["u"]), pr["i_idx"], pr["i_l"], pr["i_u"],
                dict(problems.BNB_SETTINGS, **settings), dict(problems.QP_SETTINGS, **(qp_extra or {})))
    return model


# -- 1. the choice -----------------------------------------------------------------------------------------------
def _workspace(lowers, depths, upper=np.inf):
    """leaf_index reads the leaves' lower and depth and the incumbent's value, nothing else"""
    w = bnb.Workspace.__new__(bnb.Workspace)
    w.leaves = [types.SimpleNamespace(lower=lo, depth=d) for lo, d in zip(lowers, depths)]
    w.upper_glob = upper
    return w


def test_ties_go_to_the_first_minimum():
    w = _workspace([3.0, 1.0, 2.0, 1.0, 1.0], [1, 2, 2, 3, 3])
    assert w.leaf_index(2) == 1
    # two siblings share their parent's bound: the one added first (the left child) is taken
    w = _workspace([5.0, 4.0, 4.0], [1, 2, 2])
    assert w.leaf_index(2) == 1
    taken = w.choose_leaf(2)
    assert taken.lower == 4.0 and [lf.lower for lf in w.leaves] == [5.0, 4.0]  # the rest keeps its order


def test_minimum_at_the_end_of_the_list():
    w = _workspace([3.0, 2.5, 2.0, 1.5, 0.5], [4, 3, 2, 1, 1])
    assert w.leaf_index(2) == 4
    assert w.leaf_index(3) == 0  # no incumbent: the first deepest


def test_the_root_bound_is_minus_infinity():
    w = _workspace([-np.inf], [0])
    assert w.leaf_index(2) == 0 and w.leaf_index(3) == 0
    w = _workspace([1.0, -np.inf, -np.inf, 0.5], [2, 0, 0, 3], upper=7.0)
    assert w.leaf_index(2) == 1 and w.leaf_index(3) == 1


def test_rule_3_with_and_without_an_incumbent():
    lowers, depths = [2.0, 1.0, 3.0, 1.0], [1, 2, 3, 3]
    w = _workspace(lowers, depths)
    assert w.leaf_index(3) == w.leaf_index(0) == 2  # the first deepest
    assert w.leaf_index(2) == 1
    w = _workspace(lowers, depths, upper=10.0)
    assert w.leaf_index(3) == w.leaf_index(2) == 1
    assert w.leaf_index(0) == 2 and w.leaf_index(1) == 2  # rule 1, phase two: the LARGEST bound, as before


def test_the_choice_after_set_x0(oracle_mod):
    pr = problems.random_miqp(50, 100, 10, seed=1)
    x_opt = np.array(_model(pr, oracle_mod, qp_extra=dict(rho=0.1)).solve().x, dtype=float)
    model = _model(pr, oracle_mod, qp_extra=dict(rho=0.1), tree_explor_rule=3)
    w = model.work
    root = w.leaves[0]
    mk = lambda lo, d: bnb.Node(w.data, root.l, root.u, w.solver, depth=d, lower=lo, constant=w.constant)  # noqa: E731
    w.leaves = [root, mk(-3.0, 1), mk(-5.0, 2), mk(-5.0, 4)]
    assert np.isinf(w.upper_glob) and w.leaf_index(3) == 3  # no incumbent: by depth
    model.set_x0(x_opt)
    assert np.isfinite(w.upper_glob)
    assert w.leaf_index(3) == 0  # an incumbent from outside counts at once: the root's -inf is the smallest bound
    w.leaves = w.leaves[1:]
    assert w.leaf_index(3) == 1 and w.leaf_index(2) == 1
    model.set_x0(np.full(w.data.n, 0.5))  # refused ("Invalid initial solution!"): no incumbent again
    assert np.isinf(w.upper_glob) and w.leaf_index(3) == 2


# -- 2. settings ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", [4, -1, 2.5])
def test_unknown_rules_are_refused_at_setup(oracle_mod, rule):
    pr = problems.random_miqp(50, 100, 10, seed=0)
    with pytest.raises(ValueError, match="Tree exploring strategy not recognized"):
        _model(pr, oracle_mod, tree_explor_rule=rule)


@pytest.mark.parametrize("rule", [0, 1, 2, 3])
def test_rules_0_to_3_are_accepted(oracle_mod, rule):
    pr = problems.random_miqp(50, 100, 10, seed=0)
    model = _model(pr, oracle_mod, tree_explor_rule=rule)
    assert bnb.exploration_setting(model.work.settings) == rule
    assert model.solve().status == bnb.MI_SOLVED


# -- 3. whole trees ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trees(oracle_mod):
    out = {}
    for inst in INSTANCES:
        n, m, p, seed = inst
        pr = problems.random_miqp(n, m, p, seed=seed)
        known = problems.instance_digest(pr) == TABLE[inst][0]
        out[inst, "known"] = known
        if not known:
            continue
        for rule, rf in [(0, 0), (1, 0), (2, 0), (3, 0), (1, 1), (3, 1)]:
            model = _model(pr, oracle_mod, qp_extra=dict(rho=0.1), tree_explor_rule=rule, primal_heuristic=rf)
            res = model.solve()
            out[inst, rule, rf] = types.SimpleNamespace(status=res.status, upper=res.upper_glob,
                                                        counts=(model.work.iter_num - 1, model.work.osqp_iter))
    return out


def test_the_instances_are_the_measured_ones(trees):
    unknown = [inst for inst in INSTANCES if not trees[inst, "known"]]
    assert len(unknown) <= MAX_UNKNOWN, "scipy's sampling changed for %r: measure the table again" % unknown


@pytest.mark.parametrize("inst", INSTANCES)
def test_trees_under_the_four_rules(trees, inst):
    if not trees[inst, "known"]:
        pytest.skip("another scipy sampling: not the instance the table was measured on")
    _, r1, r2, r3, r1_rf, r3_rf = TABLE[inst]
    got = {key[1:]: v for key, v in trees.items() if key[0] == inst and key[1] != "known"}
    print("%r: %r" % (inst, {k: (v.counts, v.upper) for k, v in got.items()}))
    assert all(v.status == bnb.MI_SOLVED for v in got.values())
    assert got[1, 0].counts == r1 and got[2, 0].counts == r2 and got[3, 0].counts == r3
    assert got[0, 0].counts == got[1, 0].counts  # rule 1's phase two takes the largest bound: the deepest leaf again
    assert got[1, 1].counts == r1_rf and got[3, 1].counts == r3_rf
    assert got[3, 0].counts[0] <= got[1, 0].counts[0] and got[3, 1].counts[0] <= got[1, 1].counts[0]
    # without the heuristic every rule ends at the same incumbent
    for rule in (0, 2, 3):
        assert abs(got[rule, 0].upper - got[1, 0].upper) <= 1e-5
    # with round and fix the incumbent is a candidate's ADMM answer to eps_abs = eps_rel = 1e-3, and another order of
    # the nodes meets another candidate: the bound is that tolerance relative to the value, as test_round_and_fix_cpu
    # uses between the heuristic on and off.  Measured: at most 5.5e-4 apart ((30,150,15,4): -2.30826 / -2.30771;
    # (80,40,40,2): -6.73859 / -6.73809; (100,200,50,0): -4.25470 / -4.25473), that is 2.4e-4 relative.
    ref = got[1, 0].upper
    for key in ((1, 1), (3, 1)):
        assert abs(got[key].upper - ref) <= 1e-3 * max(1.0, abs(ref))
    assert abs(got[3, 1].upper - got[1, 1].upper) <= 1e-3 * max(1.0, abs(ref))


# -- 4. solve_many through the sequential calls ----------------------------------------------------------------------
def test_solve_many_under_rule_3_is_the_sequential_calls(oracle_mod):
    pr = problems.random_miqp(50, 100, 10, seed=0)
    a, b = (_model(pr, oracle_mod, qp_extra=dict(rho=0.1), tree_explor_rule=3) for _ in range(2))
    rng = np.random.RandomState(3)
    inst = [dict(q=rng.randn(50)) for _ in range(3)]
    want = []
    for d in inst:
        a.update_vectors(q=d["q"].copy())
        r = a.solve()
        want.append((r.status, r.upper_glob, a.work.iter_num - 1, a.work.osqp_iter, np.array(r.x, dtype=float)))
    got = b.solve_many(inst)
    assert len({w[2] for w in want}) > 1 or want[0][2] > 1  # (real trees, not three roots)
    for g, w in zip(got, want):
        assert (g["status"], g["nodes"], g["osqp_iter"]) == (w[0], w[2], w[3])
        assert g["upper_glob"] == w[1]
        np.testing.assert_array_equal(g["x"], w[4])
