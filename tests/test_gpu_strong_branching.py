"""Strong branching on the device (miosqp_qp_strong_branch, csrc/kernels_derived.inc) against its CPU restatement
(Workspace with the oracle backend: the reference's four calls per child on a second solver with max_iter = sb_max_iter,
scores in numpy), and branching rules 1 and 2 over whole trees."""
import numpy as np
import pytest

from golden_cases import load_case, run_case
from miosqp_amd import problems

pytestmark = pytest.mark.gpu

SOLVED, MAX_ITER = 1, -2


def _pair(oracle_mod, pr, rule=1, qp_extra=None, **settings):
    from miosqp_amd import bnb, qp
    st = dict(problems.BNB_SETTINGS, branching_rule=rule, **settings)
    qs = dict(problems.QP_SETTINGS, **(qp_extra or {}))
    out = []
    for backend in (qp, oracle_mod):
        m = bnb.MIOSQP(backend=backend)
        m.setup(pr["P"], pr["q"], pr["A"], pr["l"], pr["u"], pr["i_idx"], pr["i_l"], pr["i_u"], dict(st), dict(qs))
        out.append(m)
    return out


def _nodes(w, count):
    """The root and nodes two levels down (both children of the root's chosen position, then both of theirs), solved
    with the CPU workspace: [(leaf, candidates)] of those still fractional in at least two positions."""
    root = w.leaves.pop()
    root.solve()
    level, out = [root], []
    for depth in range(3):
        nxt = []
        for leaf in level:
            if leaf.status not in (SOLVED, MAX_ITER) or w.is_int_feas(leaf.x, leaf) or len(leaf.frac_idx) < 2:
                continue
            if depth in (0, 2):
                out.append((leaf, w._most_fractional(leaf, sorted(leaf.frac_idx), w.sb["K"])))
            if depth < 2:
                w.pick_nextvar(leaf)
                w.branch_children(leaf)
                for child in w.leaves[-2:]:
                    child.solve()
                    nxt.append(child)
                del w.leaves[-2:]
        level = nxt
    return out[:count]


def _rel(a, b):
    return abs(a - b) / max(1.0, abs(b))


@pytest.mark.parametrize("rho", [0.1, "auto"])
@pytest.mark.parametrize("cfg", ["cfg1", "cfg2"])
def test_device_entry_equals_the_cpu_restatement(oracle_mod, cfg, rho):
    c = problems.CONFIGS[cfg]
    pr = problems.random_miqp(c["n"], c["m"], c["p"], density=c["density"], seed=0)
    g, o = _pair(oracle_mod, pr, qp_extra=dict(rho=rho))
    nodes = _nodes(o.work, 4)
    assert len(nodes) >= 2 and nodes[0][0].depth == 0 and any(lf.depth == 2 for lf, _ in nodes)
    for leaf, cand in nodes:
        rg = g.work.strong_branch(leaf, cand)
        ro = o.work.strong_branch(leaf, cand)
        np.testing.assert_array_equal(rg.status, ro.status)
        np.testing.assert_array_equal(rg.iter, ro.iter)
        for b in range(2 * len(cand)):
            if ro.status[b] in (SOLVED, MAX_ITER):
                assert _rel(rg.lower[b], ro.lower[b]) <= 1e-9, (b, rg.lower[b], ro.lower[b])
            else:
                assert np.isnan(rg.lower[b])
        assert rg.chosen == ro.chosen
        assert rg.iters == int(np.sum(ro.iter)) and rg.device_time > 0
    assert g.work.sb_stats["calls"] == len(nodes)


@pytest.mark.parametrize("rule", [1, 2])
@pytest.mark.parametrize("name", ["cfg1_n50m100p10_s0", "n30m150p15_s4", "mpc_n12m30p6_s8"])
def test_whole_trees_gpu_equal_cpu(oracle_mod, name, rule):
    from miosqp_amd import qp
    runs = []
    for backend in (qp, oracle_mod):
        case = load_case(name)
        case["settings"] = dict(case["settings"], branching_rule=rule)
        runs.append(run_case(case, backend))
    cols = load_case(name)["cols"]
    nv = cols.index("nextvar_idx")
    assert len(runs[0]) == len(runs[1])
    for a, b in zip(*runs):
        assert a["status"] == b["status"]
        assert a["iter_num"] == b["iter_num"]
        np.testing.assert_array_equal(a["trace"][:, nv], b["trace"][:, nv])
        if np.isfinite(b["upper_glob"]):
            assert abs(a["upper_glob"] - b["upper_glob"]) <= 1e-9 * max(1.0, abs(b["upper_glob"]))
        else:
            assert a["upper_glob"] == b["upper_glob"]


def test_config2_closes_under_strong_branching():
    from miosqp_amd import bnb
    c = problems.CONFIGS["cfg2"]
    pr = problems.random_miqp(c["n"], c["m"], c["p"], density=c["density"], seed=0)
    res = {}
    for rule in (0, 1):
        m = bnb.MIOSQP()
        m.setup(pr["P"], pr["q"], pr["A"], pr["l"], pr["u"], pr["i_idx"], pr["i_l"], pr["i_u"],
                dict(problems.BNB_SETTINGS, branching_rule=rule), dict(problems.QP_SETTINGS))
        r = m.solve()
        res[rule] = (r, m.work.iter_num, dict(m.work.sb_stats))
    (r0, n0, _), (r1, n1, sb1) = res[0], res[1]
    assert r0.status == "Solved" and r1.status == "Solved"
    assert abs(r1.upper_glob - r0.upper_glob) <= 1e-3 * max(1.0, abs(r0.upper_glob))
    assert sb1["calls"] > 0 and sb1["osqp_iter"] > 0
    print("config 2 seed 0: rule 0 %d nodes, rule 1 %d nodes, %d strong-branching calls" % (n0, n1, sb1["calls"]))


def test_strong_branch_leaves_no_state_behind(oracle_mod):
    c = problems.CONFIGS["cfg1"]
    pr = problems.random_miqp(c["n"], c["m"], c["p"], density=c["density"], seed=0)
    g, o = _pair(oracle_mod, pr)
    leaf, cand = _nodes(o.work, 1)[0]
    eng = g.work.solver
    r1 = eng.solve_node(leaf.l, leaf.u, leaf.x, leaf.y)
    sb = eng.strong_branch(leaf.l, leaf.u, leaf.x, leaf.y, leaf.lower, cand, 50, 1e-6)
    assert len(sb.status) == 2 * len(cand)
    r2 = eng.solve_node(leaf.l, leaf.u, leaf.x, leaf.y)
    np.testing.assert_array_equal(r1.x, r2.x)
    np.testing.assert_array_equal(r1.y, r2.y)
    assert (r1.status_val, r1.iter, r1.lower) == (r2.status_val, r2.iter, r2.lower)
    assert (r1.digest.int_inf, r1.digest.nextvar, r1.digest.heur_obj) == (r2.digest.int_inf, r2.digest.nextvar,
                                                                          r2.digest.heur_obj)
    # and a second identical call is bit-identical
    sb2 = eng.strong_branch(leaf.l, leaf.u, leaf.x, leaf.y, leaf.lower, cand, 50, 1e-6)
    np.testing.assert_array_equal(sb.lower, sb2.lower)
    np.testing.assert_array_equal(sb.score, sb2.score)
    assert sb.chosen == sb2.chosen


def test_strong_branch_argument_checks(oracle_mod):
    c = problems.CONFIGS["cfg1"]
    pr = problems.random_miqp(c["n"], c["m"], c["p"], density=c["density"], seed=0)
    g, o = _pair(oracle_mod, pr)
    leaf, cand = _nodes(o.work, 1)[0]
    eng = g.work.solver
    p = len(pr["i_idx"])
    for bad in (dict(cand=[]), dict(cand=list(range(33))), dict(max_iter=30), dict(max_iter=0), dict(cand=[0, p]),
                dict(cand=[3, 1])):
        kw = dict(cand=cand, max_iter=50)
        kw.update(bad)
        with pytest.raises(RuntimeError):
            eng.strong_branch(leaf.l, leaf.u, leaf.x, leaf.y, leaf.lower, kw["cand"], kw["max_iter"], 1e-6)
    lbad = leaf.l.copy()
    lbad[0] = leaf.u[0] + 1.0
    with pytest.raises(ValueError):
        eng.strong_branch(lbad, leaf.u, leaf.x, leaf.y, leaf.lower, cand, 50, 1e-6)


def test_streaming_searches_refuse_rules_1_and_2():
    from miosqp_amd import bnb, stream
    c = problems.CONFIGS["cfg1"]
    pr = problems.random_miqp(c["n"], c["m"], c["p"], density=c["density"], seed=0)
    m = bnb.MIOSQP()
    m.setup(pr["P"], pr["q"], pr["A"], pr["l"], pr["u"], pr["i_idx"], pr["i_l"], pr["i_u"],
            dict(problems.BNB_SETTINGS, branching_rule=2), dict(problems.QP_SETTINGS))
    with pytest.raises(ValueError):
        stream.StreamSearch(m, columns=64, capacity=4096)
    with pytest.raises(ValueError):
        stream.NativeStreamSearch(m, columns=64, capacity=4096)
