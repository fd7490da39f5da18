"""Strong branching (branching_rule 1) and reliability branching (branching_rule 2) on the CPU oracle backend.

Without an engine that has `strong_branch`, Workspace solves the 2K children of a node with the reference's four calls
on a second solver instance (max_iter = sb_max_iter) and scores them in numpy: the restatement the device entry
point miosqp_qp_strong_branch is checked against on the GPU (tests/test_gpu_strong_branching.py).
"""
import types

import numpy as np
import pytest

from golden_cases import case_names, load_case, run_case

SOLVED, MAX_ITER = 1, -2


def _model(case, backend, **settings):
    from miosqp_amd import bnb
    prob = case["prob"]
    model = bnb.MIOSQP(backend=backend)
    model.setup(prob["P"], prob["q"], prob["A"], np.copy(prob["l"]), np.copy(prob["u"]), prob["i_idx"], prob["i_l"],
                prob["i_u"], dict(case["settings"], **settings), case["qp_settings"])
    return model


def _cases():
    return [nm for nm in case_names() if not nm.startswith("rhoauto_")]


def _with_rule(name, rule):
    case = load_case(name)
    case["settings"] = dict(case["settings"], branching_rule=rule)
    return case


# -- 1. settings ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [dict(sb_candidates=0), dict(sb_candidates=33), dict(sb_max_iter=30),
                                 dict(branching_rule=3)])
def test_bad_settings_are_refused_at_setup(oracle_mod, bad):
    case = load_case("cfg1_n50m100p10_s0")
    assert case["qp_settings"].get("check_termination", 25) == 25
    settings = dict(dict(branching_rule=1), **bad)
    with pytest.raises(ValueError):
        _model(case, oracle_mod, **settings)


def test_rule_0_still_equals_the_recorded_trace(oracle_mod):
    case = load_case("cfg1_n50m100p10_s0")
    got = run_case(case, oracle_mod)
    for g, e in zip(got, case["solves"]):
        assert g["iter_num"] == e["iter_num"] and g["osqp_iter"] == e["osqp_iter"]
        np.testing.assert_array_equal(g["trace"], e["trace"])
        assert g["upper_glob"] == e["upper_glob"]


# -- 2. one decision by hand -------------------------------------------------------------------------------------
def _by_hand(oracle_mod, case, leaf, cand, sb_max_iter, eps):
    """The 2K capped children and the section-2 score, with a fresh oracle instance."""
    prob = case["prob"]
    from miosqp_amd import bnb
    data = bnb.Data(prob["P"], prob["q"], prob["A"], np.copy(prob["l"]), np.copy(prob["u"]), prob["i_idx"],
                    prob["i_l"], prob["i_u"])
    o = oracle_mod.OSQP()
    o.setup(data.P, data.q, data.A, data.l, data.u, **dict(case["qp_settings"], max_iter=sb_max_iter))
    m, ii, k = data.m, data.i_idx, data.n_int
    K = len(cand)
    lower, status = np.full(2 * K, np.nan), np.zeros(2 * K, dtype=int)
    for b in range(2 * K):
        c = cand[b % K]
        l, u = leaf.l.copy(), leaf.u.copy()
        if b < K:
            u[m + c] = np.floor(leaf.x[ii[c]])
        else:
            l[m + c] = np.ceil(leaf.x[ii[c]])
        o.update(l=l, u=u)
        o.warm_start(x=leaf.x, y=leaf.y)
        r = o.solve()
        status[b] = r.info.status_val
        if status[b] in (SOLVED, MAX_ITER):
            x = r.x.copy()
            x[ii] = np.minimum(np.maximum(x[ii], l[-k:]), u[-k:])
            lower[b] = .5 * x.dot(data.P.dot(x)) + data.q.dot(x)
    gain = np.where(np.isin(status, (SOLVED, MAX_ITER)), lower - leaf.lower, 1e30)
    gain = np.maximum(gain, 0.0)
    score = np.maximum(gain[:K], eps) * np.maximum(gain[K:], eps)
    return lower, status, score, int(np.argmax(score))


def test_one_decision_pinned_by_hand(oracle_mod):
    case = load_case("cfg1_n50m100p10_s0")
    model = _model(case, oracle_mod, branching_rule=1)
    w = model.work
    K, cap, eps = w.sb["K"], w.sb["max_iter"], w.sb["eps"]
    assert (K, cap, eps) == (8, 50, 1e-6)
    leaf = w.leaves.pop()
    leaf.solve()
    checked = 0
    for depth in range(3):
        assert not w.is_int_feas(leaf.x, leaf)
        if depth in (0, 2):
            xf = leaf.x[w.data.i_idx]
            fr = np.abs(xf - np.round(xf))
            order = sorted(leaf.frac_idx, key=lambda c: (-fr[c], c))
            cand = sorted(order[:K])
            assert len(cand) >= 2
            lower, status, score, chosen = _by_hand(oracle_mod, case, leaf, cand, cap, eps)
            r = w.strong_branch(leaf, cand)
            np.testing.assert_array_equal(r.status, status)
            np.testing.assert_array_equal(r.lower, lower)
            np.testing.assert_array_equal(r.score, score)
            assert r.chosen == chosen
            assert w.select_branching(leaf) == cand[chosen]
            checked += 1
        if depth == 2:
            break
        w.pick_nextvar(leaf)
        w.branch_children(leaf)
        # the first child (down, then up) that is still fractional in at least two positions
        for child in w.leaves[-2:]:
            child.solve()
            if child.status in (SOLVED, MAX_ITER) and not w.is_int_feas(child.x, child) and len(child.frac_idx) >= 2:
                break
        leaf = child
        assert leaf.depth == depth + 1
    assert checked == 2
    assert w.sb_stats["calls"] >= 4 and w.sb_stats["children"] >= 8 and w.sb_stats["osqp_iter"] > 0


# -- 3. reliability bookkeeping ------------------------------------------------------------------------------------
def _recording_backend(oracle_mod, calls):
    class OSQP(oracle_mod.OSQP):
        def strong_branch(self, l, u, x, y, parent_lower, cand, max_iter, eps):
            cand = list(cand)
            calls.append(cand)
            K = len(cand)
            # synthetic children: down gains 0.1 (c + 1), up gains 0.3 (c + 1); the down child of an odd position is
            # infeasible (no observation)
            lower = np.array([parent_lower + 0.1 * (c + 1) for c in cand] + [parent_lower + 0.3 * (c + 1) for c in cand])
            status = np.array([(-3 if c % 2 else 1) for c in cand] + [1] * K, dtype=np.int32)
            from miosqp_amd import bnb
            _, score, chosen = bnb.sb_scores(lower, status, parent_lower, eps, (1, -2))
            return types.SimpleNamespace(chosen=chosen, lower=lower, status=status, iter=np.full(2 * K, 7), score=score,
                                         iters=14 * K, run_time=0.0)

    return types.SimpleNamespace(OSQP=OSQP, constant=oracle_mod.constant)


def test_reliability_bookkeeping(oracle_mod):
    calls = []
    case = load_case("cfg1_n50m100p10_s0")
    model = _model(case, _recording_backend(oracle_mod, calls), branching_rule=2, sb_reliability=1, sb_candidates=3)
    w = model.work
    leaf = w.leaves.pop()
    leaf.solve()
    assert not w.is_int_feas(leaf.x, leaf)
    frac = sorted(leaf.frac_idx)
    assert len(frac) > 3
    ii = w.data.i_idx
    xf = leaf.x[ii]
    fr = np.abs(xf - np.round(xf))
    want = sorted(sorted(frac, key=lambda c: (-fr[c], c))[:3])
    # first decision: nothing observed, every candidate unreliable: the three most fractional are strong-branched
    w.pick_nextvar(leaf)
    assert calls == [want]
    for c in range(w.data.n_int):
        v = leaf.x[ii[c]]
        fd, fu = v - np.floor(v), np.ceil(v) - v
        if c in want:
            assert w.pc_cnt[0, c] == (0 if c % 2 else 1) and w.pc_cnt[1, c] == 1
            assert w.pc_sum[1, c] == pytest.approx(0.3 * (c + 1) / fu, rel=1e-12)
            if c % 2 == 0:
                assert w.pc_sum[0, c] == pytest.approx(0.1 * (c + 1) / fd, rel=1e-12)
        else:
            assert w.pc_cnt[0, c] == w.pc_cnt[1, c] == 0
    # the mean of a direction stands in for positions without observations there
    psi = w.pseudo_costs()
    have_d = [c for c in want if c % 2 == 0]
    mean_d = np.mean([w.pc_sum[0, c] / w.pc_cnt[0, c] for c in have_d]) if have_d else 1.0
    mean_u = np.mean([w.pc_sum[1, c] / w.pc_cnt[1, c] for c in want])
    for c in range(w.data.n_int):
        if c not in want or c % 2:
            assert psi[0, c] == pytest.approx(mean_d, rel=1e-12)
        if c not in want:
            assert psi[1, c] == pytest.approx(mean_u, rel=1e-12)
    # the chosen position: strong-branching score for the three, pseudo-cost score for the others, argmax
    eps = w.sb["eps"]
    x = leaf.x[ii[frac]]
    fd, fu = x - np.floor(x), np.ceil(x) - x
    last = calls[-1]
    scores = []
    for j, c in enumerate(frac):
        if c in last:
            k = last.index(c)
            gd = 1e30 if c % 2 else 0.1 * (c + 1)
            scores.append(max(gd, eps) * max(0.3 * (c + 1), eps))
        else:
            scores.append(max(psi[0, c] * fd[j], eps) * max(psi[1, c] * fu[j], eps))
    assert leaf.nextvar_idx == ii[frac[int(np.argmax(scores))]]
    # second decision on the same node: the three are now reliable in the up direction, the odd ones not down
    w.pick_nextvar(leaf)
    rest = [c for c in frac if c not in want or c % 2]
    assert calls[-1] == sorted(sorted(rest, key=lambda c: (-fr[c], c))[:3])
    assert not set(calls[-1]) & {c for c in want if c % 2 == 0}
    # the children of a rule-2 branching carry what their own solve tells the pseudo-costs
    w.branch_children(leaf)
    c = leaf.constr_idx - w.data.m
    child = w.leaves[-1]
    assert child.pc[:3] == (leaf.lower, c, 1)
    before = (w.pc_sum[1, c], w.pc_cnt[1, c])
    child.solve()
    w.bound_and_branch(child)
    if child.status in (SOLVED, MAX_ITER):
        assert w.pc_cnt[1, c] == before[1] + 1
        assert w.pc_sum[1, c] == pytest.approx(before[0] + max(child.lower - leaf.lower, 0.0) / child.pc[3], rel=1e-12)


def test_no_strong_branching_call_when_every_candidate_is_reliable(oracle_mod):
    calls = []
    case = load_case("cfg1_n50m100p10_s0")
    model = _model(case, _recording_backend(oracle_mod, calls), branching_rule=2, sb_reliability=2)
    w = model.work
    leaf = w.leaves.pop()
    leaf.solve()
    assert not w.is_int_feas(leaf.x, leaf)
    w.pc_cnt[:] = 2
    w.pc_sum[:] = np.arange(1.0, 1.0 + 2 * w.data.n_int).reshape(2, -1)
    w.pick_nextvar(leaf)
    assert calls == []
    psi = w.pc_sum / w.pc_cnt
    frac = sorted(leaf.frac_idx)
    x = leaf.x[w.data.i_idx[frac]]
    sc = [max(psi[0, c] * (v - np.floor(v)), 1e-6) * max(psi[1, c] * (np.ceil(v) - v), 1e-6) for c, v in zip(frac, x)]
    assert leaf.nextvar_idx == w.data.i_idx[frac[int(np.argmax(sc))]]
    # statistics of strong branching stay untouched, and update_vectors resets the pseudo-costs
    assert w.sb_stats == dict(calls=0, children=0, osqp_iter=0, solve_time=0.)
    model.update_vectors(q=case["prob"]["q"])
    assert not w.pc_cnt.any() and not w.pc_sum.any()


# -- 4. / 5. whole trees ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trees(oracle_mod):
    out = {}
    for nm in _cases():
        for rule in (0, 1, 2):
            out[nm, rule] = run_case(_with_rule(nm, rule), oracle_mod)
    return out


def test_thirteen_problems():
    assert len(_cases()) == 13


@pytest.mark.parametrize("rule", [1, 2])
def test_trees_close_correctly(trees, rule):
    for nm in _cases():
        r0, r = trees[nm, 0], trees[nm, rule]
        assert len(r) == len(r0)
        for a, b in zip(r0, r):
            if nm == "n20m100p10_s6_cap" and b["status"] == "Solved":
                continue
            assert b["status"] == a["status"], (nm, rule)
            if a["status"] == "Solved":
                assert abs(b["upper_glob"] - a["upper_glob"]) <= 1e-2 * max(1.0, abs(a["upper_glob"])), nm


def test_strong_branching_explores_fewer_nodes(trees):
    nodes = {rule: sum(o["iter_num"] for nm in _cases() for o in trees[nm, rule]) for rule in (0, 1)}
    assert nodes[1] < nodes[0], nodes


def test_sharded_stream_refuses_rules_1_and_2(oracle_mod):
    from miosqp_amd import dist
    model = _model(load_case("cfg1_n50m100p10_s0"), oracle_mod, branching_rule=1)
    with pytest.raises(ValueError):
        dist.ShardedStream(model)
