"""solve_models on the HIP engine (needs an MI355X): one MIQP on each of several DIFFERENT models -- own P, A, shapes and
settings --, every tree in one call of miosqp_qp_solve_trees_models (k_tree_w_m over the one-wavefront models, k_tree_m
over the one-workgroup models; workgroup b runs entry b of a table in device memory).  The yardstick is the existing
path: every result must be, bit for bit, what a second, separately set-up copy of the model returns from its own
solve_many([instance]) -- status, nodes, iterations, upper_glob, x and the fields of its TreeInfo.  No tolerance anywhere.

The shapes are those tests/test_gpu_explor_rules.py measured (every tree is small); every model has another n, M, p.
The reference of a (shape, rule, rho, instance) is computed once per session and shared."""
import numpy as np
import pytest

from miosqp_amd import problems

pytestmark = pytest.mark.gpu

WAVE = [(10, 5, 2, 0), (10, 5, 2, 1), (10, 5, 2, 2), (10, 5, 2, 3), "pc", (32, 8, 16, 0), (32, 8, 16, 6)]
GROUP = [(50, 100, 10, 0), (50, 100, 10, 1), (40, 60, 20, 2), (60, 80, 30, 3), (50, 25, 25, 1)]
TWELVE = WAVE + GROUP
RHOS = [0.1, "auto"]
INFO_FIELDS = ("nodes", "osqp_iter", "upper_glob", "lower_glob", "leaves_left", "max_leaves", "found", "overflow")
# beyond the one-launch trees: n + M = 220, a product-form factor of 80 x 221 doubles alone is 141 KB of the 160 KB and
# the iterates and the leaf list bring it to 200 KB.  The sequential path closes its tree after 35 nodes (CPU oracle).
BEYOND = (80, 120, 20, 1)


def _problem(inst):
    """(problem dict, B&B settings, QP settings, instance dict)"""
    if inst == "pc":  # the power-converter model's first MIQP with the initial solution its MPC loop hands in
        pc = problems.load_power_converter()
        pr = dict(P=pc["P"], q=pc["q"][0].copy(), A=pc["A"], l=pc["l"].copy(), u=pc["u"][0].copy(), i_idx=pc["i_idx"],
                  i_l=pc["i_l"], i_u=pc["i_u"])
        return pr, dict(pc["settings"]), dict(pc["qp_settings"]), dict(x0=pc["x0"][0].copy())
    n, m, p, seed = inst
    return problems.random_miqp(n, m, p, seed=seed), dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS), {}


def _build(inst, rule, rho, **st):
    """(model, its own instance dict, problem); rule None keeps the settings' own rule (the power converter)"""
    from miosqp_amd import bnb
    pr, settings, qs, own = _problem(inst)
    if rule is not None and inst != "pc":
        settings = dict(settings, tree_explor_rule=rule)
    mdl = bnb.MIOSQP()
    mdl.setup(pr["P"], pr["q"], pr["A"], pr["l"].copy(), pr["u"].copy(), pr["i_idx"], pr["i_l"], pr["i_u"],
              dict(settings, **st), dict(qs, rho=rho))
    return mdl, own, pr


def _variant(pr, kind, k=0):
    """instance dicts by name (deterministic): what tests 4 and 5 hand in"""
    n, m = len(pr["q"]), len(pr["l"])
    rng = np.random.RandomState(100 + k)
    if kind == "qlu":  # another q, a wider box
        return dict(q=pr["q"] + 0.1 * rng.randn(n), l=pr["l"] - 0.05 * rng.rand(m), u=pr["u"] + 0.05 * rng.rand(m))
    if kind == "x0_valid":  # A has entries in [0, 1): 0 <= A x0 < 1 lies inside [l, u] of random_miqp
        x0 = np.zeros(n)
        x0[pr["i_idx"][0]] = 1.0
        return dict(x0=x0)
    if kind == "x0_invalid":  # fractional at the integer positions
        return dict(x0=np.full(n, 0.5))
    if kind == "closed":  # alternating equalities far outside what binaries reach: no integer point (no point) is feasible
        b = 50.0 * (1 - 2 * (np.arange(m) % 2))
        return dict(l=b, u=b.copy())
    assert kind == "plain"
    return {}


_REF = {}


def _ref(inst, rule, rho, kind="own", k=0, **st):
    """what a separately set-up copy of the model returns from solve_many([instance])[0], with its TreeInfo (or None)"""
    key = (inst, rule, rho, kind, k, tuple(sorted(st.items())))
    if key not in _REF:
        mdl, own, pr = _build(inst, rule, rho, **st)
        got = mdl.solve_many([own if kind == "own" else _variant(pr, kind, k)])[0]
        ti = getattr(mdl.work, "trees_info", None)
        fields = None if not ti else {f: getattr(ti[0], f) for f in INFO_FIELDS}
        mdl.work.solver.close()
        _REF[key] = (got, fields)
    return _REF[key]


def _same(g, ref, who):
    from miosqp_amd import bnb
    w, _ = ref
    print("%s: %s %d nodes %d iterations %.17g | own solve_many %s %d %d %.17g"
          % (who, g["status"], g["nodes"], g["osqp_iter"], g["upper_glob"], w["status"], w["nodes"], w["osqp_iter"], w["upper_glob"]))
    assert (g["status"], g["nodes"], g["osqp_iter"]) == (w["status"], w["nodes"], w["osqp_iter"]), who
    assert g["upper_glob"] == w["upper_glob"], who
    assert g["x"].shape == w["x"].shape
    if w["status"] in (bnb.MI_SOLVED, bnb.MI_MAX_ITER_FEASIBLE):  # (without an incumbent solve_many returns np.empty(n))
        np.testing.assert_array_equal(g["x"], w["x"])


def _same_info(mdl, ref, who):
    ti = mdl.work.trees_info
    assert len(ti) == 1
    for f in INFO_FIELDS:
        assert getattr(ti[0], f) == ref[1][f], (who, f)


def _rule(pos):
    return pos % 4


def _close(models):
    for m in models:
        m.work.solver.close()


def _call(shapes, rho, rules=None):
    """builds the models, runs ONE solve_models; returns (models, results, info)"""
    import miosqp_amd
    rules = [_rule(k) for k in range(len(shapes))] if rules is None else rules
    built = [_build(s, r, rho) for s, r in zip(shapes, rules)]
    models, insts = [b[0] for b in built], [b[1] for b in built]
    info = {}
    got = miosqp_amd.solve_models(models, insts, info=info)
    return models, got, info


@pytest.fixture(scope="module", params=RHOS, ids=["rho0.1", "rho_auto"])
def twelve(request):
    rho = request.param
    models, got, info = _call(TWELVE, rho)
    infos = [{f: getattr(m.work.trees_info[0], f) for f in INFO_FIELDS} for m in models]
    forms = [m.work.solver.tree_form() for m in models]
    _close(models)
    return rho, got, info, infos, forms


def test_twelve_different_models_in_one_call(twelve):
    rho, got, info, infos, forms = twelve
    assert info["launches"] == 2 and info["forms"] == dict(wave=7, group=5)
    assert info["own"] == {} and info["overflow"] == [] and info["launched"] == list(range(12))
    assert forms == [1] * 7 + [2] * 5
    assert info["device_time"] > 0
    for k, shape in enumerate(TWELVE):
        ref = _ref(shape, _rule(k), rho)
        _same(got[k], ref, "model %d %r" % (k, shape))
        for f in INFO_FIELDS:
            assert infos[k][f] == ref[1][f], (k, f)
    # block b read model b: every tree is its model's own; under rule 2 at rho 0.1 (60,80,30,3) keeps 66 leaves open
    # (measured in tests/test_gpu_explor_rules.py): the best-bound choice of that workgroup ran over more than a wavefront
    assert rho != 0.1 or infos[10]["max_leaves"] > 64


@pytest.mark.parametrize("order", ["reversed", "shuffled"])
def test_order_does_not_matter(twelve, order):
    rho, first, _, infos, _ = twelve
    perm = list(range(11, -1, -1)) if order == "reversed" else [10, 3, 7, 0, 11, 5, 8, 1, 4, 9, 2, 6]
    assert sorted(perm) == list(range(12))
    models, got, info = _call([TWELVE[j] for j in perm], rho, rules=[_rule(j) for j in perm])
    assert info["launches"] == 2 and info["forms"] == dict(wave=7, group=5) and info["own"] == {}
    for k, j in enumerate(perm):
        g, w = got[k], first[j]
        assert (g["status"], g["nodes"], g["osqp_iter"], g["upper_glob"]) == (w["status"], w["nodes"], w["osqp_iter"], w["upper_glob"])
        np.testing.assert_array_equal(g["x"], w["x"])
        for f in INFO_FIELDS:
            assert getattr(models[k].work.trees_info[0], f) == infos[j][f], (k, j, f)
    _close(models)


@pytest.mark.parametrize("rho", RHOS)
def test_one_form_only_and_single_models(rho):
    for shapes, forms, base in ((WAVE, dict(wave=7, group=0), 0), (GROUP, dict(wave=0, group=5), 7)):
        rules = [_rule(base + k) for k in range(len(shapes))]
        models, got, info = _call(shapes, rho, rules=rules)
        assert info["launches"] == 1 and info["forms"] == forms and info["own"] == {} and info["overflow"] == []
        for k, shape in enumerate(shapes):
            _same(got[k], _ref(shape, rules[k], rho), "%r alone with its form" % (shape,))
        _close(models)
    for pos in (4, 5, 10, 11):  # B = 1: the power converter, a wavefront model, two workgroup models
        models, got, info = _call([TWELVE[pos]], rho, rules=[_rule(pos)])
        assert info["launches"] == 1 and info["launched"] == [0]
        _same(got[0], _ref(TWELVE[pos], _rule(pos), rho), "%r as the only model" % (TWELVE[pos],))
        _same_info(models[0], _ref(TWELVE[pos], _rule(pos), rho), pos)
        _close(models)


def test_instances_and_incumbents(capsys):
    import miosqp_amd
    from miosqp_amd import bnb
    rho = 0.1
    plan = [("pc", None, "own"), ((10, 5, 2, 0), 1, "x0_invalid"), ((10, 5, 2, 1), 2, "x0_valid"), ((32, 8, 16, 0), 1, "qlu"),
            ((50, 100, 10, 0), 0, "closed"), ((40, 60, 20, 2), 2, "qlu"), ((60, 80, 30, 3), 3, "x0_valid"),
            ((50, 25, 25, 1), 1, "qlu")]
    built = [_build(s, r, rho) for s, r, _ in plan]
    models = [b[0] for b in built]
    insts = [b[1] if kind == "own" else _variant(b[2], kind, k) for k, (b, (_, _, kind)) in enumerate(zip(built, plan))]
    refs = [_ref(s, r, rho, kind, k) for k, (s, r, kind) in enumerate(plan)]
    capsys.readouterr()
    info = {}
    got = miosqp_amd.solve_models(models, insts, info=info)
    printed = capsys.readouterr().out
    assert printed.count("Invalid initial solution!") == 1  # model 1's x0, refused and printed as solve_many prints it
    assert info["own"] == {} and info["overflow"] == [] and info["launches"] == 2
    for k in range(len(plan)):
        _same(got[k], refs[k], "model %d %r %s" % (k, plan[k][0], plan[k][2]))
        _same_info(models[k], refs[k], k)
    # the incumbents that were handed in arrived: an upper bound from the first node on
    assert models[2]._instance_incumbent(insts[2], *[v[0] for v in models[2]._instance_vectors([insts[2]])]) is not None
    assert got[4]["status"] in (bnb.MI_PRIMAL_INFEASIBLE, bnb.MI_MAX_ITER_UNSOLVED) and got[4]["upper_glob"] == np.inf
    capsys.readouterr()
    # l > u in one instance: refused by position, nothing queued ...
    bad = list(insts)
    pr5 = built[5][2]
    bad[5] = dict(l=pr5["u"] + 1.0, u=pr5["u"].copy())
    with pytest.raises(ValueError, match="instance 5: Lower bound must be lower than or equal to upper bound"):
        miosqp_amd.solve_models(models, bad)
    # ... also by the library itself, which names the model
    from miosqp_amd import qp
    solvers = [m.work.solver for m in models[4:6]]
    vec = [models[4]._instance_vectors([{}]), models[5]._instance_vectors([bad[5]])]
    with pytest.raises(ValueError, match="model 1"):
        qp.solve_trees_models(solvers, [v[0][0] for v in vec], [v[1][0] for v in vec], [v[2][0] for v in vec],
                              [np.zeros(s.n) for s in solvers], [np.zeros(s.m) for s in solvers], [np.inf, np.inf], [None, None],
                              [0, 0], [1000, 1000])
    # ... and the same call as before gives the same values again
    again = miosqp_amd.solve_models(models, insts)
    for k in range(len(plan)):
        _same(again[k], refs[k], "model %d again" % k)
    _close(models)


def test_mixed_paths():
    """(a model without integer variables is not in the list: MIOSQP.setup does not accept one)"""
    import miosqp_amd
    rho = 0.1
    plan = [(BEYOND, 1, {}), ((50, 100, 10, 0), 0, {}), ((50, 100, 10, 1), 1, dict(branching_rule=1)), ((40, 60, 20, 2), 2, {}),
            ((50, 25, 25, 1), 1, dict(device_tree=False)), ((60, 80, 30, 3), 3, {})]
    built = [_build(s, r, rho, **st) for s, r, st in plan]
    models = [b[0] for b in built]
    assert models[0].work.solver.tree_form() == 0 and models[1].work.solver.tree_form() == 2
    info = {}
    got = miosqp_amd.solve_models(models, info=info)
    assert info["launched"] == [1, 3, 5] and info["launches"] == 1 and info["forms"] == dict(wave=0, group=3)
    assert sorted(info["own"]) == [0, 2, 4] and info["overflow"] == []
    assert "tree_form 0" in info["own"][0] and "branching_rule 1" in info["own"][2] and "device_tree" in info["own"][4]
    for k, (s, r, st) in enumerate(plan):
        _same(got[k], _ref(s, r, rho, "plain", **st), "model %d %r %r" % (k, s, st))
    # no model qualifies: nothing is launched, every model is solved by its own solve_many
    info = {}
    got = miosqp_amd.solve_models([models[2], models[4]], info=info)
    assert info["launched"] == [] and info["launches"] == 0 and sorted(info["own"]) == [0, 1]
    _same(got[0], _ref(plan[2][0], 1, rho, "plain", branching_rule=1), "branching_rule 1 on its own")
    _same(got[1], _ref(plan[4][0], 1, rho, "plain", device_tree=False), "device_tree off on its own")
    _close(models)


def test_the_c_entry_directly():
    from miosqp_amd import qp
    rho = 0.1
    shapes = [(50, 100, 10, 0), (10, 5, 2, 1), (40, 60, 20, 2), "pc", (60, 80, 30, 3), (32, 8, 16, 6)]
    rules = [0, 1, 2, 1, 3, 2]
    built = [_build(s, r, rho) for s, r in zip(shapes, rules)]
    models = [b[0] for b in built]

    def run(which):
        ms = [models[k] for k in which]
        vec = [m._instance_vectors([{}]) for m in ms]
        sol = [m.work.solver for m in ms]
        return qp.solve_trees_models(sol, [v[0][0] for v in vec], [v[1][0] for v in vec], [v[2][0] for v in vec],
                                     [np.zeros(s.n) for s in sol], [np.zeros(s.m) for s in sol], [np.inf] * len(ms),
                                     [None] * len(ms), [m.work.settings["tree_explor_rule"] for m in ms],
                                     [m.work.settings["max_iter_bb"] for m in ms])

    def check(which, r):
        X, infos, stats = r
        for j, k in enumerate(which):
            want = _ref(shapes[k], rules[k], rho, "plain")
            for f in INFO_FIELDS:
                assert getattr(infos[j], f) == want[1][f], (k, f)
            if want[1]["found"]:
                x = X[j].copy()
                ii = models[k].work.data.i_idx
                x[ii] = np.round(x[ii])
                np.testing.assert_array_equal(x, want[0]["x"])
        return stats

    # an engine listed twice: refused, both positions named
    with pytest.raises(RuntimeError, match="model 0 is listed again as model 2"):
        run([0, 1, 0])
    # an engine beyond the one-launch trees: the library declines the call
    beyond, _, _ = _build(BEYOND, 1, rho)
    models.append(beyond)
    shapes.append(BEYOND)
    rules.append(1)
    assert run([0, 6, 1]) is None
    # a small call, then a larger one with the same engine first: the arena grows, the values stay
    s = check([0, 1], run([0, 1]))
    assert (s.launches, s.models_wave, s.models_group) == (2, 1, 1) and s.lds_bytes > 0
    s = check([0, 1, 2, 3, 4, 5], run([0, 1, 2, 3, 4, 5]))
    assert (s.launches, s.models_wave, s.models_group) == (2, 3, 3)
    check([0, 1], run([0, 1]))
    # the engine that owns the arena goes; the others run in a new call, the next engine first
    models[0].work.solver.close()
    s = check([1, 2, 3, 4, 5], run([1, 2, 3, 4, 5]))
    assert (s.launches, s.models_wave, s.models_group) == (2, 3, 2)
    models[1].work.solver.close()
    check([4, 2, 5, 3], run([4, 2, 5, 3]))
    _close(models[2:])
