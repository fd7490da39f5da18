"""solve_models(..., large="device") on the HIP engine (needs an MI355X): models beyond one workgroup's product form
(n + M > 192, or more than 160 KB of LDS: `tree_form()` 0) run their trees in the same call, by k_tree_r_m -- one
workgroup per model, the packed triangle of L^-1 in LDS, the relaxation in reduced form (csrc/tree_reduced_body.hpp).

The contract of such a model is not bit-for-bit equality with the sequential path (that path sums on the cooperative grid
in another order), but:
  decisions -- status, nodes, osqp_iter equal to the CPU oracle backend's tree for the same model and instance;
  values    -- x equal at the integer positions, upper_glob within 1e-8 relative, x within 1e-6 relative (the tolerances
               of test_power_converter_steps_as_one_batch);
  position  -- bit for bit the same whatever the list around the model.
Models of the existing forms in the same call are bit for bit what solve_models without the keyword gives.  The oracle's
tree of a (shape, rule, rho, instance) is computed once per session and shared."""
import numpy as np
import pytest

from miosqp_amd import problems

pytestmark = pytest.mark.gpu

LARGE = [(60, 125, 8, 0), (60, 125, 8, 1), (120, 60, 13, 0), (120, 60, 13, 1), (80, 120, 20, 1), (80, 120, 20, 2),
         (50, 200, 10, 0), (150, 100, 5, 3), (100, 200, 15, 2), (20, 530, 4, 0), (150, 300, 20, 1)]
SMALL = [(10, 5, 2, 0), (50, 100, 10, 0), (40, 60, 20, 2)]  # forms 1, 2, 2
# the eleven interleaved with the three: positions 2, 7 and 11 hold the existing forms
LIST = LARGE[:2] + SMALL[:1] + LARGE[2:6] + SMALL[1:2] + LARGE[6:9] + SMALL[2:] + LARGE[9:]
RHOS = [0.1, "auto"]
SPARSE = (60, 300, 8, 0)  # at density 0.1: the packed rows of Abar fit the LDS behind everything else


def _problem(shape):
    n, m, p, seed = shape
    if shape == SPARSE:
        return problems.random_miqp(n, m, p, density=0.1, seed=seed)
    return problems.random_miqp(n, m, p, seed=seed)


def _build(shape, rule, rho, backend=None, **st):
    from miosqp_amd import bnb
    pr = _problem(shape)
    mdl = bnb.MIOSQP() if backend is None else bnb.MIOSQP(backend=backend)
    mdl.setup(pr["P"], pr["q"], pr["A"], pr["l"].copy(), pr["u"].copy(), pr["i_idx"], pr["i_l"], pr["i_u"],
              dict(problems.BNB_SETTINGS, tree_explor_rule=rule, **st), dict(problems.QP_SETTINGS, rho=rho))
    return mdl, pr


def _variant(pr, kind, k=0):
    """the instance variants of tests/test_gpu_solve_models.py"""
    n, m = len(pr["q"]), len(pr["l"])
    rng = np.random.RandomState(100 + k)
    if kind == "qlu":
        return dict(q=pr["q"] + 0.1 * rng.randn(n), l=pr["l"] - 0.05 * rng.rand(m), u=pr["u"] + 0.05 * rng.rand(m))
    if kind == "x0_valid":
        x0 = np.zeros(n)
        x0[pr["i_idx"][0]] = 1.0
        return dict(x0=x0)
    if kind == "x0_invalid":
        return dict(x0=np.full(n, 0.5))
    if kind == "closed":
        b = 50.0 * (1 - 2 * (np.arange(m) % 2))
        return dict(l=b, u=b.copy())
    assert kind == "plain"
    return {}


_ORACLE = {}


def _oracle(shape, rule, rho, kind="plain", k=0):
    """the CPU oracle backend's tree: bnb.MIOSQP(backend=oracle).solve_many([instance])[0]"""
    key = (shape, rule, rho, kind, k)
    if key not in _ORACLE:
        from oracle import oracle
        mdl, pr = _build(shape, rule, rho, backend=oracle)
        _ORACLE[key] = mdl.solve_many([_variant(pr, kind, k)])[0]
    return _ORACLE[key]


def rel(a, b):
    return np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b)))


def _contract(g, w, ii, who):
    from miosqp_amd import bnb
    has = w["status"] in (bnb.MI_SOLVED, bnb.MI_MAX_ITER_FEASIBLE)
    print("%s: %s %d nodes %d iterations %.17g | oracle %s %d %d %.17g%s"
          % (who, g["status"], g["nodes"], g["osqp_iter"], g["upper_glob"], w["status"], w["nodes"], w["osqp_iter"], w["upper_glob"],
             "  x apart %.3e" % rel(g["x"], w["x"]) if has and g["status"] == w["status"] else ""))
    assert (g["status"], g["nodes"], g["osqp_iter"]) == (w["status"], w["nodes"], w["osqp_iter"]), who
    if has:
        np.testing.assert_array_equal(g["x"][ii], w["x"][ii])
        assert abs(g["upper_glob"] - w["upper_glob"]) <= 1e-8 * max(1.0, abs(w["upper_glob"])), who
        assert rel(g["x"], w["x"]) <= 1e-6, who
    else:
        assert g["upper_glob"] == w["upper_glob"] == np.inf, who


def _bitwise(g, w, who):
    assert (g["status"], g["nodes"], g["osqp_iter"]) == (w["status"], w["nodes"], w["osqp_iter"]), who
    assert g["upper_glob"] == w["upper_glob"], who
    np.testing.assert_array_equal(g["x"], w["x"], err_msg=who)


def _close(models):
    for m in models:
        m.work.solver.close()


@pytest.fixture(scope="module", params=RHOS, ids=["rho0.1", "rho_auto"])
def fourteen(request):
    """the fourteen models (kept open for the module), ONE call with the keyword and one without"""
    import miosqp_amd
    rho = request.param
    models = [_build(s, k % 4, rho)[0] for k, s in enumerate(LIST)]
    info, plain_info = {}, {}
    got = miosqp_amd.solve_models(models, info=info, large="device")
    plain = miosqp_amd.solve_models(models, info=plain_info)
    yield rho, models, got, info, plain, plain_info
    _close(models)


def _forms(models):
    """per position: the form that runs the model with the keyword (1, 2 or 3)"""
    return [m.work.solver.tree_form() or m.work.solver.tree_form_large() for m in models]


def test_eleven_large_models_and_three_small_ones_in_one_call(fourteen):
    rho, models, got, info, plain, plain_info = fourteen
    forms = _forms(models)
    print("forms by position:", forms)
    # what must be beyond the existing forms: the four large shapes of the reference's grid -- (150,300,20) fits the
    # reduced form with 149 KB of the 160 --, the BEYOND model of test_gpu_solve_models.py, a product form above the
    # LDS (120 x 193 doubles) and M > 512 rows; (60,125,8) still fits the workgroup form (147 KB) and keeps it
    for k, s in enumerate(LIST):
        if s[:3] in ((50, 200, 10), (100, 200, 15), (150, 100, 5), (150, 300, 20), (80, 120, 20), (120, 60, 13), (20, 530, 4)):
            assert models[k].work.solver.tree_form() == 0 and forms[k] == 3, (k, s)
    assert [forms[k] for k in (2, 7, 11)] == [1, 2, 2] and 0 not in forms
    assert all(models[k].work.solver.tree_form_large() == 0 for k in range(14) if models[k].work.solver.tree_form() != 0)
    reduced = [k for k in range(14) if forms[k] == 3]
    assert info["forms"] == dict(wave=forms.count(1), group=forms.count(2), reduced=len(reduced)) and info["launches"] == 3
    assert info["launched"] == list(range(14)) and info["own"] == {} and info["overflow"] == []
    assert info["device_time"] > 0
    for k in reduced:
        _contract(got[k], _oracle(LIST[k], k % 4, rho), models[k].work.data.i_idx, "model %d %r rule %d" % (k, LIST[k], k % 4))
    # without the keyword the same models stay out, and the others are bit for bit what they are with it
    assert plain_info["forms"] == dict(wave=forms.count(1), group=forms.count(2))
    assert plain_info["launched"] == [k for k in range(14) if forms[k] != 3] and sorted(plain_info["own"]) == reduced
    assert all(why == "tree_form 0: beyond the one-launch trees" for why in plain_info["own"].values())
    for k in plain_info["launched"]:
        _bitwise(got[k], plain[k], "model %d %r" % (k, LIST[k]))


@pytest.mark.parametrize("order", ["reversed", "rotated", "alone"])
def test_position_independence(fourteen, order):
    import miosqp_amd
    rho, models, first, _, _, _ = fourteen
    forms = _forms(models)
    if order == "alone":
        for k, s in enumerate(LIST):
            if forms[k] == 3:
                info = {}
                g = miosqp_amd.solve_models([models[k]], info=info, large="device")[0]
                assert info["forms"] == dict(wave=0, group=0, reduced=1) and info["launches"] == 1
                _bitwise(g, first[k], "model %d %r alone" % (k, s))
        return
    perm = list(range(13, -1, -1)) if order == "reversed" else [(k + 5) % 14 for k in range(14)]
    info = {}
    got = miosqp_amd.solve_models([models[j] for j in perm], info=info, large="device")
    assert info["forms"] == dict(wave=forms.count(1), group=forms.count(2), reduced=forms.count(3)) and info["own"] == {}
    for k, j in enumerate(perm):
        _bitwise(got[k], first[j], "model %d at position %d" % (j, k))


def test_instances_and_incumbents():
    import miosqp_amd
    from miosqp_amd import bnb
    rho = 0.1
    plan = [(s, kind) for s in ((80, 120, 20, 1), (50, 200, 10, 0)) for kind in ("qlu", "x0_valid", "x0_invalid", "closed")]
    built = [_build(s, k % 4, rho) for k, (s, _) in enumerate(plan)]
    models = [b[0] for b in built]
    insts = [_variant(b[1], kind, k) for k, (b, (_, kind)) in enumerate(zip(built, plan))]
    info = {}
    got = miosqp_amd.solve_models(models, insts, info=info, large="device")
    assert info["forms"] == dict(wave=0, group=0, reduced=8) and info["own"] == {} and info["overflow"] == []
    for k, (s, kind) in enumerate(plan):
        w = _oracle(s, k % 4, rho, kind, k)
        _contract(got[k], w, models[k].work.data.i_idx, "model %d %r %s" % (k, s, kind))
        if kind == "closed":  # no feasible point: the status without an incumbent
            assert got[k]["status"] in (bnb.MI_PRIMAL_INFEASIBLE, bnb.MI_MAX_ITER_UNSOLVED) and got[k]["upper_glob"] == np.inf
    # the valid x0 arrived as an incumbent
    assert models[1]._instance_incumbent(insts[1], *[v[0] for v in models[1]._instance_vectors([insts[1]])]) is not None
    _close(models)


def test_an_overflowed_tree_is_redone_by_its_own_solve_many():
    import miosqp_amd
    rho = 0.1
    shapes, rules = [(10, 5, 2, 0), (80, 120, 20, 1), (50, 100, 10, 0)], [0, 2, 1]
    models = [_build(s, r, rho)[0] for s, r in zip(shapes, rules)]
    info = {}
    got = miosqp_amd.solve_models(models, info=info, large="device", leaf_cap=2)
    assert info["overflow"] == [1] and info["launched"] == [0, 1, 2] and info["forms"] == dict(wave=1, group=1, reduced=1)
    own, _ = _build(shapes[1], rules[1], rho)
    _bitwise(got[1], own.solve_many([{}])[0], "the overflowed tree")
    plain = miosqp_amd.solve_models(models)
    for k in (0, 2):
        _bitwise(got[k], plain[k], "neighbour %d" % k)
    _close(models + [own])


def test_without_the_keyword_nothing_changes():
    import miosqp_amd
    from miosqp_amd import qp
    mdl, _ = _build((80, 120, 20, 1), 1, 0.1)
    small, _ = _build((50, 100, 10, 0), 0, 0.1)
    info = {}
    miosqp_amd.solve_models([mdl, small], info=info)
    assert info["own"] == {0: "tree_form 0: beyond the one-launch trees"} and info["forms"] == dict(wave=0, group=1)
    assert mdl.work.solver.tree_form() == 0
    ms = [small, mdl]
    vec = [m._instance_vectors([{}]) for m in ms]
    sol = [m.work.solver for m in ms]
    args = ([v[0][0] for v in vec], [v[1][0] for v in vec], [v[2][0] for v in vec], [np.zeros(s.n) for s in sol],
            [np.zeros(s.m) for s in sol], [np.inf] * 2, [None] * 2, [0, 1], [1000, 1000])
    assert qp.solve_trees_models(sol, *args) is None  # the existing C entry still declines the engine
    r = qp.solve_trees_models(sol, *args, leaf_cap=256)
    assert r is not None and (r[2].launches, r[2].models_wave, r[2].models_group, r[2].pad) == (2, 0, 1, 1)
    with pytest.raises(ValueError, match="leaf_cap must be at least 2"):
        qp.solve_trees_models(sol, *args, leaf_cap=1)
    _close(ms)


def test_polish_composes():
    import miosqp_amd
    rho = 0.1
    shapes = [(80, 120, 20, 1), (50, 100, 10, 0), (120, 60, 13, 0)]
    models = [_build(s, 1, rho)[0] for s in shapes]
    raw = miosqp_amd.solve_models(models, large="device")
    info = {}
    got = miosqp_amd.solve_models(models, info=info, large="device", polish=True)
    assert info["forms"] == dict(wave=0, group=1, reduced=2)
    assert sorted(info["polished"] + sorted(info["polish_own"])) == [0, 1, 2]  # (whichever polish path takes a model)
    for k, g in enumerate(got):
        assert all(key in g for key in ("polished", "polish_rounds", "pri_after", "dua_after"))
    for k in (0, 2):  # a form-3 model: what its own polish_many makes of the same x
        w = dict(raw[k], x=raw[k]["x"].copy())
        models[k].polish_many([{}], [w])
        for key in ("polished", "polish_rounds", "pri_after", "dua_after", "upper_glob"):
            assert got[k][key] == w[key] or (np.isnan(got[k][key]) and np.isnan(w[key])), (k, key)
        np.testing.assert_array_equal(got[k]["x"], w["x"])
    _close(models)


def test_a_sparse_model_reads_abar_from_lds_copies(monkeypatch):
    """(60,300,8) at density 0.1 is beyond the product form (60 x 369 doubles: 177 KB) while its packed rows fit the LDS
    behind the reduced form's arrays: the launch asks for more LDS than with MIOSQP_RES_SP=0, which keeps them in L2; the
    tree is the oracle's either way, and since only the source of the same rows differs, bit for bit the same."""
    from miosqp_amd import qp
    rho, rule = 0.1, 1
    mdl, _ = _build(SPARSE, rule, rho)
    assert mdl.work.solver.tree_form() == 0 and mdl.work.solver.tree_form_large() == 3
    vec = mdl._instance_vectors([{}])
    sol = [mdl.work.solver]
    args = ([vec[0][0]], [vec[1][0]], [vec[2][0]], [np.zeros(sol[0].n)], [np.zeros(sol[0].m)], [np.inf], [None], [rule], [1000])
    import miosqp_amd
    got = miosqp_amd.solve_models([mdl], large="device")[0]
    _contract(got, _oracle(SPARSE, rule, rho), mdl.work.data.i_idx, "sparse %r" % (SPARSE,))
    X1, i1, s1 = qp.solve_trees_models(sol, *args, leaf_cap=256)
    monkeypatch.setenv("MIOSQP_RES_SP", "0")
    monkeypatch.setenv("MIOSQP_TREE_R_DENSE", "0")
    X0, i0, s0 = qp.solve_trees_models(sol, *args, leaf_cap=256)
    assert s1.lds_bytes > s0.lds_bytes > 0
    assert (i1[0].nodes, i1[0].osqp_iter, i1[0].upper_glob) == (i0[0].nodes, i0[0].osqp_iter, i0[0].upper_glob)
    np.testing.assert_array_equal(X1[0], X0[0])
    mdl.work.solver.close()
