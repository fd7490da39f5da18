"""setup_models(..., prepare="device") on the HIP engine (needs an MI355X): the models of the call hand their RAW problem
to the device, and one more launch ahead of the set-up launches (k_prepare_models, one workgroup per model) equilibrates
it and packs the rows, where the host does both otherwise (scale_problem, pack_factor_rows).

The contract is bit for bit: everything below compares a call WITH the keyword with the same call WITHOUT it by
assert_array_equal -- the scalings, the panels on the device and in the host's mirror, the factors, the product form with
the scaled q and bounds, the chosen rho, and the trees.  tests/test_prepare_models_cpu.py shows the same for the phases run
on the CPU; what only the device can show is that its 1 / sqrt(.) and its divisions are correctly rounded as the host's
are: D, E and c here are ten passes of them.

The shared lists are built once per module, read-only, and closed at the end."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as spa

import setup_cases as sc
from miosqp_amd import problems

pytestmark = pytest.mark.gpu

# (shape, rho): small fixed, large auto, large fixed, large auto, large fixed with M above twice the workgroup, small auto,
# and the two sides of the threshold between the launches (n + M = 192, 193)
LIST = [((10, 5, 2), 0.1), ((20, 170, 4), "auto"), ((100, 90, 3), 0.1), ((50, 200, 10), "auto"), ((20, 530, 4), 0.1),
        ((3, 2, 1), "auto"), ((100, 80, 12), 0.1), ((100, 81, 12), 0.1)]
AUTO_KEYS = dict(rho_auto="device", large="device", large_rho_auto="device")


def _entry(e):
    """(problem, qp settings) of a list entry: (shape, rho) or (problem dict, settings dict)"""
    if isinstance(e[0], dict):
        return e[0], dict(problems.QP_SETTINGS, **e[1])
    return sc.instance(e[0])[0], dict(problems.QP_SETTINGS, rho=e[1])


def _setup(entries, info=None, **kw):
    import miosqp_amd
    both = [_entry(e) for e in entries]
    return miosqp_amd.setup_models([b[0] for b in both], dict(problems.BNB_SETTINGS), [b[1] for b in both], info=info, **kw)


def _close(models):
    for m in models:
        m.work.solver.close()


_SHARED = {}


@pytest.fixture(scope="module", autouse=True)
def _shared_models_are_closed_and_no_group_is_left():
    from miosqp_amd import qp
    live = qp.setup_groups_live()
    yield
    for models, _ in _SHARED.values():
        _close(models)
    _SHARED.clear()
    assert qp.setup_groups_live() == live


def _shared(key, make):
    if key not in _SHARED:
        info = {}
        _SHARED[key] = (make(info), info)
    return _SHARED[key]


FIXED = [(s, 0.1) for s, _ in LIST]


def _auto(prepare):
    """(models, info) of ONE call over LIST with the three existing keywords, with or without the new one"""
    return _shared(("auto", prepare), lambda info: _setup(LIST, info=info, prepare=prepare, **AUTO_KEYS))


def _fixed(prepare):
    """... over the same shapes at a fixed rho with large="device" alone"""
    return _shared(("fixed", prepare), lambda info: _setup(FIXED, info=info, prepare=prepare, large="device"))


def _arrays(g):
    """every array of an engine that the set-up writes or derives, by name"""
    D, E, c = g.scaling()
    out = dict(D=D, E=E, c=np.array([c]), rho=np.array([g.rho()]))
    for w, name in enumerate(("panel by variable", "panel by constraint", "mirror by variable", "mirror by constraint")):
        out[name] = g.debug_panel(w)
    for w, name in enumerate(("d2inv", "Linv", "LinvT")):
        out[name] = g.debug_factor(w)[1]
    residual, _, tripped = g.inverse_guard()
    if g.factor_stats()["resident"] and not tripped:  # (a tripped guard: the engine dropped W and Kc)
        out["W"], out["Kc"] = g.debug_factor(3)[1], g.debug_factor(4)[1]
    out["guard"] = np.array([residual, float(tripped)])
    for w, name in enumerate(("f_rows", "f_GmT", "f_Ad", "f_Atd", "f_Pd", "scaled q", "scaled l", "scaled u")):
        out[name] = g.debug_product_form(w)[1]
    return out


def _same_engine(a, b, who):
    x, y = _arrays(a.work.solver), _arrays(b.work.solver)
    assert sorted(x) == sorted(y), who
    for name in x:
        np.testing.assert_array_equal(x[name], y[name], err_msg="%s: %s" % (who, name))
        # (assert_array_equal takes -0.0 for 0.0: an explicit zero of A is -0.0 in the panel, a pad 0.0)
        np.testing.assert_array_equal(np.signbit(x[name]), np.signbit(y[name]), err_msg="%s: sign of %s" % (who, name))
    return x


@pytest.mark.parametrize("lists", [_auto, _fixed], ids=["rho chosen in the launches", "fixed rho"])
def test_one_call_over_a_mixed_list_bit_for_bit_the_call_without_the_keyword(lists):
    models, info = lists("device")
    plain, pinfo = lists(None)
    assert info["batched"] == pinfo["batched"] == list(range(len(LIST))) and info["own"] == pinfo["own"] == {}
    assert info["prepare"] == list(range(len(LIST))) and pinfo["prepare"] == []
    assert info["launches"] == 3 and pinfo["launches"] == 2  # the new launch ahead of the small and the large one
    assert info["forms"] == pinfo["forms"] == dict(small=3, large=5)
    assert len({m.work.solver.setup_group() for m in models}) == 1
    assert info["rho"] == pinfo["rho"]
    if lists is _auto:
        assert info["rho_auto_large"] == [1, 3] and all(info["rho"][k] != 0.1 for k in (1, 3))
    for k, (a, b) in enumerate(zip(models, plain)):
        got = _same_engine(a, b, "position %d %s" % (k, LIST[k][0]))
        assert np.all(np.isfinite(got["D"])) and np.all(got["D"] > 0) and got["c"][0] > 0
        assert np.any(got["D"] != 1.0) and np.any(got["panel by variable"] != 0.0)  # ten passes ran, the rows are there
    print("setup_models prepare: %d models, device %.3f ms with the keyword, %.3f ms without"
          % (len(LIST), 1e3 * info["device_time"], 1e3 * pinfo["device_time"]))


@pytest.mark.parametrize("lists", [_auto, _fixed], ids=["rho chosen in the launches", "fixed rho"])
def test_trees_bit_for_bit(lists):
    import miosqp_amd
    models, _ = lists("device")
    plain, _ = lists(None)
    ia, ib = {}, {}
    a = miosqp_amd.solve_models(models, info=ia, large="device")
    b = miosqp_amd.solve_models(plain, info=ib, large="device")
    assert ia["own"] == ib["own"] and ia["forms"] == ib["forms"] and ia["overflow"] == ib["overflow"]
    for k in range(len(LIST)):
        who = str(LIST[k][0])
        print("%s: %s %d nodes %d iterations %.17g" % (who, a[k]["status"], a[k]["nodes"], a[k]["osqp_iter"], a[k]["upper_glob"]))
        assert (a[k]["status"], a[k]["nodes"], a[k]["osqp_iter"]) == (b[k]["status"], b[k]["nodes"], b[k]["osqp_iter"]), who
        assert a[k]["nodes"] > 0 and a[k]["osqp_iter"] > 0
        np.testing.assert_array_equal(a[k]["x"], b[k]["x"], err_msg=who)
        assert a[k]["upper_glob"] == b[k]["upper_glob"], who


def _edge(shape, seed, zero_q=False):
    """A problem with the edge inputs of tests/prepare_models_cpu.cpp: an empty column and an empty row of A, a zero column
    of P, explicit zeros in A, a column of [P; A] with norm below 1e-4 and one above 1e4 (continuous variables, so that no
    identity row of the integer bounds fills them in); P stays a full symmetric matrix, positive semidefinite"""
    n, m, p = shape
    pr = dict(problems.random_miqp(n, m, p, seed=seed))
    cont = [j for j in range(n) if j not in set(int(i) for i in pr["i_idx"])]
    jc, jz, jt, jh = cont[:4]
    P, A = pr["P"].toarray(), pr["A"].toarray()
    A[:, jc] = 0.0
    A[1, :] = 0.0
    P[jz, :] = 0.0
    P[:, jz] = 0.0
    d = P[jt, jt]
    P[jt, :] = 0.0  # (alone on its diagonal: a principal block, the matrix stays positive semidefinite)
    P[:, jt] = 0.0
    P[jt, jt] = 1e-14 * max(d, 1.0)
    A[:, jt] *= 1e-7
    P[jh, :] *= 1e7
    P[:, jh] *= 1e7
    A[:, jh] *= 1e7
    A = spa.csc_matrix(A)
    A.sort_indices()
    A.data[::7] = 0.0  # explicit zeros: the entries stay in the pattern
    pr["P"], pr["A"] = spa.csc_matrix(P), A
    assert A.nnz == len(A.data) and np.any(A.data == 0.0) and np.diff(A.indptr)[jc] == 0 and np.diff(pr["P"].indptr)[jz] == 0
    assert len(np.unique(A.indices)) == m - 1
    if zero_q:
        pr["q"] = np.zeros(n)
    return pr


def test_edge_inputs_between_healthy_neighbours():
    small, large = (10, 5, 2), (50, 200, 10)
    entries = [(small, 0.1), (_edge(small, 1), dict(scaling=10)), (large, 0.1), (_edge(large, 2), dict(scaling=1)),
               (_edge(small, 3, zero_q=True), dict(scaling=0)), ((20, 170, 4), 0.1), (_edge(large, 4, zero_q=True), dict(scaling=10)),
               (_edge((12, 6, 2), 5), dict(scaling=1)), (small, 0.1)]
    info, pinfo = {}, {}
    models = _setup(entries, info=info, large="device", prepare="device")
    try:
        plain = _setup(entries, info=pinfo, large="device")
        try:
            assert info["prepare"] == info["batched"] == pinfo["batched"] == list(range(len(entries)))
            for k, (a, b) in enumerate(zip(models, plain)):
                got = _same_engine(a, b, "position %d" % k)
                if k in (4,):  # scaling = 0: D = E = c = 1
                    assert np.all(got["D"] == 1.0) and np.all(got["E"] == 1.0) and got["c"][0] == 1.0
                if k in (1, 3, 4, 6, 7):  # an explicit zero of A is -0.0 in the panel
                    v = got["panel by variable"]
                    assert np.any((v == 0.0) & np.signbit(v))
            # healthy neighbours are what they are in another call
            shared, _ = _fixed("device")
            _same_engine(models[0], shared[0], "neighbour 0")
            _same_engine(models[5], shared[1], "neighbour 5")
            _same_engine(models[8], shared[0], "neighbour 8")
        finally:
            _close(plain)
    finally:
        _close(models)


@pytest.mark.parametrize("order", [[7, 6, 5, 4, 3, 2, 1, 0], [3, 4, 5, 6, 7, 0, 1, 2]], ids=["reversed", "rotated"])
def test_the_result_does_not_depend_on_the_position(order):
    models, info = _auto("device")
    pinfo = {}
    again = _setup([LIST[k] for k in order], info=pinfo, prepare="device", **AUTO_KEYS)
    try:
        assert pinfo["prepare"] == list(range(len(LIST))) and pinfo["launches"] == 3
        for j, k in enumerate(order):
            assert pinfo["rho"][j] == info["rho"][k]
            _same_engine(again[j], models[k], "position %d" % k)
    finally:
        _close(again)


def test_300_small_models_in_one_call():
    import miosqp_amd
    prs = [problems.random_miqp(10, 5, 2, seed=1000 + k) for k in range(300)]
    info, pinfo = {}, {}
    models = miosqp_amd.setup_models(prs, dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS), info=info, prepare="device")
    try:
        plain = miosqp_amd.setup_models(prs, dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS), info=pinfo)
        try:
            assert info["prepare"] == list(range(300)) and info["launches"] == 2 and pinfo["launches"] == 1
            for k in range(300):
                a, b = models[k].work.solver, plain[k].work.solver
                for x, y in zip(a.scaling(), b.scaling()):
                    np.testing.assert_array_equal(x, y, err_msg=str(k))
                for w in (0, 1, 2, 3):
                    np.testing.assert_array_equal(a.debug_panel(w), b.debug_panel(w), err_msg=str(k))
                np.testing.assert_array_equal(a.debug_factor(3)[1], b.debug_factor(3)[1], err_msg=str(k))
                np.testing.assert_array_equal(a.debug_product_form(5)[1], b.debug_product_form(5)[1], err_msg=str(k))
        finally:
            _close(plain)
    finally:
        _close(models)


def test_update_vectors_and_a_solve_read_the_mirrors():
    entries = [((10, 5, 2), 0.1), ((20, 170, 4), 0.1)]
    models = _setup(entries, large="device", prepare="device")
    try:
        plain = _setup(entries, large="device")
        try:
            for k, (a, b) in enumerate(zip(models, plain)):
                pr = sc.instance(entries[k][0])[0]
                rng = np.random.RandomState(5 + k)
                q2 = np.asarray(pr["q"]) + 0.3 * rng.randn(len(pr["q"]))
                l2, u2 = np.asarray(pr["l"]) - 0.1, np.asarray(pr["u"]) + 0.2
                out = []
                for m in (a, b):
                    m.update_vectors(q=q2.copy(), l=l2.copy(), u=u2.copy())
                    out.append(m.solve())
                ra, rb = out
                print("%s: status %s upper %.17g" % (entries[k][0], ra.status, ra.upper_glob))
                assert ra.status == rb.status and ra.upper_glob == rb.upper_glob and ra.osqp_iter_avg == rb.osqp_iter_avg
                np.testing.assert_array_equal(ra.x, rb.x)
                assert a.work.iter_num == b.work.iter_num and a.work.iter_num > 0
                np.testing.assert_array_equal(a.work.solver.debug_product_form(5)[1], b.work.solver.debug_product_form(5)[1])
        finally:
            _close(plain)
    finally:
        _close(models)


def _descriptor(pr, **qs):
    Ae, l, u = problems.extended(pr)
    return dict(P=pr["P"], q=pr["q"], A=Ae, l=l, u=u, i_idx=pr["i_idx"], m_orig=pr["A"].shape[0],
                settings=dict(problems.QP_SETTINGS, **qs))


def test_an_indefinite_p_in_the_middle_of_a_list_fails_the_call_as_it_does_today():
    from miosqp_amd import qp
    n = 20
    p = np.ones(n)
    p[5] = -0.5
    bad = dict(P=spa.diags(p).tocsc(), q=np.cos(1.0 + np.arange(n)), A=(3.0 * spa.identity(n, format="csc")).tocsc(), l=-np.ones(n),
               u=np.ones(n), settings=dict(problems.QP_SETTINGS, scaling=0, rho=0.01))
    small = _descriptor(sc.instance((10, 5, 2))[0])
    live = qp.setup_groups_live()
    texts = []
    for prepare in (False, True):
        with pytest.raises(RuntimeError, match=r"non-positive pivot.*\(model 1, pivot 5\)") as ei:
            qp.setup_models([small, bad, small], prepare=prepare)
        texts.append(str(ei.value))
        assert qp.setup_groups_live() == live
    assert texts[0] == texts[1]


def test_refusals_and_the_value_error():
    import miosqp_amd
    from miosqp_amd import _lib, qp
    live = qp.setup_groups_live()
    small, big = sc.instance((10, 5, 2))[0], sc.instance((20, 170, 4))[0]
    for kw, pattern, models in [
            (dict(), r"does not take this model.*\(model 1\)", [_descriptor(small), _descriptor(big)]),
            (dict(large=True), r"builds a fixed rho only \(model 0\)", [_descriptor(big, rho="auto")]),
            (dict(large=True, large_auto=True), r"does not take this model.*\(model 0\)", [_descriptor(small, rho="auto")]),
            (dict(), r"B must be at least 1", [])]:
        texts = []
        for prepare in (False, True):
            with pytest.raises(RuntimeError, match=pattern) as ei:
                qp.setup_models(models, prepare=prepare, **kw)
            texts.append(str(ei.value))
        assert texts[0] == texts[1]
    # a flag bit the entry does not know
    desc, hs, stats = (_lib.SetupModel * 1)(), (C.c_void_p * 1)(), _lib.SetupModelsStats()
    assert _lib.load().miosqp_qp_setup_models_prepared(1, desc, hs, C.byref(stats), 8) != 0
    assert qp.setup_groups_live() == live
    with pytest.raises(ValueError, match='prepare must be None or "device"'):
        miosqp_amd.setup_models([small], dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS), prepare="host")
    assert qp.setup_groups_live() == live
    # a model that no launch takes is set up by MIOSQP.setup as before, and is not listed
    info = {}
    models = miosqp_amd.setup_models([small, big], dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS), info=info, prepare="device")
    try:
        assert info["batched"] == [0] and info["prepare"] == [0] and list(info["own"]) == [1]
        assert models[1].work.solver.setup_group() is None
    finally:
        _close(models)
    assert qp.setup_groups_live() == live


def test_the_oracle_backend_ignores_the_keyword():
    import miosqp_amd
    from oracle import oracle
    info = {}
    pr = sc.instance((10, 5, 2))[0]
    got = miosqp_amd.setup_models([pr], dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS), info=info, backend=oracle,
                                  prepare="device")
    assert info["prepare"] == [] and info["batched"] == [] and info["launches"] == 0 and len(got) == 1
