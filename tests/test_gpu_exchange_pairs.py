"""The exchange ring of the cooperative grid in its pair-unit format (kernels_coop.inc: two untagged values per
16-byte poll, four buffers, a sentinel for "not yet written") on the device: the transport changes no bit of what
travels, so everything the grid computes is what the oracle and the forms without the grid compute."""
import numpy as np
import pytest

from miosqp_amd import problems

pytestmark = pytest.mark.gpu

SOL_TOL = 1e-8  # (tests/test_gpu_parity.py)


def rel(a, b):
    return np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b)))


def _both(oracle_mod, pr, **kw):
    from miosqp_amd import qp
    A, l, u = problems.extended(pr)
    st = dict(problems.QP_SETTINGS, coop=1, resident=0)
    st.update(kw)
    g, o = qp.OSQP(), oracle_mod.OSQP()
    g.setup(pr["P"], pr["q"], A, l, u, **st)
    so = dict(st)
    so.pop("coop"), so.pop("resident")
    o.setup(pr["P"], pr["q"], A, l, u, **so)
    g.set_integer_rows(pr["i_idx"], pr["A"].shape[0])
    assert g.factor_stats()["coop"] is True
    return g, o, A, l, u


def _node_equals_oracle(g, o, pr, l, u, x0, y0):
    rg = g.solve_node(l, u, x0, y0)
    o.update(l=l, u=u)
    o.warm_start(x=x0, y=y0)
    ro = o.solve()
    print("status %s / %s, iterations %d / %d" % (rg.status_val, ro.info.status_val, rg.iter, ro.info.iter))
    assert (rg.status_val, rg.iter) == (ro.info.status_val, ro.info.iter)
    ii, p_int = pr["i_idx"], len(pr["i_idx"])
    xo = ro.x.copy()
    xo[ii] = np.minimum(np.maximum(xo[ii], l[-p_int:]), u[-p_int:])
    print("x %.3g, y %.3g" % (rel(rg.x, xo), rel(rg.y, ro.y)))
    assert rel(rg.y, ro.y) <= SOL_TOL and rel(rg.x, xo) <= SOL_TOL
    lo = 0.5 * xo.dot(pr["P"].dot(xo)) + pr["q"].dot(xo)
    assert abs(rg.lower - lo) <= 1e-9 * max(1.0, abs(lo))
    return rg


def _root_and_children(oracle_mod, pr, **kw):
    g, o, A, l, u = _both(oracle_mod, pr, **kw)
    try:
        n, M, m = pr["P"].shape[0], A.shape[0], pr["A"].shape[0]
        rg = _node_equals_oracle(g, o, pr, l, u, np.zeros(n), np.zeros(M))
        xi = rg.x[pr["i_idx"]]
        k = int(np.argmax(np.abs(xi - np.round(xi))))
        for side in (0, 1):
            l2, u2 = l.copy(), u.copy()
            if side == 0:
                u2[m + k] = np.floor(xi[k])
            else:
                l2[m + k] = np.ceil(xi[k])
            _node_equals_oracle(g, o, pr, l2, u2, rg.x, rg.y)
    finally:
        g.close()


def test_config2_root_and_two_children(oracle_mod):
    _root_and_children(oracle_mod, problems.random_miqp(**problems.CONFIGS["cfg2"], seed=0))


# one layout per number of columns per thread (NR = n + m once the integer rows are out of the exchange; the engine takes
# n + m + p <= 2048): 2 (NR just below 1024), 3 (config 2), 4 (NR just below 2048: the grid takes every CU, none is left
# for testers, the test runs inside the grid)
@pytest.mark.parametrize("n,m,p", [(340, 680, 170), (500, 1000, 250), (600, 1440, 8)])
def test_one_layout_per_columns_per_thread(oracle_mod, n, m, p):
    assert n + m + p <= 2048 and ((n, m, p) == (500, 1000, 250) or n + m in (1020, 2040))
    _root_and_children(oracle_mod, problems.random_miqp(n, m, p, seed=2))


def _search(pr, coop, monkeypatch, max_nodes):
    from miosqp_amd import bnb, search
    monkeypatch.setenv("MIOSQP_COOP", "1" if coop else "0")
    st = dict(problems.BNB_SETTINGS, tree_explor_rule=1, device_tree=False)
    mdl = bnb.MIOSQP()
    mdl.setup(pr["P"], pr["q"], pr["A"], pr["l"], pr["u"], pr["i_idx"], pr["i_l"], pr["i_u"], st,
              dict(problems.QP_SETTINGS, resident=0))
    eng = mdl.work.solver
    assert eng.factor_stats()["coop"] is bool(coop)
    hs = search.HostedSearch(mdl)
    per_node = []
    while hs.nodes < max_nodes:
        before = hs.iters
        if hs.step(1) == 0:
            break
        per_node.append(hs.iters - before)
    out = dict(nodes=hs.nodes, iters=hs.iters, per_node=per_node, upper=float(mdl.work.upper_glob),
               x=None if mdl.work.x is None else np.array(mdl.work.x, dtype=float))
    eng.close()
    return out


def test_hosted_search_on_the_grid_equals_the_search_without_it(monkeypatch):
    """Eighty nodes of config 2: thousands of rounds, the ring wraps from node to node."""
    pr = problems.random_miqp(**problems.CONFIGS["cfg2"], seed=0)
    a = _search(pr, True, monkeypatch, 80)
    b = _search(pr, False, monkeypatch, 80)
    print("nodes %d / %d, iterations %d / %d" % (a["nodes"], b["nodes"], a["iters"], b["iters"]))
    assert a["nodes"] == b["nodes"] >= 60
    assert a["per_node"] == b["per_node"]
    # (the search without the grid runs other instructions -- the factor instead of the explicit inverse in registers -- so
    #  its incumbent agrees to rounding, at the bound tests/test_gpu_parity.py sets for objective values; that the ring
    #  changes no bit is what the benchmark's dumped arrays show against the commit before it)
    print("incumbent %.17g / %.17g" % (a["upper"], b["upper"]))
    assert abs(a["upper"] - b["upper"]) <= 1e-9 * max(1.0, abs(b["upper"]))
    if a["x"] is None:
        assert b["x"] is None
    else:
        assert rel(a["x"], b["x"]) <= SOL_TOL


def test_zeros_signed_zeros_and_infinite_bounds_travel_unchanged(oracle_mod):
    """Free rows (bounds of +-infinity, scaled on the way in), a zero linear term and a zero start: the first rounds carry
    exact zeros of either sign, and none of it may look like 'not yet written'."""
    pr = problems.random_miqp(200, 300, 40, seed=11)
    pr = dict(pr)
    pr["q"] = np.zeros_like(pr["q"])
    lfree, ufree = pr["l"].copy(), pr["u"].copy()
    lfree[::3] = -np.inf
    ufree[::3] = np.inf
    lfree[1::3] = np.minimum(lfree[1::3], 0.0)
    ufree[1::3] = np.maximum(ufree[1::3], 0.0)
    pr["l"], pr["u"] = lfree, ufree
    g, o, A, l, u = _both(oracle_mod, pr)
    try:
        n, M = pr["P"].shape[0], A.shape[0]
        _node_equals_oracle(g, o, pr, l, u, np.zeros(n), np.zeros(M))
        _node_equals_oracle(g, o, pr, l, u, -np.zeros(n), -np.zeros(M))
    finally:
        g.close()
