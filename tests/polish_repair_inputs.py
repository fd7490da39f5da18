"""Inputs of the polish-repair tests (test_polish_repair_cpu.py, test_gpu_polish_repair.py): (l, u, x, y) of nodes solved
by the CPU backend, so that the restatement and the device classify the same numbers."""
import numpy as np

from miosqp_amd import problems

SOLVED, MAX_ITER = 1, -2

# the roots after 25 iterations: a crude (x, y) whose guessed set is wrong by several rows
CRUDE = [((50, 100, 10), 1), ((65, 40, 12), 0), ((65, 40, 12), 2), ((129, 30, 10), 0), ((129, 30, 10), 1),
         ((200, 50, 100), 0), ((200, 50, 100), 1)]
# adds / drops summed over the two rounds, measured with the dense numpy restatement
CRUDE_ADDS_DROPS = [(8, 4), (2, 1), (4, 2), (2, 0), (2, 1), (4, 4), (5, 4)]
# n on both sides of the factorisation's 64-wide tile; the seeds are the first whose crude root needs a repair round by
# the restatement (3, 1 and 2 rounds); (64, 20, 5) seed 0 is a fixed point as it comes
TILE_EDGES = [((63, 20, 5), 2), ((64, 20, 5), 1), ((65, 20, 5), 2), ((64, 20, 5), 0)]


def crude_name(shape, seed):
    return "crude_n%dm%dp%d_s%d" % (shape + (seed,))


def model(backend, pr, qp_extra=None, **settings):
    from miosqp_amd import bnb
    m = bnb.MIOSQP(backend=backend)
    m.setup(pr["P"], pr["q"], pr["A"], np.copy(pr["l"]), np.copy(pr["u"]), pr["i_idx"], pr["i_l"], pr["i_u"],
            dict(problems.BNB_SETTINGS, **settings), dict(problems.QP_SETTINGS, **(qp_extra or {})))
    return m


def root_input(backend, pr, **qp_extra):
    """(Data, l, u, x, y) of the root relaxation"""
    w = model(backend, pr, qp_extra=qp_extra).work
    root = w.leaves[0]
    root.solve()
    assert root.status in (SOLVED, MAX_ITER)
    return w.data, root.l.copy(), root.u.copy(), root.x.copy(), root.y.copy()


def incumbent_input(backend, pr, **qp_extra):
    """(Data, l, u, x, y) of the incumbent's node: the integers fixed, re-solved as Workspace.polish_incumbent does"""
    from miosqp_amd import bnb
    m = model(backend, pr, qp_extra=qp_extra)
    res = m.solve()
    assert res.status == bnb.MI_SOLVED
    w, d = m.work, m.work.data
    xi = np.round(res.x[d.i_idx])
    l, u = d.l.copy(), d.u.copy()
    l[d.m:] = xi
    u[d.m:] = xi
    node = bnb.Node(d, l, u, w.solver, x0=np.array(res.x), y0=np.zeros(d.m + d.n_int), constant=w.constant)
    node.solve()
    assert node.status in (SOLVED, MAX_ITER)
    return d, l, u, node.x.copy(), node.y.copy()


def named_inputs(backend, names):
    """name -> (problem, qp_extra, Data, l, u, x, y) for the names asked for"""
    makers = {
        "cfg2_root_rho0.1": lambda: ((500, 1000, 250), 0, dict(rho=0.1), root_input),
        "cfg2_root_auto": lambda: ((500, 1000, 250), 0, dict(rho="auto"), root_input),
        "cfg1_s1_root_rho0.1": lambda: ((50, 100, 10), 1, dict(rho=0.1), root_input),
        "cfg1_s1_incumbent_auto": lambda: ((50, 100, 10), 1, dict(rho="auto"), incumbent_input),
    }
    for shape, seed in CRUDE + TILE_EDGES:
        makers[crude_name(shape, seed)] = \
            lambda shape=shape, seed=seed: (shape, seed, dict(rho=0.1, max_iter=25), root_input)
    out = {}
    for name in names:
        shape, seed, extra, make = makers[name]()
        pr = problems.random_miqp(*shape, seed=seed)
        out[name] = (pr, extra) + make(backend, pr, **extra)
    return out
