"""The instances of the set-up kernel tests (test_setup_reference_cpu.py, test_gpu_setup_kernels.py) and their
references, built once per process and shared."""
import numpy as np
import scipy.sparse as spa

import setup_reference as sr
from miosqp_amd import problems

# (n, m, p) around the 64-wide tiles of dense_setup.hip: a lone partial tile; one short of, exactly and one past a
# tile; two exact tiles (the `je >= n` break after a full block); two tiles plus one row; ld != n with M = 150 no
# multiple of 16 (ks_kkt_inverse starts its row loop at a rounded-down i0 > 0 in the last tile row)
SHAPES = [(3, 2, 1), (63, 20, 5), (64, 20, 5), (65, 20, 5), (128, 30, 10), (129, 30, 10), (200, 50, 100)]
SMALL = (10, 5, 2)          # the register-resident loop's second shape
DEV2 = (200, 150, 100)      # n + M = 450 > 400: rho="auto" probes on the engine itself and refactors on the device
RHO, SIGMA, PASSES = 0.1, 1e-6, 10  # the engine's defaults, which problems.QP_SETTINGS leaves alone


def seed_of(shape):
    return shape[0]


def instance(shape):
    """(pr, P csc, A_ext csc, l, u) of one shape"""
    n, m, p = shape
    pr = problems.random_miqp(n, m, p, seed=seed_of(shape))
    A, l, u = problems.extended(pr)
    P = spa.csc_matrix(pr["P"])
    P.sort_indices()
    A.sort_indices()
    return pr, P, A, l, u


def reference(shape, rho=RHO, inverses=True):
    """(long double, float64) set-up products of one shape (setup_reference.products: shared, read-only)"""
    pr, P, A, _, _ = instance(shape)
    Pd = np.triu(P.toarray())  # the engine reads the upper triangle only
    Pd = Pd + np.triu(Pd, 1).T
    return sr.products(("random_miqp",) + tuple(shape), Pd, A.toarray(), np.asarray(pr["q"]), rho=rho, sigma=SIGMA,
                       passes=PASSES, inverses=inverses)


def check(name, Z, ref_ld, ref_64, n):
    """The tolerance rule for one product; returns (floor, device error) and prints them"""
    floor, got = sr.err(ref_64, ref_ld), sr.err(Z, ref_ld)
    print("setup-rule %-6s n=%-4d floor %.3e  measured %.3e  bound %.3e" % (name, n, floor, got, sr.bound(floor, n)))
    assert floor < 1e-8, (name, floor)  # the instance is sane: the textbook algorithm itself resolves it
    assert got <= sr.bound(floor, n), (name, got, floor, sr.bound(floor, n))
    return floor, got
