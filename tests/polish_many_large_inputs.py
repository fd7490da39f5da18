"""Inputs of the polish_many_large tests (test_polish_many_large_cpu.py, test_gpu_polish_many_large.py) and of
tools/probes/polish_many_large.py: the table of cases beyond one workgroup's LDS (n > 192 or M > 256), one case both
kernels take, and the two indefinite problems of the bad-pivot exits.  The helpers are polish_many_inputs'; what the
long-double reference must say about every case is asserted on the CPU by test_polish_many_large_cpu.py.

The kernel's panel and block width is 32 and its update tile 64: n = 255, 256, 257 lie on both edges (k 32 - 1, k 32,
k 32 + 1 with k = 8), 193 = 6 x 32 + 1, 224 = 7 x 32, 320 = 10 x 32."""
import polish_many_inputs as inputs
from polish_many_inputs import _edge, _random, _structured

PROBLEMS = {
    "r193_s0": _random((193, 4, 2), 0), "r255_s0": _random((255, 30, 5), 0), "r256_s1": _random((256, 30, 5), 1),
    "r257_s0": _random((257, 40, 5), 0), "r320_s0": _random((320, 60, 8), 0), "r224x300_s0": _random((224, 300, 10), 0),
    "r200x300_s1": _random((200, 300, 10), 1),
    "sparse5_n300": _structured("sparse_rows", n=300, m=120, p=10, density=0.05, seed=5),
    "r50_s1": inputs.PROBLEMS["r50_s1"],
}

# expect: as polish_many_inputs.EDGES
CASES = [
    _edge("r193_s0", "first", "r193_s0", "crude", 5, B=2, accepted=True, rounds=(0, 0)),
    _edge("r255_s0", "panel", "r255_s0", "crude", 5, B=2, accepted=True),
    _edge("r256_s1", "panel", "r256_s1", "crude", 5, B=2, accepted=True, rounds=(2, 3)),
    _edge("r257_s0", "panel", "r257_s0", "crude", 5, B=2, accepted=True, rounds=(3, 3)),
    _edge("r257_s0_refine0", "settings", "r257_s0", "crude", 5, B=2, refine_iter=0, accepted=True, rounds=(3, 3)),
    _edge("r257_s0_empty", "empty", "r257_s0", "empty", 20, B=2, accepted=True, reason0=2, rounds=(7, 8), added=(75, 83)),
    _edge("r320_s0", "panel", "r320_s0", "crude", 5, B=1, accepted=True, rounds=(4, 4)),
    _edge("r224x300_s0_limit", "rows", "r224x300_s0", "crude", 5, B=2, accepted=False, reason=2, stop=1, rounds=(5, 5)),
    _edge("r224x300_s0", "rows", "r224x300_s0", "crude", 20, B=2, accepted=True, rounds=(11, 13), moves=True),
    _edge("r200x300_s1", "rows", "r200x300_s1", "crude", 20, B=2, accepted=True, rounds=(12, 12)),
    _edge("sparse5_n300", "sparse", "sparse5_n300", "crude", 5, B=2, accepted=True, rounds=(0, 0)),
    _edge("r50_s1", "both", "r50_s1", "crude", 5, B=4, accepted=True),
]
CASE = {c.name: c for c in CASES}
GROUPS = ("first", "panel", "settings", "empty", "rows", "sparse", "both")

# (n, k) of polish_many_inputs.indefinite_problem: the bad pivot in the last panel and in a middle one
INDEFINITE = ((200, 196), (257, 130))

_MADE = {}


def case_inputs(backend, case):
    """(Data, Q, L, U, X, Y) of one case; made once per (problem, kind, B)"""
    key = (case.prob, case.kind, case.B)
    if key not in _MADE:
        make = dict(crude=inputs.crude_inputs_of, empty=inputs.empty_inputs_of)[case.kind]
        _MADE[key] = make(backend, PROBLEMS[case.prob](), case.B)
    return _MADE[key]


def case_references(case, data):
    """[(long double, float64)] records per instance (polish_many_inputs.edge_references: computed once, shared)"""
    return inputs.edge_references(case, data)
