"""solve_many / solve_models with heuristic="device": round and fix INSIDE the one-launch trees (miosqp_qp_solve_trees_rf,
miosqp_qp_solve_trees_models_rf; k_tree_rf, k_tree_rf_m, k_tree_rf_r_m) against
  (a) the same call without the keyword -- with primal_heuristic 1 that is the sequential host loop, one device call per
      node and one more per firing (timed on the first min(B, --seq) instances or models: the loop is linear in B);
  (b) the one-launch trees with the heuristic OFF (primal_heuristic 0): the same instances, the plain search.

Workload: random_miqp shapes (40,60,20), (60,80,30), (100,200,15); rho 0.1, rf_candidates 7, rf_max_iter 250, rf_every 3.
  instances: B instances of ONE model (seed 0), each with its own cost -- solve_many; (100,200,15) is beyond one workgroup's
             product form and has no such launch: it appears under models only;
  models:    B models (seed k), one MIQP each -- solve_models(large="device").
B = 1, 8, 64, 256.  Per row: MIQPs/s of the keyword (median of --repeats calls), nodes and firings summed over the call,
MIQPs/s of (a) and of (b) with (b)'s nodes, and the two ratios.  The keyword's trees are compared with (a)'s on the timed
part -- status, nodes, iterations -- and a difference is reported.

    python tools/probes/solve_trees_rf.py [--out profiles/solve_trees_rf.txt] [--batches 1,8,64,256] [--repeats 3] [--seq 16]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = [(40, 60, 20), (60, 80, 30), (100, 200, 15)]


def build(problems, bnb, shape, seed, on):
    pr = problems.random_miqp(*shape, seed=seed)
    m = bnb.MIOSQP()
    m.setup(pr["P"], pr["q"], pr["A"], np.copy(pr["l"]), np.copy(pr["u"]), pr["i_idx"], pr["i_l"], pr["i_u"],
            dict(problems.BNB_SETTINGS, primal_heuristic=on, rf_candidates=7, rf_max_iter=250, rf_every=3),
            dict(problems.QP_SETTINGS, rho=0.1))
    return m


def timed(call, repeats, warm=True):
    if warm:
        call()
    ts = []
    for _ in range(repeats):
        t0 = time.time()
        res = call()
        ts.append(time.time() - t0)
    return res, statistics.median(ts)


def key(res):
    return [(r["status"], r["nodes"], r["osqp_iter"]) for r in res]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="1,8,64,256")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seq", type=int, default=16, help="(a) is timed on the first min(B, SEQ) instances / models")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import miosqp_amd
    from miosqp_amd import bnb, problems
    f = open(a.out, "a") if a.out else None

    def out(s=""):
        print(s, flush=True)
        if f:
            f.write(s + "\n")
            f.flush()

    batches = [int(b) for b in a.batches.split(",") if b]
    head = ("# %-9s %-12s %4s | keyword MIQPs/s    nodes  firings improved | (a) no keyword MIQPs/s | (b) heuristic off MIQPs/s    nodes |"
            " keyword/(a) keyword/(b)")
    out("# heuristic=\"device\" (round and fix inside the one-launch trees) on one MI355X; rho 0.1, K 7, cap 250, every 3; "
        "(a) on the first min(B, %d)" % a.seq)
    out(head % ("workload", "shape", "B"))

    def row(kind, shape, B, tk, rf, nodes_k, ta, na, tb, nodes_b):
        out("  %-9s %-12s %4d | %15.1f %8d %8d %8d | %21.1f | %25.1f %8d | %11.2f %11.2f"
            % (kind, str(shape).replace(" ", ""), B, B / tk, nodes_k, sum(c["calls"] for c in rf), sum(c["improved"] for c in rf),
               na / ta, B / tb, nodes_b, (B / tk) / (na / ta), tb / tk))

    def differ(seq, got):
        bad = [k for k, (x, y) in enumerate(zip(key(seq), key(got))) if x != y]
        if bad:
            out("#   (status, nodes, iterations) of the keyword differ from the sequential path's at %s" % bad)

    for shape in SHAPES[:2]:
        on, off = build(problems, bnb, shape, 0, 1), build(problems, bnb, shape, 0, 0)
        n = on.work.data.n
        for B in batches:
            rng = np.random.RandomState(B)
            inst = [dict(q=on.work.data.q + 0.3 * rng.randn(n)) for _ in range(B)]
            got, tk = timed(lambda: on.solve_many(inst, heuristic="device"), a.repeats)
            rf = list(on.work.trees_rf)
            assert not any(t.overflow for t in on.work.trees_info)
            na = min(B, a.seq)
            seq, ta = timed(lambda: on.solve_many(inst[:na]), 1, warm=False)  # (these engines are warm)
            differ(seq, got[:na])
            plain, tb = timed(lambda: off.solve_many(inst), a.repeats)
            row("instances", shape, B, tk, rf, sum(r["nodes"] for r in got), ta, na, tb, sum(r["nodes"] for r in plain))
        on.work.solver.close()
        off.work.solver.close()
    for shape in SHAPES:
        for B in batches:
            on = [build(problems, bnb, shape, k, 1) for k in range(B)]
            off = [build(problems, bnb, shape, k, 0) for k in range(B)]
            info = {}
            got, tk = timed(lambda: miosqp_amd.solve_models(on, info=info, large="device", heuristic="device"), a.repeats)
            assert not info["own"], info["own"]
            redone = len(info["overflow"])
            na = min(B, a.seq)
            seq, ta = timed(lambda: miosqp_amd.solve_models(on[:na], large="device"), 1, warm=False)
            differ(seq, got[:na])
            plain, tb = timed(lambda: miosqp_amd.solve_models(off, large="device"), a.repeats)
            row("models", shape, B, tk, [info["rf"][k] for k in sorted(info["rf"])], sum(r["nodes"] for r in got), ta, na, tb,
                sum(r["nodes"] for r in plain))
            if redone:
                out("#   (%d of these trees overflowed their leaf list and were redone by their own model: inside the keyword's time)" % redone)
            for m in on + off:
                m.work.solver.close()
    if f:
        f.close()


if __name__ == "__main__":
    main()
