"""solve_many / solve_models with branching="device": strong and reliability branching INSIDE the one-launch trees
(miosqp_qp_solve_trees_sb, miosqp_qp_solve_trees_models_sb; k_tree_sb, k_tree_sb_m, k_tree_sb_r_m) against
  (a) the same call without the keyword -- with branching_rule 1 or 2 that is the sequential host loop, one device call
      per node and one more per strong-branching call.  It runs in a CHILD process, three repeats, on the tree given by
      --parent (a checkout of the parent commit with its library built; default: this tree, whose path without the
      keyword is the parent's), timed on the first min(B, --seq) instances or models: the loop is linear in B;
  (b) the one-launch trees at branching_rule 0: the same instances, the plain search.

Workload: random_miqp shapes (40,60,20) and (50,100,10), the four shapes of the reference's benchmark grid that one
workgroup takes -- (10,5,2), (10,100,2), (50,25,5), (100,50,2) --, and (100,200,15) in the reduced form; rho 0.1,
sb_candidates 8, sb_max_iter 50, sb_reliability 4; rules 1 and 2.
  instances: B instances of ONE model (seed 0), each with its own cost -- solve_many; (100,200,15) is beyond one
             workgroup's product form and has no such launch: it appears under models only;
  models:    B models (seed k), one MIQP each -- solve_models(large="device").
B = 1, 8, 64, 256.  Per row: MIQPs/s of the keyword (median of --repeats calls), nodes and strong-branching calls and
children summed over the call, MIQPs/s of (a) and of (b) with (b)'s nodes, and the two ratios.  The keyword's trees are
compared with (a)'s on the timed part -- status, nodes, iterations -- and a difference is reported.

    python tools/probes/solve_trees_sb.py [--out profiles/solve_trees_sb.txt] [--batches 1,8,64,256] [--repeats 3] [--seq 16]
                                          [--parent DIR] [--shapes 0,1,2,3,4,5,6] [--rules 1,2] [--child-timeout 900]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = [(40, 60, 20), (50, 100, 10), (100, 200, 15), (10, 5, 2), (10, 100, 2), (50, 25, 5), (100, 50, 2)]
REDUCED = (2,)  # beyond one workgroup's product form: no one-launch form for solve_many


def build(problems, bnb, shape, seed, rule):
    pr = problems.random_miqp(*shape, seed=seed)
    m = bnb.MIOSQP()
    m.setup(pr["P"], pr["q"], pr["A"], np.copy(pr["l"]), np.copy(pr["u"]), pr["i_idx"], pr["i_l"], pr["i_u"],
            dict(problems.BNB_SETTINGS, branching_rule=rule, sb_candidates=8, sb_max_iter=50, sb_reliability=4),
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
    return [[r["status"], int(r["nodes"]), int(r["osqp_iter"])] for r in res]


def instances(q, B):
    rng = np.random.RandomState(B)
    return [dict(q=q + 0.3 * rng.randn(len(q))) for _ in range(B)]


def child(a, shapes, rules, batches):
    """(a): the calls without the keyword on the tree at a.root, one JSON line per row"""
    sys.path.insert(0, a.root)
    import miosqp_amd
    from miosqp_amd import bnb, problems
    assert os.path.realpath(os.path.dirname(os.path.dirname(miosqp_amd.__file__))) == os.path.realpath(a.root)
    for rule in rules:
        for si in shapes:
            if si in REDUCED:
                continue
            mdl = build(problems, bnb, SHAPES[si], 0, rule)
            for B in batches:
                na = min(B, a.seq)
                inst = instances(mdl.work.data.q, B)[:na]
                seq, ta = timed(lambda: mdl.solve_many(inst), 3)
                print(json.dumps(dict(kind="instances", rule=rule, shape=si, B=B, na=na, t=ta, key=key(seq))), flush=True)
            mdl.work.solver.close()
        for si in shapes:
            for B in batches:
                na = min(B, a.seq)
                models = [build(problems, bnb, SHAPES[si], k, rule) for k in range(na)]
                seq, ta = timed(lambda: miosqp_amd.solve_models(models, large="device"), 3)
                print(json.dumps(dict(kind="models", rule=rule, shape=si, B=B, na=na, t=ta, key=key(seq))), flush=True)
                for m in models:
                    m.work.solver.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="1,8,64,256")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seq", type=int, default=16, help="(a) is timed on the first min(B, SEQ) instances / models")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: (a) runs there")
    ap.add_argument("--shapes", default="0,1,2,3,4,5,6")
    ap.add_argument("--child-timeout", type=float, default=900.0, help="seconds the child process of (a) may take")
    ap.add_argument("--rules", default="1,2")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    batches = [int(b) for b in a.batches.split(",") if b]
    shapes = [int(s) for s in a.shapes.split(",") if s]
    rules = [int(r) for r in a.rules.split(",") if r]
    if a.child:
        return child(a, shapes, rules, batches)
    # (a) first, in its own process: it has finished before this one opens the GPU
    where = os.path.abspath(a.parent) if a.parent else ROOT
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--root", where, "--batches", a.batches, "--seq", str(a.seq),
                        "--shapes", a.shapes, "--rules", a.rules], capture_output=True, text=True, cwd=where, timeout=a.child_timeout)
    if r.returncode != 0:
        raise SystemExit("the child process of (a) failed:\n" + r.stdout[-2000:] + r.stderr[-4000:])
    base = {}
    for line in r.stdout.splitlines():
        if line.startswith("{"):
            d = json.loads(line)
            base[(d["kind"], d["rule"], d["shape"], d["B"])] = d
    sys.path.insert(0, ROOT)
    import miosqp_amd
    from miosqp_amd import bnb, problems
    f = open(a.out, "a") if a.out else None

    def out(s=""):
        print(s, flush=True)
        if f:
            f.write(s + "\n")
            f.flush()

    head = ("# %-9s %-12s %4s %4s | keyword MIQPs/s    nodes sb calls children | (a) no keyword MIQPs/s | (b) rule 0 MIQPs/s    nodes |"
            " keyword/(a) keyword/(b)")
    out("# branching=\"device\" (strong / reliability branching inside the one-launch trees) on one MI355X; rho 0.1, K 8, cap 50, "
        "reliability 4; (a) in a child process on %s, three repeats, on the first min(B, %d)"
        % ("the parent commit" if a.parent else "this tree", a.seq))
    out(head % ("workload", "shape", "rule", "B"))

    def row(kind, si, rule, B, tk, sb, got, tb, plain):
        d = base[(kind, rule, si, B)]
        bad = [k for k, (x, y) in enumerate(zip(d["key"], key(got[:d["na"]]))) if x != y]
        out("  %-9s %-12s %4d %4d | %15.1f %8d %8d %8d | %21.1f | %18.1f %8d | %11.2f %11.2f"
            % (kind, str(SHAPES[si]).replace(" ", ""), rule, B, B / tk, sum(r["nodes"] for r in got), sum(c["calls"] for c in sb),
               sum(c["children"] for c in sb), d["na"] / d["t"], B / tb, sum(r["nodes"] for r in plain), (B / tk) / (d["na"] / d["t"]),
               tb / tk))
        if bad:
            out("#   (status, nodes, iterations) of the keyword differ from the sequential path's at %s" % bad)

    for rule in rules:
        for si in shapes:
            if si in REDUCED:
                continue
            on, off = build(problems, bnb, SHAPES[si], 0, rule), build(problems, bnb, SHAPES[si], 0, 0)
            for B in batches:
                inst = instances(on.work.data.q, B)
                got, tk = timed(lambda: on.solve_many(inst, branching="device"), a.repeats)
                sb = list(on.work.trees_sb)
                assert not any(t.overflow for t in on.work.trees_info)
                plain, tb = timed(lambda: off.solve_many(inst), a.repeats)
                row("instances", si, rule, B, tk, sb, got, tb, plain)
            on.work.solver.close()
            off.work.solver.close()
        for si in shapes:
            for B in batches:
                on = [build(problems, bnb, SHAPES[si], k, rule) for k in range(B)]
                off = [build(problems, bnb, SHAPES[si], k, 0) for k in range(B)]
                info = {}
                got, tk = timed(lambda: miosqp_amd.solve_models(on, info=info, large="device", branching="device"), a.repeats)
                assert not info["own"], info["own"]
                redone = len(info["overflow"])
                plain, tb = timed(lambda: miosqp_amd.solve_models(off, large="device"), a.repeats)
                row("models", si, rule, B, tk, [info["sb"][k] for k in sorted(info["sb"])], got, tb, plain)
                if redone:
                    out("#   (%d of these trees overflowed their leaf list and were redone by their own model: inside the keyword's time)" % redone)
                for m in on + off:
                    m.work.solver.close()
    if f:
        f.close()


if __name__ == "__main__":
    main()
