"""solve_many beyond the one-launch trees: B trees in lock step (one solve_batch_q per wave) against the sequential path.

Config 2 (n 500, m 1000, p 250; random_miqp seed 0) at rho 0.1 and rho "auto".  The instances are drawn the way bench.py
draws its MIQP stream: RandomState(seed + 12345), q = randn(n), l = -2 + rand(m), u = 2 + rand(m) per instance.  For
B = 1, 8, 64, 256 instances (prefixes of one list):
  * lock-step: trees/s, total nodes, waves, ADMM iterations per wave -- the mean over the waves of the columns' mean, the
    mean over the waves of the slowest column (what a wave waits for) and the largest of all --, the node-iterations/s
    that were useful (sum of the columns' own counts / wall) and the share of the wall time spent outside the engine's
    call (Python: choosing leaves, stacking the wave, bound_and_branch);
  * sequential: the first min(B, --seq) of the same instances through solve_many(lockstep=False) (hosted search, one tree
    after the other; its rate does not depend on B), and, with --parent DIR, through solve_many of the parent commit's tree
    in DIR (a child process of this one; it starts after this process's own runs of the row are done);
  * whether lock-step and sequential agree on status / nodes / ADMM iterations for those instances.

    python tools/probes/lockstep_many.py [--out profiles/lockstep_many.txt] [--batches 1,8,64,256] [--seq 16] [--parent DIR]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def draw(cfg, seed, count):
    rng = np.random.RandomState(seed + 12345)
    return [dict(q=rng.randn(cfg["n"]), l=-2 + rng.rand(cfg["m"]), u=2 + rng.rand(cfg["m"])) for _ in range(count)]


def model(problems, bnb, pr, rho, width):
    m = bnb.MIOSQP()
    m.setup(pr["P"], pr["q"], pr["A"], np.copy(pr["l"]), np.copy(pr["u"]), pr["i_idx"], pr["i_l"], pr["i_u"],
            dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS, rho=rho, max_batch=width))
    return m


def child(a):
    """the parent commit's solve_many on the first --seq instances: one JSON line"""
    sys.path.insert(0, a.parent)
    from miosqp_amd import bnb, problems
    assert os.path.abspath(bnb.__file__).startswith(os.path.abspath(a.parent))
    cfg = problems.CONFIGS["cfg2"]
    pr = problems.random_miqp(**cfg, seed=a.seed)
    rho = "auto" if a.rho == "auto" else float(a.rho)
    inst = draw(cfg, a.seed, a.seq)
    m = model(problems, bnb, pr, rho, 64)
    m.solve_many(inst[:1])  # (first use: allocations, graphs)
    t0 = time.time()
    res = m.solve_many(inst)
    dt = time.time() - t0
    print(json.dumps(dict(trees_per_s=len(inst) / dt, nodes=sum(r["nodes"] for r in res))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="1,8,64,256")
    ap.add_argument("--seq", type=int, default=16, help="instances of the sequential comparison runs")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rhos", default="0.1,auto")
    ap.add_argument("--parent", default=None, help="a built tree of the parent commit: its solve_many is timed too")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--rho", default="0.1")
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    sys.path.insert(0, ROOT)
    from miosqp_amd import bnb, problems
    f = open(a.out, "w") if a.out else None

    def out(s=""):
        print(s, flush=True)
        if f:
            f.write(s + "\n")
            f.flush()

    cfg = problems.CONFIGS["cfg2"]
    pr = problems.random_miqp(**cfg, seed=a.seed)
    batches = [int(b) for b in a.batches.split(",")]
    inst = draw(cfg, a.seed, max(batches + [a.seq]))
    out("# solve_many at config 2 (n %d, m %d, p %d, seed %d), one MI355X: lock-step trees against the sequential path"
        % (cfg["n"], cfg["m"], cfg["p"], a.seed))
    out("# rho     B | lock-step: trees/s    nodes  waves  it/wave mean  slowest mean  slowest max  useful Mit/s  Python %% |"
        " sequential (first %d): trees/s   parent commit: trees/s | same trees" % a.seq)
    for rho_s in a.rhos.split(","):
        rho = "auto" if rho_s == "auto" else float(rho_s)
        seq_m = model(problems, bnb, pr, rho, 64)
        seq_m.solve_many(inst[:1], lockstep=False)
        t0 = time.time()
        seq = seq_m.solve_many(inst[:a.seq], lockstep=False)
        seq_rate = a.seq / (time.time() - t0)
        seq_m.work.solver.close()
        par_rate = None
        if a.parent:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--parent", a.parent, "--rho", rho_s,
                                "--seq", str(a.seq), "--seed", str(a.seed)], capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                out("#   parent commit's run failed: %s" % r.stderr.strip().splitlines()[-1:])
            else:
                par_rate = json.loads(r.stdout.strip().splitlines()[-1])["trees_per_s"]
        for B in batches:
            m = model(problems, bnb, pr, rho, min(max(B, 64), 1024))
            m.solve_many(inst[:min(B, 2)], lockstep=True)  # (first use: allocations, graphs)
            eng = m.work.solver
            spent = [0.0]
            inner = eng.solve_batch_q

            def timed(*args, _inner=inner, _spent=spent):
                r = _inner(*args)
                _spent[0] += float(np.sum(r.run_time))  # the engine's own wall time of the call (shared by its columns)
                return r

            eng.solve_batch_q = timed
            t0 = time.time()
            res = m.solve_many(inst[:B])
            dt = time.time() - t0
            del eng.solve_batch_q
            rec = m.work.lockstep
            same = all((g["status"], g["nodes"], g["osqp_iter"]) == (w["status"], w["nodes"], w["osqp_iter"])
                       for g, w in zip(res, seq))
            out("%-5s %5d | %19.2f %8d %6d %13.1f %13.1f %12d %13.3f %9.1f | %30.2f %24s | %s"
                % (rho_s, B, B / dt, rec["nodes"], rec["waves"], np.mean(rec["iters_mean"]), np.mean(rec["iters_max"]),
                   max(rec["iters_max"]), 1e-6 * sum(g["osqp_iter"] for g in res) / dt, 100.0 * (1.0 - spent[0] / dt),
                   seq_rate, "-" if par_rate is None else "%.2f" % par_rate,
                   "yes (%d compared)" % min(B, a.seq) if same else "NO"))
            eng.close()
    if f:
        f.close()


if __name__ == "__main__":
    main()
