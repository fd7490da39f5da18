"""Strong and reliability branching inside the lock-step trees (solve_many(lockstep="device") with branching_rule 1 and
2): what the batched form costs and whether it pays.

Workload: config 2 (n 500, m 1000, p 250) and the shape n 100, m 200, p 50 ("s100"), random_miqp seed 0, instances drawn
the way bench.py draws its MIQP stream, max_batch = min(max(B, 64), 1024), B in {8, 64, 256} (prefixes of one list), rho
0.1 and "auto", rules 1 and 2, sb_candidates 8, sb_max_iter 50 (and, with --sweep, 100 and 250 at the largest B).  Per
row, in one session on one engine:
  new  lockstep="device" with the rule: trees/s, nodes per tree, strong-branching batches, their mean width in columns
       and the share of the call's device time spent in the branching step (its two downloads included);
  (b)  the same engine's lockstep="device" with branching_rule 0: trees/s, nodes per tree;
  seq  this library's sequential path (lockstep=False) with the rule on the first --seq instances: the yardstick every
       run of `new` is asserted equal to (status, nodes, node iterations) before any time is reported;
  (a)  with --parent DIR (a built tree of the parent commit): that library's sequential path with the same rule on the
       same instances, in a child process; its trees are asserted equal too.
Every path is run once on 16 instances first (allocations, graphs).  (a) and seq do not depend on B: they are run once
per (shape, rho, rule, sb_max_iter).

    python tools/probes/lockstep_sb.py [--out profiles/lockstep_sb.txt] [--configs cfg2,s100] [--batches 8,64,256]
                                       [--rules 1,2] [--rhos 0.1,auto] [--seq 16] [--sweep 100,250] [--parent DIR] [--append]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = {"s100": dict(n=100, m=200, p=50)}


def shape(problems, name):
    return SHAPES[name] if name in SHAPES else problems.CONFIGS[name]


def draw(cfg, seed, count):
    rng = np.random.RandomState(seed + 12345)
    return [dict(q=rng.randn(cfg["n"]), l=-2 + rng.rand(cfg["m"]), u=2 + rng.rand(cfg["m"])) for _ in range(count)]


def model(problems, bnb, pr, rho, width, rule, cap):
    st = dict(problems.BNB_SETTINGS, device_tree=False, branching_rule=rule, sb_candidates=8, sb_max_iter=cap)
    m = bnb.MIOSQP()
    m.setup(pr["P"], pr["q"], pr["A"], np.copy(pr["l"]), np.copy(pr["u"]), pr["i_idx"], pr["i_l"], pr["i_u"], st,
            dict(problems.QP_SETTINGS, rho=rho, max_batch=width))
    return m


def key(res):
    return [(r["status"], r["nodes"], r["osqp_iter"]) for r in res]


def timed(m, inst, **kw):
    t0 = time.time()
    res = m.solve_many(inst, **kw)
    return time.time() - t0, res


def child(a):
    """the parent commit's sequential path with the rule: one JSON line"""
    sys.path.insert(0, a.parent)
    from miosqp_amd import bnb, problems
    assert os.path.abspath(bnb.__file__).startswith(os.path.abspath(a.parent))
    cfg = shape(problems, a.configs)
    pr = problems.random_miqp(**cfg, seed=a.seed)
    rho = "auto" if a.rho == "auto" else float(a.rho)
    inst = draw(cfg, a.seed, a.seq)
    m = model(problems, bnb, pr, rho, 64, int(a.rules), a.cap)
    m.solve_many(inst[:1], lockstep=False)
    dt, res = timed(m, inst, lockstep=False)
    print(json.dumps(dict(dt=dt, key=key(res))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--configs", default="cfg2,s100")
    ap.add_argument("--batches", default="8,64,256")
    ap.add_argument("--rules", default="1,2")
    ap.add_argument("--rhos", default="0.1,auto")
    ap.add_argument("--seq", type=int, default=16, help="instances of the sequential comparison runs")
    ap.add_argument("--sweep", default="", help="further sb_max_iter values, run at the largest B only")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--parent", default=None, help="a built tree of the parent commit: its sequential path is timed too")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--rho", default="0.1")
    ap.add_argument("--cap", type=int, default=50)
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    sys.path.insert(0, ROOT)
    from miosqp_amd import bnb, problems
    f = open(a.out, "a" if a.append else "w") if a.out else None

    def out(s=""):
        print(s, flush=True)
        if f:
            f.write(s + "\n")
            f.flush()

    batches = [int(b) for b in a.batches.split(",")]
    caps = [50] + [int(c) for c in a.sweep.split(",") if c]
    if not a.append:
        out("# solve_many(lockstep=\"device\") with branching_rule 1 / 2 inside the trees, one MI355X, sb_candidates 8; seq and (a): "
            "lockstep=False with the rule on the first %d instances (this library / the parent commit's in a child process)" % a.seq)
        out("# shape rho   rule sb_max_iter     B | new: trees/s  nodes/tree  batches  columns/batch  branching % of device time |"
            " (b) rule 0 on \"device\": trees/s  nodes/tree | seq: trees/s  nodes/tree | (a) parent, sequential: trees/s |"
            " new/(a)  new/seq  new/(b)")
    for cname in a.configs.split(","):
        cfg = shape(problems, cname)
        pr = problems.random_miqp(**cfg, seed=a.seed)
        inst = draw(cfg, a.seed, max(batches + [a.seq, 16]))
        for rho_s in a.rhos.split(","):
            rho = "auto" if rho_s == "auto" else float(rho_s)
            for rule in [int(r) for r in a.rules.split(",")]:
                for cap in caps:
                    seq = par = None
                    for B in (batches if cap == 50 else batches[-1:]):
                        m = model(problems, bnb, pr, rho, min(max(B, 64), 1024), rule, cap)
                        work, st = m.work, m.work.settings
                        ns = min(B, a.seq)
                        m.solve_many(inst[:16], lockstep="device")  # first use of the path
                        if seq is None:
                            m.solve_many(inst[:1], lockstep=False)
                            ds, res_s = timed(m, inst[:a.seq], lockstep=False)
                            seq = (a.seq / ds, sum(x["nodes"] for x in res_s) / a.seq, key(res_s))
                            if a.parent:
                                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--parent", a.parent,
                                                    "--rho", rho_s, "--configs", cname, "--rules", str(rule), "--cap", str(cap),
                                                    "--seq", str(a.seq), "--seed", str(a.seed)], capture_output=True, text=True,
                                                   timeout=900)
                                assert r.returncode == 0, r.stderr[-2000:]
                                pj = json.loads(r.stdout.strip().splitlines()[-1])
                                assert [tuple(k) for k in pj["key"]] == seq[2], "the parent commit's trees differ"
                                par = a.seq / pj["dt"]
                        dt, res = timed(m, inst[:B], lockstep="device")
                        assert key(res[:ns]) == seq[2][:ns], "device and sequential trees differ (%s, rho %s, rule %d, B %d)" % (
                            cname, rho_s, rule, B)
                        rec = dict(work.lockstep)
                        sb = rec["sb"]
                        # (b): branching_rule 0 on the same engine
                        keep_rule, keep_sb = st["branching_rule"], work.sb
                        st["branching_rule"], work.sb = 0, dict(keep_sb, rule=0)
                        try:
                            m.solve_many(inst[:16], lockstep="device")
                            d0, res0 = timed(m, inst[:B], lockstep="device")
                        finally:
                            st["branching_rule"], work.sb = keep_rule, keep_sb
                        work.solver.close()
                        new_rate, b_rate = B / dt, B / d0
                        out("%-6s %-5s %4d %11d %5d | %12.2f %11.1f %8d %14.1f %28.1f | %32.2f %11.1f | %12.2f %11.1f | %32s |"
                            " %7s %8.2f %8.2f"
                            % (cname, rho_s, rule, cap, B, new_rate, sum(x["nodes"] for x in res) / B, sb["batches"],
                               sb["columns"] / max(sb["batches"], 1), 100.0 * sb["device_time"] / rec["device_time"], b_rate,
                               sum(x["nodes"] for x in res0) / B, seq[0], seq[1], "%.2f" % par if par else "-",
                               "%.2f" % (new_rate / par) if par else "-", new_rate / seq[0], new_rate / b_rate))
    if f:
        f.close()


if __name__ == "__main__":
    main()
