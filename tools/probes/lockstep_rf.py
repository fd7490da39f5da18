"""Round and fix inside the lock-step trees (solve_many(lockstep="device") with primal_heuristic = 1): what it costs and
what it buys.

Workload: config 2 (n 500, m 1000, p 250) and config 1 (n 50, m 100, p 10; device_tree off, so that the lock-step
driver and not the one-launch trees takes it), random_miqp seed 0, instances drawn the way bench.py draws its MIQP
stream, max_batch = B, for B = 256 and 64 instances (prefixes of one list), rho 0.1 and "auto", rf_candidates 7,
rf_max_iter 250.  Per row, in one session on one engine:
  (a) lockstep="device" with the heuristic off -- and, with --parent DIR (a built tree of the parent commit), the same call
      on the parent's library in a child process that stays alive, the two alternating run by run; both best times are
      reported: (a) is what must not get slower;
  (b) the same with the heuristic on, rf_every 10 (the default) and root-only (rf_every above max_iter_bb): trees/s, nodes
      per tree, heuristic batches, their mean width in columns and their share of the call's device time;
  (c) the sequential path (lockstep=False) with the heuristic on, on the first --seq instances.
Status, nodes and node iterations of (b) and (c) are asserted equal on those instances, and the parent library's trees
equal to this one's, before any time is reported.  Every path is run once on 16 instances first (allocations, graphs).

    python tools/probes/lockstep_rf.py [--out profiles/lockstep_rf.txt] [--configs cfg2,cfg1] [--batches 256,64] [--seq 8] [--parent DIR]
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


def model(problems, bnb, pr, rho, width, heuristic):
    st = dict(problems.BNB_SETTINGS, device_tree=False)
    if heuristic:
        st.update(primal_heuristic=1, rf_candidates=7, rf_max_iter=250, rf_every=10)
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
    """the parent commit's lockstep="device" (no heuristic there): one timed run per line read, one JSON line each"""
    sys.path.insert(0, a.parent)
    from miosqp_amd import bnb, problems
    assert os.path.abspath(bnb.__file__).startswith(os.path.abspath(a.parent))
    cfg = problems.CONFIGS[a.configs]
    pr = problems.random_miqp(**cfg, seed=a.seed)
    rho = "auto" if a.rho == "auto" else float(a.rho)
    B = int(a.batches)
    inst = draw(cfg, a.seed, B)
    m = model(problems, bnb, pr, rho, min(max(B, 64), 1024), False)
    m.solve_many(inst[:16], lockstep="device")
    print(json.dumps(dict(ready=1)), flush=True)
    for line in sys.stdin:
        if line.strip() != "go":
            break
        dt, res = timed(m, inst, lockstep="device")
        print(json.dumps(dict(dt=dt, key=key(res))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--configs", default="cfg2,cfg1")
    ap.add_argument("--batches", default="256,64")
    ap.add_argument("--seq", type=int, default=8, help="instances of the sequential comparison runs")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rhos", default="0.1,auto")
    ap.add_argument("--reps", type=int, default=2, help="alternating runs of (a) per library")
    ap.add_argument("--parent", default=None, help="a built tree of the parent commit: its (a) is timed too")
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

    batches = [int(b) for b in a.batches.split(",")]
    out("# solve_many(lockstep=\"device\") with round and fix inside the trees, one MI355X, max_batch = B, rf_candidates 7, rf_max_iter 250;"
        " sequential: lockstep=False on the first %d instances; best of %d alternating runs for (a)" % (a.seq, a.reps))
    out("# config rho     B | (a) heuristic off: trees/s  nodes/tree | parent commit (a): trees/s | (b) rf_every 10: trees/s  nodes/tree"
        "  batches  columns/batch  device %  improved | (b) root only: trees/s  nodes/tree  batches  columns/batch  device %  improved |"
        " (c) sequential, rf_every 10: trees/s  root only: trees/s | (b)/(a)  (b)/(c) at rf_every 10")
    for cname in a.configs.split(","):
        cfg = problems.CONFIGS[cname]
        pr = problems.random_miqp(**cfg, seed=a.seed)
        inst = draw(cfg, a.seed, max(batches + [a.seq]))
        for rho_s in a.rhos.split(","):
            rho = "auto" if rho_s == "auto" else float(rho_s)
            for B in batches:
                m = model(problems, bnb, pr, rho, min(max(B, 64), 1024), True)
                work = m.work
                rf_on = dict(work.rf)
                root_only = dict(rf_on, every=work.settings["max_iter_bb"] + 1)
                off = dict(rf_on, on=0)
                ns = min(B, a.seq)
                for rf in (off, rf_on):  # first use of each path
                    work.rf = rf
                    m.solve_many(inst[:16], lockstep="device")
                m.solve_many(inst[:1], lockstep=False)
                # ---- (a), alternating with the parent commit's library ----
                proc = None
                if a.parent:
                    proc = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", "--parent", a.parent, "--rho", rho_s,
                                             "--configs", cname, "--batches", str(B), "--seed", str(a.seed)], stdin=subprocess.PIPE,
                                            stdout=subprocess.PIPE, text=True)
                    assert json.loads(proc.stdout.readline())["ready"] == 1
                work.rf = off
                t_a, t_par, res_a = [], [], None
                for _ in range(a.reps):
                    dt, res_a = timed(m, inst[:B], lockstep="device")
                    t_a.append(dt)
                    if proc:
                        proc.stdin.write("go\n")
                        proc.stdin.flush()
                        pj = json.loads(proc.stdout.readline())
                        assert [tuple(k) for k in pj["key"]] == key(res_a), "the parent commit's trees differ"
                        t_par.append(pj["dt"])
                if proc:
                    proc.stdin.write("end\n")
                    proc.stdin.flush()
                    proc.wait(timeout=60)
                # ---- (b) and (c) ----
                cols = []
                seq_rate = []
                for rf in (rf_on, root_only):
                    work.rf = rf
                    dt, res = timed(m, inst[:B], lockstep="device")
                    rec = dict(work.lockstep)
                    r = rec["rf"]
                    ds, seq = timed(m, inst[:ns], lockstep=False)
                    assert key(res[:ns]) == key(seq), "device and sequential trees differ (%s, rho %s, B %d)" % (cname, rho_s, B)
                    cols.append((B / dt, sum(x["nodes"] for x in res) / B, r["batches"], r["columns"] / max(r["batches"], 1),
                                 100.0 * r["device_time"] / rec["device_time"], r["improved"]))
                    seq_rate.append(ns / ds)
                work.solver.close()
                a_rate = B / min(t_a)
                par = "%25.2f" % (B / min(t_par)) if t_par else "%25s" % "-"
                out("%-6s %-5s %5d | %26.2f %11.1f | %s | %24.2f %11.1f %8d %14.1f %9.1f %9d | %22.2f %11.1f %8d %14.1f %9.1f %9d |"
                    " %37.2f %20.2f | %7.2f %8.2f"
                    % ((cname, rho_s, B, a_rate, sum(x["nodes"] for x in res_a) / B, par) + cols[0] + cols[1] +
                       (seq_rate[0], seq_rate[1], cols[0][0] / a_rate, cols[0][0] / seq_rate[0])))
    if f:
        f.close()


if __name__ == "__main__":
    main()
