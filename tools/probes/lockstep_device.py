"""solve_many beyond the one-launch trees: the lock-step trees driven in the library (lockstep="device") against the
Python driver (lockstep=True) and the sequential path (lockstep=False).

The workload of tools/probes/lockstep_many.py: config 2 (n 500, m 1000, p 250; random_miqp seed 0) at rho 0.1 and rho
"auto", instances drawn the way bench.py draws its MIQP stream, max_batch = B.  For B = 8, 64, 256 instances (prefixes
of one list), all in one session and on one engine per B:
  * device: trees/s, nodes, waves, the engine's share of the wall time (the library call without its tree logic on the
    host: (run_time - host_time) / wall seconds of solve_many) and the host's share per node (the tree logic in C++ plus
    everything of solve_many outside the call, / nodes, in microseconds);
  * python: trees/s of lockstep=True and the share of its wall time outside the engine's calls;
  * sequential: trees/s of the first min(B, --seq) instances through lockstep=False (its rate does not depend on B);
  * with --parent DIR (a built tree of the parent commit): its lockstep=True and lockstep=False, timed in a child process
    that starts after this process's runs of the row are done.
Status, nodes and ADMM iterations of device, python and sequential are asserted equal before any time is reported.

    python tools/probes/lockstep_device.py [--out profiles/lockstep_device.txt] [--batches 8,64,256] [--seq 16] [--parent DIR]
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


def key(res):
    return [(r["status"], r["nodes"], r["osqp_iter"]) for r in res]


def child(a):
    """the parent commit's lockstep=True on B instances and lockstep=False on the first --seq: one JSON line"""
    sys.path.insert(0, a.parent)
    from miosqp_amd import bnb, problems
    assert os.path.abspath(bnb.__file__).startswith(os.path.abspath(a.parent))
    cfg = problems.CONFIGS["cfg2"]
    pr = problems.random_miqp(**cfg, seed=a.seed)
    rho = "auto" if a.rho == "auto" else float(a.rho)
    B = int(a.batches)
    inst = draw(cfg, a.seed, max(B, a.seq))
    m = model(problems, bnb, pr, rho, min(max(B, 64), 1024))
    m.solve_many(inst[:2], lockstep=True)
    t0 = time.time()
    res = m.solve_many(inst[:B], lockstep=True)
    dt = time.time() - t0
    m.solve_many(inst[:1], lockstep=False)
    t0 = time.time()
    m.solve_many(inst[:a.seq], lockstep=False)
    ds = time.time() - t0
    print(json.dumps(dict(python=B / dt, sequential=a.seq / ds, key=key(res))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="8,64,256")
    ap.add_argument("--seq", type=int, default=16, help="instances of the sequential comparison runs")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rhos", default="0.1,auto")
    ap.add_argument("--parent", default=None, help="a built tree of the parent commit: its drivers are timed too")
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
    out("# solve_many at config 2 (n %d, m %d, p %d, seed %d), one MI355X, max_batch = B: the lock-step trees driven in the"
        " library (device) against the Python driver and the sequential path" % (cfg["n"], cfg["m"], cfg["p"], a.seed))
    out("# rho     B | device: trees/s    nodes  waves  engine %%  host us/node  store grew | python: trees/s  outside engine %% |"
        " sequential (first %d): trees/s | device / python  device / sequential | parent commit: python  sequential" % a.seq)
    for rho_s in a.rhos.split(","):
        rho = "auto" if rho_s == "auto" else float(rho_s)
        for B in batches:
            m = model(problems, bnb, pr, rho, min(max(B, 64), 1024))
            eng = m.work.solver
            m.solve_many(inst[:2], lockstep=True)  # (first use of each path: allocations, graphs)
            m.solve_many(inst[:B], lockstep="device")
            m.solve_many(inst[:1], lockstep=False)
            # ---- device ----
            t0 = time.time()
            dev = m.solve_many(inst[:B], lockstep="device")
            dt_dev = time.time() - t0
            rec = dict(m.work.lockstep)
            # ---- python ----
            spent = [0.0]
            inner = eng.solve_batch_q

            def timed(*args, _inner=inner, _spent=spent):
                r = _inner(*args)
                _spent[0] += float(np.sum(r.run_time))  # the engine's own wall time of the call (shared by its columns)
                return r

            eng.solve_batch_q = timed
            t0 = time.time()
            py = m.solve_many(inst[:B], lockstep=True)
            dt_py = time.time() - t0
            del eng.solve_batch_q
            # ---- sequential ----
            ns = min(B, a.seq)
            t0 = time.time()
            seq = m.solve_many(inst[:ns], lockstep=False)
            dt_seq = time.time() - t0
            assert key(dev) == key(py), "device and python trees differ (rho %s, B %d)" % (rho_s, B)
            assert key(dev[:ns]) == key(seq), "device and sequential trees differ (rho %s, B %d)" % (rho_s, B)
            assert rec["driver"] == "device" and rec["waves"] == max(r["nodes"] for r in dev)
            eng.close()
            par = "-"
            if a.parent:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--parent", a.parent, "--rho", rho_s,
                                    "--batches", str(B), "--seq", str(ns), "--seed", str(a.seed)], capture_output=True,
                                   text=True, timeout=900)
                if r.returncode != 0:
                    par = "failed: %s" % r.stderr.strip().splitlines()[-1:]
                else:
                    pj = json.loads(r.stdout.strip().splitlines()[-1])
                    assert [tuple(k) for k in pj["key"]] == key(dev), "the parent commit's trees differ"
                    par = "%21.2f %11.2f" % (pj["python"], pj["sequential"])
            out("%-5s %5d | %16.2f %8d %6d %9.1f %13.1f %11d | %15.2f %17.1f | %29.2f | %15.2f %20.2f | %s"
                % (rho_s, B, B / dt_dev, rec["nodes"], rec["waves"], 100.0 * (rec["run_time"] - rec["host_time"]) / dt_dev,
                   1e6 * (dt_dev - rec["run_time"] + rec["host_time"]) / rec["nodes"], rec["grown"], B / dt_py,
                   100.0 * (1.0 - spent[0] / dt_py), ns / dt_seq, dt_py / dt_dev, (B / dt_dev) / (ns / dt_seq), par))
    if f:
        f.close()


if __name__ == "__main__":
    main()
