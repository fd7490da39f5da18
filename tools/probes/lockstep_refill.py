"""solve_many beyond the one-launch trees: the trees on columns refilled between chunks (lockstep="refill") against the
wave driver in the library (lockstep="device") and the sequential path (lockstep=False).

The workload of tools/probes/lockstep_device.py: config 2 (n 500, m 1000, p 250; random_miqp seed 0) at rho 0.1 and rho
"auto", instances drawn the way bench.py draws its MIQP stream.  For B = 8, 64, 256 instances max_batch = max(B, 64); the
last row has more trees than columns (512 under max_batch 256: the wave driver cuts its waves in two slices there).  All
in one session, one engine per row:
  * first the trees are compared: status, nodes and ADMM iterations of refill and device equal for all B, and equal to
    lockstep=False on the first --seq instances; upper_glob and x of refill and device equal bit for bit;
  * refill: trees/s, nodes, chunks, columns, occupancy (busy column-chunks / all column-chunks), the boundary's cost
    per chunk (the call's device time minus the time inside the chunks, / chunks, in microseconds: harvest, epilogue,
    scatter, download, the host's tree logic and upload, refill) and the host's share per node (the tree logic in C++
    plus everything of solve_many outside the call, / nodes, in microseconds);
  * device and sequential of THIS tree: trees/s (device also: the chunks its waves took, iters_slowest / check_termination);
  * with --parent DIR (a built tree of the parent commit): its lockstep="device" and lockstep=False, timed in a child
    process that starts after this process's runs of the row are done -- the yardstick of the row.

    python tools/probes/lockstep_refill.py [--out profiles/lockstep_refill.txt] [--batches 8,64,256,512] [--seq 16] [--parent DIR]
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


def timed(m, inst, **kw):
    t0 = time.time()
    res = m.solve_many(inst, **kw)
    return res, time.time() - t0


def child(a):
    """the parent commit's lockstep="device" on B instances and lockstep=False on the first --seq: one JSON line"""
    sys.path.insert(0, a.parent)
    from miosqp_amd import bnb, problems
    assert os.path.abspath(bnb.__file__).startswith(os.path.abspath(a.parent))
    cfg = problems.CONFIGS["cfg2"]
    pr = problems.random_miqp(**cfg, seed=a.seed)
    rho = "auto" if a.rho == "auto" else float(a.rho)
    B = int(a.batches)
    inst = draw(cfg, a.seed, max(B, a.seq))
    m = model(problems, bnb, pr, rho, min(max(B, 64), a.width))
    m.solve_many(inst[:B], lockstep="device")
    res, dt = timed(m, inst[:B], lockstep="device")
    m.solve_many(inst[:1], lockstep=False)
    _, ds = timed(m, inst[:a.seq], lockstep=False)
    print(json.dumps(dict(device=B / dt, sequential=a.seq / ds, key=key(res))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="8,64,256,512")
    ap.add_argument("--width", type=int, default=256, help="largest max_batch (a row with more instances has more trees than columns)")
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
    out("# solve_many at config 2 (n %d, m %d, p %d, seed %d), one MI355X, max_batch = min(max(B, 64), %d): the trees on columns "
        "refilled between chunks (refill) against the wave driver in the library (device) and the sequential path"
        % (cfg["n"], cfg["m"], cfg["p"], a.seed, a.width))
    out("# rho     B | refill: trees/s    nodes  chunks  columns  occupancy  boundary us/chunk  host us/node  store grew |"
        " device: trees/s  chunks | sequential (first %d): trees/s | refill / device  refill / sequential |"
        " parent commit: device  sequential | refill / parent's device" % a.seq)
    for rho_s in a.rhos.split(","):
        rho = "auto" if rho_s == "auto" else float(rho_s)
        for B in batches:
            m = model(problems, bnb, pr, rho, min(max(B, 64), a.width))
            eng = m.work.solver
            ct = int(eng.settings.check_termination)
            # (first use of each path: allocations, graphs) -- and the comparison of the trees
            ref0 = m.solve_many(inst[:B], lockstep="refill")
            dev0 = m.solve_many(inst[:B], lockstep="device")
            ns = min(B, a.seq)
            seq0 = m.solve_many(inst[:ns], lockstep=False)
            assert key(ref0) == key(dev0), "refill and device trees differ (rho %s, B %d)" % (rho_s, B)
            assert key(ref0[:ns]) == key(seq0), "refill and sequential trees differ (rho %s, B %d)" % (rho_s, B)
            for g, w in zip(ref0, dev0):
                assert g["upper_glob"] == w["upper_glob"] and np.array_equal(g["x"], w["x"]), "refill and device bits differ"
            # ---- refill ----
            ref, dt_ref = timed(m, inst[:B], lockstep="refill")
            rec = dict(m.work.lockstep)
            assert rec["driver"] == "refill" and key(ref) == key(ref0)
            # ---- device ----
            dev, dt_dev = timed(m, inst[:B], lockstep="device")
            drec = dict(m.work.lockstep)
            # ---- sequential ----
            _, dt_seq = timed(m, inst[:ns], lockstep=False)
            eng.close()
            par, ratio = "-", "-"
            if a.parent:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--parent", a.parent, "--rho", rho_s,
                                    "--batches", str(B), "--seq", str(ns), "--seed", str(a.seed), "--width", str(a.width)],
                                   capture_output=True, text=True, timeout=900)
                if r.returncode != 0:
                    par = "failed: %s" % r.stderr.strip().splitlines()[-1:]
                else:
                    pj = json.loads(r.stdout.strip().splitlines()[-1])
                    assert [tuple(k) for k in pj["key"]] == key(ref), "the parent commit's trees differ"
                    par = "%21.2f %11.2f" % (pj["device"], pj["sequential"])
                    ratio = "%.2f" % ((B / dt_ref) / pj["device"])
            out("%-5s %5d | %15.2f %8d %7d %8d %10.3f %18.1f %13.1f %11d | %15.2f %7d | %29.2f | %15.2f %19.2f | %s | %s"
                % (rho_s, B, B / dt_ref, rec["nodes"], rec["chunks"], rec["columns"], rec["occupancy"],
                   1e6 * (rec["device_time"] - rec["chunk_time"]) / max(rec["chunks"], 1),
                   1e6 * (dt_ref - rec["run_time"] + rec["host_time"]) / rec["nodes"], rec["grown"], B / dt_dev,
                   drec["iters_slowest"] // ct, ns / dt_seq, dt_dev / dt_ref, (B / dt_ref) / (ns / dt_seq), par, ratio))
    if f:
        f.close()


if __name__ == "__main__":
    main()
