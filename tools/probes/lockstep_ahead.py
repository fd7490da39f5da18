"""solve_many beyond the one-launch trees: the lock-step trees whose spare columns solve open leaves early
(lockstep="ahead", ahead = 2, 4, 8) against the wave driver in the library (lockstep="device") and the sequential path
(lockstep=False).

Two workloads: config 2 (n 500, m 1000, p 250; random_miqp seed 0), the workload of tools/probes/lockstep_device.py, and
the 100 / 200 / 50 shape of the GPU tests; rho 0.1 and rho "auto"; instances drawn the way bench.py draws its MIQP stream;
max_batch = min(max(B, 64), 256).  All in one session, one engine per row:
  * first the results are compared: every dict of "ahead" equal to "device" (status, nodes, iterations, upper_glob and x bit
    for bit) for every `ahead`, and status, nodes, iterations equal to lockstep=False on the first --seq instances;
  * ahead: trees/s, waves, ahead columns sent, hits, discarded, called off, and the wasted iterations (those of the
    discarded and called-off columns; the hits' iterations are the trees' own);
  * device and sequential of THIS tree: trees/s and waves;
  * with --parent DIR (a built tree of the parent commit): its lockstep="device" and lockstep=False, timed in a child
    process that starts after this process's runs of the row are done -- the yardstick of the row.

    python tools/probes/lockstep_ahead.py [--out profiles/lockstep_ahead.txt] [--shapes cfg2,small] [--batches 1,8,32,64,256]
                                          [--aheads 2,4,8] [--seq 16] [--parent DIR]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SMALL = dict(n=100, m=200, p=50)


def shape(problems, name):
    return dict(problems.CONFIGS["cfg2"]) if name == "cfg2" else dict(SMALL)


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


def bits(res):
    return [(r["status"], r["nodes"], r["osqp_iter"], float(r["upper_glob"]).hex(), np.asarray(r["x"]).tobytes()) for r in res]


def timed(m, inst, **kw):
    t0 = time.time()
    res = m.solve_many(inst, **kw)
    return res, time.time() - t0


def child(a):
    """the parent commit's lockstep="device" on B instances and lockstep=False on the first --seq: one JSON line"""
    sys.path.insert(0, a.parent)
    from miosqp_amd import bnb, problems
    assert os.path.abspath(bnb.__file__).startswith(os.path.abspath(a.parent))
    cfg = shape(problems, a.shapes)
    pr = problems.random_miqp(**cfg, seed=a.seed)
    rho = "auto" if a.rho == "auto" else float(a.rho)
    B = int(a.batches)
    inst = draw(cfg, a.seed, max(B, a.seq))
    m = model(problems, bnb, pr, rho, min(max(B, 64), a.width))
    m.solve_many(inst[:B], lockstep="device")
    res, dt = timed(m, inst[:B], lockstep="device")
    m.solve_many(inst[:1], lockstep=False)
    _, ds = timed(m, inst[:a.seq], lockstep=False)
    print(json.dumps(dict(device=B / dt, sequential=a.seq / ds, key=key(res),
                          upper=[float(r["upper_glob"]).hex() for r in res])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="cfg2,small")
    ap.add_argument("--batches", default="1,8,32,64,256")
    ap.add_argument("--aheads", default="2,4,8")
    ap.add_argument("--width", type=int, default=256, help="largest max_batch")
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
    f = open(a.out, "a") if a.out else None

    def out(s=""):
        print(s, flush=True)
        if f:
            f.write(s + "\n")
            f.flush()

    batches = [int(b) for b in a.batches.split(",")]
    aheads = [int(k) for k in a.aheads.split(",")]
    for name in a.shapes.split(","):
        cfg = shape(problems, name)
        pr = problems.random_miqp(**cfg, seed=a.seed)
        inst = draw(cfg, a.seed, max(batches + [a.seq]))
        out("# solve_many at n %d, m %d, p %d (seed %d), one MI355X, max_batch = min(max(B, 64), %d): spare columns solving open "
            "leaves early (ahead) against the wave driver in the library (device) and the sequential path"
            % (cfg["n"], cfg["m"], cfg["p"], a.seed, a.width))
        out("# rho     B ahead | ahead: trees/s  waves    nodes     sent     hits  discarded  called off  wasted iters (of the trees')"
            " | device: trees/s  waves | sequential (first %d): trees/s | ahead / device  ahead / sequential |"
            " parent commit: device  sequential | ahead / parent's device  ahead / parent's sequential" % a.seq)
        for rho_s in a.rhos.split(","):
            rho = "auto" if rho_s == "auto" else float(rho_s)
            for B in batches:
                m = model(problems, bnb, pr, rho, min(max(B, 64), a.width))
                eng = m.work.solver
                ns = min(B, a.seq)
                # (first use of each path: allocations, graphs) -- and the comparison of the results
                dev0 = m.solve_many(inst[:B], lockstep="device")
                seq0 = m.solve_many(inst[:ns], lockstep=False)
                assert key(dev0[:ns]) == key(seq0), "device and sequential trees differ (rho %s, B %d)" % (rho_s, B)
                m.solve_many(inst[:B], lockstep="ahead", ahead=aheads[-1])
                rows = []
                for k in aheads:
                    res, dt = timed(m, inst[:B], lockstep="ahead", ahead=k)
                    rec = dict(m.work.lockstep)
                    assert rec["driver"] == "ahead" and bits(res) == bits(dev0), "ahead %d and device differ (rho %s, B %d)" % (k, rho_s, B)
                    rows.append((k, dt, rec))
                dev, dt_dev = timed(m, inst[:B], lockstep="device")
                drec = dict(m.work.lockstep)
                _, dt_seq = timed(m, inst[:ns], lockstep=False)
                eng.close()
                pj = None
                par = "-"
                if a.parent:
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--parent", a.parent, "--rho", rho_s,
                                        "--batches", str(B), "--seq", str(ns), "--seed", str(a.seed), "--width", str(a.width),
                                        "--shapes", name], capture_output=True, text=True, timeout=900)
                    if r.returncode != 0:
                        par = "failed: %s" % r.stderr.strip().splitlines()[-1:]
                    else:
                        pj = json.loads(r.stdout.strip().splitlines()[-1])
                        assert [tuple(t) for t in pj["key"]] == key(dev0), "the parent commit's trees differ"
                        assert pj["upper"] == [float(g["upper_glob"]).hex() for g in dev0], "the parent commit's bits differ"
                        par = "%21.2f %11.2f" % (pj["device"], pj["sequential"])
                for k, dt, rec in rows:
                    ah = rec["ahead"]
                    wasted = ah["discarded_iters"] + ah["called_off_iters"]
                    ratio = "-" if pj is None else "%22.2f %27.2f" % ((B / dt) / pj["device"], (B / dt) / pj["sequential"])
                    out("%-5s %5d %5d | %14.2f %6d %8d %8d %8d %10d %11d %13d (%4.1f%%) | %15.2f %6d | %29.2f | %14.2f %18.2f | %s | %s"
                        % (rho_s, B, k, B / dt, rec["waves"], rec["nodes"], ah["sent"], ah["hits"], ah["discarded"],
                           ah["called_off"], wasted, 100.0 * wasted / max(rec["iters_all"], 1), B / dt_dev, drec["waves"],
                           ns / dt_seq, dt_dev / dt, (B / dt) / (ns / dt_seq), par, ratio))
    if f:
        f.close()


if __name__ == "__main__":
    main()
