"""setup_models(..., large="device"): the set-up of models BEYOND n + M = 192 in one call (miosqp_qp_setup_models_large,
k_setup_models_large: one workgroup per model, the packed triangle in LDS, Abar read from L2) against what setup_models
does with such models without the keyword -- the loop over MIOSQP.setup, which builds the cooperative grid's engine one
model at a time.

Workload: the four large shapes of the reference's benchmark grid; model k has shape k mod 4 and random_miqp seed k;
B = 1, 8, 64, 256 models; rho 0.1.  Per row:
  (a) set-up per model of setup_models(large="device") (median of --repeats calls; the models are closed between calls,
      so from the second call on the group's stream, arena and slab are the parked ones when they are below 32 MB), the
      device time of a call (upload, the launch, records back), its launches;
  (b) set-up per model of the yardstick: the library of --parent DIR (a built tree of the parent commit) in a child
      process, its setup_models over the same list (= the loop over MIOSQP.setup); median of --repeats, and their spread;
  (b)/(a);
  (c) end to end: MIQPs/s of setup_models(large="device") + solve_models(large="device") on the list, against the
      parent's setup_models + solve_models(large="device") in the child.
Then, per shape, one model alone: the device time of a B = 1 call (median of --repeats).

    python tools/probes/setup_models_large.py [--out profiles/setup_models_large.txt] [--batches 1,8,64,256]
                                              [--repeats 3] [--parent DIR]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = [(50, 200, 10), (100, 200, 15), (150, 100, 5), (150, 300, 20)]
RHO = 0.1


def problems_of(problems, shapes, B):
    return [problems.random_miqp(*shapes[k % len(shapes)], seed=k) for k in range(B)]


def close(models):
    for m in models:
        m.work.solver.close()


def run(miosqp_amd, problems, prs, repeats, **kw):
    """(set-up seconds per repeat, end-to-end seconds per repeat, device seconds per repeat, last info, keys)"""
    st, qs = dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS, rho=RHO)
    close(miosqp_amd.setup_models(prs, st, qs, **kw))  # warm-up
    ts, te, dev, info, keys = [], [], [], {}, None
    for _ in range(repeats):
        info = {}
        t0 = time.time()
        models = miosqp_amd.setup_models(prs, st, qs, info=info, **kw)
        ts.append(time.time() - t0)
        res = miosqp_amd.solve_models(models, large="device")
        te.append(time.time() - t0)
        dev.append(info["device_time"])
        keys = [(r["status"], r["nodes"], r["osqp_iter"]) for r in res]
        close(models)
    return ts, te, dev, info, keys


def child(a):
    """the parent commit's library: its setup_models over the same list, one JSON line"""
    sys.path.insert(0, a.parent)
    import miosqp_amd
    from miosqp_amd import problems
    assert os.path.abspath(miosqp_amd.__file__).startswith(os.path.abspath(a.parent))
    prs = problems_of(problems, SHAPES, int(a.batches))
    ts, te, _, info, keys = run(miosqp_amd, problems, prs, a.repeats)
    assert info["batched"] == [], info
    print(json.dumps(dict(setup=ts, end=te, key=keys)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="1,8,64,256")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built tree of the parent commit: the yardstick (b)")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    sys.path.insert(0, ROOT)
    import miosqp_amd
    from miosqp_amd import problems
    f = open(a.out, "a") if a.out else None

    def out(s=""):
        print(s, flush=True)
        if f:
            f.write(s + "\n")
            f.flush()

    out("# setup_models(large=\"device\") against the parent's setup_models (= the loop over MIOSQP.setup), one MI355X, rho %g; "
        "model k: shape k mod 4 of %s, seed k" % (RHO, str(SHAPES).replace(" ", "")))
    out("#     B | (a) large=\"device\" ms/model  device ms  launches | (b) parent ms/model  [min .. max of %d] | (b)/(a) | "
        "(c) end to end MIQPs/s: large  parent  ratio" % a.repeats)
    for B in [int(b) for b in a.batches.split(",") if b]:
        prs = problems_of(problems, SHAPES, B)
        ts, te, dev, info, keys = run(miosqp_amd, problems, prs, a.repeats, large="device")
        assert info["batched"] == list(range(B)) and info["forms"] == dict(small=0, large=B), info
        sa, ea = statistics.median(ts), statistics.median(te)
        btxt = "%19s  [%8s .. %8s] | %7s | %31.1f %7s %6s" % ("-", "-", "-", "-", B / ea, "-", "-")
        if a.parent:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--parent", a.parent, "--batches", str(B),
                                "--repeats", str(a.repeats)], capture_output=True, text=True, timeout=1100)
            if r.returncode != 0:  # (nothing more is started on the device after a child that ended badly)
                out("# the parent's child process ended with %d: %s" % (r.returncode, r.stderr.strip().splitlines()[-3:]))
                sys.exit(1)
            pj = json.loads(r.stdout.strip().splitlines()[-1])
            same = sum(tuple(x) == y for x, y in zip(pj["key"], keys))
            sb, eb = statistics.median(pj["setup"]), statistics.median(pj["end"])
            btxt = "%19.3f  [%8.3f .. %8.3f] | %7.2f | %31.1f %7.1f %6.2f" % (
                1e3 * sb / B, 1e3 * min(pj["setup"]) / B, 1e3 * max(pj["setup"]) / B, sb / sa, B / ea, B / eb, eb / ea)
            if same != B:
                out("# B = %d: %d of %d trees have the parent's status, nodes and iterations" % (B, same, B))
        out("%7d | %27.3f %10.3f %9d | %s" % (B, 1e3 * sa / B, 1e3 * statistics.median(dev), info["launches"], btxt))
    out("# one model alone (seed 0): device time of the call (upload, k_setup_models_large, records back)")
    out("# shape          n + M   LDS bytes | device ms")
    st, qs = dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS, rho=RHO)
    for s in SHAPES:
        pr = problems.random_miqp(*s, seed=0)
        dev = []
        for _ in range(a.repeats + 1):
            info = {}
            close(miosqp_amd.setup_models([pr], st, qs, info=info, large="device"))
            dev.append(info["device_time"])
        n = s[0]
        out("%-14s %6d %11d | %9.3f" % (str(s).replace(" ", ""), s[0] + s[1] + s[2], 8 * (n * (n + 1) // 2 + 3 * n + 8),
                                         1e3 * statistics.median(dev[1:])))
    if f:
        f.close()


if __name__ == "__main__":
    main()
