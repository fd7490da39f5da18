"""setup_models(..., large="device", large_rho_auto="device"): models BEYOND n + M = 192 with rho="auto" set up in one call
(miosqp_qp_setup_models_large_auto, k_setup_models_large_auto: the workgroup that builds a model chooses its rho) against
what setup_models does with such models without the keyword -- the loop over MIOSQP.setup, which for rho="auto" makes two
complete set-ups and fifty iterations on a throw-away engine per model.

Workload: the four large shapes of the reference's benchmark grid; model k has shape k mod 4 and random_miqp seed k;
B = 1, 8, 64, 256 models; every model at rho="auto".  Per row:
  (a) set-up per model of setup_models(large="device", large_rho_auto="device") (median of --repeats calls; the models are
      closed between calls), the device time of a call (upload, the launch, records back), and beside it the device time
      of the fixed-rho large launch on the same list (rho 0.1, large="device");
  (b) set-up per model of the yardstick: the library of --parent DIR (a built tree of the parent commit) in a child
      process, its setup_models(large="device") over the same list (= the loop over MIOSQP.setup); median of --repeats, and
      their spread;
  (b)/(a);
  (c) end to end: MIQPs/s of the set-up + solve_models(large="device") on the list, against the same two calls of the
      parent in the child.
Then, per shape, one model alone: the device time of a B = 1 call with the keyword and at a fixed rho (median of --repeats).

    python tools/probes/setup_models_large_rho_auto.py [--out profiles/setup_models_large_rho_auto.txt]
                                                       [--batches 1,8,64,256] [--repeats 3] [--parent DIR]
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
KEYS = dict(large="device", large_rho_auto="device")


def problems_of(problems, shapes, B):
    return [problems.random_miqp(*shapes[k % len(shapes)], seed=k) for k in range(B)]


def close(models):
    for m in models:
        m.work.solver.close()


def run(miosqp_amd, problems, prs, repeats, rho="auto", solve=True, **kw):
    """(set-up seconds per repeat, end-to-end seconds per repeat, device seconds per repeat, last info, keys)"""
    st, qs = dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS, rho=rho)
    close(miosqp_amd.setup_models(prs, st, qs, **kw))  # warm-up
    ts, te, dev, info, keys = [], [], [], {}, None
    for _ in range(repeats):
        info = {}
        t0 = time.time()
        models = miosqp_amd.setup_models(prs, st, qs, info=info, **kw)
        ts.append(time.time() - t0)
        if solve:
            res = miosqp_amd.solve_models(models, large="device")
            te.append(time.time() - t0)
            keys = [(r["status"], r["nodes"], r["osqp_iter"]) for r in res]
        dev.append(info["device_time"])
        close(models)
    return ts, te, dev, info, keys


def child(a):
    """the parent commit's library: its setup_models over the same list, one JSON line"""
    sys.path.insert(0, a.parent)
    import miosqp_amd
    from miosqp_amd import problems
    assert os.path.abspath(miosqp_amd.__file__).startswith(os.path.abspath(a.parent))
    prs = problems_of(problems, SHAPES, int(a.batches))
    ts, te, _, info, keys = run(miosqp_amd, problems, prs, a.repeats, large="device")
    assert info["batched"] == [], info
    print(json.dumps(dict(setup=ts, end=te, key=keys, rho=info["rho"])))


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

    out("# setup_models(large=\"device\", large_rho_auto=\"device\") against the parent's setup_models (= the loop over MIOSQP.setup), "
        "one MI355X, every model at rho=\"auto\"; model k: shape k mod 4 of %s, seed k" % str(SHAPES).replace(" ", ""))
    out("#     B | (a) keyword ms/model  device ms  (fixed-rho launch: device ms)  launches | (b) parent ms/model  [min .. max of %d] "
        "| (b)/(a) | (c) end to end MIQPs/s: keyword  parent  ratio" % a.repeats)
    for B in [int(b) for b in a.batches.split(",") if b]:
        prs = problems_of(problems, SHAPES, B)
        ts, te, dev, info, keys = run(miosqp_amd, problems, prs, a.repeats, **KEYS)
        assert info["batched"] == list(range(B)) and info["forms"] == dict(small=0, large=B), info
        assert info["rho_auto_large"] == list(range(B)), info
        _, _, dev_fixed, finfo, _ = run(miosqp_amd, problems, prs, a.repeats, rho=0.1, solve=False, large="device")
        assert finfo["batched"] == list(range(B)), finfo
        sa, ea = statistics.median(ts), statistics.median(te)
        btxt = "%19s  [%8s .. %8s] | %7s | %33.1f %7s %6s" % ("-", "-", "-", "-", B / ea, "-", "-")
        if a.parent:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--parent", a.parent, "--batches", str(B),
                                "--repeats", str(a.repeats)], capture_output=True, text=True, timeout=1100)
            if r.returncode != 0:  # (nothing more is started on the device after a child that ended badly)
                out("# the parent's child process ended with %d: %s" % (r.returncode, r.stderr.strip().splitlines()[-3:]))
                sys.exit(1)
            pj = json.loads(r.stdout.strip().splitlines()[-1])
            same = sum(tuple(x) == y for x, y in zip(pj["key"], keys))
            same_rho = sum(x == y for x, y in zip(pj["rho"], info["rho"]))
            sb, eb = statistics.median(pj["setup"]), statistics.median(pj["end"])
            btxt = "%19.3f  [%8.3f .. %8.3f] | %7.2f | %33.1f %7.1f %6.2f" % (
                1e3 * sb / B, 1e3 * min(pj["setup"]) / B, 1e3 * max(pj["setup"]) / B, sb / sa, B / ea, B / eb, eb / ea)
            if same != B or same_rho != B:
                out("# B = %d: %d of %d models have the parent's rho, %d of %d trees its status, nodes and iterations" % (B, same_rho, B, same, B))
        out("%7d | %20.3f %10.3f %31.3f %10d | %s" % (B, 1e3 * sa / B, 1e3 * statistics.median(dev), 1e3 * statistics.median(dev_fixed),
                                                      info["launches"], btxt))
    out("# one model alone (seed 0): device time of the call (upload, the launch, records back), with the keyword and at a fixed rho")
    out("# shape          n + M   LDS bytes   rho chosen | device ms: k_setup_models_large_auto   k_setup_models_large (rho 0.1)")
    st = dict(problems.BNB_SETTINGS)
    for s in SHAPES:
        pr = problems.random_miqp(*s, seed=0)
        dev, dev_fixed, info = [], [], {}
        for _ in range(a.repeats + 1):
            info, finfo = {}, {}
            close(miosqp_amd.setup_models([pr], st, dict(problems.QP_SETTINGS, rho="auto"), info=info, **KEYS))
            close(miosqp_amd.setup_models([pr], st, dict(problems.QP_SETTINGS, rho=0.1), info=finfo, large="device"))
            dev.append(info["device_time"])
            dev_fixed.append(finfo["device_time"])
        n, M = s[0], s[1] + s[2]
        out("%-14s %6d %11d %12g | %37.3f %22.3f" % (str(s).replace(" ", ""), n + M, 8 * (n * (n + 1) // 2 + 4 * n + 3 * M + 16),
                                                      info["rho"][0], 1e3 * statistics.median(dev[1:]), 1e3 * statistics.median(dev_fixed[1:])))
    if f:
        f.close()


if __name__ == "__main__":
    main()
