"""setup_models(..., prepare="device"): equilibration and packed rows by a launch of the call (k_prepare_models,
miosqp_qp_setup_models_prepared) against the same call without the keyword, here and on the parent commit.

1. The stage table of the parent commit's call (MIOSQP_SETUP_TIMING=1, in a child process with the library of --parent DIR):
   the four large shapes of the reference's benchmark grid, every model at rho="auto", B = 1, 8, 64, 256 -- "host:
   equilibration + packed rows" against the rest.  Then this library's table with the keyword on the same lists.
2. Per list -- LARGE (model k: large shape k mod 4, seed k, rho="auto", large="device", large_rho_auto="device"), SMALL
   (the list of profiles/setup_models.txt at rho 0.1) and SMALL AUTO (the same at rho="auto", rho_auto="device") -- and per
   B: set-up ms per model and end-to-end MIQPs/s (set-up + solve_models) with the keyword, without it, and of the parent
   commit in a child process; --repeats calls each, median [min .. max]; the device time of the call with and without.
3. Per large shape, one model alone and 64 copies of the shape: the device time of the call with and without the keyword.

    python tools/probes/setup_models_prepare.py --parent DIR [--out profiles/setup_models_prepare.txt] [--batches 1,8,64,256]
                                                [--repeats 3] [--parts 1,2,3]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import setup_models as small_probe  # noqa: E402  (the list of profiles/setup_models.txt)

LARGE_SHAPES = [(50, 200, 10), (100, 200, 15), (150, 100, 5), (150, 300, 20)]
LISTS = {
    "large": dict(keys=dict(large="device", large_rho_auto="device"), solve=dict(large="device")),
    "small": dict(keys=dict(), solve=dict()),
    "small auto": dict(keys=dict(rho_auto="device"), solve=dict()),
}


def draw(problems, which, B, shapes=None):
    """(problems, B&B settings, QP settings, instances) of a list"""
    if which == "large":
        shapes = shapes or LARGE_SHAPES
        prs = [problems.random_miqp(*shapes[k % len(shapes)], seed=k) for k in range(B)]
        return prs, [dict(problems.BNB_SETTINGS) for _ in prs], [dict(problems.QP_SETTINGS, rho="auto") for _ in prs], None
    d = small_probe.draw(problems, B)
    qss = [dict(x[2], rho="auto") if which == "small auto" else x[2] for x in d]
    return [x[0] for x in d], [x[1] for x in d], qss, [x[3] for x in d]


def close(models):
    for m in models:
        m.work.solver.close()


def run(miosqp_amd, problems, which, B, repeats, prepare, solve=True, shapes=None):
    prs, sts, qss, inst = draw(problems, which, B, shapes)
    kw = dict(LISTS[which]["keys"])
    if prepare:
        kw["prepare"] = "device"
    close(miosqp_amd.setup_models(prs, sts, qss, **kw))  # warm-up
    ts, te, dev, keys, info = [], [], [], None, {}
    for _ in range(repeats):
        info = {}
        t0 = time.time()
        models = miosqp_amd.setup_models(prs, sts, qss, info=info, **kw)
        ts.append(time.time() - t0)
        if solve:
            res = miosqp_amd.solve_models(models, instances=inst, **LISTS[which]["solve"])
            te.append(time.time() - t0)
            keys = [(r["status"], r["nodes"], r["osqp_iter"]) for r in res]
        dev.append(info["device_time"])
        close(models)
    if prepare:
        assert info["prepare"] == info["batched"], info
    return dict(setup=ts, end=te, dev=dev, key=keys, rho=info["rho"], launches=info["launches"], batched=len(info["batched"]))


def child(a):
    """the library of --parent (or this one with --prepare) in a process of its own: one JSON line; with --ticks one call
    under MIOSQP_SETUP_TIMING, whose table goes to stderr"""
    root = a.parent if a.parent else ROOT
    sys.path.insert(0, root)
    import miosqp_amd
    from miosqp_amd import problems
    assert os.path.abspath(miosqp_amd.__file__).startswith(os.path.abspath(root))
    B = int(a.batches)
    if a.ticks:
        prs, sts, qss, _ = draw(problems, a.list, B)
        kw = dict(LISTS[a.list]["keys"])
        if a.prepare:
            kw["prepare"] = "device"
        close(miosqp_amd.setup_models(prs, sts, qss, **kw))
        sys.stderr.write("[ticks begin]\n")
        sys.stderr.flush()
        close(miosqp_amd.setup_models(prs, sts, qss, **kw))
        return
    print(json.dumps(run(miosqp_amd, problems, a.list, B, a.repeats, a.prepare)))


def spawn(a, B, which, parent, prepare=False, ticks=False):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--batches", str(B), "--repeats", str(a.repeats), "--list", which]
    if parent:
        cmd += ["--parent", parent]
    if prepare:
        cmd += ["--prepare"]
    env = dict(os.environ)
    if ticks:
        cmd += ["--ticks"]
        env["MIOSQP_SETUP_TIMING"] = "1"
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    if r.returncode != 0:  # (nothing more is started on the device after a child that ended badly)
        print("# a child process ended with %d: %s" % (r.returncode, r.stderr.strip().splitlines()[-3:]), flush=True)
        sys.exit(1)
    return r


def med(v, B, scale=1e3):
    return "%7.3f [%7.3f .. %7.3f]" % (scale * statistics.median(v) / B, scale * min(v) / B, scale * max(v) / B)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="1,8,64,256")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built tree of the parent commit")
    ap.add_argument("--parts", default="1,2,3")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--ticks", action="store_true")
    ap.add_argument("--prepare", action="store_true")
    ap.add_argument("--list", default="large")
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

    batches = [int(b) for b in a.batches.split(",") if b]
    parts = a.parts.split(",")
    if "1" in parts:
        out("# 1. stage tables (MIOSQP_SETUP_TIMING=1, ms per CALL, the second call of a process), large list, every model at rho=\"auto\"")
        for who, parent, prepare in (("parent commit", a.parent, False), ("this commit, prepare=\"device\"", None, True)):
            if who == "parent commit" and not a.parent:
                continue
            for B in batches:
                r = spawn(a, B, "large", parent, prepare=prepare, ticks=True)
                lines = r.stderr.split("[ticks begin]")[-1].splitlines()
                out("# %s, B = %d" % (who, B))
                for ln in lines:
                    m = re.match(r"\[miosqp setup_models\] (.*?)\s+([0-9.]+) ms", ln)
                    if m:
                        out("    %-64s %10.3f ms  %8.3f ms/model" % (m.group(1), float(m.group(2)), float(m.group(2)) / B))
    if "2" in parts:
        out("# 2. set-up ms per model and end-to-end MIQPs/s (set-up + solve_models), median [min .. max] of %d calls" % a.repeats)
        out("# list        B | set-up ms/model: keyword                 without                    parent commit              | device ms of "
            "the call: keyword  without | end to end MIQPs/s: keyword  without  parent")
        for which in ("large", "small", "small auto"):
            for B in batches:
                k = run(miosqp_amd, problems, which, B, a.repeats, True)
                w = run(miosqp_amd, problems, which, B, a.repeats, False)
                assert k["key"] == w["key"] and k["rho"] == w["rho"], (which, B)
                ptxt, pe = "%27s" % "-", "-"
                if a.parent:
                    pj = json.loads(spawn(a, B, which, a.parent).stdout.strip().splitlines()[-1])
                    assert [tuple(x) for x in pj["key"]] == k["key"] and pj["rho"] == k["rho"], (which, B)
                    ptxt, pe = med(pj["setup"], B), "%7.1f" % (B / statistics.median(pj["end"]))
                out("%-10s %4d | %s  %s  %s | %17.3f %8.3f | %27.1f %8.1f %7s" % (
                    which, B, med(k["setup"], B), med(w["setup"], B), ptxt, 1e3 * statistics.median(k["dev"]),
                    1e3 * statistics.median(w["dev"]), B / statistics.median(k["end"]), B / statistics.median(w["end"]), pe))
    if "3" in parts:
        out("# 3. per large shape: device ms of the call (upload, launches, download) with the keyword and without, rho=\"auto\"")
        out("# shape            B | keyword   without | difference per model")
        for s in LARGE_SHAPES:
            for B in (1, 64):
                k = run(miosqp_amd, problems, "large", B, a.repeats, True, solve=False, shapes=[s])
                w = run(miosqp_amd, problems, "large", B, a.repeats, False, solve=False, shapes=[s])
                dk, dw = 1e3 * statistics.median(k["dev"]), 1e3 * statistics.median(w["dev"])
                out("%-14s %4d | %8.3f %8.3f | %8.3f" % (str(s).replace(" ", ""), B, dk, dw, (dk - dw) / B))
    if f:
        f.close()


if __name__ == "__main__":
    main()
