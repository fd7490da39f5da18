"""setup_models: the set-up of B DIFFERENT models with one launch (miosqp_qp_setup_models) against the loop it replaces,
`MIOSQP().setup(...)` model by model.

Workload: the shapes of profiles/solve_models.txt (those of the reference's benchmark grid that the one-launch trees take,
plus the power-converter model); model k has shape k mod 5 and random_miqp seed k -- its own P and A --, rho 0.1,
B = 1, 8, 64, 256.  Per row, three repeats each (median, and the spread of the yardstick):
  (a) set-up ms per model of `miosqp_amd.setup_models` (the device time of its launch beside it) and end-to-end MIQPs/s of
      setup_models + solve_models;
  (b) the yardstick: the library of --parent DIR (a built tree of the parent commit) in a child process, looping
      MIOSQP.setup over the same problems, then solve_models: set-up ms per model [fastest .. slowest], end-to-end MIQPs/s;
  (c) this library running that same loop (the per-model set-up did not move if (c) lies within the spread of (b)).
Before anything is timed, status, nodes and iterations of the trees of (a) are asserted equal to (b)'s.
Then: the stage table of a per-model set-up and of the one-launch call (MIOSQP_SETUP_TIMING=1, eight models, in a child
process), and the device time of the launch per shape at B = 1 and B = 64.

    python tools/probes/setup_models.py [--out profiles/setup_models.txt] [--batches 1,8,64,256] [--repeats 3] [--parent DIR]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = [(10, 5, 2), (10, 100, 2), (50, 25, 5), (100, 50, 2), "pc"]


def problem(problems, shape, seed):
    """(problem dict, B&B settings, QP settings, instance)"""
    if shape == "pc":
        pc = problems.load_power_converter()
        k = seed % len(pc["q"])
        pr = dict(P=pc["P"], q=pc["q"][k].copy(), A=pc["A"], l=pc["l"].copy(), u=pc["u"][k].copy(), i_idx=pc["i_idx"],
                  i_l=pc["i_l"], i_u=pc["i_u"])
        return pr, dict(pc["settings"]), dict(pc["qp_settings"], rho=0.1), dict(x0=pc["x0"][k].copy())
    return problems.random_miqp(*shape, seed=seed), dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS, rho=0.1), {}


def draw(problems, B, shapes=SHAPES):
    return [problem(problems, shapes[k % len(shapes)], k) for k in range(B)]


def loop_setup(bnb, drawn):
    t0 = time.time()
    models = []
    for pr, st, qs, _ in drawn:
        m = bnb.MIOSQP()
        m.setup(pr["P"], pr["q"], pr["A"], np.copy(pr["l"]), np.copy(pr["u"]), pr["i_idx"], pr["i_l"], pr["i_u"], dict(st), dict(qs))
        models.append(m)
    return models, time.time() - t0


def close(models):
    for m in models:
        m.work.solver.close()


def key(res):
    return [(r["status"], r["nodes"], r["osqp_iter"]) for r in res]


def loop_rows(pkg, bnb, problems, B, repeats):
    """the loop over MIOSQP.setup, then solve_models: (set-up seconds per repeat, end-to-end seconds per repeat, tree keys)"""
    drawn = draw(problems, B)
    models, _ = loop_setup(bnb, drawn)  # warm-up: caches, kernels
    res = pkg.solve_models(models, [d[3] for d in drawn])
    close(models)
    ts, te = [], []
    for _ in range(repeats):
        t0 = time.time()
        models, t = loop_setup(bnb, drawn)
        pkg.solve_models(models, [d[3] for d in drawn])
        te.append(time.time() - t0)
        ts.append(t)
        close(models)
    return ts, te, key(res)


def child(a):
    sys.path.insert(0, a.parent)
    import miosqp_amd as pkg
    from miosqp_amd import bnb, problems
    assert os.path.abspath(bnb.__file__).startswith(os.path.abspath(a.parent))
    assert not hasattr(bnb, "setup_models")
    ts, te, k = loop_rows(pkg, bnb, problems, int(a.batches), a.repeats)
    print(json.dumps(dict(setup=ts, total=te, key=k)))


def stages(a):
    """MIOSQP_SETUP_TIMING=1 is set by the caller: eight models by the loop, eight by the one-launch call; wall times on stdout"""
    sys.path.insert(0, ROOT)
    import miosqp_amd as pkg
    from miosqp_amd import bnb, problems
    drawn = draw(problems, 8)
    close(loop_setup(bnb, drawn)[0])
    close(pkg.setup_models([d[0] for d in drawn], [d[1] for d in drawn], [d[2] for d in drawn]))
    sys.stderr.write("@@ loop\n")
    sys.stderr.flush()
    models, t_loop = loop_setup(bnb, drawn)
    close(models)
    sys.stderr.write("@@ call\n")
    sys.stderr.flush()
    t0 = time.time()
    models = pkg.setup_models([d[0] for d in drawn], [d[1] for d in drawn], [d[2] for d in drawn])
    t_call = time.time() - t0
    close(models)
    print(json.dumps(dict(loop=t_loop, call=t_call)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="1,8,64,256")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built tree of the parent commit: the yardstick (b)")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--stages", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.stages:
        return stages(a)
    sys.path.insert(0, ROOT)
    import miosqp_amd as pkg
    from miosqp_amd import bnb, problems, qp
    f = open(a.out, "a") if a.out else None

    def out(s=""):
        print(s, flush=True)
        if f:
            f.write(s + "\n")
            f.flush()

    out("# setup_models against the loop MIOSQP().setup(...), one MI355X; model k: shape k mod %d of %s, seed k, rho 0.1"
        % (len(SHAPES), " ".join(str(s).replace(" ", "") for s in SHAPES)))
    out("#     B | (a) setup_models: ms per model  device ms of the call  end-to-end MIQPs/s | (b) parent's loop: ms per model "
        "[fastest .. slowest of %d]  end-to-end MIQPs/s [min .. max] | (c) this library's loop: ms per model  end-to-end MIQPs/s | "
        "(b)/(a) set-up  end-to-end (a)/(b)" % a.repeats)
    for B in [int(b) for b in a.batches.split(",")]:
        drawn = draw(problems, B)
        args = ([d[0] for d in drawn], [d[1] for d in drawn], [d[2] for d in drawn])
        insts = [d[3] for d in drawn]
        info = {}
        models = pkg.setup_models(*args, info=info)  # warm-up
        assert not info["own"], info
        got = key(pkg.solve_models(models, insts))
        close(models)
        pj = None
        if a.parent:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--parent", a.parent, "--batches", str(B),
                                "--repeats", str(a.repeats)], capture_output=True, text=True, timeout=900)
            if r.returncode != 0:  # (nothing more is started on the device after a child that ended badly)
                out("# the parent's child process ended with %d: %s" % (r.returncode, r.stderr.strip().splitlines()[-3:]))
                sys.exit(1)
            pj = json.loads(r.stdout.strip().splitlines()[-1])
            assert [tuple(t) for t in pj["key"]] == got, "the trees differ from the parent commit's"
        ts, te, dev = [], [], []
        for _ in range(a.repeats):
            info = {}
            t0 = time.time()
            models = pkg.setup_models(*args, info=info)
            ts.append(time.time() - t0)
            pkg.solve_models(models, insts)
            te.append(time.time() - t0)
            dev.append(info["device_time"])
            close(models)
        cs, ce, ck = loop_rows(pkg, bnb, problems, B, a.repeats)
        assert ck == got
        sa, ea = statistics.median(ts), statistics.median(te)
        sc_, ec = statistics.median(cs), statistics.median(ce)
        if pj:
            sb, eb = statistics.median(pj["setup"]), statistics.median(pj["total"])
            btxt = "%9.3f [%9.3f .. %9.3f] %10.1f [%8.1f .. %8.1f]" % (1e3 * sb / B, 1e3 * min(pj["setup"]) / B, 1e3 * max(pj["setup"]) / B,
                                                                   B / eb, B / max(pj["total"]), B / min(pj["total"]))
            rtxt = "%7.2f %7.2f" % (sb / sa, eb / ea)
        else:
            btxt, rtxt = "-", "-"
        out("%7d | %9.3f [%9.3f .. %9.3f] %10.3f %10.1f | %s | %9.3f %10.1f | %s"
            % (B, 1e3 * sa / B, 1e3 * min(ts) / B, 1e3 * max(ts) / B, 1e3 * statistics.median(dev), B / ea, btxt, 1e3 * sc_ / B, B / ec, rtxt))
    # ---- the stages of a set-up, eight models ----
    env = dict(os.environ, MIOSQP_SETUP_TIMING="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--stages"], capture_output=True, text=True, timeout=600, env=env)
    if r.returncode != 0:
        out("# the stage run ended with %d: %s" % (r.returncode, r.stderr.strip().splitlines()[-3:]))
        sys.exit(1)
    walls = json.loads(r.stdout.strip().splitlines()[-1])
    part, acc = None, {"loop": {}, "call": {}}
    for line in r.stderr.splitlines():
        if line.startswith("@@ "):
            part = line[3:].strip()
            continue
        hit = re.match(r"\[miosqp setup(_models)?\]\s+(.*?)\s+([0-9.]+) ms", line)
        if hit and part:
            acc[part][hit.group(2)] = acc[part].get(hit.group(2), 0.0) + float(hit.group(3))
    out("")
    out("# stages, eight models (MIOSQP_SETUP_TIMING=1; sums over the eight set-ups, ms)")
    out("# the loop over MIOSQP.setup: wall %.3f ms, i.e. %.3f per model" % (1e3 * walls["loop"], 1e3 * walls["loop"] / 8))
    lib = acc["loop"].get("miosqp_qp_setup, all of it", 0.0)
    for k, v in acc["loop"].items():
        out("#   %-52s %9.3f" % (k, v))
    out("#   %-52s %9.3f" % ("Python, scipy, ctypes (wall - the library's calls)", 1e3 * walls["loop"] - lib))
    out("# one setup_models call: wall %.3f ms, i.e. %.3f per model" % (1e3 * walls["call"], 1e3 * walls["call"] / 8))
    lib = acc["call"].get("miosqp_qp_setup_models, all of it", 0.0)
    for k, v in acc["call"].items():
        out("#   %-52s %9.3f" % (k, v))
    out("#   %-52s %9.3f" % ("Python, scipy, ctypes (wall - the library's call)", 1e3 * walls["call"] - lib))
    # ---- device time of the launch per shape ----
    out("")
    out("# device time of one call (upload, k_setup_models, records back) per shape, ms: B = 1, B = 64 (median of %d)" % a.repeats)
    for s in SHAPES:
        row = []
        for B in (1, 64):
            desc = []
            for k in range(B):
                pr, st, qs, _ = problem(problems, s, k)
                d = bnb.Data(pr["P"], pr["q"], pr["A"], pr["l"], pr["u"], pr["i_idx"], pr["i_l"], pr["i_u"])
                desc.append(dict(P=d.P, q=d.q, A=d.A, l=d.l, u=d.u, settings=qs, i_idx=d.i_idx, m_orig=d.m))
            dev = []
            for _ in range(a.repeats + 1):
                solvers, stats = qp.setup_models(desc)
                dev.append(stats.device_time)
                lds = stats.lds_bytes
                for g in solvers:
                    g.close()
            row.append("%8.3f" % (1e3 * statistics.median(dev[1:])))
        out("#   %-12s n + M = %3d  LDS %6d B | %s" % (str(s).replace(" ", ""), d.n + d.A.shape[0], lds, "  ".join(row)))
    if f:
        f.close()


if __name__ == "__main__":
    main()
