"""setup_models(rho_auto="device"): rho="auto" models set up in ONE launch (miosqp_qp_setup_models_auto), the workgroup that
builds a model choosing its rho, against the yardstick: the PARENT commit running the same list, where every rho="auto"
model goes through MIOSQP.setup (two complete per-model set-ups and fifty iterations on a throw-away engine).

Workload: that of tools/probes/setup_models.py (model k: shape k mod 5, random_miqp seed k), every model at rho="auto",
B = 1, 8, 64, 256.  Per row, three repeats each (median, fastest and slowest):
  (a) set-up ms per model of `miosqp_amd.setup_models(..., rho_auto="device")`, the device time of its launch, and
      end-to-end MIQPs/s of that call + solve_models;
  (b) the library of --parent DIR (a built tree of the parent commit) in a child process: the loop over MIOSQP.setup on
      the same problems at rho="auto", then solve_models;
  (c) this library on that same loop (the keyword is opt-in: the default path must not have moved).
Before anything is timed the chosen rho of every model and status, nodes and iterations of every tree of (a) are asserted
equal to (b)'s.  Then the device time of one call per shape at B = 1 and 64, k_setup_models_auto beside k_setup_models
(rho 0.1) on the same problems.

    python tools/probes/setup_models_rho_auto.py [--out FILE] [--batches 1,8,64,256] [--repeats 3] [--parent DIR]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import setup_models as base  # noqa: E402  (the fixed-rho probe: its workload and its loop)


def draw_auto(problems, B):
    return [(pr, st, dict(qs, rho="auto"), inst) for pr, st, qs, inst in base.draw(problems, B)]


def loop_rows(pkg, bnb, drawn, repeats):
    models, _ = base.loop_setup(bnb, drawn)  # warm-up: caches, kernels
    res = pkg.solve_models(models, [d[3] for d in drawn])
    rho = [float(m.work.solver.rho()) for m in models]
    base.close(models)
    ts, te = [], []
    for _ in range(repeats):
        t0 = time.time()
        models, t = base.loop_setup(bnb, drawn)
        pkg.solve_models(models, [d[3] for d in drawn])
        te.append(time.time() - t0)
        ts.append(t)
        base.close(models)
    return ts, te, base.key(res), rho


def child(a):
    sys.path.insert(0, a.parent)
    import miosqp_amd as pkg
    from miosqp_amd import bnb, problems
    assert os.path.abspath(bnb.__file__).startswith(os.path.abspath(a.parent))
    import inspect
    assert "rho_auto" not in inspect.signature(pkg.setup_models).parameters  # the parent commit
    ts, te, k, rho = loop_rows(pkg, bnb, draw_auto(problems, int(a.batches)), a.repeats)
    print(json.dumps(dict(setup=ts, total=te, key=k, rho=rho)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="1,8,64,256")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built tree of the parent commit: the yardstick (b)")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    sys.path.insert(0, ROOT)
    import miosqp_amd as pkg
    from miosqp_amd import bnb, problems, qp
    f = open(a.out, "a") if a.out else None

    def out(s=""):
        print(s, flush=True)
        if f:
            f.write(s + "\n")
            f.flush()

    med = statistics.median
    out("# setup_models(rho_auto=\"device\") against the parent commit's loop MIOSQP().setup(..., rho=\"auto\"), one MI355X; "
        "model k: shape k mod %d of %s, seed k" % (len(base.SHAPES), " ".join(str(s).replace(" ", "") for s in base.SHAPES)))
    out("#     B | (a) rho_auto=\"device\": ms per model [fastest .. slowest of %d]  device ms of the call  end-to-end MIQPs/s | "
        "(b) parent's loop: ms per model [fastest .. slowest]  end-to-end MIQPs/s [min .. max] | (c) this library's loop: "
        "ms per model  end-to-end MIQPs/s | (b)/(a) set-up  end-to-end (a)/(b)" % a.repeats)
    for B in [int(b) for b in a.batches.split(",")]:
        drawn = draw_auto(problems, B)
        args = ([d[0] for d in drawn], [d[1] for d in drawn], [d[2] for d in drawn])
        insts = [d[3] for d in drawn]
        info = {}
        models = pkg.setup_models(*args, info=info, rho_auto="device")  # warm-up
        assert not info["own"] and info["launches"] == 1, info
        got, rho = base.key(pkg.solve_models(models, insts)), list(info["rho"])
        base.close(models)
        pj = None
        if a.parent:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--parent", a.parent, "--batches", str(B),
                                "--repeats", str(a.repeats)], capture_output=True, text=True, timeout=900)
            if r.returncode != 0:  # (nothing more is started on the device after a child that ended badly)
                out("# the parent's child process ended with %d: %s" % (r.returncode, r.stderr.strip().splitlines()[-3:]))
                sys.exit(1)
            pj = json.loads(r.stdout.strip().splitlines()[-1])
            assert pj["rho"] == rho, "the chosen rho differs from the parent commit's"
            assert [tuple(t) for t in pj["key"]] == got, "the trees differ from the parent commit's"
        ts, te, dev = [], [], []
        for _ in range(a.repeats):
            info = {}
            t0 = time.time()
            models = pkg.setup_models(*args, info=info, rho_auto="device")
            ts.append(time.time() - t0)
            pkg.solve_models(models, insts)
            te.append(time.time() - t0)
            dev.append(info["device_time"])
            base.close(models)
        cs, ce, ck, crho = loop_rows(pkg, bnb, drawn, a.repeats)
        assert ck == got and crho == rho
        sa, ea = med(ts), med(te)
        if pj:
            sb, eb = med(pj["setup"]), med(pj["total"])
            btxt = "%9.3f [%9.3f .. %9.3f] %10.1f [%8.1f .. %8.1f]" % (1e3 * sb / B, 1e3 * min(pj["setup"]) / B, 1e3 * max(pj["setup"]) / B,
                                                                   B / eb, B / max(pj["total"]), B / min(pj["total"]))
            rtxt = "%7.2f %7.2f" % (sb / sa, eb / ea)
        else:
            btxt, rtxt = "-", "-"
        out("%7d | %9.3f [%9.3f .. %9.3f] %10.3f %10.1f | %s | %9.3f %10.1f | %s"
            % (B, 1e3 * sa / B, 1e3 * min(ts) / B, 1e3 * max(ts) / B, 1e3 * med(dev), B / ea, btxt, 1e3 * med(cs) / B, B / med(ce), rtxt))
    out("")
    out("# device time of one call (upload, launch, records back) per shape, ms, median of %d [fastest .. slowest]: "
        "k_setup_models_auto (rho=\"auto\") beside k_setup_models (rho 0.1), B = 1 and B = 64" % a.repeats)
    for s in base.SHAPES:
        row = []
        for B in (1, 64):
            for auto in (True, False):
                desc = []
                for k in range(B):
                    pr, st, qs, _ = base.problem(problems, s, k)
                    d = bnb.Data(pr["P"], pr["q"], pr["A"], pr["l"], pr["u"], pr["i_idx"], pr["i_l"], pr["i_u"])
                    desc.append(dict(P=d.P, q=d.q, A=d.A, l=d.l, u=d.u, settings=dict(qs, rho="auto") if auto else qs, i_idx=d.i_idx,
                                     m_orig=d.m))
                dev = []
                for _ in range(a.repeats + 1):
                    solvers, stats = qp.setup_models(desc, rho_auto_in_launch=auto)
                    dev.append(stats.device_time)
                    lds = stats.lds_bytes
                    for g in solvers:
                        g.close()
                dev = dev[1:]
                row.append("%s %7.3f [%7.3f .. %7.3f] LDS %6d" % ("auto" if auto else "fixed", 1e3 * med(dev), 1e3 * min(dev), 1e3 * max(dev), lds))
        out("#   %-12s n + M = %3d | B = 1: %s | B = 64: %s" % (str(s).replace(" ", ""), d.n + d.A.shape[0], "  ".join(row[:2]), "  ".join(row[2:])))
    if f:
        f.close()


if __name__ == "__main__":
    main()
