"""solve_models: one MIQP on each of B DIFFERENT models in one call (miosqp_qp_solve_trees_models) against the loop it
replaces, `models[k].solve_many([instance])` model by model.

Workload: the shapes of the reference's benchmark grid that the one-launch trees take (tree_form() != 0, asked of one
model per shape at the start and printed) plus the power-converter model; model k has shape k mod (number of shapes) and
random_miqp seed k -- its own P and A, as the reference's benchmark draws them; B = 1, 8, 64, 256 models; rho 0.1 and
"auto".  One session, every path once on 16 models first, one warm-up call per row.  Per row:
  (a) MIQPs/s of solve_models (median of --repeats calls), the device time of a call and its launches;
  (b) MIQPs/s of the yardstick: the library of --parent DIR (a built tree of the parent commit) in a child process,
      looping models[k].solve_many([inst]) over the same models; median of --repeats loops, and their spread;
  (c) this library running that same loop: the parent path did not move if (c) lies within the spread of (b);
  set-up per model (MIOSQP.setup wall time, mean and total), timed separately and not part of (a) .. (c); and the share
  of an end-to-end MIQP (set-up + solve) that is set-up, with the loop's solve time and with solve_models' solve time.
Before anything is timed, status, nodes and iterations of (a) are asserted equal to (b)'s on the first 16 models (and all
results of (a) bit for bit equal to (c)'s).

    python tools/probes/solve_models.py [--out profiles/solve_models.txt] [--batches 1,8,64,256] [--rhos 0.1,auto]
                                        [--repeats 3] [--parent DIR]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GRID = [(10, 5, 2), (10, 100, 2), (50, 25, 5), (50, 200, 10), (100, 50, 2), (100, 200, 15), (150, 100, 5), (150, 300, 20)]


def build(problems, bnb, shape, seed, rho):
    """(model, instance, set-up seconds)"""
    if shape == "pc":
        pc = problems.load_power_converter()
        k = seed % len(pc["q"])  # (one plant: the models differ in the MPC step they start from)
        pr = dict(P=pc["P"], q=pc["q"][k].copy(), A=pc["A"], l=pc["l"].copy(), u=pc["u"][k].copy(), i_idx=pc["i_idx"],
                  i_l=pc["i_l"], i_u=pc["i_u"])
        st, qs, inst = dict(pc["settings"]), dict(pc["qp_settings"]), dict(x0=pc["x0"][k].copy())
    else:
        pr = problems.random_miqp(*shape, seed=seed)
        st, qs, inst = dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS), {}
    m = bnb.MIOSQP()
    t0 = time.time()
    m.setup(pr["P"], pr["q"], pr["A"], np.copy(pr["l"]), np.copy(pr["u"]), pr["i_idx"], pr["i_l"], pr["i_u"], st, dict(qs, rho=rho))
    return m, inst, time.time() - t0


def build_many(problems, bnb, shapes, B, rho):
    built = [build(problems, bnb, shapes[k % len(shapes)], k, rho) for k in range(B)]
    return [b[0] for b in built], [b[1] for b in built], [b[2] for b in built]


def loop(models, insts):
    t0 = time.time()
    res = [m.solve_many([i])[0] for m, i in zip(models, insts)]
    return res, time.time() - t0


def key(res):
    return [(r["status"], r["nodes"], r["osqp_iter"]) for r in res]


def bits(res):
    return [(r["status"], r["nodes"], r["osqp_iter"], float(r["upper_glob"]).hex(),
             np.asarray(r["x"]).tobytes() if np.isfinite(r["upper_glob"]) else b"") for r in res]


def child(a):
    """the parent commit's library: the loop over the same models, one JSON line"""
    sys.path.insert(0, a.parent)
    from miosqp_amd import bnb, problems
    assert os.path.abspath(bnb.__file__).startswith(os.path.abspath(a.parent))
    assert not hasattr(bnb, "solve_models")
    shapes = [s if s == "pc" else tuple(s) for s in json.loads(a.shapes)]
    rho = "auto" if a.rho == "auto" else float(a.rho)
    models, insts, ts = build_many(problems, bnb, shapes, int(a.batches), rho)
    res, _ = loop(models, insts)  # warm-up
    times = [loop(models, insts)[1] for _ in range(a.repeats)]
    print(json.dumps(dict(times=times, key=key(res), setup=ts)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="1,8,64,256")
    ap.add_argument("--rhos", default="0.1,auto")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built tree of the parent commit: the yardstick (b)")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--rho", default="0.1")
    ap.add_argument("--shapes", default="[]")
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    sys.path.insert(0, ROOT)
    import miosqp_amd
    from miosqp_amd import bnb, problems
    f = open(a.out, "a") if a.out else None

    def out(s=""):
        print(s, flush=True)
        if f:
            f.write(s + "\n")
            f.flush()

    # which shapes of the grid do the one-launch trees take?
    shapes, forms = [], []
    for s in GRID + ["pc"]:
        m, _, _ = build(problems, bnb, s, 0, 0.1)
        form = m.work.solver.tree_form()
        m.work.solver.close()
        forms.append((s, form))
        if form:
            shapes.append(s)
    out("# solve_models against the loop models[k].solve_many([inst]), one MI355X; model k: shape k mod %d, seed k" % len(shapes))
    out("# tree_form per shape (0: beyond the one-launch trees, left out; 1 one wavefront; 2 one workgroup): "
        + "  ".join("%s:%d" % (str(s).replace(" ", ""), fo) for s, fo in forms))
    # every path once on 16 models
    models, insts, _ = build_many(problems, bnb, shapes, 16, 0.1)
    miosqp_amd.solve_models(models, insts)
    loop(models, insts)
    for m in models:
        m.work.solver.close()
    out("# rho      B | (a) solve_models MIQPs/s  device ms  launches  forms w/g | (b) parent's loop MIQPs/s  [min .. max of %d] | "
        "(c) this library's loop MIQPs/s  (c)/(b) | (a)/(b) | set-up per model ms (mean)  total s | "
        "set-up share of an end-to-end MIQP: with the loop  with solve_models" % a.repeats)
    for rho_s in a.rhos.split(","):
        rho = "auto" if rho_s == "auto" else float(rho_s)
        for B in [int(b) for b in a.batches.split(",")]:
            models, insts, ts = build_many(problems, bnb, shapes, B, rho)
            info = {}
            got = miosqp_amd.solve_models(models, insts, info=info)  # warm-up of (a)
            assert not info["own"] and not info["overflow"], info
            own, _ = loop(models, insts)  # warm-up of (c)
            assert bits(got) == bits(own), "solve_models and this library's loop differ (rho %s, B %d)" % (rho_s, B)
            pj = None
            if a.parent:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--parent", a.parent, "--rho", rho_s,
                                    "--batches", str(B), "--repeats", str(a.repeats), "--shapes", json.dumps(shapes)],
                                   capture_output=True, text=True, timeout=900)
                if r.returncode != 0:  # (nothing more is started on the device after a child that ended badly)
                    out("# the parent's child process ended with %d: %s" % (r.returncode, r.stderr.strip().splitlines()[-3:]))
                    sys.exit(1)
                pj = json.loads(r.stdout.strip().splitlines()[-1])
                ns = min(16, B)
                assert [tuple(t) for t in pj["key"]][:ns] == key(got)[:ns], "the parent commit's trees differ"
            ta, dev = [], []
            for _ in range(a.repeats):
                info = {}
                t0 = time.time()
                miosqp_amd.solve_models(models, insts, info=info)
                ta.append(time.time() - t0)
                dev.append(info["device_time"])
            tc = [loop(models, insts)[1] for _ in range(a.repeats)]
            for m in models:
                m.work.solver.close()
            sa, sc = statistics.median(ta), statistics.median(tc)
            setup = float(np.mean(ts))
            if pj:
                tb = pj["times"]
                sb = statistics.median(tb)
                btxt = "%25.1f  [%8.1f .. %8.1f]" % (B / sb, B / max(tb), B / min(tb))
                rtxt = "%7.2f | %7.2f" % (sb / sc, sb / sa)
                solve_loop = sb / B
            else:
                btxt, rtxt, solve_loop = "%25s  [%8s .. %8s]" % ("-", "-", "-"), "%7s | %7s" % ("-", "-"), sc / B
            out("%-5s %5d | %24.1f %10.3f %9d %6d/%-4d | %s | %31.1f  %s | %26.3f %8.3f | %50.1f%% %20.1f%%"
                % (rho_s, B, B / sa, 1e3 * statistics.median(dev), info["launches"], info["forms"]["wave"], info["forms"]["group"],
                   btxt, B / sc, rtxt, 1e3 * setup, float(np.sum(ts)),
                   100.0 * setup / (setup + solve_loop), 100.0 * setup / (setup + sa / B)))
    if f:
        f.close()


if __name__ == "__main__":
    main()
