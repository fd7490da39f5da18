"""solve_models(..., large="device"): the trees of models BEYOND one workgroup's product form in one call
(miosqp_qp_solve_trees_models_large, k_tree_r_m: the relaxation in reduced form) against what solve_models does with such
models without the keyword -- the loop `models[k].solve_many([instance])`, node by node on the cooperative grid.

Workload: the shapes of the reference's benchmark grid with tree_form() 0 and tree_form_large() 3 (asked of one model per
shape at the start and printed); model k has shape k mod (number of shapes) and random_miqp seed k; B = 1, 8, 64, 256
models; rho 0.1 and "auto".  Per row:
  (a) MIQPs/s of solve_models(large="device") (median of --repeats calls), the device time of a call, its launches;
  (b) MIQPs/s of the yardstick: the library of --parent DIR (a built tree of the parent commit) in a child process,
      looping models[k].solve_many([inst]) over the same models; median of --repeats loops, and their spread;
  (a)/(b).
Before anything is timed, status, nodes and iterations of (a) are asserted equal to (b)'s on the first 16 models.
Then, per shape, one model alone: microseconds per iteration of the reduced loop (device time of a B = 1 call over its
iterations, upload and tree logic included) with Abar read from the dense copies (f_Atd, f_Ad) and from the packed panels
(pv_At, pc_A) -- MIOSQP_TREE_R_DENSE=1 / 0 --, median of --repeats.

    python tools/probes/solve_models_large.py [--out profiles/solve_models_large.txt] [--batches 1,8,64,256]
                                              [--rhos 0.1,auto] [--repeats 3] [--parent DIR]
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
    pr = problems.random_miqp(*shape, seed=seed)
    m = bnb.MIOSQP()
    m.setup(pr["P"], pr["q"], pr["A"], np.copy(pr["l"]), np.copy(pr["u"]), pr["i_idx"], pr["i_l"], pr["i_u"],
            dict(problems.BNB_SETTINGS), dict(problems.QP_SETTINGS, rho=rho))
    return m


def build_many(problems, bnb, shapes, B, rho):
    return [build(problems, bnb, shapes[k % len(shapes)], k, rho) for k in range(B)]


def loop(models):
    t0 = time.time()
    res = [m.solve_many([{}])[0] for m in models]
    return res, time.time() - t0


def key(res):
    return [(r["status"], r["nodes"], r["osqp_iter"]) for r in res]


def child(a):
    """the parent commit's library: the loop over the same models, one JSON line"""
    sys.path.insert(0, a.parent)
    from miosqp_amd import bnb, problems
    assert os.path.abspath(bnb.__file__).startswith(os.path.abspath(a.parent))
    shapes = [tuple(s) for s in json.loads(a.shapes)]
    rho = "auto" if a.rho == "auto" else float(a.rho)
    models = build_many(problems, bnb, shapes, int(a.batches), rho)
    res, _ = loop(models)  # warm-up
    times = [loop(models)[1] for _ in range(a.repeats)]
    print(json.dumps(dict(times=times, key=key(res))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="1,8,64,256")
    ap.add_argument("--rhos", default="0.1,auto")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built tree of the parent commit: the yardstick (b)")
    ap.add_argument("--per-shape", type=int, default=1, help="0: leave the per-shape part out")
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

    shapes, forms = [], []
    for s in GRID:
        m = build(problems, bnb, s, 0, 0.1)
        fo = m.work.solver.tree_form() or m.work.solver.tree_form_large()
        m.work.solver.close()
        forms.append((s, fo))
        if fo == 3:
            shapes.append(s)
    out("# solve_models(large=\"device\") against the parent's solve_models (= the loop models[k].solve_many([inst])), one MI355X; "
        "model k: shape k mod %d, seed k" % len(shapes))
    out("# form per grid shape (1 one wavefront, 2 one workgroup, 3 reduced form -- the workload): "
        + "  ".join("%s:%d" % (str(s).replace(" ", ""), fo) for s, fo in forms))
    out("# rho      B | (a) large=\"device\" MIQPs/s  device ms  launches  reduced | (b) parent's loop MIQPs/s  [min .. max of %d] | (a)/(b)"
        % a.repeats)
    for rho_s in a.rhos.split(","):
        rho = "auto" if rho_s == "auto" else float(rho_s)
        for B in [int(b) for b in a.batches.split(",") if b]:
            models = build_many(problems, bnb, shapes, B, rho)
            info = {}
            got = miosqp_amd.solve_models(models, info=info, large="device")  # warm-up of (a)
            assert not info["own"] and not info["overflow"] and info["forms"]["reduced"] == B, info
            pj = None
            if a.parent:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--parent", a.parent, "--rho", rho_s,
                                    "--batches", str(B), "--repeats", str(a.repeats), "--shapes", json.dumps(shapes)],
                                   capture_output=True, text=True, timeout=1100)
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
                miosqp_amd.solve_models(models, info=info, large="device")
                ta.append(time.time() - t0)
                dev.append(info["device_time"])
            for m in models:
                m.work.solver.close()
            sa = statistics.median(ta)
            if pj:
                tb = pj["times"]
                sb = statistics.median(tb)
                btxt = "%25.1f  [%8.1f .. %8.1f] | %7.2f" % (B / sb, B / max(tb), B / min(tb), sb / sa)
            else:
                btxt = "%25s  [%8s .. %8s] | %7s" % ("-", "-", "-", "-")
            out("%-5s %5d | %26.1f %10.3f %9d %8d | %s"
                % (rho_s, B, B / sa, 1e3 * statistics.median(dev), info["launches"], info["forms"]["reduced"], btxt))
    if a.per_shape:
        out("# one model alone (rho 0.1, seed 0): us per iteration of the reduced loop = device time of the call / iterations")
        out("# shape          nodes  iterations | dense copies (f_Atd, f_Ad) us/iter | packed panels (pv_At, pc_A) us/iter")
        for s in shapes:
            m = build(problems, bnb, s, 0, 0.1)
            row = []
            for dense in ("1", "0"):
                os.environ["MIOSQP_TREE_R_DENSE"] = dense
                miosqp_amd.solve_models([m], large="device")
                dev = []
                for _ in range(a.repeats):
                    info = {}
                    r = miosqp_amd.solve_models([m], info=info, large="device")[0]
                    dev.append(info["device_time"])
                row.append(1e6 * statistics.median(dev) / r["osqp_iter"])
            os.environ.pop("MIOSQP_TREE_R_DENSE", None)
            m.work.solver.close()
            out("%-14s %6d %11d | %34.2f | %35.2f" % (str(s).replace(" ", ""), r["nodes"], r["osqp_iter"], row[0], row[1]))
    if f:
        f.close()


if __name__ == "__main__":
    main()
