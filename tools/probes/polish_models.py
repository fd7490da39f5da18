"""solve_models(polish=True): one MIQP on each of B DIFFERENT models, every tree in one call and every incumbent
polished in one more launch (miosqp_qp_polish_models), against the parent commit's way of getting the same answers:
solve_models followed by the loop models[k].polish_many([inst], [result]) -- whose first call on every engine builds
that engine's polish scratch.

Workload: the shapes of profiles/solve_models.txt (those of the reference's benchmark grid that the one-launch trees take,
plus the power-converter model); model k has shape k mod (number of shapes) and random_miqp seed k; B = 1, 8, 64, 256;
rho 0.1 and "auto".  Every model is polished exactly ONCE: each repeat sets up FRESH models (set-up is not timed).  One
warm-up cycle on 16 fresh models per process.  Per row, over --repeats repeats (median, [min .. max]):
  (a) MIQPs/s of solve_models(polish=True);
  (b) MIQPs/s of the yardstick: the library of --parent DIR (a built tree of the parent commit) in a child process,
      solve_models + the loop over polish_many;
  (d) MIQPs/s of solve_models(polish=True, polish_guess="device").
Before anything is timed, (a)'s polished, polish_rounds, x and upper_glob are asserted equal, bit for bit, to (b)'s on the
first repeat.  For B = 256 the split of the polish of one call: host preparation in the package (vectors, the guess),
staging in the library (rows of A, table), upload, launch, download, and the package's adoption of the points.

    python tools/probes/polish_models.py [--out FILE] [--batches 1,8,64,256] [--rhos 0.1,auto] [--repeats 3] [--parent DIR]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from solve_models import GRID, build_many  # noqa: E402


def digest(res):
    return [(bool(r["polished"]), int(r["polish_rounds"]), float(r["upper_glob"]).hex(),
             np.asarray(r["x"]).tobytes().hex() if np.isfinite(r["upper_glob"]) else "") for r in res]


def parent_way(pkg, models, insts):
    """what the parent commit offers: the trees in one call, then the polish model by model"""
    t0 = time.time()
    res = pkg.solve_models(models, insts)
    t1 = time.time()
    for m, i, r in zip(models, insts, res):
        m.polish_many([i], [r])
    return res, time.time() - t0, t1 - t0


def close(models):
    for m in models:
        m.work.solver.close()


def child(a):
    """the parent commit's library: solve_models + the loop over polish_many on fresh models per repeat, one JSON line"""
    sys.path.insert(0, a.parent)
    import miosqp_amd as pkg
    from miosqp_amd import bnb, problems
    assert os.path.abspath(bnb.__file__).startswith(os.path.abspath(a.parent))
    assert not hasattr(bnb, "polish_models")
    shapes = [s if s == "pc" else tuple(s) for s in json.loads(a.shapes)]
    rho = "auto" if a.rho == "auto" else float(a.rho)
    models, insts, _ = build_many(problems, bnb, shapes, 16, rho)  # warm-up
    parent_way(pkg, models, insts)
    close(models)
    times, trees, dig = [], [], None
    for _ in range(a.repeats):
        models, insts, _ = build_many(problems, bnb, shapes, int(a.batches), rho)
        res, t, tt = parent_way(pkg, models, insts)
        close(models)
        times.append(t)
        trees.append(tt)
        dig = dig or digest(res)
    print(json.dumps(dict(times=times, trees=trees, digest=dig)))


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
    import miosqp_amd as pkg
    from miosqp_amd import bnb, problems, qp
    f = open(a.out, "a") if a.out else None

    def out(s=""):
        print(s, flush=True)
        if f:
            f.write(s + "\n")
            f.flush()

    shapes = []
    for s in GRID + ["pc"]:
        m = build_many(problems, bnb, [s], 1, 0.1)[0][0]
        if m.work.solver.tree_form():
            shapes.append(s)
        m.work.solver.close()
    out("# solve_models(polish=True) against the parent commit's solve_models + loop over models[k].polish_many, one MI355X;")
    out("# model k: shape k mod %d of %s, seed k; fresh models per repeat (every model is polished once), %d repeats"
        % (len(shapes), " ".join(str(s).replace(" ", "") for s in shapes), a.repeats))
    models, insts, _ = build_many(problems, bnb, shapes, 16, 0.1)  # warm-up of every path
    pkg.solve_models(models, insts, polish=True)
    pkg.solve_models(models, insts, polish=True, polish_guess="device")
    close(models)
    out("# rho      B | (a) solve_models(polish=True) MIQPs/s [min .. max] | (b) parent: solve_models + polish loop MIQPs/s "
        "[min .. max]  of it trees ms | (a)/(b) | (d) polish_guess=\"device\" MIQPs/s [min .. max]  (d)/(a) | polished  launches")
    splits = []
    for rho_s in a.rhos.split(","):
        rho = "auto" if rho_s == "auto" else float(rho_s)
        for B in [int(b) for b in a.batches.split(",")]:
            pj = None
            if a.parent:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--parent", a.parent, "--rho", rho_s,
                                    "--batches", str(B), "--repeats", str(a.repeats), "--shapes", json.dumps(shapes)],
                                   capture_output=True, text=True, timeout=900)
                if r.returncode != 0:  # (nothing more is started on the device after a child that ended badly)
                    out("# the parent's child process ended with %d: %s" % (r.returncode, r.stderr.strip().splitlines()[-3:]))
                    sys.exit(1)
                pj = json.loads(r.stdout.strip().splitlines()[-1])
            ta, td, info = [], [], {}
            for rep in range(a.repeats):
                for guess, ts in (("host", ta), ("device", td)):
                    models, insts, _ = build_many(problems, bnb, shapes, B, rho)
                    info = {}
                    t0 = time.time()
                    res = pkg.solve_models(models, insts, info=info, polish=True, polish_guess=guess)
                    ts.append(time.time() - t0)
                    assert not info["own"] and not info["overflow"] and not info["polish_own"], info
                    if rep == 0 and guess == "host" and pj:
                        assert [tuple(t) for t in pj["digest"]] == digest(res), "the parent's answers differ (rho %s, B %d)" % (rho_s, B)
                    if rep == a.repeats - 1 and guess == "host" and B == 256:
                        # the polish of this call once more, by part (fresh models again: nothing of it has run on them)
                        close(models)
                        models, insts, _ = build_many(problems, bnb, shapes, B, rho)
                        plain = pkg.solve_models(models, insts)
                        seen = {}
                        inner = qp.polish_models

                        def spy(*args, **kw):
                            t1 = time.time()
                            r2 = inner(*args, **kw)
                            seen.update(call=time.time() - t1, stats=r2[1], at=t1, end=time.time())
                            return r2
                        qp.polish_models = spy
                        try:
                            t1 = time.time()
                            pkg.polish_models(models, insts, plain)
                            t2 = time.time()
                        finally:
                            qp.polish_models = inner
                        st = seen["stats"]
                        splits.append((rho_s, B, t2 - t1, seen["at"] - t1, seen["call"] - st.run_time, st.run_time - st.device_time,
                                       st.upload_time, st.launch_time, st.download_time, t2 - seen["end"], int(st.arena_bytes),
                                       int(st.lds_bytes)))
                    polished = sum(bool(r["polished"]) for r in res)
                    close(models)
            sa, sd = statistics.median(ta), statistics.median(td)
            if pj:
                tb = pj["times"]
                sb = statistics.median(tb)
                btxt = "%12.1f [%9.1f .. %9.1f] %12.3f" % (B / sb, B / max(tb), B / min(tb), 1e3 * statistics.median(pj["trees"]))
                rtxt = "%7.2f" % (sb / sa)
            else:
                btxt, rtxt = "%12s [%9s .. %9s] %12s" % ("-", "-", "-", "-"), "%7s" % "-"
            out("%-5s %5d | %12.1f [%9.1f .. %9.1f] | %s | %s | %12.1f [%9.1f .. %9.1f] %7.2f | %5d/%-5d %d"
                % (rho_s, B, B / sa, B / max(ta), B / min(ta), btxt, rtxt, B / sd, B / max(td), B / min(td), sa / sd, polished, B,
                   info["polish_launches"]))
    out("# the polish of one %d-model call by part, ms: total | package: vectors and the guess | package: lists into the entry's arrays | "
        "library: rows of A, vectors, table | upload | launch | download | package: adoption | arena KB  LDS bytes" % 256)
    for s in splits:
        out("%-5s %5d | %8.3f | %8.3f | %8.3f | %8.3f | %8.3f | %8.3f | %8.3f | %8.3f | %8.1f %8d"
            % (s[0], s[1], 1e3 * s[2], 1e3 * s[3], 1e3 * s[4], 1e3 * s[5], 1e3 * s[6], 1e3 * s[7], 1e3 * s[8], 1e3 * s[9],
               s[10] / 1024.0, s[11]))
    if f:
        f.close()


if __name__ == "__main__":
    main()
