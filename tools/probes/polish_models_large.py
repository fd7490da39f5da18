"""The third leg of the "own P and A per MIQP" path beyond one workgroup: `polish_models(large="device")` -- ONE launch
of k_pol_many_gm for the models k_pol_many_m cannot hold -- against the same call without the keyword, which polishes
such a model by its own `polish_many`: the host's dense restatement, once per model.

Shapes: the four large ones of the reference benchmark's grid, (50,200,10) (100,200,15) (150,100,5) (150,300,20), B = 1, 8,
64, 256 models per call (model b: problems.random_miqp(shape, seed=b)), rho 0.1, set up by setup_models(large="device"),
solved by solve_models(large="device"); what is polished are the trees' incumbents.  (50,200,10) fits the 160 KB of
k_pol_many_m: the launch without the keyword has always taken it, so its two columns measure the same path.
  * polish: wall time of `polish_models(..., large="device")` and of `polish_models(...)` on copies of the same raw
    results, both after a warm-up call in the same session; medians of `reps` -- the host path stops repeating once it has
    used `budget` seconds (it takes minutes at 256 models; the number of repetitions is printed);
  * launch: stats.launch_time against stats.run_time of one `qp.polish_models_large` call on the same inputs (median of
    `reps`): how much of the call is the kernel and how much host work (staging, upload, download);
  * end to end: `solve_models(large="device", polish=True)` with and without polish_large="device", B = 8 and 64.

    python tools/probes/polish_models_large.py [--out profiles/polish_models_large.txt] [--reps 5] [--budget 20]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import miosqp_amd  # noqa: E402
from miosqp_amd import bnb, problems, qp  # noqa: E402

SHAPES = [(50, 200, 10), (100, 200, 15), (150, 100, 5), (150, 300, 20)]
BATCHES = [1, 8, 64, 256]
END_TO_END = [8, 64]
RHO = 0.1


def build(shape, B):
    prs = [problems.random_miqp(*shape, seed=b) for b in range(B)]
    return miosqp_amd.setup_models(prs, dict(problems.BNB_SETTINGS, tree_explor_rule=1), dict(problems.QP_SETTINGS, rho=RHO),
                                   large="device")


def timed(fn, reps, budget):
    """(median seconds, repetitions): fn() up to `reps` times, no further repetition once `budget` seconds are used"""
    ts, used = [], 0.0
    while len(ts) < reps and (not ts or used < budget):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
        used += ts[-1]
    return float(np.median(ts)), len(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--budget", type=float, default=20.0)
    ap.add_argument("--batches", type=int, nargs="*", default=BATCHES)
    a = ap.parse_args()
    f = open(a.out, "w") if a.out else None

    def out(s=""):
        print(s, flush=True)
        if f:
            f.write(s + "\n")
            f.flush()

    out("# polish_models(large=\"device\") (k_pol_many_gm, ONE launch for the models beyond k_pol_many_m) against the same call "
        "without the keyword (such a model: the host's polish_restatement); one MI355X, random_miqp seeds 0 .. B-1, rho %g, "
        "tree_explor_rule 1, repair_iter 20; wall times in ms, medians of %d after a warm-up call (host path: fewer once %g s "
        "are used, the count is printed)" % (RHO, a.reps, a.budget))
    out("# shape            B | keyword: call   /model  forms(small,large) W | without: call   /model  own  reps | speed-up | "
        "large entry: launch   run  launch/run | polished kw / without")
    for shape in SHAPES:
        for B in a.batches:
            models = build(shape, B)
            insts = [{} for _ in models]
            raw = miosqp_amd.solve_models(models, insts, large="device")
            fresh = lambda: [dict(r, x=np.array(r["x"], dtype=float)) for r in raw]  # noqa: E731
            info, plain_info = {}, {}
            miosqp_amd.polish_models(models, insts, fresh(), large="device", info=info)  # (warm-up: the arena)
            kw, _ = timed(lambda: miosqp_amd.polish_models(models, insts, fresh(), large="device", info=info), a.reps, 1e9)
            got = miosqp_amd.polish_models(models, insts, fresh(), large="device")
            # the engine-level call on the same inputs, for the split of its time
            ks = [k for k, r in enumerate(raw) if r["status"] in (bnb.MI_SOLVED, bnb.MI_MAX_ITER_FEASIBLE)]
            launch = run = W = float("nan")
            if ks and info["polish_forms"]["large"]:
                inp = []
                for k in ks:
                    d = models[k].work.data
                    x = np.array(raw[k]["x"], dtype=float)
                    xi = np.round(x[d.i_idx])
                    x[d.i_idx] = xi
                    l, u = d.l.copy(), d.u.copy()
                    l[d.m:] = xi
                    u[d.m:] = xi
                    inp.append((d.q, l, u, x, bnb.primal_guess_multipliers(l, u, d.A.dot(x), 10 * problems.QP_SETTINGS["eps_abs"])))
                stats = []
                for _ in range(a.reps):
                    stats.append(qp.polish_models_large([models[k].work.solver for k in ks], *[[v[j] for v in inp] for j in range(5)],
                                                        1e-6, 3, 20)[1])
                launch = 1e3 * float(np.median([s.launch_time for s in stats]))
                run = 1e3 * float(np.median([s.run_time for s in stats]))
                W = stats[0].workgroups
            # without the keyword (the parent's path); at 256 models the warm-up is the first two models only
            warm = list(range(B)) if B <= 64 else [0, 1]
            miosqp_amd.polish_models([models[k] for k in warm], [insts[k] for k in warm], [fresh()[k] for k in warm])
            plain, reps = timed(lambda: miosqp_amd.polish_models(models, insts, fresh(), info=plain_info), a.reps, a.budget)
            want = miosqp_amd.polish_models(models, insts, fresh()) if B <= 8 else None
            pk = sum(bool(r["polished"]) for r in got)
            pw = sum(bool(r["polished"]) for r in want) if want is not None else -1
            out("%-15s %4d | %12.2f %8.3f  (%d,%d) %5s | %12.2f %8.3f %4d %5d | %8.1f | %18.2f %6.2f %8.2f | %d / %s of %d"
                % ("(%d,%d,%d)" % shape, B, 1e3 * kw, 1e3 * kw / B, info["polish_forms"]["small"], info["polish_forms"]["large"],
                   "-" if W != W else "%d" % W, 1e3 * plain, 1e3 * plain / B, len(plain_info["polish_own"]), reps, plain / kw,
                   launch, run, launch / run if run == run else float("nan"), pk, "-" if pw < 0 else "%d" % pw, B))
            for m in models:
                m.work.solver.close()
    out("# end to end: solve_models(large=\"device\", polish=True) with / without polish_large=\"device\"; ms, medians of 3 "
        "after a warm-up call (without: fewer once %g s are used)" % a.budget)
    out("# shape            B | with: call   /model | without: call   /model reps | speed-up")
    for shape in SHAPES:
        for B in END_TO_END:
            models = build(shape, B)
            miosqp_amd.solve_models(models, large="device", polish=True, polish_large="device")
            kw, _ = timed(lambda: miosqp_amd.solve_models(models, large="device", polish=True, polish_large="device"), 3, 1e9)
            miosqp_amd.solve_models(models, large="device", polish=True)
            plain, reps = timed(lambda: miosqp_amd.solve_models(models, large="device", polish=True), 3, a.budget)
            out("%-15s %4d | %10.2f %8.3f | %13.2f %8.3f %4d | %8.1f" % ("(%d,%d,%d)" % shape, B, 1e3 * kw, 1e3 * kw / B,
                                                                        1e3 * plain, 1e3 * plain / B, reps, plain / kw))
            for m in models:
                m.work.solver.close()
    if f:
        f.close()


if __name__ == "__main__":
    main()
