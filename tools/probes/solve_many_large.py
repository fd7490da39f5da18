"""solve_many(..., large="device"): B MIQPs on ONE model beyond one workgroup's product form, every tree in one launch
(miosqp_qp_solve_trees_large, k_tree_r: the batch form of k_tree_r_m) against what the library offered such a user so far.

Workload: the four shapes of the reference's benchmark grid with tree_form() 0 and tree_form_large() 3, one model per
shape (random_miqp seed 0), instance k another q, l, u (q + 0.1 randn, the box widened by 0.05 rand; RandomState(100 + k));
B = 1, 8, 64, 256 instances; rho 0.1 and "auto".  Per row, MIQPs/s by a host clock around the call (every call ends in a
device synchronise), after one untimed call of the same B:
  new  solve_many(inst, large="device"): median of --repeats calls and their spread;
  (a)  solve_many(inst): what lockstep=None picks without the keyword (that path's code is the parent commit's, unchanged);
  (b)  solve_many(inst, lockstep="device");
  (c)  solve_models over B separately set-up copies of the model with large="device" (the set-up is not timed).
(a), (b), (c): one call each (--baseline-repeats).  Before a row is timed, status, nodes and iterations of `new` are
asserted equal to (c)'s on the first min(B, 8) instances.  (c) is built up to --copies-max copies.
Then round and fix and strong / reliability branching on (100,200,15) at B = 64 and 256: the same call with and without
`large`.  The probe stops at --deadline seconds and says which rows it did not reach.

    python tools/probes/solve_many_large.py [--out profiles/solve_many_large.txt] [--batches 1,8,64,256] [--rhos 0.1,auto]
                                            [--repeats 3] [--deadline 600]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = [(50, 200, 10), (100, 200, 15), (150, 100, 5), (150, 300, 20)]


def build(problems, bnb, pr, rho, **st):
    m = bnb.MIOSQP()
    m.setup(pr["P"], pr["q"], pr["A"], np.copy(pr["l"]), np.copy(pr["u"]), pr["i_idx"], pr["i_l"], pr["i_u"],
            dict(problems.BNB_SETTINGS, **st), dict(problems.QP_SETTINGS, rho=rho))
    return m


def instance(pr, k):
    rng = np.random.RandomState(100 + k)
    n, m = len(pr["q"]), len(pr["l"])
    return dict(q=pr["q"] + 0.1 * rng.randn(n), l=pr["l"] - 0.05 * rng.rand(m), u=pr["u"] + 0.05 * rng.rand(m))


def rate(call, B, repeats):
    """MIQPs/s of `call`: (median, min, max) over `repeats` timed calls"""
    r = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        r.append(B / (time.perf_counter() - t0))
    return statistics.median(r), min(r), max(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solve_many_large.txt"))
    ap.add_argument("--batches", default="1,8,64,256")
    ap.add_argument("--rhos", default="0.1,auto")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline-repeats", type=int, default=1)
    ap.add_argument("--deadline", type=float, default=600.0)
    ap.add_argument("--copies-max", type=int, default=256, help="(c) is measured up to this many copies of the model")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import miosqp_amd
    from miosqp_amd import bnb, problems
    batches = [int(b) for b in a.batches.split(",")]
    rhos = [r if r == "auto" else float(r) for r in a.rhos.split(",")]
    t_start = time.perf_counter()
    left = lambda: a.deadline - (time.perf_counter() - t_start)  # noqa: E731
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w")

    def say(line=""):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    say("# solve_many(large=\"device\") on one MI355X; one model per shape (seed 0), instance k: RandomState(100 + k); MIQPs/s")
    say("# new: median [min .. max] of %d calls; (a) lockstep=None without the keyword, (b) lockstep=\"device\", (c) solve_models over B"
        % a.repeats)
    say("# separately set-up copies with large=\"device\": %d call each" % a.baseline_repeats)
    say("# shape          rho      B |      new  [    min ..     max] |      (a)  new/(a) |      (b)  new/(b) |      (c)  new/(c)")
    skipped = []
    for rho in rhos:
        for shape in SHAPES:
            pr = problems.random_miqp(*shape, seed=0)
            mdl = build(problems, bnb, pr, rho)
            assert mdl.work.solver.tree_form() == 0 and mdl.work.solver.tree_form_large() == 3, shape
            copies = []
            for B in batches:
                if left() < 100:  # (the last 100 s belong to the second table)
                    skipped.append((shape, rho, B))
                    continue
                inst = [instance(pr, k) for k in range(B)]
                new = mdl.solve_many(inst, large="device")  # (untimed: the arena of this B)
                assert len(mdl.work.trees_info) == B
                while len(copies) < min(B, a.copies_max):
                    copies.append(build(problems, bnb, pr, rho))
                C = len(copies)
                ref = miosqp_amd.solve_models(copies, inst[:C], large="device")
                for k in range(min(B, 8, C)):
                    assert (new[k]["status"], new[k]["nodes"], new[k]["osqp_iter"]) == \
                        (ref[k]["status"], ref[k]["nodes"], ref[k]["osqp_iter"]), (shape, rho, B, k)
                r_new = rate(lambda: mdl.solve_many(inst, large="device"), B, a.repeats)
                cols = []
                for name, call, count in (
                        ("a", lambda: mdl.solve_many(inst), B),
                        ("b", lambda: mdl.solve_many(inst, lockstep="device"), B),
                        ("c", lambda: miosqp_amd.solve_models(copies, inst[:C], large="device"), C)):
                    if left() < 100 or (name == "c" and C < B):
                        cols.append("%8s  %7s" % ("-", "-"))
                        continue
                    if name != "c" and B <= 8:
                        call()  # (untimed; the large rows take too long to run twice)
                    r = rate(call, count, a.baseline_repeats)
                    cols.append("%8.1f  %7.2f" % (r[0], r_new[0] / r[0]))
                say("%-14s %5s %6d | %8.1f  [%7.1f .. %7.1f] | %s" % ("(%d,%d,%d)" % shape, rho, B, r_new[0], r_new[1], r_new[2],
                                                                     " | ".join(cols)))
            for m in copies + [mdl]:
                m.work.solver.close()
    # ---- round and fix, strong / reliability branching: the same call with and without `large` ----
    say("# (100,200,15), rho 0.1: the same call with and without large=\"device\"; MIQPs/s, one call each after an untimed one of new")
    say("# variant                       B |     with  without  with/without")
    shape = (100, 200, 15)
    pr = problems.random_miqp(*shape, seed=0)
    for name, st, kw in (("heuristic=\"device\"", dict(primal_heuristic=1, rf_every=3, rf_candidates=7), dict(heuristic="device")),
                         ("branching=\"device\" rule 1", dict(branching_rule=1), dict(branching="device")),
                         ("branching=\"device\" rule 2", dict(branching_rule=2), dict(branching="device"))):
        mdl = build(problems, bnb, pr, 0.1, **st)
        for B in (64, 256):
            if left() < 20:
                skipped.append((name, B))
                continue
            inst = [instance(pr, k) for k in range(B)]
            mdl.solve_many(inst, large="device", **kw)
            w = rate(lambda: mdl.solve_many(inst, large="device", **kw), B, 1)
            if left() < 20:
                say("%-28s %4d | %8.1f  %7s  %7s" % (name, B, w[0], "-", "-"))
                continue
            o = rate(lambda: mdl.solve_many(inst, **kw), B, 1)
            say("%-28s %4d | %8.1f  %7.1f  %7.2f" % (name, B, w[0], o[0], w[0] / o[0]))
        mdl.work.solver.close()
    if skipped:
        say("# not measured (the probe's deadline of %.0f s): %r" % (a.deadline, skipped))
    say("# %.0f s" % (time.perf_counter() - t_start))
    out.close()


if __name__ == "__main__":
    main()
