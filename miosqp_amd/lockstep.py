"""B branch-and-bound trees on one factorisation, advanced in lock step: one node of every unfinished tree per wave.

`MIOSQP.solve_many` calls `run` for problems beyond the one-launch trees (`miosqp_qp_solve_trees`: a whole tree per
workgroup, n + M <= 192).  Every tree keeps its own state -- leaf list, incumbent, counters and a view of the model's
`Data` whose q, l, u are the instance's -- in a `Workspace` that shares the model's solver and settings and was never
set up itself (`_Tree`).  One wave:

  * every tree that can continue takes its next leaf by `leaf_index(tree_explor_rule)`;
  * the chosen leaves go out together, each with its tree's linear cost: ONE `solve_batch_q` on the HIP engine
    (`miosqp_qp_solve_batch_q`, which slices a wave wider than max_batch), column by column (`update(q=)` +
    `Node.solve`) on a solver without it -- the generic wave, which is the restatement the CPU tests run;
  * every tree runs the unchanged `Workspace.bound_and_branch` on its leaf and counts the node.

`run_device` is the same wave loop in the library (`OSQP.solve_trees_lockstep`, miosqp_qp_solve_trees_lockstep): the
leaves of all trees stay in device slots, the per-tree logic runs in C++ and Python sees the B results.  It is asked for
by name: `solve_many(lockstep="device")`.  It is also the one driver that runs round and fix (primal_heuristic = 1)
inside the trees (`OSQP.solve_trees_lockstep_rf`): the candidates of every tree that fires in a wave go out as one more
batch.  And the one that runs branching_rule 1 and 2 (`OSQP.solve_trees_lockstep_sb`): the strong-branching children of
every node with candidates in a wave go out as one more batch, and the position is chosen per tree as
`Workspace.select_branching` chooses it.

`run_refill` drops the wave (`OSQP.solve_trees_refill`, miosqp_qp_solve_trees_refill): a column of the batch holds one
node of one tree and counts its own iterations; after every chunk of check_termination iterations the decided columns
are harvested and, at that same boundary, loaded again with the next leaf of a tree that has no node in flight.  A tree
still has at most one node in flight, so its decisions are those of the wave drivers.  Asked for by name as well:
`solve_many(lockstep="refill")`.

`run_ahead` keeps the wave and fills its spare columns (`OSQP.solve_trees_lockstep_ahead`,
miosqp_qp_solve_trees_lockstep_ahead): a wave launches whole tiles of 64 columns, and behind the chosen leaves a tree
solves other open leaves and children of nodes it has solved ahead; such a record waits with its node until the tree's
rule reaches it.  Asked for by name: `solve_many(lockstep="ahead", ahead=8)`.

A node is a pure function of (q, l, u, x0, y0), so every tree makes exactly the decisions of its sequential solve
(`update_vectors` + `set_x0` + `solve`), node for node.  The wave waits for its slowest column; trees finish at
different waves and later waves are narrower.

The rounding heuristic of the device digest tests the rounded point against the ENGINE's root bounds (set_root: the
model's).  For an instance with l, u of its own that verdict is replaced on the host with the test against the
instance's root bounds (`Workspace.satisfies_lin_constraints`, one product with A) at the nodes where
`bound_and_branch` asks for it -- those whose rounded point would improve the incumbent; everything else of the digest
depends on the node alone.
"""
import copy
from time import time

import numpy as np

from miosqp_amd import bnb


class _Tree(bnb.Workspace):
    """One instance's tree: a Workspace on the model's solver and settings with its own data view and state"""

    def __init__(self, work, q, l, u, own_bounds, upper, x0):
        # (no Workspace.__init__: nothing is set up, the solver is the model's)
        for name in ('settings', 'sb', 'rf', 'pol', 'pol_repair_iter', '_second', 'backend', 'constant', 'ok', 'solver',
                     'qp_settings', 'root_on_device'):
            setattr(self, name, getattr(work, name))
        data = copy.copy(work.data)
        data.q, data.l, data.u = q, l, u
        self.data = data
        self.own_bounds = own_bounds
        self._reset_counters()
        self.defer_lower = True  # lower_glob is only reported: once, when the trees are done (as a wave of solve_wave defers it)
        self.leaves = [self._make_root()]
        # Workspace.set_x0 (workspace.py:94-111), judged by solve_many on the instance's vectors
        self.upper_glob = upper
        self.x = x0 if np.isfinite(upper) else np.empty(data.n)

    def absorb_digest(self, leaf):
        """see the module text: the heuristic's feasibility verdict against this instance's root bounds"""
        dg = leaf.digest
        if dg is None or not self.own_bounds or leaf.status not in self.ok:
            return
        if not dg.heur_obj < self.upper_glob:
            return  # bound_and_branch asks for the verdict only when the rounded point would improve the incumbent
        x_int = self.get_integer_solution(leaf.x)
        dg.heur_feasible = bool(self.satisfies_lin_constraints(x_int, self.data.l, self.data.u))


def supported(work):
    """the settings the lock-step trees cover: most-fractional branching, no round and fix, rules 0-3"""
    st = work.settings
    return st['branching_rule'] == 0 and not work.rf['on'] and st['tree_explor_rule'] in (0, 1, 2, 3)


def _wave_batched(solver, trees, live, leaves):
    r = solver.solve_batch_q(np.stack([trees[k].data.q for k in live]),
                             np.stack([lf.l for lf in leaves]), np.stack([lf.u for lf in leaves]),
                             np.stack([lf.x for lf in leaves]), np.stack([lf.y for lf in leaves]))
    for c, lf in enumerate(leaves):
        lower = None if np.isnan(r.lower[c]) else float(r.lower[c])
        lf._absorb(int(r.status_val[c]), int(r.iter[c]), float(r.run_time[c]), r.x[c].copy(), r.y[c].copy(), lower)
        lf.digest = r.digest[c] if getattr(r, 'digest', None) is not None else None
    return int(np.max(r.iter)), float(np.mean(r.iter))


def _wave_generic(model, trees, live, leaves):
    work = model.work
    for k, lf in zip(live, leaves):
        q = trees[k].data.q
        work.solver.update(q=q)
        for second in work._second.values():
            second.update(q=q)
        lf.solve()
    it = [lf.num_iter for lf in leaves]
    return int(max(it)), float(np.mean(it))


def run(model, todo, Q, L, U, up, XI, instances, out, batched):
    """The trees of instances `todo` in lock step; fills out[k] with what the sequential path of solve_many puts there.
    Q, L, U: instance-major vectors; up, XI: upper bound and point of an accepted x0 (inf without one).  batched: the
    wave is one solve_batch_q; otherwise the generic wave, after which the solver's q is put back.  Leaves
    work.lockstep = dict(instances, waves, nodes, batched, max_width, iters_max, iters_mean, finished_at, driver): per
    wave the largest and the mean ADMM iteration count of its columns; per instance the wave after which its tree was
    done; driver 'python' (run_device leaves 'device')."""
    work, data = model.work, model.work.data
    rule = work.settings['tree_explor_rule']
    t0 = time()
    trees = {}
    for k in todo:
        inst = instances[k]
        own = inst.get('l') is not None or inst.get('u') is not None
        trees[k] = _Tree(work, Q[k].copy(), L[k].copy(), U[k].copy(), own, float(up[k]), XI[k].copy())
    info = dict(instances=len(todo), waves=0, nodes=0, batched=bool(batched), max_width=0, iters_max=[], iters_mean=[],
                finished_at={}, driver='python')
    q_keep = data.q
    try:
        while True:
            live = [k for k in todo if trees[k].can_continue()]
            if not live:
                break
            leaves = [trees[k].choose_leaf(rule) for k in live]
            if batched:
                imax, imean = _wave_batched(work.solver, trees, live, leaves)
            else:
                imax, imean = _wave_generic(model, trees, live, leaves)
            info['waves'] += 1
            info['nodes'] += len(live)
            info['max_width'] = max(info['max_width'], len(live))
            info['iters_max'].append(imax)
            info['iters_mean'].append(imean)
            for k, lf in zip(live, leaves):
                tree = trees[k]
                tree.absorb_digest(lf)
                tree.bound_and_branch(lf)
                tree.iter_num += 1
                if not tree.can_continue():
                    info['finished_at'][k] = info['waves']
    finally:
        if not batched:
            work.solver.update(q=q_keep)
            for second in work._second.values():
                second.update(q=q_keep)
        work.lockstep = info
    dt = time() - t0
    for k in todo:
        tree = trees[k]
        info['finished_at'].setdefault(k, 0)  # (a tree with nothing to do: max_iter_bb <= 1)
        if tree.leaves:
            tree.lower_glob = min(lf.lower for lf in tree.leaves)
        tree.osqp_iter_avg = tree.osqp_iter / tree.iter_num
        tree.get_return_status()
        tree.get_return_solution()
        out[k] = dict(x=np.array(tree.x, dtype=float), upper_glob=tree.upper_glob, status=tree.status,
                      nodes=tree.iter_num - 1, osqp_iter=tree.osqp_iter, run_time=dt / len(todo))


def device_supported(work):
    """the device driver needs the HIP engine's entry and the on-device digest (set_root)"""
    return hasattr(work.solver, 'solve_trees_lockstep') and work.root_on_device and work.data.n_int > 0


def device_rf_supported(work):
    """round and fix inside the device driver (`OSQP.solve_trees_lockstep_rf`): the entry, the on-device digest,
    most-fractional branching, rules 0-3"""
    st = work.settings
    return hasattr(work.solver, 'solve_trees_lockstep_rf') and work.root_on_device and work.data.n_int > 0 \
        and st['branching_rule'] == 0 and st['tree_explor_rule'] in (0, 1, 2, 3)


def device_sb_supported(work):
    """strong and reliability branching inside the device driver (`OSQP.solve_trees_lockstep_sb`): the entry, the
    on-device digest, branching_rule 1 or 2, no round and fix, rules 0-3"""
    st = work.settings
    return hasattr(work.solver, 'solve_trees_lockstep_sb') and work.root_on_device and work.data.n_int > 0 \
        and st['branching_rule'] in (1, 2) and not work.rf['on'] and st['tree_explor_rule'] in (0, 1, 2, 3)


def run_device(model, todo, Q, L, U, up, XI, instances, out, capacity=0):
    """`run` in the library: the trees of instances `todo` advance in lock step inside ONE call of
    `OSQP.solve_trees_lockstep` -- leaves in device slots, the tree logic in C++ (csrc/lockstep_trees.hpp), per wave five
    integers per column up and a 64-byte record per column down.  Fills out[k] with the dicts `run` forms and leaves
    work.lockstep with the same keys, driver='device', plus grown (times the slot store grew), iters_slowest,
    iters_all, device_time, run_time and host_time (the library's call and, of it, the tree logic between the waves).  The value of an incumbent found by the rounding heuristic is the device's sum
    (`run` recomputes it with numpy: ~1e-12 relative apart), as in the hosted search.  The model's q, l, u, leaves and
    counters are not touched.  capacity: starting number of node slots (0: the engine's default).
    With primal_heuristic = 1 (work.rf['on']) the call is `OSQP.solve_trees_lockstep_rf`: round and fix runs inside the
    trees, the candidates of all trees that fire in a wave as one more batch (rf_candidates, rf_max_iter, rf_every as
    `Workspace.primal_heuristic` reads them), and work.lockstep['rf'] = dict(calls, candidates, feasible, improved,
    osqp_iter -- the sums of what `rf_stats` counts per sequential solve --, batches, columns, iters_slowest,
    device_time, per_instance={k: dict(calls, candidates, feasible, improved, osqp_iter)}); the dicts' osqp_iter counts
    node relaxations only, as work.osqp_iter does.
    With branching_rule 1 or 2 (work.sb['rule']) the call is `OSQP.solve_trees_lockstep_sb`: every node that branches
    chooses its position as `Workspace.select_branching` does, the strong-branching children of all nodes with
    candidates in a wave as one more batch (sb_candidates, sb_max_iter, sb_reliability, sb_eps as the workspace reads
    them), and work.lockstep['sb'] = dict(calls, children, osqp_iter -- the sums of what `sb_stats` counts per
    sequential solve --, batches, columns, iters_slowest, device_time, per_instance={k: dict(calls, children,
    osqp_iter)}).  The model's own sb_stats and pseudo-costs are not touched."""
    work, data, st = model.work, model.work.data, model.work.settings
    todo = list(todo)
    n, M = data.n, data.m + data.n_int
    t0 = time()
    any_inc = bool(np.any(np.isfinite(up[todo])))
    args = (Q[todo], L[todo], U[todo], np.zeros((len(todo), n)), np.zeros((len(todo), M)), up[todo],
            XI[todo] if any_inc else None, st['tree_explor_rule'], st['max_iter_bb'])
    r = b = None
    if work.sb['rule'] in (1, 2):
        sb = work.sb
        X, infos, s, b = work.solver.solve_trees_lockstep_sb(*args, sb['rule'], sb['K'], sb['max_iter'], sb['reliability'],
                                                             sb['eps'], capacity=capacity)
    elif work.rf['on']:
        X, infos, s, r = work.solver.solve_trees_lockstep_rf(*args, work.rf['K'], work.rf['max_iter'], work.rf['every'],
                                                             capacity=capacity)
    else:
        X, infos, s = work.solver.solve_trees_lockstep(*args, capacity=capacity)
    dt = time() - t0
    work.lockstep = dict(instances=len(todo), waves=s.waves, nodes=int(s.nodes), batched=True, max_width=s.max_width,
                         iters_max=s.iters_max, iters_mean=s.iters_mean,
                         finished_at={k: int(s.finished_at[j]) for j, k in enumerate(todo)}, driver='device',
                         grown=s.grown, iters_slowest=int(s.iters_slowest), iters_all=int(s.iters_all),
                         device_time=s.device_time, run_time=s.run_time, host_time=s.host_time)
    if r is not None:
        per = {k: dict(calls=r.calls[j], candidates=r.candidates[j], feasible=r.feasible[j], improved=r.improved[j],
                       osqp_iter=r.iters[j]) for j, k in enumerate(todo)}
        work.lockstep['rf'] = dict(calls=sum(r.calls), candidates=sum(r.candidates), feasible=sum(r.feasible),
                                   improved=sum(r.improved), osqp_iter=sum(r.iters), batches=r.batches,
                                   columns=int(r.columns), iters_slowest=int(r.iters_slowest),
                                   device_time=r.device_time, per_instance=per)
    if b is not None:
        per = {k: dict(calls=b.calls[j], children=b.children[j], osqp_iter=b.iters[j]) for j, k in enumerate(todo)}
        work.lockstep['sb'] = dict(calls=sum(b.calls), children=sum(b.children), osqp_iter=sum(b.iters), batches=b.batches,
                                   columns=int(b.columns), iters_slowest=int(b.iters_slowest), device_time=b.device_time,
                                   per_instance=per)
    for j, k in enumerate(todo):
        info = infos[j]
        upper = info.upper_glob
        # workspace.py:352-373 decides on the loop counter (iter_num = nodes + 1), as solve_many's one-launch path does
        finished = int(info.nodes) + 1 < st['max_iter_bb']
        if upper != np.inf:
            status = bnb.MI_SOLVED if finished else bnb.MI_MAX_ITER_FEASIBLE
        elif upper >= 0:
            status = bnb.MI_PRIMAL_INFEASIBLE if finished else bnb.MI_MAX_ITER_UNSOLVED
        else:
            status = bnb.MI_DUAL_INFEASIBLE
        x = X[j].copy() if (info.found or np.isfinite(up[k])) else np.empty(n)
        if status in (bnb.MI_SOLVED, bnb.MI_MAX_ITER_FEASIBLE):
            x[data.i_idx] = np.round(x[data.i_idx])
        out[k] = dict(x=x, upper_glob=upper, status=status, nodes=int(info.nodes), osqp_iter=int(info.osqp_iter),
                      run_time=dt / len(todo))


def refill_supported(work):
    """the refill driver needs the HIP engine's entry and the on-device digest (set_root)"""
    return hasattr(work.solver, 'solve_trees_refill') and work.root_on_device and work.data.n_int > 0


def run_refill(model, todo, Q, L, U, up, XI, instances, out, capacity=0):
    """`run_device` without the wave: the trees of instances `todo` inside ONE call of `OSQP.solve_trees_refill` -- a
    column holds one node of one tree, the columns decided in a chunk are harvested at its boundary and refilled there
    with the next leaf of a tree that has no node in flight (csrc/lockstep_refill.hpp, csrc/host_refill.inc).  Fills out[k]
    with the dicts `run_device` forms (the same device sums: upper_glob and x are equal bit for bit) and leaves
    work.lockstep = dict(driver='refill', instances, chunks, nodes, columns, occupancy (busy column-chunks / all
    column-chunks), chunk_busy (busy columns per chunk), finished_at (per instance, a chunk number), grown, iters_all,
    device_time, run_time, host_time, chunk_time, batched=True).  The model's q, l, u, leaves and counters are not
    touched.  capacity: starting number of node slots (0: the engine's default)."""
    work, data, st = model.work, model.work.data, model.work.settings
    todo = list(todo)
    n, M = data.n, data.m + data.n_int
    t0 = time()
    any_inc = bool(np.any(np.isfinite(up[todo])))
    X, infos, s = work.solver.solve_trees_refill(
        Q[todo], L[todo], U[todo], np.zeros((len(todo), n)), np.zeros((len(todo), M)), up[todo],
        XI[todo] if any_inc else None, st['tree_explor_rule'], st['max_iter_bb'], capacity=capacity)
    dt = time() - t0
    work.lockstep = dict(instances=len(todo), chunks=s.chunks, nodes=int(s.nodes), batched=True, columns=s.columns,
                         occupancy=(s.busy / s.total if s.total else 0.0), chunk_busy=s.chunk_busy,
                         finished_at={k: int(s.finished_at[j]) for j, k in enumerate(todo)}, driver='refill',
                         grown=s.grown, iters_all=int(s.iters_all), device_time=s.device_time, run_time=s.run_time,
                         host_time=s.host_time, chunk_time=s.chunk_time)
    for j, k in enumerate(todo):
        info = infos[j]
        upper = info.upper_glob
        # workspace.py:352-373 decides on the loop counter (iter_num = nodes + 1), as run_device does
        finished = int(info.nodes) + 1 < st['max_iter_bb']
        if upper != np.inf:
            status = bnb.MI_SOLVED if finished else bnb.MI_MAX_ITER_FEASIBLE
        elif upper >= 0:
            status = bnb.MI_PRIMAL_INFEASIBLE if finished else bnb.MI_MAX_ITER_UNSOLVED
        else:
            status = bnb.MI_DUAL_INFEASIBLE
        x = X[j].copy() if (info.found or np.isfinite(up[k])) else np.empty(n)
        if status in (bnb.MI_SOLVED, bnb.MI_MAX_ITER_FEASIBLE):
            x[data.i_idx] = np.round(x[data.i_idx])
        out[k] = dict(x=x, upper_glob=upper, status=status, nodes=int(info.nodes), osqp_iter=int(info.osqp_iter),
                      run_time=dt / len(todo))


def ahead_supported(work):
    """the ahead driver needs the HIP engine's entry and the on-device digest (set_root)"""
    return hasattr(work.solver, 'solve_trees_lockstep_ahead') and work.root_on_device and work.data.n_int > 0


def run_ahead(model, todo, Q, L, U, up, XI, instances, out, ahead=8, capacity=0):
    """`run_device` with the spare columns of every wave put to use: the trees of instances `todo` inside ONE call of
    `OSQP.solve_trees_lockstep_ahead` -- a tree may hold up to `ahead` columns of a wave, its chosen leaf and, in the free
    columns of the tiles the wave launches anyway, other open leaves and children of nodes solved ahead; a record waits
    with its node until the tree's rule reaches it (csrc/lockstep_ahead.hpp, csrc/host_lockstep_ahead.inc).  Fills
    out[k] with the dicts `run_device` forms, equal to them bit for bit, and leaves work.lockstep with `run_device`'s
    keys, driver='ahead' (nodes: the absorbed nodes over all trees; max_width counts all columns; iters_max and
    iters_mean the mandatory columns of each wave), plus work.lockstep['ahead'] = dict(ahead, columns, sent, hits,
    discarded, called_off, hit_iters, discarded_iters, called_off_iters, free_slots, slot_cap, width, iter_mandatory,
    chunks -- the last three per wave).  The model's q, l, u, leaves and counters are not touched.  capacity: starting
    number of node slots (0: the engine's default)."""
    work, data, st = model.work, model.work.data, model.work.settings
    todo = list(todo)
    n, M = data.n, data.m + data.n_int
    t0 = time()
    any_inc = bool(np.any(np.isfinite(up[todo])))
    X, infos, s, a = work.solver.solve_trees_lockstep_ahead(
        Q[todo], L[todo], U[todo], np.zeros((len(todo), n)), np.zeros((len(todo), M)), up[todo],
        XI[todo] if any_inc else None, st['tree_explor_rule'], st['max_iter_bb'], ahead, capacity=capacity)
    dt = time() - t0
    work.lockstep = dict(instances=len(todo), waves=s.waves, nodes=int(s.nodes), batched=True, max_width=s.max_width,
                         iters_max=s.iters_max, iters_mean=s.iters_mean,
                         finished_at={k: int(s.finished_at[j]) for j, k in enumerate(todo)}, driver='ahead',
                         grown=s.grown, iters_slowest=int(s.iters_slowest), iters_all=int(s.iters_all),
                         device_time=s.device_time, run_time=s.run_time, host_time=s.host_time,
                         ahead=dict(ahead=int(ahead), columns=int(a.columns), sent=int(a.sent), hits=int(a.hits),
                                    discarded=int(a.discarded), called_off=int(a.called_off), hit_iters=int(a.hit_iters),
                                    discarded_iters=int(a.discarded_iters), called_off_iters=int(a.called_off_iters),
                                    free_slots=int(a.free_slots), slot_cap=int(a.slot_cap), width=a.width,
                                    iter_mandatory=a.iter_mandatory, chunks=a.chunks))
    for j, k in enumerate(todo):
        info = infos[j]
        upper = info.upper_glob
        # workspace.py:352-373 decides on the loop counter (iter_num = nodes + 1), as run_device does
        finished = int(info.nodes) + 1 < st['max_iter_bb']
        if upper != np.inf:
            status = bnb.MI_SOLVED if finished else bnb.MI_MAX_ITER_FEASIBLE
        elif upper >= 0:
            status = bnb.MI_PRIMAL_INFEASIBLE if finished else bnb.MI_MAX_ITER_UNSOLVED
        else:
            status = bnb.MI_DUAL_INFEASIBLE
        x = X[j].copy() if (info.found or np.isfinite(up[k])) else np.empty(n)
        if status in (bnb.MI_SOLVED, bnb.MI_MAX_ITER_FEASIBLE):
            x[data.i_idx] = np.round(x[data.i_idx])
        out[k] = dict(x=x, upper_glob=upper, status=status, nodes=int(info.nodes), osqp_iter=int(info.osqp_iter),
                      run_time=dt / len(todo))
