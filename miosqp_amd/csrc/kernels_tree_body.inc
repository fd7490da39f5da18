// part of kernels_tree.inc (included there INSIDE k_tree, k_tree_m, k_tree_r_m and their forms with round and fix, nowhere
// else): the one body of the kernels.  TREE_LIST_CAP: the leaf list's capacity; TREE_REDUCED (k_tree_r_m): the carve-up, the factor load and the call
// that runs the relaxation are those of the reduced form -- nothing else differs.  TREE_RF (k_tree_rf, k_tree_rf_m,
// k_tree_rf_r_m): round and fix on the nodes that are about to branch (kernels_tree_rf_block.inc) -- nothing else differs.
// TREE_SB (k_tree_sb, k_tree_sb_m, k_tree_sb_r_m): the branching position by strong or reliability branching
// (kernels_tree_sb_block.inc), the pseudo-cost observation of a node's own solve, and what its children remember.
// In scope: `sm` (the dynamic LDS block), `d` (Dev) and `ta` (TreeArgs) with final pointers -- kernel arguments moved to
// the block's instance (k_tree), or references to the block's entry of a table in device memory (k_tree_m).  Everything
// per block -- shapes, the LDS carve-up, sp_off, lane groupings, search settings, tolerances -- is read from them.
  const int n = d.n, M = d.M, p = d.n_int, m0 = d.m_orig, tid = threadIdx.x;
#ifndef TREE_REDUCED
  const bool wform = d.W != nullptr && n + M <= RES_W_MAX;
  const ResCtx c = res_carve(sm, n, M, wform);
  double *xf = c.res + NQ + 8, *xi = xf + n, *prow = xi + n;  // prow: 2 n (objective rows at xf / xi)
  double *yf = prow + 2 * n, *rowbuf = yf + M;                 // rowbuf: M (heuristic margins)
  double *lf_lower = rowbuf + M;                               // TREE_CAP
  int *order = reinterpret_cast<int *>(lf_lower + TREE_CAP);   // the leaf list: slots in list order
  int *lf_depth = order + TREE_CAP;
  int *freelist = lf_depth + TREE_CAP;
  double *sc = reinterpret_cast<double *>(freelist + TREE_CAP);  // scalars shared by the workgroup
  double *fm_v = sc + 16;                                         // best-bound choice: a pair per wavefront
  int *fm_k = reinterpret_cast<int *>(fm_v + RES_WAVES);
  int *iiL = reinterpret_cast<int *>(sc + 32);                    // i_idx (thread 0 walks it for every node)
#else  // k_tree_r_m: the carve-up of tree_reduced_body.hpp -- no product form, the test's scratch shared with the epilogue's
  // vectors, a leaf list of ta.leaf_cap places
  namespace tr = miosqp::tree_reduced;
  const tr::Carve cv = tr::carve(n, M, ta.leaf_cap);
  const tr::State rs = tr::state(sm, n, M, ta.leaf_cap);
  const ResCtx c = res_carve_r(sm, rs, cv);
  double *xf = sm + cv.scr, *xi = xf + n, *prow = xi + n;
  double *yf = prow + 2 * n, *rowbuf = yf + M;
  double *lf_lower = sm + cv.lf_lower;
  int *order = reinterpret_cast<int *>(sm + cv.order);
  int *lf_depth = order + ta.leaf_cap;
  int *freelist = lf_depth + ta.leaf_cap;
  double *sc = sm + cv.sc;
  double *fm_v = sc + 16;
  int *fm_k = reinterpret_cast<int *>(fm_v + RES_WAVES);
  int *iiL = reinterpret_cast<int *>(sm + cv.iiL);
#endif
  // sc[0] upper, sc[1] action, sc[2] slot, sc[3] status, sc[4] lower, sc[5] heur_obj, sc[6] nextvar, sc[7] child0, sc[8] child1
  // (TREE_RF: sc[15] the candidate just judged is the best so far; TREE_SB: sc[15] candidates whose children are solved)
  const double rinv = d.rho_inv, sigma = d.sigma;
  const int unsolved = MIOSQP_QP_UNSOLVED;
  (void)unsolved;

#ifndef TREE_REDUCED
  if (!wform) res_load_factor(d, c);
  const ResSp sp = res_sp_load(d, ta.sp_off >= 0 ? sm + ta.sp_off : nullptr);
#else  // the packed triangle of L^-1 instead of the product form; Abar by variable beside the rows the test walks
  TreeRExec rex;
  tr::load_triangle(rex, rs, d.f_rows, d.ldf, d.d2inv);
  const ResSp sp = res_sp_load(d, ta.sp_off >= 0 ? sm + ta.sp_off : nullptr);
  const tr::Abar ra = tree_r_abar(d, ta, sp, sm);
#endif
  for (int i = tid; i < n; i += RES_THREADS) c.q[i] = d.q[i];
  for (int k = tid; k < p; k += RES_THREADS) iiL[k] = d.i_idx[k];
  // this thread's entries of the vectors every node's prologue and epilogue need (row / variable tid: the sizes that fit
  // the LDS have at most RES_THREADS of either -- the reduced form also takes more rows: the strided loops cover them):
  // read once instead of once per node and loop
  const bool cj = tid < M, ci = tid < n;
  const double E_t = cj ? d.E[tid] : 0.0, Einv_t = cj ? d.Einv[tid] : 0.0, D_t = ci ? d.D[tid] : 0.0,
               Dinv_t = ci ? d.Dinv[tid] : 0.0;
  const double rawl_t = (cj && tid < m0) ? d.raw_l[tid] : 0.0, rawu_t = (cj && tid < m0) ? d.raw_u[tid] : 0.0;
  const int pos_t = ci ? d.int_pos[tid] : -1;
  for (int k = tid; k < TREE_LIST_CAP; k += RES_THREADS) freelist[k] = TREE_LIST_CAP - 1 - k;  // pop hands out slot 0 first
  __syncthreads();
  // the root: slot 0, bounds and warm start from the staging block (raw_l | raw_u | raw_x | raw_y)
  for (int k = tid; k < p; k += RES_THREADS) {
    ta.lf_lo[k] = d.raw_l[m0 + k];
    ta.lf_hi[k] = d.raw_u[m0 + k];
  }
  for (int i = tid; i < n; i += RES_THREADS) ta.lf_x[i] = d.raw_x[i];
  for (int j = tid; j < M; j += RES_THREADS) ta.lf_y[j] = d.raw_y[j];
  int count = 1, nfree = TREE_LIST_CAP - 1, nodes = 0, osqp_iter = 0, max_leaves = 1, overflow = 0, found = 0;
  double lower_glob = -1.0 / 0.0;
#ifdef TREE_RF  // round and fix (kernels_tree_rf_block.inc): nodes that were about to branch, and what rf_stats counts
  int rf_nodes = 0, rf_calls = 0, rf_cand = 0, rf_feas = 0, rf_impr = 0, rf_iter = 0;
#endif
#ifdef TREE_SB  // strong / reliability branching (kernels_tree_sb_block.inc): what sb_stats counts
  int sb_calls = 0, sb_children = 0, sb_iter = 0;
  if (tid == 0) {  // the tree's pseudo-costs start empty, the root was made by no branching
    miosqp::tree_sb::start(miosqp::tree_sb::view(ta.sb_work, p));
    ta.sb_pc[3] = -1.0;
  }
#endif
  if (tid == 0) {
    order[0] = 0;
    lf_depth[0] = 0;
    lf_lower[0] = -1.0 / 0.0;
    sc[0] = ta.upper0;
  }
  __syncthreads();

  unsigned long long tq[4] = {0, 0, 0, 0}, tql = (d.prof && tid == 0) ? wall_clock64() : 0;  // debug: ticks per phase
#define KT_STAMP(k)                                   \
  if (d.prof && tid == 0) {                           \
    const unsigned long long now__ = wall_clock64(); \
    tq[k] += now__ - tql;                             \
    tql = now__;                                      \
  }
  while (count > 0 && nodes + 1 < ta.max_nodes && !overflow) {
    // ---- choose_leaf (workspace.py:128-155): deepest leaf, or -- once an incumbent exists under rule 1 -- the leaf
    //      with the LARGEST bound (sic); first index on ties; the rest of the list keeps its order.  Rule 2, and rule 3
    //      once an incumbent exists: the SMALLEST bound, by all threads (sc[0] was written before the last barrier)
    const bool best_bound = ta.rule == 2 || (ta.rule == 3 && !isinf(sc[0]));
    if (best_bound) {
      double bv;
      int bk;
      first_min_scan<RES_THREADS>(lf_lower, order, count, tid, bv, bk);
      first_min_wave(bv, bk);
      if ((tid & 63) == 0) {
        fm_v[tid >> 6] = bv;
        fm_k[tid >> 6] = bk;
      }
      __syncthreads();
      bv = fm_v[0];
      bk = fm_k[0];
#pragma unroll
      for (int w = 1; w < RES_WAVES; w++) first_min_take(bv, bk, fm_v[w], fm_k[w]);
      const int chosen = order[bk];  // (read by every thread before the barrier inside order_remove, or never overwritten)
      order_remove<RES_THREADS>(order, bk, count, tid);
      if (tid == 0) sc[2] = (double)chosen;
    } else if (tid == 0) {
      const double upper = sc[0];
      const bool by_depth = ta.rule == 0 || isinf(upper);
      int best = 0;
      if (by_depth) {
        int bd = lf_depth[order[0]];
        for (int k = 1; k < count; k++)
          if (lf_depth[order[k]] > bd) { bd = lf_depth[order[k]]; best = k; }
      } else {
        // np.argmax semantics: a NaN would win; bounds are never NaN here
        double bl = lf_lower[order[0]];
        for (int k = 1; k < count; k++)
          if (lf_lower[order[k]] > bl) { bl = lf_lower[order[k]]; best = k; }
      }
      const int slot = order[best];
      for (int k = best; k + 1 < count; k++) order[k] = order[k + 1];
      sc[2] = (double)slot;
    }
    count--;
    __syncthreads();
    const int slot = (int)sc[2];
    const double *lo_n = ta.lf_lo + (size_t)slot * p, *hi_n = ta.lf_hi + (size_t)slot * p;
    // ---- Node.solve prologue (node.py:102-105): scaled bounds, scaled warm start, z = Abar x ----
    for (int j = tid; j < M; j += RES_THREADS) {
      const bool mine = j == tid;
      const double lo = j < m0 ? (mine ? rawl_t : d.raw_l[j]) : lo_n[j - m0],
                   hi = j < m0 ? (mine ? rawu_t : d.raw_u[j]) : hi_n[j - m0];
      const double Ej = mine ? E_t : d.E[j];
      c.l[j] = Ej * fmax(lo, -QP_INFTY);
      c.u[j] = Ej * fmin(hi, QP_INFTY);
      c.y[j] = d.c * (mine ? Einv_t : d.Einv[j]) * ta.lf_y[(size_t)slot * M + j];
      c.dy[j] = 0.0;
    }
    for (int i = tid; i < n; i += RES_THREADS) {
      const double xs = (i == tid ? Dinv_t : d.Dinv[i]) * ta.lf_x[(size_t)slot * n + i];
      c.x[i] = xs;
      c.dx[i] = 0.0;
      c.wr[M + i] = sigma * xs - c.q[i];
    }
    __syncthreads();
    {
      // (TG1 lanes per row as in res_check_rows: one thread per row walked its row's entries -- each a dependent load
      //  from L2 -- one after the other: 10-30 us per product at config 1)
      const int TG = ta.TG1, NG = RES_THREADS / TG, g = tid / TG, t = tid % TG;
      for (int j = g; j < M; j += NG) {
        double acc[1] = {0.0};
        for (int k = sp.Ap[j] + t; k < sp.Ap[j + 1]; k += TG) acc[0] = fma(sp.A[k], c.x[sp.Ai[k]], acc[0]);
        group_reduce<1>(acc, TG);
        if (t == 0) {
          c.z[j] = acc[0];
          c.wr[j] = acc[0] - rinv * c.y[j];
        }
      }
    }
    if (tid == 0) {  // what k_node_pre resets
      Ctrl *cb = d.ctrl;
      cb->done = 0;
      cb->status = MIOSQP_QP_UNSOLVED;
      cb->iter = 0;
    }
    __syncthreads();
    // ---- the relaxation ----
    KT_STAMP(0)
    int it = 0;
#ifndef TREE_REDUCED
    int st = res_admm(d, c, ta.max_iter, ta.check_every, 1, ta.TG1, ta.TG2, &it, sp);
#else
    int st = res_admm_r(d, c, rs, ra, ta.max_iter, ta.check_every, 1, ta.TG1, &it, sp);
#endif
    KT_STAMP(1)
    if (st == 0) st = MIOSQP_QP_MAX_ITER_REACHED;
    nodes++;
    osqp_iter += it;
    const bool ok = st == MIOSQP_QP_SOLVED || st == MIOSQP_QP_MAX_ITER_REACHED;
    // ---- epilogue (node.py:111-143; workspace.py:232-272): unscale, clamp, digest, heuristic, objectives ----
    if (ok) {
      for (int i = tid; i < n; i += RES_THREADS) {
        double v = (i == tid ? D_t : d.D[i]) * c.x[i];
        const int pos = i == tid ? pos_t : d.int_pos[i];
        if (pos >= 0) v = fmin(fmax(v, lo_n[pos]), hi_n[pos]);
        xf[i] = v;
        const double r = pos >= 0 ? rint(v) : v;
        xi[i] = r;
        c.ut[i] = (i == tid ? Dinv_t : d.Dinv[i]) * r;  // the scaled rounded candidate (c.ut is free outside the relaxation)
      }
      for (int j = tid; j < M; j += RES_THREADS) yf[j] = d.cinv * (j == tid ? E_t : d.E[j]) * c.y[j];
      __syncthreads();
      {
        const int TG = ta.TG1, NG = RES_THREADS / TG, g = tid / TG, t = tid % TG;
        for (int j = g; j < M; j += NG) {  // margins of the rounded candidate against the ROOT bounds
          double acc[1] = {0.0};
          const double ej = d.Einv[j], rl = d.root_l[j], ru = d.root_u[j];  // (requested before the row, used after it)
          for (int k = sp.Ap[j] + t; k < sp.Ap[j + 1]; k += TG) acc[0] = fma(sp.A[k], c.ut[sp.Ai[k]], acc[0]);
          group_reduce<1>(acc, TG);
          if (t == 0) {
            const double zz = ej * acc[0];
            rowbuf[j] = fmax(rl - d.eps_lin - zz, zz - ru - d.eps_lin);
          }
        }
        for (int i = g; i < n; i += NG) {  // rows of the unscaled P against x and the rounded candidate
          double acc[2] = {0.0, 0.0};
          const double qi = d.qraw[i];
          for (int k = d.pr_ptr[i] + t; k < d.pr_ptr[i + 1]; k += TG) {
            const double a = d.pr_val[k];
            const int cc = d.pr_idx[k];
            acc[0] = fma(a, xf[cc], acc[0]);
            acc[1] = fma(a, xi[cc], acc[1]);
          }
          group_reduce<2>(acc, TG);
          if (t == 0) {
            prow[i] = xf[i] * (0.5 * acc[0] + qi);
            prow[n + i] = xi[i] * (0.5 * acc[1] + qi);
          }
        }
      }
      __syncthreads();
    }
    KT_STAMP(2)
    // ---- bound_and_branch (workspace.py:282-334) ----
    // the node's sums, worst margin, integrality count and branching variable on the first wavefront (thread 0 walking
    // n + M + p LDS entries one after the other was 9 us of a 100 us node): lane-strided partial results, then a
    // butterfly in a fixed order; the first of the largest fractions wins, as in a loop over k
    double w_lower = 0.0, w_hobj = 0.0, w_hviol = -1.7e308;
    int w_intinf = 0, w_next = -1;
    if (tid < 64 && ok) {
      double a = 0.0, b = 0.0, cmax = -1.7e308, f = -1.0;
      int cnt = 0, kk = 0x7fffffff;
      for (int i = tid; i < n; i += 64) { a += prow[i]; b += prow[n + i]; }
      for (int j = tid; j < M; j += 64) cmax = fmax(cmax, rowbuf[j]);
      for (int k = tid; k < p; k += 64) {
        const double v = xf[iiL[k]], fk = fabs(v - rint(v));
        cnt += fk > d.eps_int;
        if (fk > f) { f = fk; kk = k; }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const double oa = __shfl_xor(a, off, 64), ob = __shfl_xor(b, off, 64), oc = __shfl_xor(cmax, off, 64),
                     of = __shfl_xor(f, off, 64);
        const int ok2 = __shfl_xor(kk, off, 64), ocnt = __shfl_xor(cnt, off, 64);
        a += oa;
        b += ob;
        cmax = fmax(cmax, oc);
        cnt += ocnt;
        if (of > f || (of == f && ok2 < kk)) { f = of; kk = ok2; }
      }
      w_lower = a; w_hobj = b; w_hviol = cmax; w_intinf = cnt; w_next = kk == 0x7fffffff ? -1 : kk;
    }
    if (tid == 0) {
      double upper = sc[0];
      int action = 0;  // 0: nothing, 1: incumbent = x of this node, 2: incumbent = rounded candidate; +4: branch
      double lower = 0.0, hobj = 0.0, hviol = -1.7e308;
      int int_inf = 0, nextvar = -1;
      if (ok) {
        lower = w_lower; hobj = w_hobj; hviol = w_hviol; int_inf = w_intinf; nextvar = w_next;
      }
#ifdef TREE_SB  // Node.pc, read at the top of bound_and_branch: before the infeasible and pruned returns
      miosqp::tree_sb::node_solved(miosqp::tree_sb::view(ta.sb_work, p), ta.sb_pc, slot, ok, lower);
#endif
      bool prune_now = false;
      if (ok && !(lower > upper)) {
        if (int_inf == 0) {
          action = 1;
          upper = lower;
          prune_now = true;
        } else {
          if (hviol <= 0.0 && hobj < upper) {
            action = 2;
            upper = hobj;
            prune_now = true;
          }
          action |= 4;
        }
      }
      if (prune_now) {
        // workspace.py:278-280 removes from the list it iterates: the element behind a removed one is skipped
        int k = 0;
        while (k < count) {
          if (lf_lower[order[k]] > upper) {
            freelist[nfree++] = order[k];
            for (int q = k; q + 1 < count; q++) order[q] = order[q + 1];
            count--;
          }
          k++;
        }
        found = 1;
      }
#ifdef TREE_RF
      // Workspace.primal_heuristic sits here, between the node's own pruning and its branching: thread 0's block is
      // closed around it (the whole workgroup solves the candidates) and opened again with its values
      sc[0] = upper;
      sc[1] = (double)action;
      sc[4] = lower;
      sc[6] = (double)nextvar;
    }
#include "kernels_tree_rf_block.inc"
    if (tid == 0) {
      double upper = sc[0];
      const int action = (int)sc[1] & 4;  // (the block has written the node's own incumbent)
      const double lower = sc[4];
      const int nextvar = (int)sc[6];
#endif
#ifdef TREE_SB
      // Workspace.select_branching sits here, where the node picks its position: thread 0's block is closed around it
      // (the whole workgroup solves the children) and opened again with its values
      sc[0] = upper;
      sc[1] = (double)action;
      sc[4] = lower;
      sc[6] = (double)nextvar;
    }
#include "kernels_tree_sb_block.inc"
    if (tid == 0) {
      double upper = sc[0];
      const int action = (int)sc[1] & 4;  // (the block has written the node's own incumbent)
      const double lower = sc[4];
      const int nextvar = (int)sc[6];
#endif
      int c0 = -1, c1 = -1;
      if (action & 4) {
        if (nfree < 2 || count + 2 > TREE_LIST_CAP) {
          overflow = 1;
        } else {
          c0 = freelist[--nfree];
          c1 = freelist[--nfree];
          const int dep = lf_depth[slot] + 1;
          lf_depth[c0] = lf_depth[c1] = dep;
          lf_lower[c0] = lf_lower[c1] = lower;
          order[count++] = c0;  // add_left, then add_right
          order[count++] = c1;
#ifdef TREE_SB  // branch_children: Node.pc of the two children
          miosqp::tree_sb::branched(miosqp::tree_sb::Par{ta.sb_rule, ta.sb_K, ta.sb_rel, ta.sb_eps, d.eps_int}, ta.sb_pc, c0, c1, nextvar,
                                    xf[iiL[nextvar]], lower);
#endif
          double lg = 1.0 / 0.0;
          for (int k = 0; k < count; k++) lg = fmin(lg, lf_lower[order[k]]);
          sc[9] = lg;
        }
      }
      freelist[nfree++] = slot;  // the node itself is done (its children hold copies of what they need)
      sc[0] = upper;
      sc[1] = (double)action;
      sc[6] = (double)nextvar;
      sc[7] = (double)c0;
      sc[8] = (double)c1;
      sc[10] = (double)count;
      sc[11] = (double)nfree;
      sc[12] = (double)overflow;
      sc[13] = (double)found;
    }
    __syncthreads();
    {
      const int action = (int)sc[1], nextvar = (int)sc[6], c0 = (int)sc[7], c1 = (int)sc[8];
      count = (int)sc[10];
      nfree = (int)sc[11];
      overflow = (int)sc[12];
      found = (int)sc[13];
      if (count > max_leaves) max_leaves = count;
      if ((action & 3) == 1)
        for (int i = tid; i < n; i += RES_THREADS) ta.inc_x[i] = xf[i];
      if ((action & 3) == 2)
        for (int i = tid; i < n; i += RES_THREADS) ta.inc_x[i] = xi[i];
      if ((action & 4) && c0 >= 0) {
        lower_glob = sc[9];
        const double xv = xf[iiL[nextvar]];
        for (int k = tid; k < p; k += RES_THREADS) {
          const double lo = lo_n[k], hi = hi_n[k];
          ta.lf_lo[(size_t)c0 * p + k] = lo;
          ta.lf_hi[(size_t)c0 * p + k] = k == nextvar ? floor(xv) : hi;
          ta.lf_lo[(size_t)c1 * p + k] = k == nextvar ? ceil(xv) : lo;
          ta.lf_hi[(size_t)c1 * p + k] = hi;
        }
        for (int i = tid; i < n; i += RES_THREADS) {
          ta.lf_x[(size_t)c0 * n + i] = xf[i];
          ta.lf_x[(size_t)c1 * n + i] = xf[i];
        }
        for (int j = tid; j < M; j += RES_THREADS) {
          ta.lf_y[(size_t)c0 * M + j] = yf[j];
          ta.lf_y[(size_t)c1 * M + j] = yf[j];
        }
      }
    }
    __threadfence_block();
    __syncthreads();
    KT_STAMP(3)
  }
#undef KT_STAMP
  if (d.prof && tid == 0) {
    for (int k = 0; k < 4; k++) d.prof[8 + k] += tq[k];
  }
  if (tid == 0) {
    TreeOut *o = ta.out;
    o->nodes = nodes;
    o->osqp_iter = osqp_iter;
    o->leaves_left = count;
    o->overflow = overflow;
    o->max_leaves = max_leaves;
    o->found = found;
    o->upper = sc[0];
    o->lower_glob = lower_glob;
#ifdef TREE_RF
    TreeRfOut *r = ta.rf_out;
    r->calls = rf_calls;
    r->candidates = rf_cand;
    r->feasible = rf_feas;
    r->improved = rf_impr;
    r->osqp_iter = rf_iter;
#endif
#ifdef TREE_SB
    TreeSbOut *s = ta.sb_out;
    s->calls = sb_calls;
    s->children = sb_children;
    s->osqp_iter = sb_iter;
#endif
  }
