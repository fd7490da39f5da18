// part of engine.hip (included there, not compiled alone): a whole branch-and-bound tree in ONE launch (small problems)
// ------------------------------------------------------------------------------------------
// SURVEY sec. 8f rank 2: the MPC re-solve path (BASELINE configs[3]: power converter, n = 18, 45 rows, ~12 nodes
// of ~50 iterations per MIQP, thousands of MIQPs in sequence).  With the LDS-resident solver a node costs ~0.1 ms
// on the device and as much again in host round trips (ctypes call, six launches, two copies, the wait).  Here the
// whole tree search of /root/reference/miosqp/solver.py:85-123 runs inside one launch of one workgroup: the factor
// and the iterates live in LDS as in k_resident, the leaf list lives in LDS / global memory, and thread 0 takes
// the decisions of Workspace.choose_leaf / bound_and_branch / prune (workspace.py:128-155, 274-334) exactly as
// miosqp_amd/bnb.py takes them on the host -- same order, same strict comparisons, same list semantics
// (argmax = first maximum; pop keeps the order of the rest; prune skips the element behind a removed one).
// The host sends the root and receives (incumbent x, upper bound, node and iteration counts).
// ------------------------------------------------------------------------------------------
constexpr int TREE_CAP = 1024;  // leaves alive at once (the list is checked for overflow; the host falls back)

struct TreeOut {
  int nodes, osqp_iter, leaves_left, overflow;
  int max_leaves, found, pad0, pad1;
  double upper, lower_glob;
};

struct TreeArgs {
  int rule, max_nodes, max_iter, check_every, TG1, TG2;
  double upper0;
  double *lf_lo, *lf_hi;  // [TREE_CAP][n_int] integer-row bounds (unscaled)
  double *lf_x, *lf_y;    // [TREE_CAP][n], [TREE_CAP][M] warm starts (unscaled)
  double *inc_x;          // [n] incumbent: in (when upper0 is finite), out
  TreeOut *out;
  // k_tree_w with its inputs and outputs in host memory (no copies around the launch): done[0] = 1 (release, system
  // scope) after everything else has been written, done[1], done[2] = 100 MHz ticks at kernel start / end; or nullptr
  unsigned long long *done;
  int sp_off;  // k_tree: offset (doubles) of the LDS copy of the sparse Abar / Pbar rows inside the dynamic block, or -1
  // miosqp_qp_solve_trees: workgroup b runs MIQP b of a batch that shares P, A (the factor) and differs in q, l, u, warm
  // start and incumbent -- every per-instance array holds `batch` instances back to back; upper_b[b]: its incumbent value
  int batch;
  const double *upper_b;
};

// workgroup b of a batched launch: the per-instance pointers of Dev and TreeArgs moved to instance b (the staging block
// raw_l | raw_u | raw_x | raw_y holds 3 M + n doubles per instance; the root bounds of an instance are its l, u)
__device__ __forceinline__ void tree_instance(Dev &d, TreeArgs &ta) {
  if (!ta.batch) return;
  const size_t b = blockIdx.x, n = d.n, M = d.M, p = d.n_int, blk = 3 * M + n;
  d.q += b * n;
  d.qraw += b * n;
  d.raw_l += b * blk;
  d.raw_u += b * blk;
  d.raw_x += b * blk;
  d.raw_y += b * blk;
  d.root_l = d.raw_l;
  d.root_u = d.raw_u;
  ta.lf_lo += b * TREE_CAP * p;
  ta.lf_hi += b * TREE_CAP * p;
  ta.lf_x += b * TREE_CAP * n;
  ta.lf_y += b * TREE_CAP * M;
  ta.inc_x += b * n;
  ta.out += b;
  ta.upper0 = ta.upper_b[b];
}

__host__ __device__ inline size_t tree_lds_doubles(int n, int M, bool wform) {
  // resident arrays + epilogue vectors (xf, xi: n; yf, rowbuf: M; prow: 2 n) + list (lower: CAP doubles; order, depth,
  // freelist: 3 CAP ints = 1.5 CAP doubles) + a few scalars
  // (+ 16: the per-wavefront (value, position) pairs of the best-bound choice, first_min_wave)
  return resident_lds_doubles(n, M, wform) + 4 * (size_t)n + 2 * (size_t)M + (size_t)TREE_CAP * 5 / 2 + 16 + 16 + ((size_t)n + 1) / 2 + 1;
}

// ------------------------------------------------------------------------------------------
// The best-bound choice (tree_explor_rule 2, and 3 once an incumbent exists): the open leaf with the SMALLEST inherited
// bound, the FIRST one in list order on ties (np.argmin; two siblings share their parent's bound, so ties are the
// normal case and the tie rule decides the tree).  Under best bound the list is several times as long as under depth
// first (up to TREE_CAP), and one thread walking it sits between every two nodes.  Every thread takes the positions
// k = tid, tid + T, ... and keeps the pair (lf_lower[order[k]], k); pairs are reduced with "smaller value wins; on equal
// values the smaller k wins", a total order, so the result is the same whatever the order of the reduction.
// ------------------------------------------------------------------------------------------
constexpr int TREE_NO_POS = 0x7fffffff;

__device__ __forceinline__ void first_min_take(double &v, int &k, double ov, int ok) {
  if (ov < v || (ov == v && ok < k)) { v = ov; k = ok; }
}

// this thread's pair over its positions of the list (ascending k: the strict comparison keeps the first)
template <int T>
__device__ __forceinline__ void first_min_scan(const double *lf_lower, const int *order, int count, int tid, double &v, int &k) {
  v = 1.0 / 0.0;
  k = TREE_NO_POS;
  for (int q = tid; q < count; q += T) {
    const double lv = lf_lower[order[q]];
    if (lv < v || k == TREE_NO_POS) { v = lv; k = q; }
  }
}

// across the wavefront: a butterfly, every lane ends with the winning pair
__device__ __forceinline__ void first_min_wave(double &v, int &k) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double ov = __shfl_xor(v, off, 64);
    const int ok = __shfl_xor(k, off, 64);
    first_min_take(v, k, ov, ok);
  }
}

// order[best] leaves the list and the tail moves down by one, T positions at a time: every thread reads its element,
// a barrier, every thread writes it one position lower (a round reads [base + 1, base + T] and writes [base, base + T):
// nothing a later round reads).  Called by all T threads of the workgroup with the same best and count.
template <int T>
__device__ __forceinline__ void order_remove(int *order, int best, int count, int tid) {
  for (int base = best; base + 1 < count; base += T) {
    const int src = base + 1 + tid;
    const int moved = src < count ? order[src] : 0;
    __syncthreads();
    if (src < count) order[src - 1] = moved;
  }
}

__global__ __launch_bounds__(RES_THREADS) void k_tree(Dev d, TreeArgs ta) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  tree_instance(d, ta);
  const int n = d.n, M = d.M, p = d.n_int, m0 = d.m_orig, tid = threadIdx.x;
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
  // sc[0] upper, sc[1] action, sc[2] slot, sc[3] status, sc[4] lower, sc[5] heur_obj, sc[6] nextvar, sc[7] child0, sc[8] child1
  const double rinv = d.rho_inv, sigma = d.sigma;
  const int unsolved = MIOSQP_QP_UNSOLVED;
  (void)unsolved;

  if (!wform) res_load_factor(d, c);
  const ResSp sp = res_sp_load(d, ta.sp_off >= 0 ? sm + ta.sp_off : nullptr);
  for (int i = tid; i < n; i += RES_THREADS) c.q[i] = d.q[i];
  for (int k = tid; k < p; k += RES_THREADS) iiL[k] = d.i_idx[k];
  // this thread's entries of the vectors every node's prologue and epilogue need (row / variable tid: the sizes that fit
  // the LDS have at most RES_THREADS of either): read once instead of once per node and loop
  const bool cj = tid < M, ci = tid < n;
  const double E_t = cj ? d.E[tid] : 0.0, Einv_t = cj ? d.Einv[tid] : 0.0, D_t = ci ? d.D[tid] : 0.0,
               Dinv_t = ci ? d.Dinv[tid] : 0.0;
  const double rawl_t = (cj && tid < m0) ? d.raw_l[tid] : 0.0, rawu_t = (cj && tid < m0) ? d.raw_u[tid] : 0.0;
  const int pos_t = ci ? d.int_pos[tid] : -1;
  for (int k = tid; k < TREE_CAP; k += RES_THREADS) freelist[k] = TREE_CAP - 1 - k;  // pop hands out slot 0 first
  __syncthreads();
  // the root: slot 0, bounds and warm start from the staging block (raw_l | raw_u | raw_x | raw_y)
  for (int k = tid; k < p; k += RES_THREADS) {
    ta.lf_lo[k] = d.raw_l[m0 + k];
    ta.lf_hi[k] = d.raw_u[m0 + k];
  }
  for (int i = tid; i < n; i += RES_THREADS) ta.lf_x[i] = d.raw_x[i];
  for (int j = tid; j < M; j += RES_THREADS) ta.lf_y[j] = d.raw_y[j];
  int count = 1, nfree = TREE_CAP - 1, nodes = 0, osqp_iter = 0, max_leaves = 1, overflow = 0, found = 0;
  double lower_glob = -1.0 / 0.0;
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
    int st = res_admm(d, c, ta.max_iter, ta.check_every, 1, ta.TG1, ta.TG2, &it, sp);
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
      int c0 = -1, c1 = -1;
      if (action & 4) {
        if (nfree < 2 || count + 2 > TREE_CAP) {
          overflow = 1;
        } else {
          c0 = freelist[--nfree];
          c1 = freelist[--nfree];
          const int dep = lf_depth[slot] + 1;
          lf_depth[c0] = lf_depth[c1] = dep;
          lf_lower[c0] = lf_lower[c1] = lower;
          order[count++] = c0;  // add_left, then add_right
          order[count++] = c1;
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
  }
}

// ------------------------------------------------------------------------------------------
// The same tree search for n + M <= 64 in ONE WAVEFRONT (BASELINE configs[3]: n + M = 63).  k_tree's iteration costs
// ~5000 cycles at this size: eight waves, two barriers and two LDS round trips for two 63-wide sweeps.  Here lane r
// owns row r of the explicit KKT inverse W (the matrix k_coop spreads over the chip: [nu + rho wh ; x~] = W [wh ; rx],
// dense_setup.hip) in 64 register pairs and the iterates of that row; an iteration is ONE matrix-vector product whose
// right-hand side is read from LDS as broadcasts (every lane reads the same address), then purely lane-local
// updates and one LDS store per lane -- no barrier anywhere (a single wavefront runs in lock step and its LDS
// operations complete in order).  The termination test applies lane r's row of Kc = [0 Abar ; Abar^T Pbar] (kept
// in LDS, 32 KB) to [y ; x] and [proj(dy) ; dx] and reduces the 17 norms / sums with a butterfly.
// Decisions, list semantics and results are those of k_tree; only the summation order inside a node differs.
// ------------------------------------------------------------------------------------------
constexpr int TW = 64;

__device__ __forceinline__ double wave_max64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ double wave_sum64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// y[q] of lane l = x of lane 16 q + l % 16: the four rows of 16 lanes copied to every row, without the LDS crossbar
// (permlane16_swap exchanges the odd rows of its first operand with the even rows of its second, permlane32_swap the
// upper half of the first with the lower half of the second; with both operands equal that duplicates rows / halves)
__device__ __forceinline__ void row_replicate(double x, double (&y)[4]) {
  const unsigned lo = (unsigned)__double2loint(x), hi = (unsigned)__double2hiint(x);
  const auto l16 = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);  // [0] = rows 0 0 2 2, [1] = rows 1 1 3 3
  const auto h16 = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  const auto le = __builtin_amdgcn_permlane32_swap(l16[0], l16[0], false, false);  // [0] = row 0 everywhere, [1] = row 2
  const auto he = __builtin_amdgcn_permlane32_swap(h16[0], h16[0], false, false);
  const auto lod = __builtin_amdgcn_permlane32_swap(l16[1], l16[1], false, false);  // [0] = row 1 everywhere, [1] = row 3
  const auto hod = __builtin_amdgcn_permlane32_swap(h16[1], h16[1], false, false);
  y[0] = __hiloint2double((int)he[0], (int)le[0]);
  y[1] = __hiloint2double((int)hod[0], (int)lod[0]);
  y[2] = __hiloint2double((int)he[1], (int)le[1]);
  y[3] = __hiloint2double((int)hod[1], (int)lod[1]);
}

// acc[v] += sum_c mat[c][r] * x_v[c], c = 0..63 in order, where lane c holds x_v[c] in own[v]: lane r's column of a
// 64 x 64 matrix in LDS against NV vectors that live one entry per lane.  The vectors are copied across the four rows
// of 16 lanes once (xr[v][q] of lane l = own[v] of lane 16 q + l % 16), the matrix entries come 16 at a time from LDS
// (one read per lane, conflict-free), and product c = 16 q + j takes its vector operand from lane j of the row through
// the DPP row broadcast of the FMA.  (A plain loop over LDS paid a round trip per column: 4 us per termination test.)
template <int NV>
__device__ __forceinline__ void lds_col_dot(const double *mat, int r, const double (&own)[NV], double (&acc)[NV]) {
  double xr[NV][4];
#pragma unroll
  for (int v = 0; v < NV; v++) row_replicate(own[v], xr[v]);
  asm volatile("s_nop 1");
#define CD_F(Q, J)                                                                                                   \
  _Pragma("unroll") for (int v = 0; v < NV; v++)                                                                     \
      asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:" #J " row_mask:0xf bank_mask:0xf" : "+v"(acc[v]) : "v"(xr[v][Q]), "v"(a[J]));
#define CD_ROW(Q)                                                                      \
  {                                                                                    \
    double a[16];                                                                      \
    _Pragma("unroll") for (int j = 0; j < 16; j++) a[j] = mat[(16 * (Q) + j) * TW + r]; \
    __builtin_amdgcn_sched_barrier(0);                                                 \
    CD_F(Q, 0) CD_F(Q, 1) CD_F(Q, 2) CD_F(Q, 3) CD_F(Q, 4) CD_F(Q, 5) CD_F(Q, 6) CD_F(Q, 7) CD_F(Q, 8) CD_F(Q, 9)       \
    CD_F(Q, 10) CD_F(Q, 11) CD_F(Q, 12) CD_F(Q, 13) CD_F(Q, 14) CD_F(Q, 15)             \
    __builtin_amdgcn_sched_barrier(0);                                                 \
  }
  CD_ROW(0) CD_ROW(1) CD_ROW(2) CD_ROW(3)
#undef CD_ROW
#undef CD_F
}

__global__ __launch_bounds__(64) void k_tree_w(Dev d, TreeArgs ta) {
  __shared__ __attribute__((aligned(16))) double xfL[TW], xiL[TW], yfL[TW];
  __shared__ double KcL[TW * TW];
  __shared__ double PrL[TW * TW];  // unscaled P, dense, indexed by lanes: element (M + j, M + i) = P_ij
  __shared__ int iiL[TW];          // i_idx
  __shared__ double lf_lower[TREE_CAP];
  __shared__ int order[TREE_CAP], lf_depth[TREE_CAP], freelist[TREE_CAP];
  __shared__ double sc[16];
  tree_instance(d, ta);
  const int n = d.n, M = d.M, N = n + M, p = d.n_int, m0 = d.m_orig;
  const int r = threadIdx.x;
  const unsigned long long t_begin = ta.done ? wall_clock64() : 0ull;
  const bool own = r < N, con = r < M;
  const int vi = r - M;  // variable index of a variable lane
  const double rho = d.rho, rinv = d.rho_inv, alpha = d.alpha, sigma = d.sigma;

  // ---- one-time loads: this lane's row of W, Kc into LDS, the row's scalings ----
  // (unconditional loads from clamped rows -- both buffers end with 64 entries of slack -- and a select afterwards: all
  //  64 requests of a row are in flight together; Kc first, while the registers of the row of W are still free)
  const size_t rowoff = (size_t)(own ? r : 0) * d.ldw;
  {
    double kc[TW];
#pragma unroll
    for (int c = 0; c < TW; c++) kc[c] = d.Kc[rowoff + c];
#pragma unroll
    for (int c = 0; c < TW; c++) KcL[c * TW + r] = (own && c < N) ? kc[c] : 0.0;  // symmetric
  }
  double Wr[TW];
#pragma unroll
  for (int k = 0; k < TW; k++) Wr[k] = d.W[rowoff + k];
#pragma unroll
  for (int k = 0; k < TW; k++) Wr[k] = (own && k < N) ? Wr[k] : 0.0;
  for (int c = 0; c < TW; c++) PrL[c * TW + r] = 0.0;
  xfL[r] = xiL[r] = yfL[r] = 0.0;
  iiL[r] = r < d.n_int ? d.i_idx[r] : 0;
  if (own && !con) {  // this lane's row of P (row-compressed in memory), sixteen entries requested at a time
    const int pb = d.pr_ptr[r - d.M], pe = d.pr_ptr[r - d.M + 1];
    for (int k = pb; k < pe; k += 16) {
      double pv[16];
      int pj[16];
#pragma unroll
      for (int j = 0; j < 16; j++) {
        const int kk = k + j < pe ? k + j : pe - 1;
        pv[j] = d.pr_val[kk];
        pj[j] = d.pr_idx[kk];
      }
#pragma unroll
      for (int j = 0; j < 16; j++)
        // (column = the lane that owns variable pj; rows are padded to even length with a zero that REPEATS a column
        //  index: a zero must not overwrite the entry it repeats)
        if (k + j < pe && pv[j] != 0.0) PrL[(M + pj[j]) * TW + r] = pv[j];
    }
  }
  const double sc_dir = own ? (con ? d.E[r] : d.D[vi]) : 0.0, sc_inv = own ? (con ? d.Einv[r] : d.Dinv[vi]) : 0.0;
  const double qbar = (own && !con) ? d.q[vi] : 0.0, qraw = (own && !con) ? d.qraw[vi] : 0.0;
  const double rootl = con ? d.root_l[r] : 0.0, rootu = con ? d.root_u[r] : 0.0;
  const double gl = (con && r < m0) ? d.raw_l[r] : 0.0, gu = (con && r < m0) ? d.raw_u[r] : 0.0;  // general rows: the root's
  const int ipos = (own && !con) ? d.int_pos[vi] : -1;
  for (int k = r; k < TREE_CAP; k += TW) freelist[k] = TREE_CAP - 1 - k;
  // root -> slot 0
  if (r < p) {
    ta.lf_lo[r] = d.raw_l[m0 + r];
    ta.lf_hi[r] = d.raw_u[m0 + r];
  }
  if (r < n) ta.lf_x[r] = d.raw_x[r];
  if (r < M) ta.lf_y[r] = d.raw_y[r];
  int count = 1, nfree = TREE_CAP - 1, nodes = 0, osqp_iter = 0, max_leaves = 1, overflow = 0, found = 0;
  double lower_glob = -1.0 / 0.0;
  if (r == 0) {
    order[0] = 0;
    lf_depth[0] = 0;
    lf_lower[0] = -1.0 / 0.0;
    sc[0] = ta.upper0;
  }
  __syncthreads();

  unsigned long long tp[6] = {0, 0, 0, 0, 0, 0}, tl = d.prof ? wall_clock64() : 0;  // debug: 100 MHz ticks per phase
#define TW_STAMP(k)                                   \
  if (d.prof) {                                       \
    const unsigned long long now__ = wall_clock64(); \
    tp[k] += now__ - tl;                              \
    tl = now__;                                       \
  }
  while (count > 0 && nodes + 1 < ta.max_nodes && !overflow) {
    // ---- choose_leaf (as k_tree; the best-bound choice inside the one wavefront) ----
    const bool best_bound = ta.rule == 2 || (ta.rule == 3 && !isinf(sc[0]));
    if (best_bound) {
      double bv;
      int bk;
      first_min_scan<TW>(lf_lower, order, count, r, bv, bk);
      first_min_wave(bv, bk);
      const int chosen = order[bk];
      order_remove<TW>(order, bk, count, r);
      if (r == 0) sc[2] = (double)chosen;
    } else if (r == 0) {
      const double upper = sc[0];
      const bool by_depth = ta.rule == 0 || isinf(upper);
      int best = 0;
      if (by_depth) {
        int bd = lf_depth[order[0]];
        for (int k = 1; k < count; k++)
          if (lf_depth[order[k]] > bd) { bd = lf_depth[order[k]]; best = k; }
      } else {
        double bl = lf_lower[order[0]];
        for (int k = 1; k < count; k++)
          if (lf_lower[order[k]] > bl) { bl = lf_lower[order[k]]; best = k; }
      }
      const int sl = order[best];
      for (int k = best; k + 1 < count; k++) order[k] = order[k + 1];
      sc[2] = (double)sl;
    }
    count--;
    __syncthreads();
    const int slot = (int)sc[2];
    const double *lo_n = ta.lf_lo + (size_t)slot * p, *hi_n = ta.lf_hi + (size_t)slot * p;
    // ---- prologue: scaled bounds, scaled warm start, z = Abar x ----
    double lo = 0.0, up = 0.0, sa = 0.0, sb = 0.0, sw = 0.0, delta = 0.0;
    double clo = 0.0, chi = 0.0;  // a variable lane: its integer bounds (clamp of node.py:131-136)
    if (con) {
      const double rl = r < m0 ? gl : lo_n[r - m0], ru = r < m0 ? gu : hi_n[r - m0];
      lo = sc_dir * fmax(rl, -QP_INFTY);
      up = sc_dir * fmin(ru, QP_INFTY);
      sb = d.c * sc_inv * ta.lf_y[(size_t)slot * M + r];
    } else if (own) {
      sa = sc_inv * ta.lf_x[(size_t)slot * n + vi];
      sb = qbar;
      if (ipos >= 0) { clo = lo_n[ipos]; chi = hi_n[ipos]; }
    }
    {
      // z = Abar x: the vector is zero outside the variable lanes, so the sum over all 64 columns is the sum over
      // c = M .. N-1
      const double vx[1] = {(own && !con) ? sa : 0.0};  // scaled x, by variable lane
      double zz[1] = {0.0};
      lds_col_dot<1>(KcL, r, vx, zz);
      if (con) {
        sa = zz[0];
        sw = zz[0] - rinv * sb;
      }
    }
    double ucur = own ? (con ? sw : sigma * sa - sb) : 0.0;  // this lane's entry of the right-hand side [wh ; rx]
    TW_STAMP(0)
    // ---- ADMM ----
    int it = 0, st = 0;
    int to_test = ta.check_every > 0 ? ta.check_every : -1;
    for (it = 1; it <= ta.max_iter; it++) {
      // The right-hand side is broadcast inside the registers: ur[q] of lane l holds u of lane 16 q + l % 16 (four
      // cross-row copies of this lane's entry), and product k = 16 q + j takes its operand from lane j of the row
      // through the DPP row broadcast of the FMA itself.  (Through LDS -- 32 broadcast reads of 16 bytes -- an iteration
      // was bound by the LDS read path: 1100 cycles.)  Accumulation order: k ascending, accumulator k % 4, as before.
      double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
      {
        double ur[4];
        row_replicate(ucur, ur);
        asm volatile("s_nop 1");
#define TW_F(ACC, Q, J) \
  asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:" #J " row_mask:0xf bank_mask:0xf" : "+v"(ACC) : "v"(ur[Q]), "v"(Wr[16 * (Q) + (J)]));
#define TW_ROW(Q)                                                                                             \
  TW_F(s0, Q, 0) TW_F(s1, Q, 1) TW_F(s2, Q, 2) TW_F(s3, Q, 3) TW_F(s0, Q, 4) TW_F(s1, Q, 5) TW_F(s2, Q, 6) TW_F(s3, Q, 7) \
  TW_F(s0, Q, 8) TW_F(s1, Q, 9) TW_F(s2, Q, 10) TW_F(s3, Q, 11) TW_F(s0, Q, 12) TW_F(s1, Q, 13) TW_F(s2, Q, 14) TW_F(s3, Q, 15)
        TW_ROW(0) TW_ROW(1) TW_ROW(2) TW_ROW(3)
#undef TW_ROW
#undef TW_F
      }
      const double s = (s0 + s1) + (s2 + s3);
      double pub = 0.0;
      if (con) {
        const double zt = sa + rinv * ((s - rho * sw) - sb);
        const double zr = alpha * zt + (1.0 - alpha) * sa;
        const double vv = zr + rinv * sb;
        const double zn = fmin(fmax(vv, lo), up);
        pub = 2.0 * zn - vv;
        delta = rho * (zr - zn);
        sa = zn;
        sb += delta;
        sw = pub;
      } else if (own) {
        const double xn = alpha * s + (1.0 - alpha) * sa;
        pub = sigma * xn - sb;
        delta = xn - sa;
        sa = xn;
      }
      ucur = pub;
      bool chk = it == ta.max_iter;
      if (--to_test == 0) {
        chk = true;
        to_test = ta.check_every;
      }
      if (!chk) continue;
      TW_STAMP(1)
      // ---- termination test (OSQP paper sec. 3.4), as coop_test ----
      double vproj = 0.0;
      if (con) {
        const bool uinf = up > QP_INFTY * QP_MIN_SCALING, linf = lo < -QP_INFTY * QP_MIN_SCALING;
        vproj = delta;
        if (uinf && linf) vproj = 0.0;
        else if (uinf) vproj = fmin(vproj, 0.0);
        else if (linf) vproj = fmax(vproj, 0.0);
      }
      // [y ; x] and [proj(dy) ; dx], each as a constraint part (zero on the variable lanes) and a variable part: the
      // four sums over all 64 columns are then the sums over c < M and over c >= M of the plain loops, term for term
      double sA1, sA2, sP1, sP2;
      {
        const double vv4[4] = {con ? sb : 0.0, con ? vproj : 0.0, (own && !con) ? sa : 0.0, (own && !con) ? delta : 0.0};
        double acc4[4] = {0.0, 0.0, 0.0, 0.0};
        lds_col_dot<4>(KcL, r, vv4, acc4);
        sA1 = acc4[0];
        sA2 = acc4[1];
        sP1 = acc4[2];
        sP2 = acc4[3];
      }
      double v[NQ];
#pragma unroll
      for (int k = 0; k < NQ; k++) v[k] = (k == 4 || k == 5) ? -1.7e308 : 0.0;
      if (con) {
        const double ei = sc_inv;
        const bool uinf = up > QP_INFTY * QP_MIN_SCALING, linf = lo < -QP_INFTY * QP_MIN_SCALING;
        const double adx = ei * sP2;
        v[0] = fabs(ei * (sP1 - sa));
        v[1] = fabs(ei * sP1);
        v[2] = fabs(ei * sa);
        v[3] = fabs(sc_dir * vproj);
        v[4] = uinf ? -1.7e308 : adx;
        v[5] = -(linf ? 1.7e308 : adx);
        v[13] = up * fmax(vproj, 0.0) + lo * fmin(vproj, 0.0);
      } else if (own) {
        const double di = sc_inv, px = sP1, aty = sA1;
        v[6] = fabs(di * (px + sb + aty));
        v[7] = fabs(di * px);
        v[8] = fabs(di * aty);
        v[9] = fabs(di * sb);
        v[10] = fabs(di * sP2);
        v[11] = fabs(di * sA2);
        v[12] = fabs(sc_dir * delta);
        v[14] = sb * delta;
        v[15] = sa * px;
        v[16] = sb * sa;
      }
      {
        // the thirteen maxima through DPP / permlane swaps (exact in any order); the four sums with the shuffles of
        // wave_sum64, all four in flight per step (one after the other they were 17 x 6 dependent LDS-crossbar round
        // trips: 4 us of a 5 us test)
        double vm[NQ_MAX];
#pragma unroll
        for (int k = 0; k < NQ_MAX; k++) vm[k] = v[k];
        group_max<NQ_MAX>(vm, 64);
#pragma unroll
        for (int k = 0; k < NQ_MAX; k++) v[k] = vm[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          double o4[NQ - NQ_MAX];
#pragma unroll
          for (int k = NQ_MAX; k < NQ; k++) o4[k - NQ_MAX] = __shfl_xor(v[k], off, 64);
#pragma unroll
          for (int k = NQ_MAX; k < NQ; k++) v[k] += o4[k - NQ_MAX];
        }
      }
      Norms nm{v[0], v[1], v[2], v[3], v[4], -v[5], v[6] * d.cinv, v[7], v[8], v[9], v[10], v[11], v[12], v[13], v[14],
               v[15], v[16]};
      double obj;
      st = decide_status(d, nm, obj);
      TW_STAMP(2)
      if (st) break;
    }
    if (it > ta.max_iter) it = ta.max_iter;
    if (st == 0) st = MIOSQP_QP_MAX_ITER_REACHED;
    nodes++;
    osqp_iter += it;
    const bool ok = st == MIOSQP_QP_SOLVED || st == MIOSQP_QP_MAX_ITER_REACHED;
    // ---- epilogue ----
    double lower = 0.0, hobj = 0.0, hviol = -1.7e308;
    int int_inf = 0, nextvar = -1;
    if (ok) {
      double xf = 0.0, xi = 0.0;
      if (own && !con) {
        xf = sc_dir * sa;
        if (ipos >= 0) xf = fmin(fmax(xf, clo), chi);
        xi = ipos >= 0 ? rint(xf) : xf;
        xfL[vi] = xf;
        xiL[vi] = xi;
      }
      if (con) yfL[r] = d.cinv * sc_dir * sb;
      __syncthreads();
      double margin = -1.7e308;
      {
        const double vx[1] = {(own && !con) ? sc_inv * xi : 0.0};  // scaled rounded candidate, by variable lane
        double aa[1] = {0.0};
        lds_col_dot<1>(KcL, r, vx, aa);
        if (con) {
          const double zz = sc_inv * aa[0];
          margin = fmax(rootl - d.eps_lin - zz, zz - rootu - d.eps_lin);
        }
      }
      double t1 = 0.0, t2 = 0.0;
      {
        const double vo[2] = {(own && !con) ? xf : 0.0, (own && !con) ? xi : 0.0};
        double ab[2] = {0.0, 0.0};
        lds_col_dot<2>(PrL, r, vo, ab);  // (entries in column order: the order of the compressed row; the rest is zero)
        if (own && !con) {
          t1 = xf * (0.5 * ab[0] + qraw);
          t2 = xi * (0.5 * ab[1] + qraw);
        }
      }
      {
        double mm[1] = {margin};
        group_max<1>(mm, 64);
        hviol = mm[0];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {  // (wave_sum64's order, both sums in flight)
          const double o1 = __shfl_xor(t1, off, 64), o2 = __shfl_xor(t2, off, 64);
          t1 += o1;
          t2 += o2;
        }
        lower = t1;
        hobj = t2;
      }
      // is_int_feas + pick_nextvar: lane k looks at integer variable k; the first of the largest fractions wins
      {
        double f = -1.0;
        int cnt = 0, kk = 0x7fffffff;
        if (r < p) {
          const double vv = xfL[iiL[r]];
          f = fabs(vv - rint(vv));
          cnt = f > d.eps_int;
          kk = r;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const double of = __shfl_xor(f, off, 64);
          const int ok2 = __shfl_xor(kk, off, 64);
          cnt += __shfl_xor(cnt, off, 64);
          if (of > f || (of == f && ok2 < kk)) { f = of; kk = ok2; }
        }
        int_inf = cnt;
        nextvar = kk == 0x7fffffff ? -1 : kk;
      }
    }
    TW_STAMP(3)
    // ---- bound_and_branch ----
    if (r == 0) {
      double upper = sc[0];
      int action = 0;
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
      int c0 = -1, c1 = -1;
      if (action & 4) {
        if (nfree < 2 || count + 2 > TREE_CAP) {
          overflow = 1;
        } else {
          c0 = freelist[--nfree];
          c1 = freelist[--nfree];
          const int dep = lf_depth[slot] + 1;
          lf_depth[c0] = lf_depth[c1] = dep;
          lf_lower[c0] = lf_lower[c1] = lower;
          order[count++] = c0;
          order[count++] = c1;
          double lg = 1.0 / 0.0;
          for (int k = 0; k < count; k++) lg = fmin(lg, lf_lower[order[k]]);
          sc[9] = lg;
        }
      }
      freelist[nfree++] = slot;
      sc[0] = upper;
      sc[1] = (double)action;
      sc[7] = (double)c0;
      sc[8] = (double)c1;
      sc[10] = (double)count;
      sc[11] = (double)nfree;
      sc[12] = (double)overflow;
      sc[13] = (double)found;
    }
    __syncthreads();
    {
      const int action = (int)sc[1], c0 = (int)sc[7], c1 = (int)sc[8];
      count = (int)sc[10];
      nfree = (int)sc[11];
      overflow = (int)sc[12];
      found = (int)sc[13];
      if (count > max_leaves) max_leaves = count;
      if ((action & 3) == 1 && r < n) ta.inc_x[r] = xfL[r];
      if ((action & 3) == 2 && r < n) ta.inc_x[r] = xiL[r];
      if ((action & 4) && c0 >= 0) {
        lower_glob = sc[9];
        const double xv = xfL[iiL[nextvar]];
        if (r < p) {
          const double l0 = lo_n[r], h0 = hi_n[r];
          ta.lf_lo[(size_t)c0 * p + r] = l0;
          ta.lf_hi[(size_t)c0 * p + r] = r == nextvar ? floor(xv) : h0;
          ta.lf_lo[(size_t)c1 * p + r] = r == nextvar ? ceil(xv) : l0;
          ta.lf_hi[(size_t)c1 * p + r] = h0;
        }
        if (r < n) {
          ta.lf_x[(size_t)c0 * n + r] = xfL[r];
          ta.lf_x[(size_t)c1 * n + r] = xfL[r];
        }
        if (r < M) {
          ta.lf_y[(size_t)c0 * M + r] = yfL[r];
          ta.lf_y[(size_t)c1 * M + r] = yfL[r];
        }
      }
    }
    __threadfence_block();
    __syncthreads();
    TW_STAMP(4)
  }
#undef TW_STAMP
  if (d.prof && r == 0) {
    for (int k = 0; k < 6; k++) d.prof[k] += tp[k];
  }
  if (r == 0) {
    TreeOut *o = ta.out;
    o->nodes = nodes;
    o->osqp_iter = osqp_iter;
    o->leaves_left = count;
    o->overflow = overflow;
    o->max_leaves = max_leaves;
    o->found = found;
    o->upper = sc[0];
    o->lower_glob = lower_glob;
  }
  if (ta.done) {
    __threadfence_system();  // this wave's stores (incumbent, outcome) have reached host memory
    if (r == 0) {
      ta.done[1] = t_begin;
      ta.done[2] = wall_clock64();
      __hip_atomic_store(&ta.done[0], 1ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}
