// part of engine.hip (included there, not compiled alone): polishing of one node's solution (miosqp_qp_polish) -- the
// active set guessed from (x, y), the delta-regularised KKT system on it reduced to S = P + delta I + A_act^T A_act / delta,
// factorised by the set-up's blocked LDL^T (dense_setup.hip), solved and refined against the UNregularised system, and
// the acceptance test.  Everything here works on the UNSCALED problem: P (pr_*), q (qraw) and the values of A as they
// were given at set-up, laid out like the scaled rows (pc_* by constraint, pv_* by variable; pads are zeros).  Plain
// fp64; every sum has a fixed order (lanes stride a row, partial sums meet in an xor butterfly), the two counters are
// integer atomics: two identical calls give identical bits.
//
// The repair loop (miosqp_qp_polish_repair) goes round steps 2-3: after a round's solves k_pol_revise classifies every
// row again from the polished point (rows it violates join the set, rows whose multiplier has the wrong sign leave it),
// the host reads the four counters and either queues the next round on the revised set or goes on to the acceptance.
constexpr double POL_TOL = 1e-10;  // the revision's tolerance: the floor of the acceptance test
constexpr int POL_MAX_ROUNDS = 21;  // round 0 and at most 20 repair rounds
struct PolRec {
  int accepted, reason;  // reason: 0 ok, 1 factorisation, 2 primal, 3 dual
  int n_lower, n_upper;
  double pri_before, dua_before, pri_after, dua_after, obj;
};
constexpr size_t POL_REC_DOUBLES = (sizeof(PolRec) + 7) / 8;

struct Pol {
  int n, M, ld;
  double delta, inv_delta;
  const int *pc_ptr, *pc_idx, *pv_ptr, *pv_idx, *pr_ptr, *pr_idx;
  const double *A, *At, *pr_val, *q;  // unscaled: rows of A, rows of A^T, rows of the full symmetric P, linear cost
  const double *l, *u, *x, *y;        // the node's bounds and the solution to polish
  double *w, *b;                      // per row: 1 / delta when active, else 0; the active bound
  double *S, *LinvT, *dd;             // S, later strict_lower(L^-1) in place; its transpose; the pivots
  double *xh, *yh, *r1, *r2, *t, *v, *dx;
  double *prow0, *prow1, *dcol0, *dcol1, *ocol;  // per row / per variable terms of the two norms before and after, of the objective
  int *cnt;                           // [0] lower-active rows, [1] upper-active rows, [2] the factorisation's flag;
                                      // the revision's: [4] rows added, [5] dropped, [6] / [7] lower / upper of the new set
  PolRec *rec;                        // followed by the returned x (n) and y (M)
  signed char *cls, *cls_next;        // per row -1 lower-active, 1 upper-active, 0 inactive: of this round's set, of the revised one
};

__device__ __forceinline__ double pol_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
// maximum that keeps a NaN (fmax would drop it and a broken point would pass the acceptance test)
__device__ __forceinline__ double pol_max(double m, double v) { return (v > m || v != v) ? v : m; }

// sum over one padded row of val[k] * vec[idx[k]] by one wavefront (every lane returns it)
__device__ __forceinline__ double pol_row_dot(const int *__restrict__ idx, const double *__restrict__ val, int s, int e,
                                              int lane, const double *__restrict__ vec) {
  double acc = 0.0;
  for (int k = s + lane; k < e; k += 64) acc = fma(val[k], vec[idx[k]], acc);
  return pol_wave_sum(acc);
}

// Step 1, one wavefront per row: z = A x, the row's class by OSQP's rule (plus: an equality row is always active, an
// infinite bound never is), its weight and bound, the two counts, and the row's term of the input's primal residual.
__global__ __launch_bounds__(256) void k_pol_classify(Pol p) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= p.M) return;
  const double z = pol_row_dot(p.pc_idx, p.A, p.pc_ptr[row], p.pc_ptr[row + 1], lane, p.x);
  if (lane) return;
  const double l = p.l[row], u = p.u[row], y = p.y[row];
  double w = 0.0, b = 0.0;
  signed char c = 0;
  if (l > -QP_INFTY && (l == u || z - l < -y)) {
    w = p.inv_delta;
    b = l;
    c = -1;
    atomicAdd(p.cnt, 1);
  } else if (u < QP_INFTY && u - z < y) {
    w = p.inv_delta;
    b = u;
    c = 1;
    atomicAdd(p.cnt + 1, 1);
  }
  p.w[row] = w;
  p.b[row] = b;
  p.cls[row] = c;
  p.prow0[row] = pol_max(pol_max(0.0, l - z), z - u);
}

// The revision after a round's solves, one wavefront per row: z = A xh and the row's class in the revised set.  An
// equality row stays; a lower-active row whose multiplier is above POL_TOL and an upper-active one whose multiplier is
// below -POL_TOL leave; an inactive row violated by more than POL_TOL joins on that side (a row that just left is not
// looked at again).  Weight, bound and class of the revised set, and the four counters.  After a round whose
// factorisation broke there is no point to revise from: nothing is written and the counters stay zero.
__global__ __launch_bounds__(256) void k_pol_revise(Pol p) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= p.M) return;
  if (p.cnt[2] != 0) return;
  const double z = pol_row_dot(p.pc_idx, p.A, p.pc_ptr[row], p.pc_ptr[row + 1], lane, p.xh);
  if (lane) return;
  const double l = p.l[row], u = p.u[row], y = p.yh[row];
  const signed char c = p.cls[row];
  signed char cn = c;
  if (l != u) {
    if (c < 0) cn = y > POL_TOL ? 0 : c;
    else if (c > 0) cn = y < -POL_TOL ? 0 : c;
    else if (l > -QP_INFTY && l - z > POL_TOL) cn = -1;
    else if (u < QP_INFTY && z - u > POL_TOL) cn = 1;
  }
  if (cn != c) atomicAdd(p.cnt + (c == 0 ? 4 : 5), 1);
  if (cn != 0) atomicAdd(p.cnt + (cn < 0 ? 6 : 7), 1);
  p.w[row] = cn != 0 ? p.inv_delta : 0.0;
  p.b[row] = cn < 0 ? l : cn > 0 ? u : 0.0;
  p.cls_next[row] = cn;
}

// Row i1 of S = P + delta I + sum over active rows r of (1 / delta) A[r][i1] A[r][:] (lower triangle; the rest of the
// row is written as zeros) by ONE workgroup in LDS -- ks_schur_row (dense_setup.hip) with a weight per constraint row:
// P's entries, delta on the diagonal, then for every constraint row that holds variable i1, ascending, rows of weight 0
// skipped, weight * A[r][i1] times row r up to column i1, one fused multiply-add per entry.  The entries of one row are
// distinct columns (the pad that repeats the last column is skipped), so the lanes never collide.
__global__ __launch_bounds__(256) void k_pol_schur_row(Pol p) {
  extern __shared__ double pol_acc[];
  const int i1 = blockIdx.x, tid = threadIdx.x;
  for (int c = tid; c < p.ld; c += 256) pol_acc[c] = 0.0;
  __syncthreads();
  {
    const int k0 = p.pr_ptr[i1], k1 = p.pr_ptr[i1 + 1];
    for (int k = k0 + tid; k < k1; k += 256) {
      const int i2 = p.pr_idx[k];
      if (i2 > i1 || (k > k0 && p.pr_idx[k - 1] == i2)) continue;
      pol_acc[i2] += p.pr_val[k];
    }
  }
  __syncthreads();
  if (tid == 0) pol_acc[i1] += p.delta;
  __syncthreads();
  const int a0 = p.pv_ptr[i1], a1 = p.pv_ptr[i1 + 1];
  for (int a = a0; a < a1; a++) {
    const int r = p.pv_idx[a];
    if (a > a0 && p.pv_idx[a - 1] == r) continue;  // the pad
    const double wr = p.w[r];
    if (wr == 0.0) continue;  // (uniform over the workgroup)
    const double wgt = wr * p.At[a];
    const int k0 = p.pc_ptr[r], k1 = p.pc_ptr[r + 1];
    for (int k = k0 + tid; k < k1; k += 256) {
      const int i2 = p.pc_idx[k];
      if (i2 > i1 || (k > k0 && p.pc_idx[k - 1] == i2)) continue;
      pol_acc[i2] = fma(wgt, p.A[k], pol_acc[i2]);
    }
    __syncthreads();
  }
  for (int c = tid; c < p.ld; c += 256) p.S[(size_t)i1 * p.ld + c] = pol_acc[c];
}

// r2 = b - A_act xh on the active rows, 0 elsewhere (one wavefront per row)
__global__ __launch_bounds__(256) void k_pol_r2(Pol p) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= p.M) return;
  const double ax = pol_row_dot(p.pc_idx, p.A, p.pc_ptr[row], p.pc_ptr[row + 1], lane, p.xh);
  if (lane == 0) p.r2[row] = p.w[row] != 0.0 ? p.b[row] - ax : 0.0;
}

// r1 = -q - P xh - A^T yh (yh is zero on inactive rows) and t = r1 + A_act^T r2 / delta (one wavefront per variable)
__global__ __launch_bounds__(256) void k_pol_rhs(Pol p) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= p.n) return;
  const double px = pol_row_dot(p.pr_idx, p.pr_val, p.pr_ptr[i], p.pr_ptr[i + 1], lane, p.xh);
  double aty = 0.0, atr = 0.0;
  for (int k = p.pv_ptr[i] + lane; k < p.pv_ptr[i + 1]; k += 64) {
    const int r = p.pv_idx[k];
    const double a = p.At[k];
    aty = fma(a, p.yh[r], aty);
    atr = fma(a, p.w[r] * p.r2[r], atr);
  }
  aty = pol_wave_sum(aty);
  atr = pol_wave_sum(atr);
  if (lane == 0) {
    const double r1 = (-p.q[i] - px) - aty;
    p.r1[i] = r1;
    p.t[i] = r1 + atr;
  }
}

// v = D^-1 L^-1 t: row i of the strict lower triangle of L^-1 (unit diagonal implied) times t (one wavefront per row)
__global__ __launch_bounds__(256) void k_pol_lower(Pol p) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= p.n) return;
  const double *__restrict__ row = p.S + (size_t)i * p.ld;
  double acc = 0.0;
  for (int j = lane; j < i; j += 64) acc = fma(row[j], p.t[j], acc);
  acc = pol_wave_sum(acc);
  if (lane == 0) p.v[i] = (p.t[i] + acc) / p.dd[i];
}

// dx = L^-T v, xh += dx
__global__ __launch_bounds__(256) void k_pol_upper(Pol p) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= p.n) return;
  const double *__restrict__ row = p.LinvT + (size_t)i * p.ld;
  double acc = 0.0;
  for (int j = i + 1 + lane; j < p.n; j += 64) acc = fma(row[j], p.v[j], acc);
  acc = pol_wave_sum(acc);
  if (lane == 0) {
    const double dx = p.v[i] + acc;
    p.dx[i] = dx;
    p.xh[i] += dx;
  }
}

// dy = (A_act dx - r2) / delta on the active rows, yh += dy
__global__ __launch_bounds__(256) void k_pol_dy(Pol p) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= p.M) return;
  const double wr = p.w[row];
  if (wr == 0.0) return;  // (uniform over the wavefront)
  const double ax = pol_row_dot(p.pc_idx, p.A, p.pc_ptr[row], p.pc_ptr[row + 1], lane, p.dx);
  if (lane == 0) p.yh[row] += wr * (ax - p.r2[row]);
}

// the polished point's term of the primal residual, over ALL rows
__global__ __launch_bounds__(256) void k_pol_rows_after(Pol p) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= p.M) return;
  const double z = pol_row_dot(p.pc_idx, p.A, p.pc_ptr[row], p.pc_ptr[row + 1], lane, p.xh);
  if (lane == 0) p.prow1[row] = pol_max(pol_max(0.0, p.l[row] - z), z - p.u[row]);
}

// per variable: |P x + q + A^T y| of the input and of the polished point, and the polished point's term of the objective
__global__ __launch_bounds__(256) void k_pol_cols(Pol p) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= p.n) return;
  const int s = p.pr_ptr[i], e = p.pr_ptr[i + 1];
  const double px0 = pol_row_dot(p.pr_idx, p.pr_val, s, e, lane, p.x);
  const double px1 = pol_row_dot(p.pr_idx, p.pr_val, s, e, lane, p.xh);
  double a0 = 0.0, a1 = 0.0;
  for (int k = p.pv_ptr[i] + lane; k < p.pv_ptr[i + 1]; k += 64) {
    const int r = p.pv_idx[k];
    const double a = p.At[k];
    a0 = fma(a, p.y[r], a0);
    a1 = fma(a, p.yh[r], a1);
  }
  a0 = pol_wave_sum(a0);
  a1 = pol_wave_sum(a1);
  if (lane == 0) {
    const double q = p.q[i];
    p.dcol0[i] = fabs((px0 + q) + a0);
    p.dcol1[i] = fabs((px1 + q) + a1);
    p.ocol[i] = p.xh[i] * fma(0.5, px1, q);
  }
}

// The four norms and the objective (one workgroup; thread t takes entries t, t + 256, .. in order, then a fixed tree),
// the decision, the record, and the point that goes back: the polished one when accepted, the input bit for bit otherwise.
__global__ __launch_bounds__(256) void k_pol_decide(Pol p) {
  __shared__ double red[5][256];
  __shared__ int take;
  const int tid = threadIdx.x;
  double m0 = 0.0, m1 = 0.0, d0 = 0.0, d1 = 0.0, ob = 0.0;
  for (int j = tid; j < p.M; j += 256) {
    m0 = pol_max(m0, p.prow0[j]);
    m1 = pol_max(m1, p.prow1[j]);
  }
  for (int i = tid; i < p.n; i += 256) {
    d0 = pol_max(d0, p.dcol0[i]);
    d1 = pol_max(d1, p.dcol1[i]);
    ob += p.ocol[i];
  }
  red[0][tid] = m0; red[1][tid] = m1; red[2][tid] = d0; red[3][tid] = d1; red[4][tid] = ob;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int k = 0; k < 4; k++) red[k][tid] = pol_max(red[k][tid], red[k][tid + s]);
      red[4][tid] += red[4][tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    PolRec r;
    const bool broke = p.cnt[2] != 0;
    const double nan = __builtin_nan("");
    r.n_lower = p.cnt[0];
    r.n_upper = p.cnt[1];
    r.pri_before = red[0][0];
    r.dua_before = red[2][0];
    r.pri_after = broke ? nan : red[1][0];
    r.dua_after = broke ? nan : red[3][0];
    r.obj = broke ? nan : red[4][0];
    r.reason = 0;
    if (broke) r.reason = 1;
    else if (!(r.pri_after <= fmax(r.pri_before, 1e-10))) r.reason = 2;
    else if (!(r.dua_after <= fmax(r.dua_before, 1e-10))) r.reason = 3;
    r.accepted = r.reason == 0;
    *p.rec = r;
    take = r.accepted;
  }
  __syncthreads();
  double *xo = (double *)p.rec + POL_REC_DOUBLES, *yo = xo + p.n;
  const double *xs = take ? p.xh : p.x, *ys = take ? p.yh : p.y;
  for (int i = tid; i < p.n; i += 256) xo[i] = xs[i];
  for (int j = tid; j < p.M; j += 256) yo[j] = ys[j];
}

// host side of one engine's polishing: the kernels' argument block, scratch of the factorisation, the pinned block both
// directions go through (l | u | x | y in, record | x | y out), events around the stages
struct PolishScratch {
  Pol p{};
  double *din = nullptr, *X = nullptr, *W = nullptr;
  double *h = nullptr;
  hipEvent_t ev[6] = {};
  double stage_s[4] = {0, 0, 0, 0};  // classification, Schur rows, factorisation, solves + acceptance of the last call
  // the repair loop: the kept point of the round before (n + M), the second class array, the second record (+ x + y), the
  // counters' pinned copy, an event per round (the host waits for it), and the last call's trace
  double *xk = nullptr, *yk = nullptr;
  signed char *cls_buf[2] = {nullptr, nullptr};  // the set of round k is in cls_buf[k & 1]
  PolRec *rec2 = nullptr;
  int *hcnt = nullptr;
  signed char *hcls = nullptr;
  hipEvent_t evr[POL_MAX_ROUNDS] = {};
  int rounds_run = 0;                 // rounds of the last repair call, round 0 included (0: none yet)
  double round_s[POL_MAX_ROUNDS] = {}, wait_s[POL_MAX_ROUNDS] = {};  // device seconds of a round up to its counters, host wait for them
};
