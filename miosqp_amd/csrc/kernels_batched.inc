// part of engine.hip (included there, not compiled alone): batched mode: sparse row kernels, dense vector-FMA tiles, fp64 matrix-core tiles, batched test
// ------------------------------------------------------------------------------------------
// batched mode: B independent nodes share the factor (leaves of one wave).  Vectors are
// [len][Bs] with the batch index fastest, so one wavefront = one matrix row x 64 nodes: the
// row's entries are wave-uniform (scalar loads, read once for 64 nodes) and every vector access
// is one coalesced 512-byte line.  No cross-lane reduction is needed at all.
// ------------------------------------------------------------------------------------------
#define BSETUP                                                                \
  const int lane = threadIdx.x & 63;                                          \
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));     \
  const int b = blockIdx.y * 64 + lane;                                       \
  const size_t Bs = (size_t)d.Bs;

// sum_k val[k] * V[idx[k]][b] over one padded row (wave-uniform row)
__device__ __forceinline__ double brow_dot(const int *__restrict__ idx, const double *__restrict__ val, int s,
                                           int e, const double *__restrict__ V, size_t Bs) {
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int k = s;
  for (; k + 4 <= e; k += 4) {
    a0 = fma(val[k], V[(size_t)idx[k] * Bs], a0);
    a1 = fma(val[k + 1], V[(size_t)idx[k + 1] * Bs], a1);
    a2 = fma(val[k + 2], V[(size_t)idx[k + 2] * Bs], a2);
    a3 = fma(val[k + 3], V[(size_t)idx[k + 3] * Bs], a3);
  }
  for (; k < e; k += 2) {
    a0 = fma(val[k], V[(size_t)idx[k] * Bs], a0);
    a1 = fma(val[k + 1], V[(size_t)idx[k + 1] * Bs], a1);
  }
  return (a0 + a1) + (a2 + a3);
}
__device__ __forceinline__ void brow_dot2(const int *__restrict__ idx, const double *__restrict__ val, int s, int e,
                                          const double *__restrict__ V, const double *__restrict__ W, size_t Bs,
                                          double &rv, double &rw) {
  double a0 = 0.0, a1 = 0.0, c0 = 0.0, c1 = 0.0;
  for (int k = s; k < e; k += 2) {
    const size_t o0 = (size_t)idx[k] * Bs, o1 = (size_t)idx[k + 1] * Bs;
    a0 = fma(val[k], V[o0], a0);
    a1 = fma(val[k + 1], V[o1], a1);
    c0 = fma(val[k], W[o0], c0);
    c1 = fma(val[k + 1], W[o1], c1);
  }
  rv = a0 + a1;
  rw = c0 + c1;
}
// dense contiguous row segment [j0, j1) against V[j][b]
__device__ __forceinline__ double bdense_dot(const double *__restrict__ row, int j0, int j1,
                                             const double *__restrict__ V, size_t Bs) {
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int j = j0;
  for (; j + 4 <= j1; j += 4) {
    a0 = fma(row[j], V[(size_t)j * Bs], a0);
    a1 = fma(row[j + 1], V[(size_t)(j + 1) * Bs], a1);
    a2 = fma(row[j + 2], V[(size_t)(j + 2) * Bs], a2);
    a3 = fma(row[j + 3], V[(size_t)(j + 3) * Bs], a3);
  }
  for (; j < j1; j++) a0 = fma(row[j], V[(size_t)j * Bs], a0);
  return (a0 + a1) + (a2 + a3);
}

// The linear cost of column b at `row` (o = row * Bs + b).  PQ = false: the engine's own scaled q, one value per row shared
// by every column (solve_batch, the derived batches, the pool, kbs).  PQ = true: the column's own cost from the
// batch-fastest array b_q[n x Bs] (miosqp_qp_solve_batch_q: one MIQP per column on the shared factor).
template <bool PQ>
__device__ __forceinline__ double bq_at(const Dev &d, int row, size_t o) {
  if constexpr (PQ) return d.b_q[o];
  else return d.q[row];
}

template <bool PQ>
__global__ __launch_bounds__(256) void kb_panel_fwd(Dev d) {
  if (d.ctrl->done) return;
  BSETUP
  const int row = blockIdx.x * 4 + wv;
  if (row >= d.n) return;
  const double acc = brow_dot(d.pv_idx, d.pv_L, d.pv_ptr[row], d.pv_ptr[row + 1], d.b_wh + b, Bs);
  d.b_cv[row * Bs + b] = d.sigma * d.b_x[row * Bs + b] - bq_at<PQ>(d, row, row * Bs + b) - acc;
}

__global__ __launch_bounds__(256) void kb_tail_fwd(Dev d) {
  if (d.ctrl->done) return;
  BSETUP
  const int row = blockIdx.x * 4 + wv;
  if (row >= d.n) return;
  const double acc = bdense_dot(d.Linv + (size_t)row * d.ld, 0, row, d.b_cv + b, Bs);
  d.b_ut[row * Bs + b] = d.d2inv[row] * (d.b_cv[row * Bs + b] + acc);
}

__global__ __launch_bounds__(256) void kb_tail_bwd(Dev d) {
  if (d.ctrl->done) return;
  BSETUP
  const int row = blockIdx.x * 4 + wv;
  if (row >= d.n) return;
  const double acc = bdense_dot(d.LinvT + (size_t)row * d.ld, row + 1, d.n, d.b_ut + b, Bs);
  const double xt = d.b_ut[row * Bs + b] + acc;
  d.b_xt[row * Bs + b] = xt;
  if (!d.c_done[b]) {
    const double xp = d.b_x[row * Bs + b];
    const double xn = d.alpha * xt + (1.0 - d.alpha) * xp;
    d.b_x[row * Bs + b] = xn;
    d.b_dx[row * Bs + b] = xn - xp;
  }
}

__global__ __launch_bounds__(256) void kb_panel_bwd(Dev d) {
  if (d.ctrl->done) return;
  BSETUP
  const int row = blockIdx.x * 4 + wv;
  if (row >= d.M) return;
  const double acc = brow_dot(d.pc_idx, d.pc_L, d.pc_ptr[row], d.pc_ptr[row + 1], d.b_xt + b, Bs);
  if (d.c_done[b]) return;
  const size_t o = row * Bs + b;
  const double rho = d.rho, rinv = d.rho_inv, alpha = d.alpha;
  const double zp = d.b_z[o], yp = d.b_y[o];
  const double nu = -rho * d.b_wh[o] - acc;
  const double zt = zp + rinv * (nu - yp);
  const double zr = alpha * zt + (1.0 - alpha) * zp;
  const double v = zr + rinv * yp;
  const double zn = fmin(fmax(v, d.b_l[o]), d.b_u[o]);
  const double dy = rho * (zr - zn);
  const double yn = yp + dy;
  d.b_z[o] = zn;
  d.b_y[o] = yn;
  d.b_dy[o] = dy;
  d.b_wh[o] = zn - rinv * yn;
}

__global__ __launch_bounds__(256) void kb_check_con(Dev d) {
  if (d.ctrl->done) return;
  BSETUP
  const int row = blockIdx.x * 4 + wv;
  if (row >= d.M) return;
  double ax, adx0;
  brow_dot2(d.pc_idx, d.pc_A, d.pc_ptr[row], d.pc_ptr[row + 1], d.b_x + b, d.b_dx + b, Bs, ax, adx0);
  const size_t o = row * Bs + b, MB = (size_t)d.M * Bs;
  const double ei = d.Einv[row], z = d.b_z[o], l = d.b_l[o], u = d.b_u[o];
  const bool uinf = u > QP_INFTY * QP_MIN_SCALING, linf = l < -QP_INFTY * QP_MIN_SCALING;
  double v = d.b_dy[o];
  if (uinf && linf) v = 0.0;
  else if (uinf) v = fmin(v, 0.0);
  else if (linf) v = fmax(v, 0.0);
  const double adx = ei * adx0;
  d.b_sm[0 * MB + o] = ei * (ax - z);
  d.b_sm[1 * MB + o] = ei * ax;
  d.b_sm[2 * MB + o] = ei * z;
  d.b_sm[3 * MB + o] = v;
  d.b_sm[4 * MB + o] = d.E[row] * v;
  d.b_sm[5 * MB + o] = u * fmax(v, 0.0) + l * fmin(v, 0.0);
  d.b_sm[6 * MB + o] = uinf ? -1.7e308 : adx;
  d.b_sm[7 * MB + o] = linf ? 1.7e308 : adx;
}

// blockIdx.x in [0, nrb): P rows; [nrb, 2 nrb): A^T rows
__global__ __launch_bounds__(256) void kb_check_var(Dev d) {
  if (d.ctrl->done) return;
  BSETUP
  const int nrb = (d.n + 3) / 4;
  const bool second = (int)blockIdx.x >= nrb;
  const int row = ((int)blockIdx.x - (second ? nrb : 0)) * 4 + wv;
  if (row >= d.n) return;
  const size_t o = row * Bs + b, NB = (size_t)d.n * Bs;
  double r0, r1;
  if (!second) {
    brow_dot2(d.pb_idx, d.pb_val, d.pb_ptr[row], d.pb_ptr[row + 1], d.b_x + b, d.b_dx + b, Bs, r0, r1);
    d.b_sn[0 * NB + o] = r0;
    d.b_sn[1 * NB + o] = d.Dinv[row] * r1;
  } else {
    brow_dot2(d.pv_idx, d.pv_At, d.pv_ptr[row], d.pv_ptr[row + 1], d.b_y + b, d.b_sm + 3 * (size_t)d.M * Bs + b, Bs,
              r0, r1);
    d.b_sn[2 * NB + o] = r0;
    d.b_sn[3 * NB + o] = d.Dinv[row] * r1;
  }
}

// ------------------------------------------------------------------------------------------
// batched mode on the product-form factor: dense row blocks.  One workgroup = 8 waves =
// 4 row groups x 2 halves of the k range; a wave owns 2 rows x 64 nodes.  The right-hand tile
// V[k0..k0+16)[64 nodes] is staged once per workgroup in LDS (double-buffered, next tile's global
// loads in flight during the FMAs), matrix entries are wave-uniform scalar loads, each LDS value
// feeds both rows.  The two k halves are added in LDS in a fixed order.
// ------------------------------------------------------------------------------------------
constexpr int BD_KT = 16, BD_R = 2;

// RG row groups x KS slices of the k range = RG*KS waves per workgroup, 2*RG rows per workgroup
template <int RG, int KS>
__device__ __forceinline__ void bd_dot(const double *__restrict__ A, int ld, int nrows, int row0, int kbeg,
                                       int kend, const double *__restrict__ V, size_t Bs, double *lds,
                                       double (&acc)[BD_R]) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int rg = w % RG, kh = w / RG;
  constexpr int LPT = BD_KT / RG;  // tile rows staged per wave
  const int k0 = kbeg & ~(BD_KT - 1);
  const int nt_slice = ((kend - k0 + BD_KT - 1) / BD_KT + KS - 1) / KS;
  const int kstart = k0 + kh * nt_slice * BD_KT;
  double *buf = lds + kh * (2 * BD_KT * 64);
  int ra = row0 + rg * BD_R, rb = ra + 1;
  ra = ra < nrows ? ra : nrows - 1;
  rb = rb < nrows ? rb : nrows - 1;
  const double *__restrict__ a0 = A + (size_t)ra * ld;
  const double *__restrict__ a1 = A + (size_t)rb * ld;
  acc[0] = acc[1] = 0.0;
  double p[LPT];
#pragma unroll
  for (int i = 0; i < LPT; i++) {
    const int k = kstart + rg + RG * i;
    p[i] = k < kend ? V[(size_t)k * Bs] : 0.0;
  }
#pragma unroll
  for (int i = 0; i < LPT; i++) buf[(rg + RG * i) * 64 + lane] = p[i];
  __syncthreads();
  for (int t = 0; t < nt_slice; t++) {
    const int kt = kstart + t * BD_KT;
    const bool more = t + 1 < nt_slice;
    if (more) {
#pragma unroll
      for (int i = 0; i < LPT; i++) {
        const int k = kt + BD_KT + rg + RG * i;
        p[i] = k < kend ? V[(size_t)k * Bs] : 0.0;
      }
    }
    const double *cur = buf + (t & 1) * (BD_KT * 64);
#pragma unroll
    for (int kk = 0; kk < BD_KT; kk++) {
      const double v = cur[kk * 64 + lane];
      acc[0] = fma(a0[kt + kk], v, acc[0]);
      acc[1] = fma(a1[kt + kk], v, acc[1]);
    }
    if (more) {
      double *nxt = buf + ((t + 1) & 1) * (BD_KT * 64);
#pragma unroll
      for (int i = 0; i < LPT; i++) nxt[(rg + RG * i) * 64 + lane] = p[i];
    }
    __syncthreads();
  }
  // add the k slices in a fixed order: slice 0 + slice 1 + ...
  double *red = lds + KS * 2 * BD_KT * 64;
  if (kh > 0) {
    red[((kh - 1) * RG * BD_R + rg * BD_R + 0) * 64 + lane] = acc[0];
    red[((kh - 1) * RG * BD_R + rg * BD_R + 1) * 64 + lane] = acc[1];
  }
  __syncthreads();
  if (kh == 0) {
#pragma unroll
    for (int s = 1; s < KS; s++) {
      acc[0] += red[((s - 1) * RG * BD_R + rg * BD_R + 0) * 64 + lane];
      acc[1] += red[((s - 1) * RG * BD_R + rg * BD_R + 1) * 64 + lane];
    }
  }
}

template <int RG, int KS>
struct BdCfg {
  static constexpr int ROWS = RG * BD_R, THREADS = RG * KS * 64;
  static constexpr int LDS = KS * 2 * BD_KT * 64 + (KS - 1) * RG * BD_R * 64;
};

// ut = D22^-1 ( rx + [ -G | strict_lower(Linv) ] [wh ; rx] ), rows of L^-1
template <int RG, int KS>
__global__ __launch_bounds__(RG *KS * 64) void kbd_fwd(Dev d) {
  if (d.ctrl->done) return;
  using C = BdCfg<RG, KS>;
  __shared__ double lds[C::LDS];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const size_t Bs = (size_t)d.Bs;
  const int b = blockIdx.y * 64 + lane;
  const int row0 = blockIdx.x * C::ROWS;
  int kend = d.M + row0 + C::ROWS;
  if (kend > d.M + d.n) kend = d.M + d.n;
  double acc[BD_R];
  bd_dot<RG, KS>(d.f_rows, d.ldf, d.n, row0, 0, kend, d.b_wh + b, Bs, lds, acc);
  if (w >= RG) return;
#pragma unroll
  for (int r = 0; r < BD_R; r++) {
    const int row = row0 + w * BD_R + r;
    if (row < d.n) d.b_ut[row * Bs + b] = d.d2inv[row] * (d.b_rx[row * Bs + b] + acc[r]);
  }
}

// rows of L^-T: blocks [0, nbx) the x rows (strict upper Linv^T), the rest the constraint rows (-G)^T
template <int RG, int KS, bool PQ = false>
__global__ __launch_bounds__(RG *KS * 64) void kbd_bwd(Dev d) {
  if (d.ctrl->done) return;
  using C = BdCfg<RG, KS>;
  __shared__ double lds[C::LDS];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const size_t Bs = (size_t)d.Bs;
  const int b = blockIdx.y * 64 + lane;
  const int nbx = (d.n + C::ROWS - 1) / C::ROWS;
  double acc[BD_R];
  if ((int)blockIdx.x < nbx) {
    const int row0 = blockIdx.x * C::ROWS;
    bd_dot<RG, KS>(d.LinvT, d.ld, d.n, row0, row0 + 1, d.n, d.b_ut + b, Bs, lds, acc);
    if (w >= RG) return;
    const bool frozen = d.c_done[b] != 0;
#pragma unroll
    for (int r = 0; r < BD_R; r++) {
      const int row = row0 + w * BD_R + r;
      if (row >= d.n) continue;
      const size_t o = row * Bs + b;
      const double xt = d.b_ut[o] + acc[r];
      d.b_xt[o] = xt;
      if (!frozen) {
        const double xp = d.b_x[o];
        const double xn = d.alpha * xt + (1.0 - d.alpha) * xp;
        d.b_x[o] = xn;
        d.b_dx[o] = xn - xp;
        d.b_rx[o] = d.sigma * xn - bq_at<PQ>(d, row, o);
      }
    }
    return;
  }
  const int row0 = (blockIdx.x - nbx) * C::ROWS;
  bd_dot<RG, KS>(d.f_GmT, d.ldn, d.M, row0, 0, d.n, d.b_ut + b, Bs, lds, acc);
  if (w >= RG) return;
  if (d.c_done[b]) return;
  const double rho = d.rho, rinv = d.rho_inv, alpha = d.alpha;
#pragma unroll
  for (int r = 0; r < BD_R; r++) {
    const int row = row0 + w * BD_R + r;
    if (row >= d.M) continue;
    const size_t o = row * Bs + b;
    const double zp = d.b_z[o], yp = d.b_y[o];
    const double nu = -rho * d.b_wh[o] + acc[r];
    const double zt = zp + rinv * (nu - yp);
    const double zr = alpha * zt + (1.0 - alpha) * zp;
    const double v = zr + rinv * yp;
    const double zn = fmin(fmax(v, d.b_l[o]), d.b_u[o]);
    const double dy = rho * (zr - zn);
    const double yn = yp + dy;
    d.b_z[o] = zn;
    d.b_y[o] = yn;
    d.b_dy[o] = dy;
    d.b_wh[o] = zn - rinv * yn;
  }
}

// ------------------------------------------------------------------------------------------
// batched mode, product-form factor, fp64 matrix cores.  With 256 right-hand sides the sweeps are
// dense fp64 GEMMs (500 x 1750 x 256 for config 2); v_mfma_f64_16x16x4_f64 sustains the chip's full
// fp64 rate (78 TFLOP/s measured, tools/probes/fp64_rate.hip; the vector pipe 46-60) and needs no
// wave-uniform operand (the scalar cache is what limits the kbd_* kernels).  One workgroup = KS waves
// sharing ONE 16 x 32 output tile: wave w takes the 16-deep k chunks w, w+KS, ...; partial tiles are
// added in LDS in wave order (fixed order).
// Fragment layout (MI355X_MICROARCH / cdna_hip_programming sec. 3): A[i = l&15][k = l>>4],
// B[k = l>>4][j = l&15], C/D row = (l>>4) + 4*reg, col = l&15.  Within a 16-deep chunk MFMA step s
// covers k = k0 + 4*(l>>4) + s, so a lane reads its four A values as one 32-byte segment.  The two
// 16-column tiles of a workgroup interleave: tile t holds columns col0 + 2 j + t, so a lane reads the
// B operands of BOTH tiles for one k as ONE 16-byte load (16 lanes = 256 contiguous bytes).
// Operands travel global -> registers through a three-deep software pipeline with no branch and no
// mask inside: every row of the matrices is zero-padded to a multiple of 16, the right-hand arrays
// carry 16 zero rows of slack, and a wave whose chunk lies beyond the end reads a page of zeros
// instead (pointer select), so out-of-range products are exact zeros.
// ------------------------------------------------------------------------------------------
typedef double double4_t __attribute__((ext_vector_type(4)));
constexpr int BM_NT = 2, BM_COLS = 16 * BM_NT, BM_OUT = BM_NT * 256;

struct BmStage {
  double2 a01, a23;   // A[row][kc + 4 j + 0..3]
  double2 b[4];       // step s: columns (col0 + 2 r, col0 + 2 r + 1) at k = kc + 4 j + s
};

// Placement: block L runs on XCD L % 8 (observed, MI355X_MICROARCH; used for speed only).  The workgroups that
// share a row block -- its C column blocks -- are numbered so that they land on ONE XCD, back to back: the row
// block's rows then cross the fabric once instead of once per XCD (measured on kbm_bwd: 40 % L2 misses with the
// plain 2-D grid).  Grid = 8 * ceil(R / 8) * C blocks; returns false for the padding blocks.
__device__ __forceinline__ bool bm_place(int R, int C, int &rb, int &cb) {
  const int L = blockIdx.x, xcd = L & 7, s = L >> 3;
  rb = xcd + 8 * (s / C);
  cb = s % C;
  return rb < R;
}
inline int bm_grid(int R, int C) { return 8 * ((R + 7) / 8) * C; }

// zeros: a 256-byte aligned page of >= 32 zero doubles (wave-uniform address: one cache line for everybody)
template <int KS, int DEPTH, int ABL = 0>
__device__ __forceinline__ void bm_tile(const double *__restrict__ A, int ld, int nrows, int row0, int kbeg, int kend,
                                        const double *__restrict__ V, size_t Bs, const double *__restrict__ zeros,
                                        double4_t (&acc)[BM_NT], unsigned long long *stamp = nullptr) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int r = lane & 15, j = lane >> 4;
  int row = row0 + r;
  row = row < nrows ? row : nrows - 1;
  const int k0 = kbeg & ~15;
  const double *__restrict__ ap = A + (size_t)row * ld + 4 * j;
  const double *__restrict__ vp = V + 2 * r + (size_t)(4 * j) * Bs;
  const double *__restrict__ zp = zeros + 4 * j;
  const int nit = (kend - k0 + 16 * KS - 1) / (16 * KS);  // the same for every wave of the workgroup
  double4_t acc2[BM_NT];
#pragma unroll
  for (int t = 0; t < BM_NT; t++) {
    acc[t] = (double4_t){0.0, 0.0, 0.0, 0.0};
    acc2[t] = (double4_t){0.0, 0.0, 0.0, 0.0};
  }
  BmStage st[DEPTH];
  auto fetch = [&](BmStage &s, int i) {
    const int kc = k0 + 16 * (w + KS * i);
    const bool in = kc < kend;                          // wave-uniform
    // beyond the end: both operands come from the zero page (one cache line for the whole wave, no traffic)
    const double *pa = in ? ap + kc : zp;
    const double *pv = in ? vp + (size_t)kc * Bs : zp;
    const size_t vs = in ? Bs : 0;
    s.a01 = *reinterpret_cast<const double2 *>(pa);
    s.a23 = *reinterpret_cast<const double2 *>(pa + 2);
#pragma unroll
    for (int q = 0; q < 4; q++) s.b[q] = *reinterpret_cast<const double2 *>(pv + (size_t)q * vs);
  };
  auto compute = [&](const BmStage &s) {
    // four independent accumulator chains: (step 0, 2) -> acc, (step 1, 3) -> acc2, two tiles each
    acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(s.a01.x, s.b[0].x, acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(s.a01.x, s.b[0].y, acc[1], 0, 0, 0);
    acc2[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(s.a01.y, s.b[1].x, acc2[0], 0, 0, 0);
    acc2[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(s.a01.y, s.b[1].y, acc2[1], 0, 0, 0);
    acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(s.a23.x, s.b[2].x, acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(s.a23.x, s.b[2].y, acc[1], 0, 0, 0);
    acc2[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(s.a23.y, s.b[3].x, acc2[0], 0, 0, 0);
    acc2[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(s.a23.y, s.b[3].y, acc2[1], 0, 0, 0);
  };
  // sched_barrier: the scheduler would otherwise sink every load to just before its use (fewer live
  // registers, no latency hiding at all: measured 2x slower)
#pragma unroll
  for (int q = 0; q < DEPTH; q++) fetch(st[q], q);
  __builtin_amdgcn_sched_barrier(0);
  if (stamp) stamp[1] = wall_clock64();  // debug: prologue done, first loads issued
  for (int i = 0; i < nit; i += DEPTH) {
#pragma unroll
    for (int q = 0; q < DEPTH; q++) {
      if (ABL != 2) compute(st[q]);    // chunk i + q (zeros when it lies beyond the end)
      if (stamp && i == 0 && q == 0) stamp[2] = wall_clock64();  // debug: the first chunk's operands have arrived
      __builtin_amdgcn_sched_barrier(0);
      if (ABL != 1) fetch(st[q], i + q + DEPTH);     // its registers take the chunk DEPTH ahead
      if (ABL == 2) acc[0][0] += st[q].a01.x + st[q].a23.y + st[q].b[0].x + st[q].b[1].y + st[q].b[2].x + st[q].b[3].y;
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll
  for (int t = 0; t < BM_NT; t++) acc[t] += acc2[t];
  if (stamp) stamp[3] = wall_clock64();  // debug: sweep done
}

// Output element owned by thread e < 512 of a tile: row e / 32, column e % 32 (consecutive threads = consecutive
// columns: coalesced epilogue).  In fragment terms: tile t = col & 1, fragment column (col >> 1), reg g = row >> 2,
// source lane ll = (col >> 1) + 16 (row & 3).
struct BmOut {
  int row, col, t, g, ll;
};
__device__ __forceinline__ BmOut bm_out(int e) {
  BmOut o;
  o.row = (e >> 5) & 15;
  o.col = e & 31;
  o.t = o.col & 1;
  o.g = o.row >> 2;
  o.ll = (o.col >> 1) + 16 * (o.row & 3);
  return o;
}

// adds the KS partial tiles in wave order; thread e < 512 gets output element bm_out(e)
template <int KS>
__device__ __forceinline__ double bm_reduce(const double4_t (&acc)[BM_NT], double *lds, const BmOut &o) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int t = 0; t < BM_NT; t++) {
#pragma unroll
    for (int g = 0; g < 4; g++) lds[((w * BM_NT + t) * 4 + g) * 64 + lane] = acc[t][g];
  }
  __syncthreads();
  if ((int)threadIdx.x >= BM_OUT) return 0.0;
  const int idx = (o.t * 4 + o.g) * 64 + o.ll;
  double s = lds[idx];
#pragma unroll
  for (int ww = 1; ww < KS; ww++) s += lds[ww * BM_OUT + idx];
  return s;
}

// Identity rows.  The p integer-bound rows of A (rows m .. M-1 = I[i_idx,:], /root/reference/miosqp/data.py:19-29) have ONE
// entry each, a_j at column i_j.  Their columns of G = L22^-1 L21 are therefore scaled columns of L22^-1,
//   -G[:, j] = rho a_j Linv_full[:, i_j],
// so their contribution to the forward sweep is Linv_full t with t[i_j] = rho a_j wh_j: it rides on the
// tail part of the product once the right-hand side carries r~ = rx + t instead of rx; and their rows of the
// backward sweep are (-G[:, j])^T ut = rho a_j x~[i_j]: no product at all, the thread that finishes x~[i_j] updates
// the bound row of that variable on the spot and forms r~[i_j] with the NEW wh_j.  The products shrink from
// K = M + n to m + n columns (forward) and from M to m rows (backward): -17 % work at config 2.  Layout: the
// right-hand array holds [ wh(general rows) | r~ | wh(bound rows) ], i.e. constraint row j sits at
// j < wh_m ? j : j + n, and b_rx = b_wh + wh_m * Bs.  Off (wh_m = M) when the rows are not of that form.
__device__ __forceinline__ size_t whrow(const Dev &d, int j) { return (size_t)(j < d.wh_m ? j : j + d.n); }

template <int KS, int DEPTH, int ABL = 0>
__global__ __launch_bounds__(KS * 64, KS / 4) void kbm_fwd(Dev d, int ncol) {
  // no `ctrl->done` test here: solve_slice never queues a chunk ahead of the host's decision, and the test is a
  // dependent memory round trip at the head of every workgroup
  __shared__ double lds[KS * BM_NT * 256];
  int rb, cb;
  if (!bm_place((d.n + 15) / 16, ncol, rb, cb)) return;
  const size_t Bs = (size_t)d.Bs;
  const int row0 = rb * 16, col0 = cb * BM_COLS;
  const BmOut o = bm_out(threadIdx.x);
  const int row = row0 + o.row, b = col0 + o.col;
  const bool mine = (int)threadIdx.x < BM_OUT && row < d.n;
  // the epilogue's operands are requested before the sweep: their latency hides behind it
  const double di = mine ? d.d2inv[row] : 0.0, rx = mine ? d.b_rx[row * Bs + b] : 0.0;
  int kend = d.wh_m + row0 + 16;
  if (kend > d.wh_m + d.n) kend = d.wh_m + d.n;
  double4_t acc[BM_NT];
  // debug timeline (miosqp_qp_debug_timeline which = 3): 100 MHz stamps of wave 0 per workgroup
  unsigned long long *stamp = (d.prof && threadIdx.x == 0) ? d.prof + 8 * blockIdx.x : nullptr;
  if (stamp) stamp[0] = wall_clock64();
  bm_tile<KS, DEPTH, ABL>(d.f_rows2, d.ldf2, d.n, row0, 0, kend, d.b_wh + col0, Bs, d.b_zero, acc, stamp);
  const double s = bm_reduce<KS>(acc, lds, o);
  if (stamp) stamp[4] = wall_clock64();
  if (mine) d.b_ut[row * Bs + b] = di * (rx + s);
  if (stamp) stamp[5] = wall_clock64();
}

template <int KS, int DEPTH, bool PQ = false>
__global__ __launch_bounds__(KS * 64, KS / 4) void kbm_bwd(Dev d, int ncol) {
  __shared__ double lds[KS * BM_NT * 256];
  const int nbx = (d.n + 15) / 16, nbc = (d.wh_m + 15) / 16;
  int rb, cb;
  if (!bm_place(nbx + nbc, ncol, rb, cb)) return;
  const size_t Bs = (size_t)d.Bs;
  const int col0 = cb * BM_COLS;
  const BmOut o = bm_out(threadIdx.x);
  const int b = col0 + o.col;
  const bool out = (int)threadIdx.x < BM_OUT;
  const double rho = d.rho, rinv = d.rho_inv, alpha = d.alpha;
  double4_t acc[BM_NT];
  if (rb < nbx) {
    const int row0 = rb * 16, row = row0 + o.row;
    const bool mine = out && row < d.n;
    const size_t oo = (size_t)row * Bs + b;
    const double ut = mine ? d.b_ut[oo] : 0.0, xp = mine ? d.b_x[oo] : 0.0, q = mine ? bq_at<PQ>(d, row, oo) : 0.0;
    const bool frozen = mine ? d.c_done[b] != 0 : true;
    // the variable's own bound row (identity rows, see above): its operands are requested before the sweep too
    const int pos = (mine && d.wh_m < d.M) ? d.int_pos[row] : -1;
    const size_t oj = pos >= 0 ? (size_t)(d.m_orig + pos) * Bs + b : 0;             // row of z, y, l, u, dy
    const size_t ow = pos >= 0 ? whrow(d, d.m_orig + pos) * Bs + b : 0;             // its wh entry
    double zp = 0, yp = 0, whp = 0, lo = 0, up = 0, aj = 0;
    if (pos >= 0 && !frozen) { zp = d.b_z[oj]; yp = d.b_y[oj]; whp = d.b_wh[ow]; lo = d.b_l[oj]; up = d.b_u[oj]; aj = d.a_int[row]; }
    bm_tile<KS, DEPTH>(d.LinvT, d.ld, d.n, row0, row0 + 1, d.n, d.b_ut + col0, Bs, d.b_zero, acc);
    const double s = bm_reduce<KS>(acc, lds, o);
    if (!mine) return;
    const double xt = ut + s;
    d.b_xt[oo] = xt;
    if (!frozen) {
      const double xn = alpha * xt + (1.0 - alpha) * xp;
      d.b_x[oo] = xn;
      d.b_dx[oo] = xn - xp;
      double rx = d.sigma * xn - q;
      if (pos >= 0) {
        const double nu = -rho * whp + aj * xt;  // aj = rho a_j
        const double zt = zp + rinv * (nu - yp);
        const double zr = alpha * zt + (1.0 - alpha) * zp;
        const double v = zr + rinv * yp;
        const double zn = fmin(fmax(v, lo), up);
        const double dy = rho * (zr - zn);
        const double yn = yp + dy;
        const double whn = zn - rinv * yn;
        d.b_z[oj] = zn;
        d.b_y[oj] = yn;
        d.b_dy[oj] = dy;
        d.b_wh[ow] = whn;
        rx += aj * whn;  // r~ = rx + t
      }
      d.b_rx[oo] = rx;
    }
    return;
  }
  const int row0 = (rb - nbx) * 16, row = row0 + o.row;
  const bool mine = out && row < d.wh_m && !d.c_done[b];
  const size_t oo = (size_t)row * Bs + b;  // general rows: wh sits at its own row index
  double zp = 0, yp = 0, whp = 0, lo = 0, up = 0;
  if (mine) { zp = d.b_z[oo]; yp = d.b_y[oo]; whp = d.b_wh[oo]; lo = d.b_l[oo]; up = d.b_u[oo]; }
  bm_tile<KS, DEPTH>(d.f_GmT, d.ldn, d.M, row0, 0, d.n, d.b_ut + col0, Bs, d.b_zero, acc);
  const double s = bm_reduce<KS>(acc, lds, o);
  if (!mine) return;
  const double nu = -rho * whp + s;
  const double zt = zp + rinv * (nu - yp);
  const double zr = alpha * zt + (1.0 - alpha) * zp;
  const double v = zr + rinv * yp;
  const double zn = fmin(fmax(v, lo), up);
  const double dy = rho * (zr - zn);
  const double yn = yp + dy;
  d.b_z[oo] = zn;
  d.b_y[oo] = yn;
  d.b_dy[oo] = dy;
  d.b_wh[oo] = zn - rinv * yn;
}

// column-wise reductions: 1024 threads = 64 columns x 16 row groups; fixed order
#define COLRED(name, OP, init)                                                          \
  __device__ __forceinline__ double name(double v, double *lds, int bl, int rg) {       \
    __syncthreads();                                                                    \
    lds[rg * 64 + bl] = v;                                                              \
    __syncthreads();                                                                    \
    double r = lds[bl];                                                                 \
    for (int w = 1; w < 16; w++) r = OP(r, lds[w * 64 + bl]);                           \
    return r;                                                                           \
  }
__device__ __forceinline__ double op_add(double a, double b) { return a + b; }
COLRED(colred_max, fmax, 0)
COLRED(colred_sum, op_add, 0)

// batched termination test on the dense copies, same matrix-core tiles as the sweeps
constexpr int BMC_KS = 8, BMC_DEPTH = 2;  // the test's tiles: two products per workgroup, short K
__global__ __launch_bounds__(BMC_KS * 64, 2) void kbm_check_con(Dev d, int ncol) {
  if (d.ctrl->done) return;
  __shared__ double lds[BMC_KS * BM_NT * 256];
  int rb, cb;
  if (!bm_place((d.M + 15) / 16, ncol, rb, cb)) return;
  const size_t Bs = (size_t)d.Bs, MB = (size_t)d.M * Bs;
  const int row0 = rb * 16, col0 = cb * BM_COLS;
  const BmOut bo = bm_out(threadIdx.x);
  const int row = row0 + bo.row, b = col0 + bo.col;
  double4_t acc[BM_NT];
  bm_tile<BMC_KS, BMC_DEPTH>(d.f_Ad, d.ldn, d.M, row0, 0, d.n, d.b_x + col0, Bs, d.b_zero, acc);
  const double ax = bm_reduce<BMC_KS>(acc, lds, bo);
  __syncthreads();
  bm_tile<BMC_KS, BMC_DEPTH>(d.f_Ad, d.ldn, d.M, row0, 0, d.n, d.b_dx + col0, Bs, d.b_zero, acc);
  const double adx0 = bm_reduce<BMC_KS>(acc, lds, bo);
  if ((int)threadIdx.x >= BM_OUT || row >= d.M) return;
  const size_t o = row * Bs + b;
  const double ei = d.Einv[row], z = d.b_z[o], l = d.b_l[o], u = d.b_u[o];
  const bool uinf = u > QP_INFTY * QP_MIN_SCALING, linf = l < -QP_INFTY * QP_MIN_SCALING;
  double v = d.b_dy[o];
  if (uinf && linf) v = 0.0;
  else if (uinf) v = fmin(v, 0.0);
  else if (linf) v = fmax(v, 0.0);
  const double adx = ei * adx0;
  d.b_sm[0 * MB + o] = ei * (ax - z);
  d.b_sm[1 * MB + o] = ei * ax;
  d.b_sm[2 * MB + o] = ei * z;
  d.b_sm[3 * MB + o] = v;
  d.b_sm[4 * MB + o] = d.E[row] * v;
  d.b_sm[5 * MB + o] = u * fmax(v, 0.0) + l * fmin(v, 0.0);
  d.b_sm[6 * MB + o] = uinf ? -1.7e308 : adx;
  d.b_sm[7 * MB + o] = linf ? 1.7e308 : adx;
}

// blocks [0, nbx): rows of Pbar against x, dx; blocks [nbx, 2 nbx): rows of Abar^T against y, projected dy
__global__ __launch_bounds__(BMC_KS * 64, 2) void kbm_check_var(Dev d, int ncol) {
  if (d.ctrl->done) return;
  __shared__ double lds[BMC_KS * BM_NT * 256];
  const size_t Bs = (size_t)d.Bs, NB = (size_t)d.n * Bs;
  const int nbx = (d.n + 15) / 16;
  int rb, cb;
  if (!bm_place(2 * nbx, ncol, rb, cb)) return;
  const bool second = rb >= nbx;
  const int row0 = (rb - (second ? nbx : 0)) * 16, col0 = cb * BM_COLS;
  const BmOut bo = bm_out(threadIdx.x);
  const int row = row0 + bo.row, b = col0 + bo.col;
  double4_t acc[BM_NT];
  const double *A = second ? d.f_Atd : d.f_Pd;
  const int ld = second ? d.ldm : d.ldn, K = second ? d.M : d.n;
  const double *V0 = (second ? d.b_y : d.b_x) + col0;
  const double *V1 = (second ? d.b_sm + 3 * (size_t)d.M * Bs : d.b_dx) + col0;
  bm_tile<BMC_KS, BMC_DEPTH>(A, ld, d.n, row0, 0, K, V0, Bs, d.b_zero, acc);
  const double r0 = bm_reduce<BMC_KS>(acc, lds, bo);
  __syncthreads();
  bm_tile<BMC_KS, BMC_DEPTH>(A, ld, d.n, row0, 0, K, V1, Bs, d.b_zero, acc);
  const double r1 = bm_reduce<BMC_KS>(acc, lds, bo);
  if ((int)threadIdx.x >= BM_OUT || row >= d.n) return;
  const size_t o = row * Bs + b;
  d.b_sn[(second ? 2 : 0) * NB + o] = r0;
  d.b_sn[(second ? 3 : 1) * NB + o] = d.Dinv[row] * r1;
}

// Stage 1 of the batched decision: grid (column tiles, KR row slices); every workgroup folds its
// slice of rows for 64 columns and 17 quantities into b_part[tile][slice][q][64].
constexpr int KR = 32;
template <bool PQ>
__global__ __launch_bounds__(256) void kb_check_reduce(Dev d) {
  if (d.ctrl->done) return;
  __shared__ double part[NQ][4][64];
  const int n = d.n, M = d.M, tid = threadIdx.x, bl = tid & 63, rg = tid >> 6;
  const int b = blockIdx.x * 64 + bl, sl = blockIdx.y;
  const size_t Bs = (size_t)d.Bs, MB = (size_t)M * Bs, NB = (size_t)n * Bs;
  double v[NQ];
#pragma unroll
  for (int q = 0; q < NQ; q++) v[q] = 0.0;
  v[4] = -1.7e308;
  v[5] = -1.7e308;
  for (int j = sl * 4 + rg; j < M; j += 4 * KR) {
    const size_t o = j * Bs + b;
    v[0] = fmax(v[0], fabs(d.b_sm[0 * MB + o]));
    v[1] = fmax(v[1], fabs(d.b_sm[1 * MB + o]));
    v[2] = fmax(v[2], fabs(d.b_sm[2 * MB + o]));
    v[3] = fmax(v[3], fabs(d.b_sm[4 * MB + o]));
    v[4] = fmax(v[4], d.b_sm[6 * MB + o]);
    v[5] = fmax(v[5], -d.b_sm[7 * MB + o]);
    v[13] += d.b_sm[5 * MB + o];
  }
  for (int i = sl * 4 + rg; i < n; i += 4 * KR) {
    const size_t o = i * Bs + b;
    const double di = d.Dinv[i], px = d.b_sn[0 * NB + o], aty = d.b_sn[2 * NB + o], q = bq_at<PQ>(d, i, o), x = d.b_x[o],
                 dx = d.b_dx[o];
    v[6] = fmax(v[6], fabs(di * (px + q + aty)));
    v[7] = fmax(v[7], fabs(di * px));
    v[8] = fmax(v[8], fabs(di * aty));
    v[9] = fmax(v[9], fabs(di * q));
    v[10] = fmax(v[10], fabs(d.b_sn[1 * NB + o]));
    v[11] = fmax(v[11], fabs(d.b_sn[3 * NB + o]));
    v[12] = fmax(v[12], fabs(d.D[i] * dx));
    v[14] += q * dx;
    v[15] += x * px;
    v[16] += q * x;
  }
#pragma unroll
  for (int q = 0; q < NQ; q++) part[q][rg][bl] = v[q];
  __syncthreads();
  if (rg != 0) return;
  double *out = d.b_part + ((size_t)(blockIdx.x * KR + sl) * NQ) * 64;
#pragma unroll
  for (int q = 0; q < NQ; q++) {
    double r = part[q][0][bl];
#pragma unroll
    for (int w = 1; w < 4; w++) r = q < NQ_MAX ? fmax(r, part[q][w][bl]) : r + part[q][w][bl];
    out[q * 64 + bl] = r;
  }
}

// Stage 2: one workgroup per column tile: four waves fold eight slices each (in slice order), wave 0 adds the four
// partial results in order and decides.  (One wave walking all 32 slices was 14-16 us of dependent round trips.)
__global__ __launch_bounds__(256) void kb_check_decide(Dev d) {
  // pad: the chunk's persistent launch (kbp) was called off and iterated nothing -- no decision on a chunk that did not
  // happen (a freshly loaded column would pass the residual test on its warm start); the host repeats it as launches
  if (d.ctrl->done || d.ctrl->pad) return;
  __shared__ double part[3][NQ][64];
  const int bl = threadIdx.x & 63, wg = threadIdx.x >> 6, b = blockIdx.x * 64 + bl;
  double v[NQ];
  const double *in = d.b_part + ((size_t)blockIdx.x * KR * NQ) * 64 + (size_t)(wg * (KR / 4)) * NQ * 64;
#pragma unroll
  for (int q = 0; q < NQ; q++) v[q] = in[q * 64 + bl];
#pragma unroll 4
  for (int sl = 1; sl < KR / 4; sl++) {
    const double *p = in + (size_t)sl * NQ * 64;
    double t[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) t[q] = p[q * 64 + bl];
#pragma unroll
    for (int q = 0; q < NQ; q++) v[q] = q < NQ_MAX ? fmax(v[q], t[q]) : v[q] + t[q];
  }
  if (wg > 0) {
#pragma unroll
    for (int q = 0; q < NQ; q++) part[wg - 1][q][bl] = v[q];
  }
  __syncthreads();
  if (wg > 0) return;
#pragma unroll
  for (int g = 0; g < 3; g++) {
#pragma unroll
    for (int q = 0; q < NQ; q++) v[q] = q < NQ_MAX ? fmax(v[q], part[g][q][bl]) : v[q] + part[g][q][bl];
  }
  Norms nm{v[0], v[1], v[2], v[3], v[4], -v[5], v[6] * d.cinv, v[7], v[8], v[9], v[10], v[11], v[12], v[13], v[14],
           v[15], v[16]};
  Ctrl *c = d.ctrl;
  bool newly = false;
  if (!d.c_done[b]) {
    double obj;
    int st = decide_status(d, nm, obj);
    // streaming batch: a column counts from the chunk it was loaded in and reaches max_iter on its own
    const int it = d.stream ? c->iter - d.c_start[b] : c->iter;  // kb_tick already counted this chunk
    if (d.stream && !st && it >= d.max_iter_s) st = MIOSQP_QP_MAX_ITER_REACHED;
    d.c_pri[b] = nm.pri;
    d.c_dua[b] = nm.dua;
    d.c_obj[b] = obj;
    if (st) {
      d.c_status[b] = st;
      d.c_iter[b] = it;
      d.c_done[b] = 1;
      newly = true;
    }
  }
  if (d.stream) return;  // nobody waits for "all columns decided" there
  const int cnt = __popcll(__ballot(newly));
  if (bl == 0 && cnt > 0) {
    const int before = atomicAdd(&c->ndone, cnt);
    if (before + cnt >= c->B) c->done = 1;
  }
}

// first kernel of a batched chunk: counts the chunk's iterations unless everything is decided
__global__ void kb_tick(Dev d, int iters_in_chunk) {
  if (!d.ctrl->done) d.ctrl->iter += iters_in_chunk;
}

__global__ void kb_reset(Dev d, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < d.Bs) {
    d.c_done[b] = b >= B;
    d.c_node[b] = b;
    d.c_status[b] = MIOSQP_QP_UNSOLVED;
    d.c_iter[b] = 0;
    d.c_pri[b] = d.c_dua[b] = d.c_obj[b] = 0.0;
    d.c_lower[b] = __builtin_nan("");
  }
  if (b == 0) {
    Ctrl *c = d.ctrl;
    c->done = 0;
    c->status = MIOSQP_QP_UNSOLVED;
    c->iter = 0;
    c->pad = 0;
    c->B = B;
    c->ndone = 0;
  }
}

// node-major staging -> scaled, batch-fastest working vectors (block = 64 columns x 4 rows).  PQ: the columns' scaled costs
// (instance-major b_qs, from k_scale_q_batch) are laid out batch-fastest in b_q on the way; padding columns get a zero cost
template <bool PQ>
__global__ __launch_bounds__(256) void kb_prepare(Dev d, int B) {
  const int lane = threadIdx.x & 63, b = blockIdx.y * 64 + lane;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  const size_t Bs = (size_t)d.Bs, n = d.n, M = d.M;
  const bool act = b < B;
  const double *rl = d.b_raw, *ru = rl + (size_t)B * M, *rx = ru + (size_t)B * M, *ry = rx + (size_t)B * n;
  if (j < d.M) {
    const size_t o = j * Bs + b;
    d.b_l[o] = act ? d.E[j] * fmax(rl[(size_t)b * M + j], -QP_INFTY) : 0.0;
    d.b_u[o] = act ? d.E[j] * fmin(ru[(size_t)b * M + j], QP_INFTY) : 0.0;
    d.b_y[o] = act ? d.c * d.Einv[j] * ry[(size_t)b * M + j] : 0.0;
    d.b_dy[o] = 0.0;
  }
  if (j < d.n) {
    const size_t o = j * Bs + b;
    const double xs = act ? d.Dinv[j] * rx[(size_t)b * n + j] : 0.0;
    d.b_x[o] = xs;
    d.b_dx[o] = 0.0;
    if constexpr (PQ) {
      const double qs = act ? d.b_qs[(size_t)b * n + j] : 0.0;
      d.b_q[o] = qs;
      d.b_rx[o] = d.sigma * xs - qs;
    } else {
      d.b_rx[o] = d.sigma * xs - d.q[j];
    }
  }
}

__global__ __launch_bounds__(256) void kb_warm_z(Dev d) {
  BSETUP
  const int row = blockIdx.x * 4 + wv;
  if (row >= d.M) return;
  const double z = brow_dot(d.pc_idx, d.pc_A, d.pc_ptr[row], d.pc_ptr[row + 1], d.b_x + b, Bs);
  const size_t o = row * Bs + b;
  const double wh = z - d.rho_inv * d.b_y[o];
  d.b_z[o] = z;
  d.b_wh[whrow(d, row) * Bs + b] = wh;
  if (row >= d.wh_m) {  // a bound row taken out of the products: its share of the right-hand side, r~ = rx + t
    const int i = d.i_idx[row - d.m_orig];
    d.b_rx[(size_t)i * Bs + b] += d.a_int[i] * wh;  // kb_prepare wrote rx in the launch before; one row per variable
  }
}

// Compaction of a wave: decided columns are swapped towards the tail so that the columns still
// iterating fill the first tiles and later chunks launch fewer tiles.  grid (row chunks, pairs).  PQ: the column's scaled
// cost moves with its iterates (its raw cost stays where it is: kb_obj_rows finds it through c_node).
template <bool PQ>
__global__ __launch_bounds__(256) void kb_swap_cols(Dev d, int npairs) {
  const int p = blockIdx.y;
  if (p >= npairs) return;
  const int a = d.c_pairs[2 * p], b = d.c_pairs[2 * p + 1];
  const size_t Bs = (size_t)d.Bs;
  const int r = blockIdx.x * 256 + threadIdx.x;
#define SWAPROW(arr, rows)                                  \
  if (r < (rows)) {                                         \
    const double t_ = arr[r * Bs + a];                      \
    arr[r * Bs + a] = arr[r * Bs + b];                      \
    arr[r * Bs + b] = t_;                                   \
  }
  SWAPROW(d.b_l, d.M) SWAPROW(d.b_u, d.M) SWAPROW(d.b_z, d.M) SWAPROW(d.b_y, d.M) SWAPROW(d.b_dy, d.M)
  SWAPROW(d.b_wh, d.M + d.n)  // wh | rx
  SWAPROW(d.b_x, d.n) SWAPROW(d.b_dx, d.n)
  if constexpr (PQ) { SWAPROW(d.b_q, d.n) }
#undef SWAPROW
  if (r == 0) {
#define SWAP1(T, arr) { const T t_ = arr[a]; arr[a] = arr[b]; arr[b] = t_; }
    SWAP1(int, d.c_done) SWAP1(int, d.c_status) SWAP1(int, d.c_iter) SWAP1(int, d.c_node)
    SWAP1(double, d.c_pri) SWAP1(double, d.c_dua) SWAP1(double, d.c_obj)
#undef SWAP1
  }
}

// unscale (or build the certificate) per column, then the integer clamp of node.py:131-136
__global__ __launch_bounds__(1024) void kb_finish(Dev d, int B) {
  __shared__ double lds[16 * 64];
  const int n = d.n, M = d.M, tid = threadIdx.x, bl = tid & 63, rg = tid >> 6;
  const int b = blockIdx.x * 64 + bl;
  const size_t Bs = (size_t)d.Bs;
  if (d.stream && !d.t_has[blockIdx.x]) return;  // streaming batch: no column of this tile was decided in this chunk
  const bool live = d.stream ? d.c_harv[b] != 0 : b < B;
  int st = d.c_status[b];
  if (st == MIOSQP_QP_UNSOLVED) st = MIOSQP_QP_MAX_ITER_REACHED;
  double ndy = 0, ndx = 0;
  for (int j = rg; j < M; j += 16) ndy = fmax(ndy, fabs(d.E[j] * d.b_dy[j * Bs + b]));
  for (int i = rg; i < n; i += 16) ndx = fmax(ndx, fabs(d.D[i] * d.b_dx[i * Bs + b]));
  ndy = colred_max(ndy, lds, bl, rg);
  ndx = colred_max(ndx, lds, bl, rg);
  const double nan = __builtin_nan("");
  for (int i = rg; i < n; i += 16) {
    const size_t o = i * Bs + b;
    double v;
    if (st == MIOSQP_QP_PRIMAL_INFEASIBLE) v = nan;
    else if (st == MIOSQP_QP_DUAL_INFEASIBLE) v = d.D[i] * d.b_dx[o] / ndx;
    else v = d.D[i] * d.b_x[o];
    d.b_xfin[o] = v;
  }
  for (int j = rg; j < M; j += 16) {
    const size_t o = j * Bs + b;
    double v;
    if (st == MIOSQP_QP_PRIMAL_INFEASIBLE) v = d.E[j] * d.b_dy[o] / ndy;
    else if (st == MIOSQP_QP_DUAL_INFEASIBLE) v = nan;
    else v = d.cinv * d.E[j] * d.b_y[o];
    d.b_yfin[o] = v;
  }
  __syncthreads();
  if (live && (st == MIOSQP_QP_SOLVED || st == MIOSQP_QP_MAX_ITER_REACHED)) {
    const double *rl = d.b_raw, *ru = rl + (size_t)B * M;
    for (int k = rg; k < d.n_int; k += 16) {
      const size_t o = (size_t)d.i_idx[k] * Bs + b;
      const size_t nb_ = (size_t)d.c_node[b];  // the node this column holds (after compaction swaps) / its pool slot
      const double lo = d.stream ? d.pl_lo[nb_ * d.n_int + k] : rl[nb_ * M + d.m_orig + k];
      const double hi = d.stream ? d.pl_hi[nb_ * d.n_int + k] : ru[nb_ * M + d.m_orig + k];
      d.b_xfin[o] = fmin(fmax(d.b_xfin[o], lo), hi);
    }
  }
  if (d.digest) {
    // per column: is_int_feas + pick_nextvar + rounded candidate (workspace.py:245-272)
    const bool okc = live && (st == MIOSQP_QP_SOLVED || st == MIOSQP_QP_MAX_ITER_REACHED);
    __syncthreads();
    for (int i = rg; i < n; i += 16) d.b_xi[i * Bs + b] = d.b_xfin[i * Bs + b];
    __syncthreads();
    int cnt = 0, bestk = 0x7fffffff;
    double best = -1.0;
    for (int k = rg; k < d.n_int; k += 16) {
      const size_t o = (size_t)d.i_idx[k] * Bs + b;
      const double v = d.b_xfin[o], r = rint(v), f = fabs(v - r);
      d.b_xi[o] = r;
      cnt += f > d.eps_int;
      if (f > best) { best = f; bestk = k; }
    }
    __syncthreads();
    lds[rg * 64 + bl] = best;
    __shared__ int lk[16 * 64], lc[16 * 64];
    lk[rg * 64 + bl] = bestk;
    lc[rg * 64 + bl] = cnt;
    __syncthreads();
    if (rg == 0) {
      for (int w = 1; w < 16; w++) {
        const double ob = lds[w * 64 + bl];
        const int ok = lk[w * 64 + bl];
        cnt += lc[w * 64 + bl];
        if (ob > best || (ob == best && ok < bestk)) { best = ob; bestk = ok; }
      }
      d.c_intinf[b] = okc ? cnt : -1;
      d.c_nextvar[b] = okc && bestk != 0x7fffffff ? bestk : -1;
    }
    for (int i = rg; i < n; i += 16) d.b_xis[i * Bs + b] = d.Dinv[i] * d.b_xi[i * Bs + b];
  }
  if (!d.stream && rg == 0 && d.c_status[b] == MIOSQP_QP_UNSOLVED) {
    d.c_status[b] = MIOSQP_QP_MAX_ITER_REACHED;
    d.c_iter[b] = d.ctrl->iter;
  }
}

// rounding heuristic per column: rows of A against the rounded candidates (workspace.py:232-243)
__global__ __launch_bounds__(256) void kb_heur_rows(Dev d) {
  if (d.stream && !d.t_has[blockIdx.y]) return;
  BSETUP
  const int row = blockIdx.x * 4 + wv;
  if (row >= d.M) return;
  const double acc = brow_dot(d.pc_idx, d.pc_A, d.pc_ptr[row], d.pc_ptr[row + 1], d.b_xis + b, Bs);
  const double z = d.Einv[row] * acc;
  d.b_sm[row * Bs + b] = fmax(d.root_l[row] - d.eps_lin - z, z - d.root_u[row] - d.eps_lin);
}

// PQ: the raw cost of the node this column holds, instance-major b_qraw, through c_node (columns move when a wave is compacted)
template <bool PQ>
__global__ __launch_bounds__(256) void kb_obj_rows(Dev d) {
  if (d.stream && !d.t_has[blockIdx.y]) return;
  BSETUP
  const int row = blockIdx.x * 4 + wv;
  if (row >= d.n) return;
  double qr;
  if constexpr (PQ) qr = d.b_qraw[(size_t)d.c_node[b] * d.n + row];
  else qr = d.qraw[row];
  double acc, acc2;
  brow_dot2(d.pr_idx, d.pr_val, d.pr_ptr[row], d.pr_ptr[row + 1], d.b_xfin + b, (d.digest ? d.b_xi : d.b_xfin) + b, Bs,
            acc, acc2);
  d.b_sn[row * Bs + b] = d.b_xfin[row * Bs + b] * (0.5 * acc + qr);
  if (d.digest) d.b_sn[(size_t)d.n * Bs + row * Bs + b] = d.b_xi[row * Bs + b] * (0.5 * acc2 + qr);
}

__global__ __launch_bounds__(1024) void kb_obj_sum(Dev d) {
  if (d.stream && !d.t_has[blockIdx.x]) return;
  __shared__ double lds[16 * 64];
  const int tid = threadIdx.x, bl = tid & 63, rg = tid >> 6, b = blockIdx.x * 64 + bl;
  const size_t Bs = (size_t)d.Bs;
  double s = 0, s2 = 0, vmax = -1.7e308;
  for (int i = rg; i < d.n; i += 16) s += d.b_sn[i * Bs + b];
  s = colred_sum(s, lds, bl, rg);
  if (d.digest) {
    for (int i = rg; i < d.n; i += 16) s2 += d.b_sn[(size_t)d.n * Bs + i * Bs + b];
    for (int j = rg; j < d.M; j += 16) vmax = fmax(vmax, d.b_sm[j * Bs + b]);
    s2 = colred_sum(s2, lds, bl, rg);
    vmax = colred_max(vmax, lds, bl, rg);
  }
  if (rg == 0) {
    const int st = d.c_status[b];
    const bool ok = st == MIOSQP_QP_SOLVED || st == MIOSQP_QP_MAX_ITER_REACHED;
    d.c_lower[b] = ok ? s : __builtin_nan("");
    d.c_hobj[b] = ok && d.digest ? s2 : __builtin_nan("");
    d.c_hviol[b] = ok && d.digest ? vmax : __builtin_nan("");
  }
}

// batch-fastest answers -> node-major staging out
__global__ __launch_bounds__(256) void kb_export(Dev d, int B) {
  const int lane = threadIdx.x & 63, b = blockIdx.y * 64 + lane;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const size_t Bs = (size_t)d.Bs, n = d.n, M = d.M;
  double *ox = d.b_out, *oy = ox + (size_t)B * n;
  if (j < d.n) ox[(size_t)b * n + j] = d.b_xfin[j * Bs + b];
  if (j < d.M) oy[(size_t)b * M + j] = d.b_yfin[j * Bs + b];
}
