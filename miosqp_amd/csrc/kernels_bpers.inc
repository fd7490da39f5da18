// part of engine.hip (included there, not compiled alone): a whole chunk of lock-step batched iterations in ONE launch
// ------------------------------------------------------------------------------------------
// kbp: the matrix-core sweeps of kernels_batched.inc (kbm_fwd / kbm_bwd) as a persistent kernel with the factor in
// registers and LDS.  Two launches per lock-step iteration cost ~5 us each at 256 columns, where a sweep holds 6 us of
// matrix-core work (DESIGN.md sec. 3e): fifty kernel boundaries per 25-iteration chunk are a third of the chunk.
//
// Grid = 256 workgroups of 512 threads = 8 column groups x 32 members, group g = blockIdx % 8 (workgroups are dealt to
// the XCDs round robin, so a group's members share one L2: used for speed only, correctness does not depend on it).
// A group owns the 32-column tiles g, g + 8, ... of the batch.  Member m owns, for the whole launch,
//   rows 16 m .. 16 m + 15 of the forward factor  [ -G(general rows) | strict_lower(Linv) ]   (kbm_fwd's row block m),
//   rows 16 m .. 16 m + 15 of strict_upper(Linv^T)                                             (kbm_bwd's x block m),
//   rows 16 m .. and 16 (m + 32) .. of (-G)^T                                                   (kbm_bwd's constraint blocks),
// as matrix-core A fragments: the first two in registers (64 doubles per lane), the constraint blocks in LDS (128 KB).
// Eight groups hold eight copies of the factor (12 MB each) in 256 CUs' registers and LDS; what travels per iteration
// is the right-hand side only: ut (n x 32 per tile) and [wh | r~] ((m + n) x 32) through L2 with agent-scope loads and
// stores, two group barriers per iteration (one counter per group, 32 arrivals).
//
// Arithmetic: the chunk-to-wave assignment, the four accumulator chains, the reduction order over the waves and the
// epilogues are those of bm_tile / kbm_fwd / kbm_bwd (chunks beyond a block's extent add zero products: an accumulator
// that starts at +0 never holds -0), so a chunk through kbp leaves the same bits as the same chunk through the launches
// (tests/test_gpu_parity.py::test_batched_persistent_chunks_equal_the_launches, ..._over_shapes).
// Limits (host: kbp_capable): n <= 512, rows in the products wh_m <= 1024, wh_m + n <= 1536, one workgroup per CU on a
// device with >= 256 CUs.  Registration as for k_coop / k_pers: nobody depends on anybody before all 256 workgroups
// are resident; called off (ctrl->pad = 1, nothing modified) when they are not within 100 ms -- the host then runs the
// chunk through the launches, keeps to them for a while and tries the persistent launch again later (host.inc: kbp_leave,
// maybe_rejoin_kbp).
// Where the time goes (tools/probes/kbp_phases.py, config 3, 256 columns: 18.1 us per iteration against 30.4 for the
// launches; matrix-core floor 10.2): forward sweep 5.3 us (every member runs all twelve chunks per wave: at the
// matrix-core bound), the three backward tiles 9.0 (short sweeps: four exposed pipeline fills and reductions), the two
// group barriers 1.2 + 1.7 (latency: the members arrive together).
// The sweeps are STRAIGHT-LINE: a chunk beyond a row block's extent is not skipped, its (zero) fragment multiplies
// chunk 0 of the array again.  Skipping them -- a wave-uniform branch per chunk -- looked like 17 % less matrix-core
// work and cost 6 us per iteration (24.5): the members' K extents differ (1016 .. 1512), the barrier waits for the
// longest anyway, and the branches cut the unrolled sweep into blocks the scheduler no longer overlaps.
// Tried and not kept: arrival words per member instead of the counter (no faster); no barrier at all -- an epoch word
// per 16-row block, every sweep waiting for exactly the blocks it is about to load (correct, same bits, slower: a block
// that is not there yet costs two dependent round trips instead of one); the first chunk of the next sweep requested
// before the reduction of the tile at hand (16 more live registers: more spills); one wave per SIMD playing two of the
// eight k-slices with 512 registers per lane (tools/probes/kbr_probe2.hip: 19.7 us against 25.4 on synthetic data; as a
// real kernel with per-slice branches 30.4); 8-byte agent-scope loads / stores (0.54-0.70 of the 16-byte rate; an 8-byte
// write-through store is a fabric write of its own); a branch per fragment entry in the prologue (60 us per launch).
// ------------------------------------------------------------------------------------------
constexpr int KBP_KS = 8, KBP_FC = 12, KBP_BC = 4, KBP_G = 8, KBP_MEMBERS = 32, KBP_WGS = KBP_G * KBP_MEMBERS;
constexpr int KBP_LDS_DOUBLES = KBP_KS * 512 + 2 * KBP_BC * 4 * 512;

struct KbpArgs {
  unsigned long long *reg;  // registration words (pers_register's layout: count | +16 go | +32 called off)
  unsigned long long *bar;  // group barrier counters, 16 words apart
  int ncol;                 // 32-column tiles in use
  int iters;                // lock-step iterations of this launch
};

__device__ __forceinline__ double kbp_ld(const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void kbp_st(double *p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// all 256 workgroups resident, the group counters zeroed by workgroup 0 before it says so
__device__ __forceinline__ void kbp_register(const KbpArgs &ka, Ctrl *ctrl, int *s_fail) {
  if (threadIdx.x == 0) {
    *s_fail = 0;
    const unsigned G = gridDim.x;
    const unsigned long long old = __hip_atomic_fetch_add(ka.reg, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long target = (old / G + 1ull) * G;
    unsigned spins = 0;
    unsigned long long since = 0;
    if (blockIdx.x == 0) {
      for (;;) {
        if (__hip_atomic_load(ka.reg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= target) {
          for (int g = 0; g < KBP_G; g++) __hip_atomic_store(ka.bar + 16 * g, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          __hip_atomic_store(ka.reg + 16, target, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
          break;
        }
        if (coop_expired(spins, since, COOP_LIMIT_REGISTER)) {
          __hip_atomic_store(ka.reg + 32, target, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          *s_fail = 1;
          ctrl->pad = 1;
          break;
        }
      }
    } else {
      for (;;) {
        if (__hip_atomic_load(ka.reg + 16, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == target) break;
        if (__hip_atomic_load(ka.reg + 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == target) {
          *s_fail = 1;
          break;
        }
        if (coop_expired(spins, since)) {
          *s_fail = 1;
          ctrl->pad = 6;
          break;
        }
      }
    }
  }
  __syncthreads();
}

// the group's 32 members meet: every store of the phase acknowledged, then one arrival per workgroup on the group's
// counter (zeroed by workgroup 0 at registration).  Arrival words per member, polled 32 at a time, were tried: no faster.
// Returns true when the wait ran out (2 s: a lost workgroup; reported through ctrl->pad, the launch gives up)
__device__ __forceinline__ bool kbp_barrier(unsigned long long *ctr, unsigned long long target, int *flag, Ctrl *ctrl, int stage) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __hip_atomic_fetch_add(ctr, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned spins = 0;
    unsigned long long since = 0;
    int f = 0;
    while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
      __builtin_amdgcn_s_sleep(1);
      if (coop_expired(spins, since)) {
        f = 1;
        ctrl->pad = stage;
        break;
      }
    }
    *flag = f;
  }
  __syncthreads();
  const int f = *flag;
  __syncthreads();  // (the word lies in the reduction buffer)
  return f != 0;
}

// One sweep of NCH chunks per wave with the A fragments at hand: chunk c of wave w is rows k0 + 16 (w + 8 c) .. + 15 of the
// right-hand array, as in bm_tile; `nch` of them lie below the sweep's end (wave-uniform); the others, zeros times zeros in
// bm_tile, multiply their zero fragment with rows 0 .. 15 of the array (finite, in range) -- no branch in the sweep.
// V: buffer descriptor of the right-hand array, voff: this lane's byte offset of (row 4 j, column col0 + 2 r) in it.
// 16-byte loads, agent scope (sc1: served by L2, past this CU's L1).
typedef unsigned kbp_u4 __attribute__((ext_vector_type(4)));
template <int NCH, class AF>
__device__ __forceinline__ void kbp_sweep(AF a, __amdgpu_buffer_rsrc_t V, unsigned voff, unsigned rowbytes, int k0, int nch, int w,
                                          double4_t (&acc)[2]) {
  double4_t acc2[2];
#pragma unroll
  for (int t = 0; t < 2; t++) {
    acc[t] = (double4_t){0.0, 0.0, 0.0, 0.0};
    acc2[t] = (double4_t){0.0, 0.0, 0.0, 0.0};
  }
  double2 b[2][4];
  // opaque per call: the per-chunk offsets would otherwise be hoisted out of the loop of iterations and kept in registers
  asm volatile("" : "+v"(voff));
  // straight-line: a chunk beyond the end loads chunk 0 of the array again (finite values) against its zero fragment
  auto fetch = [&](int c, int slot) {
    const unsigned o = voff + (c < nch ? (unsigned)(k0 + 16 * (w + KBP_KS * c)) * rowbytes : 0u);
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const kbp_u4 v = __builtin_amdgcn_raw_buffer_load_b128(V, o + (unsigned)q * rowbytes, 0, 16);
      b[slot][q] = __builtin_bit_cast(double2, v);
    }
  };
  fetch(0, 0);
#pragma unroll
  for (int c = 0; c < NCH; c++) {
    {
    const int s = c & 1;
    if (c + 1 < NCH) fetch(c + 1, s ^ 1);
    __builtin_amdgcn_sched_barrier(0);
    const double a0 = a(c, 0), a1 = a(c, 1), a2 = a(c, 2), a3 = a(c, 3);
    acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b[s][0].x, acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b[s][0].y, acc[1], 0, 0, 0);
    acc2[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b[s][1].x, acc2[0], 0, 0, 0);
    acc2[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b[s][1].y, acc2[1], 0, 0, 0);
    acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, b[s][2].x, acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, b[s][2].y, acc[1], 0, 0, 0);
    acc2[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a3, b[s][3].x, acc2[0], 0, 0, 0);
    acc2[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a3, b[s][3].y, acc2[1], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    }
  }
  acc[0] += acc2[0];
  acc[1] += acc2[1];
}
// chunks of wave w below `kend` when chunk c starts at k0 + 16 (w + 8 c)
__device__ __forceinline__ int kbp_nch(int k0, int kend, int w) {
  const int left = kend - k0 - 16 * w;  // rows from this wave's first chunk to the end
  return left <= 0 ? 0 : (left + 16 * KBP_KS - 1) / (16 * KBP_KS);
}

// bm_reduce<8> for a workgroup whose 512 threads all own an output element; the buffer is free again on return
__device__ __forceinline__ double kbp_reduce(const double4_t (&acc)[2], double *lds, const BmOut &o) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int t = 0; t < 2; t++)
#pragma unroll
    for (int g = 0; g < 4; g++) lds[((w * 2 + t) * 4 + g) * 64 + lane] = acc[t][g];
  __syncthreads();
  const int idx = (o.t * 4 + o.g) * 64 + o.ll;
  double s = lds[idx];
#pragma unroll
  for (int ww = 1; ww < KBP_KS; ww++) s += lds[ww * 512 + idx];
  __syncthreads();
  return s;
}

// the member's fragments (bm_tile's addressing: rows beyond the end repeat the last one, their results are dropped).
// No branch around a load: a chunk beyond the end reads chunk 0 and is zeroed by a select -- with a branch per entry the
// 128 loads of a lane went out one round trip at a time (~60 us per launch).
__device__ __forceinline__ void kbp_frag4(const double *__restrict__ p, bool in, int kc, double (&f)[4]) {
  const double *q = p + (in ? kc : 0);
  const double2 v01 = *reinterpret_cast<const double2 *>(q), v23 = *reinterpret_cast<const double2 *>(q + 2);
  f[0] = in ? v01.x : 0.0;
  f[1] = in ? v01.y : 0.0;
  f[2] = in ? v23.x : 0.0;
  f[3] = in ? v23.y : 0.0;
}
__device__ __forceinline__ void kbp_fragments(const Dev &d, int m, int w, int r, int j, int kend_f, double (&af)[KBP_FC][4],
                                              double (&ab)[KBP_BC][4], double *la) {
  const int n = d.n, row0 = 16 * m;
  int row = row0 + r;
  row = row < n ? row : n - 1;
  const double *ap = d.f_rows2 + (size_t)row * d.ldf2 + 4 * j;
#pragma unroll
  for (int c = 0; c < KBP_FC; c++) {
    const int kc = 16 * (w + KBP_KS * c);
    kbp_frag4(ap, kc < kend_f, kc, af[c]);
  }
  const double *bp = d.LinvT + (size_t)row * d.ld + 4 * j;
#pragma unroll
  for (int c = 0; c < KBP_BC; c++) {
    const int kc = row0 + 16 * (w + KBP_KS * c);
    kbp_frag4(bp, kc < n, kc, ab[c]);
  }
#pragma unroll
  for (int t = 0; t < 2; t++) {
    int crow = 16 * (m + KBP_MEMBERS * t) + r;
    crow = crow < d.M ? crow : d.M - 1;
    const double *cp = d.f_GmT + (size_t)crow * d.ldn + 4 * j;
#pragma unroll
    for (int c = 0; c < KBP_BC; c++) {
      const int kc = 16 * (w + KBP_KS * c);
      double f[4];
      kbp_frag4(cp, kc < n, kc, f);
#pragma unroll
      for (int q = 0; q < 4; q++) la[((t * KBP_BC + c) * 4 + q) * 512 + threadIdx.x] = f[q];
    }
  }
}

// the value of the neighbouring lane (lane ^ 1): adjacent threads own adjacent columns of one row
__device__ __forceinline__ double kbp_neighbour(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, 0xB1, 0xf, 0xf, true);  // quad_perm [1, 0, 3, 2]
  hi = __builtin_amdgcn_update_dpp(0, hi, 0xB1, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
// two columns as ONE 16-byte agent-scope (write-through) store, issued by the even lane of the pair; byte offset `off` of the
// even column.  (An 8-byte sc1 store is a fabric write of its own: 2.7x the time per byte.)
__device__ __forceinline__ void kbp_st_pair(__amdgpu_buffer_rsrc_t rs, unsigned off, double mine, bool on) {
  const double other = kbp_neighbour(mine);
  if (on && !(threadIdx.x & 1)) {
    const double2 v = make_double2(mine, other);
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(kbp_u4, v), rs, off, 0, 16);
  }
}

// PROF (miosqp_qp_debug_timeline which = 5): shader clocks of thread 0 per phase, 16 words per workgroup in d.prof
// PQ: one linear cost per column (b_q, batch-fastest) instead of the engine's shared q
template <bool PROF, bool PQ = false>
__global__ __launch_bounds__(512) void kbp(Dev d, KbpArgs ka) {
  extern __shared__ __attribute__((aligned(16))) double kbp_smem[];
  double *lds = kbp_smem;                  // the reduction (and, between uses, the barrier's flag word)
  double *la = kbp_smem + KBP_KS * 512;    // constraint blocks m and m + 32 of (-G)^T as fragments: [tile][chunk][step][thread]
  int *s_flag = reinterpret_cast<int *>(lds);
  const int g = blockIdx.x & (KBP_G - 1), m = blockIdx.x >> 3;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), r = lane & 15, j = lane >> 4;
  const size_t Bs = (size_t)d.Bs;
  const int n = d.n, whm = d.wh_m;
  const BmOut o = bm_out(threadIdx.x);
  const int row0 = 16 * m;

  // an earlier launch of this engine was called off and the host has not acknowledged it yet (kbp_leave clears the
  // word): chunks queued behind it iterate nothing -- their tests decide nothing either (kb_check_decide) -- instead of
  // each trying the registration again (up to 100 ms apiece) and, should one succeed, iterating a chunk that is not tested
  if (d.ctrl->pad != 0) return;
  if ((d.coop_dbg & 64) && blockIdx.x == 1) return;  // fault injection (tests): one workgroup never shows up
  kbp_register(ka, d.ctrl, s_flag);
  const bool called_off = *s_flag != 0;
  __syncthreads();
  if (called_off) return;
  if (blockIdx.x == 0 && threadIdx.x == 0 && !d.ctrl->done) d.ctrl->iter += ka.iters;  // (kb_tick)

  int kend_f = whm + row0 + 16;
  if (kend_f > whm + n) kend_f = whm + n;
  double af[KBP_FC][4], ab[KBP_BC][4];
  kbp_fragments(d, m, w, r, j, kend_f, af, ab, la);
  const int xrow = row0 + o.row;
  const bool xmine = xrow < n;
  const double di = xmine ? d.d2inv[xrow] : 0.0, qx = xmine ? d.q[xrow] : 0.0;
  const int pos = (xmine && whm < d.M) ? d.int_pos[xrow] : -1;
  const double aj = pos >= 0 ? d.a_int[xrow] : 0.0;
  const double rho = d.rho, rinv = d.rho_inv, alpha = d.alpha, sigma = d.sigma;
  unsigned long long *ctr = ka.bar + 16 * g;
  unsigned long long target = 0;
  // the two right-hand arrays as buffers (16 rows of slack behind the last row read)
  const unsigned rowbytes = (unsigned)(Bs * sizeof(double));
  const __amdgpu_buffer_rsrc_t rs_wh = __builtin_amdgcn_make_buffer_rsrc((void *)d.b_wh, 0, (int)((unsigned)(d.M + n + 16) * rowbytes), 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_ut = __builtin_amdgcn_make_buffer_rsrc((void *)d.b_ut, 0, (int)((unsigned)(n + 16) * rowbytes), 0x00020000);
  const unsigned lane_off = (unsigned)(4 * j) * rowbytes + (unsigned)(2 * r) * (unsigned)sizeof(double);
  const int nch_f = kbp_nch(0, kend_f, w), nch_x = kbp_nch(row0, n, w), nch_c = kbp_nch(0, n, w);
  __syncthreads();

  long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  long long tc = PROF ? clock64() : 0;
#define KBP_PH(k)                                   \
  if (PROF) {                                       \
    const long long now = clock64();                \
    ph[k] += now - tc;                              \
    tc = now;                                       \
  }
  for (int it = 0; it < ka.iters; it++) {
    // ================= forward: ut = D22^-1 ( r~ + [ -G | strict_lower(Linv) ] [wh ; r~] ), row block m =================
    for (int cb = g; cb < ka.ncol; cb += KBP_G) {
      const int col0 = cb * BM_COLS, b = col0 + o.col;
      const size_t oo = (size_t)xrow * Bs + b;
      const double rx = xmine ? kbp_ld(d.b_rx + oo) : 0.0;  // requested before the sweep
      double4_t acc[2];
      kbp_sweep<KBP_FC>([&](int c, int q) { return af[c][q]; }, rs_wh, lane_off + (unsigned)col0 * 8u, rowbytes, 0, nch_f, w, acc);
      KBP_PH(0)
      const double s = kbp_reduce(acc, lds, o);
      if (xmine) kbp_st(d.b_ut + oo, di * (rx + s));
      KBP_PH(1)
    }
    target += KBP_MEMBERS;
    if (kbp_barrier(ctr, target, s_flag, d.ctrl, 2)) return;
    KBP_PH(2)
    // ================= backward: x~ = ut + strict_upper(Linv^T) ut; nu = -rho wh + (-G)^T ut; the vector updates =================
    for (int cb = g; cb < ka.ncol; cb += KBP_G) {
      const int col0 = cb * BM_COLS, b = col0 + o.col;
      const bool live = d.c_done[b] == 0;
      double4_t acc[2];
      {
        const size_t oo = (size_t)xrow * Bs + b;
        const double ut = xmine ? kbp_ld(d.b_ut + oo) : 0.0, xp = xmine ? d.b_x[oo] : 0.0;
        const double qc = PQ ? (xmine ? bq_at<PQ>(d, xrow, oo) : 0.0) : qx;  // this column block's cost, requested before the sweep
        const size_t oj = pos >= 0 ? (size_t)(d.m_orig + pos) * Bs + b : 0;  // the variable's own bound row: z, y, l, u, dy
        const size_t ow = pos >= 0 ? whrow(d, d.m_orig + pos) * Bs + b : 0;  // its wh entry
        double zp = 0, yp = 0, whp = 0, lo = 0, up = 0;
        if (pos >= 0 && live) { zp = d.b_z[oj]; yp = d.b_y[oj]; whp = kbp_ld(d.b_wh + ow); lo = d.b_l[oj]; up = d.b_u[oj]; }
        kbp_sweep<KBP_BC>([&](int c, int q) { return ab[c][q]; }, rs_ut, lane_off + (unsigned)col0 * 8u, rowbytes, row0, nch_x, w, acc);
        KBP_PH(3)
        const double s = kbp_reduce(acc, lds, o);
        if (xmine) {
          const double xt = ut + s;
          d.b_xt[oo] = xt;
          if (live) {
            const double xn = alpha * xt + (1.0 - alpha) * xp;
            d.b_x[oo] = xn;
            d.b_dx[oo] = xn - xp;
            double rx = sigma * xn - qc;
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
              kbp_st(d.b_wh + ow, whn);
              rx += aj * whn;  // r~ = rx + t
            }
            kbp_st(d.b_rx + oo, rx);
          }
        }
        KBP_PH(4)
      }
#pragma unroll
      for (int t = 0; t < 2; t++) {
        const int crow0 = 16 * (m + KBP_MEMBERS * t);
        if (crow0 >= whm) continue;  // (uniform over the workgroup)
        const int row = crow0 + o.row;
        const bool mine = row < whm && live;
        const size_t oo = (size_t)row * Bs + b;  // general rows: wh sits at its own row index
        double zp = 0, yp = 0, whp = 0, lo = 0, up = 0;
        if (mine) { zp = d.b_z[oo]; yp = d.b_y[oo]; whp = kbp_ld(d.b_wh + oo); lo = d.b_l[oo]; up = d.b_u[oo]; }
        kbp_sweep<KBP_BC>([&](int c, int q) { return la[((t * KBP_BC + c) * 4 + q) * 512 + threadIdx.x]; }, rs_ut,
                          lane_off + (unsigned)col0 * 8u, rowbytes, 0, nch_c, w, acc);
        const double s = kbp_reduce(acc, lds, o);
        if (mine) {
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
          kbp_st(d.b_wh + oo, zn - rinv * yn);
        }
      }
      KBP_PH(5)
    }
    target += KBP_MEMBERS;
    if (kbp_barrier(ctr, target, s_flag, d.ctrl, 3)) return;
    KBP_PH(6)
  }
#undef KBP_PH
  if (PROF && d.prof && threadIdx.x == 0) {
    for (int k = 0; k < 7; k++) d.prof[16 * blockIdx.x + k] = (unsigned long long)ph[k];
    d.prof[16 * blockIdx.x + 7] = (unsigned long long)ka.iters;
  }
}

// ------------------------------------------------------------------------------------------
// kbp1: the same for batches of at most 256 columns -- ONE 32-column tile per group, so every thread owns the same
// elements in every iteration (x-tile element (o.row, o.col) of block m, the bound row of that variable, one element of
// each of its two constraint blocks) and keeps them in REGISTERS for the whole launch: x, r~, the z / y / wh / l / u of its
// three rows.  Per iteration nothing is loaded but the right-hand sides of the sweeps, and nothing is stored but what the
// other members read (ut, wh, r~: agent-scope 16-byte stores, two columns per even lane); x, z, y and the last iteration's
// x~, dx, dy go to memory once, when the launch ends.  Same arithmetic, same bits as kbm_fwd / kbm_bwd.
// ------------------------------------------------------------------------------------------
template <bool PROF, bool PQ = false>
__global__ __launch_bounds__(512) void kbp1(Dev d, KbpArgs ka) {
  extern __shared__ __attribute__((aligned(16))) double kbp_smem[];
  double *lds = kbp_smem;
  double *la = kbp_smem + KBP_KS * 512;
  int *s_flag = reinterpret_cast<int *>(lds);
  const int g = blockIdx.x & (KBP_G - 1), m = blockIdx.x >> 3;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), r = lane & 15, j = lane >> 4;
  const size_t Bs = (size_t)d.Bs;
  const int n = d.n, whm = d.wh_m;
  const BmOut o = bm_out(threadIdx.x);
  const int row0 = 16 * m;

  // an earlier launch of this engine was called off and the host has not acknowledged it yet (kbp_leave clears the
  // word): chunks queued behind it iterate nothing -- their tests decide nothing either (kb_check_decide) -- instead of
  // each trying the registration again (up to 100 ms apiece) and, should one succeed, iterating a chunk that is not tested
  if (d.ctrl->pad != 0) return;
  if ((d.coop_dbg & 64) && blockIdx.x == 1) return;  // fault injection (tests): one workgroup never shows up
  // the fragments are requested before the registration: their 384 KB per workgroup travel while the grid assembles
  // (nothing here depends on anybody; a launch that is called off has read them for nothing)
  int kend_f = whm + row0 + 16;
  if (kend_f > whm + n) kend_f = whm + n;
  double af[KBP_FC][4], ab[KBP_BC][4];
  if (g < ka.ncol) kbp_fragments(d, m, w, r, j, kend_f, af, ab, la);
  kbp_register(ka, d.ctrl, s_flag);
  const bool called_off = *s_flag != 0;
  __syncthreads();
  if (called_off) return;
  if (blockIdx.x == 0 && threadIdx.x == 0 && !d.ctrl->done) d.ctrl->iter += ka.iters;  // (kb_tick)
  if (g >= ka.ncol) return;  // (groups do not depend on each other)

  const int col0 = g * BM_COLS, b = col0 + o.col;
  const bool live = d.c_done[b] == 0;
  const double rho = d.rho, rinv = d.rho_inv, alpha = d.alpha, sigma = d.sigma;
  // ---- this thread's elements ----
  const int xrow = row0 + o.row;
  const bool xmine = xrow < n;
  const size_t ox = (size_t)xrow * Bs + b;
  // (PQ: the thread owns one column for the whole launch, so its column's cost is one register as the shared one is)
  const double di = xmine ? d.d2inv[xrow] : 0.0, qx = xmine ? bq_at<PQ>(d, xrow, ox) : 0.0;
  const int pos = (xmine && whm < d.M) ? d.int_pos[xrow] : -1;  // the variable's own bound row (identity rows)
  const double aj = pos >= 0 ? d.a_int[xrow] : 0.0;
  const size_t oj = pos >= 0 ? (size_t)(d.m_orig + pos) * Bs + b : 0;   // its z, y, l, u, dy
  const size_t ow = pos >= 0 ? whrow(d, d.m_orig + pos) * Bs + b : 0;   // its wh entry
  double sx = xmine ? d.b_x[ox] : 0.0, srx = xmine ? d.b_rx[ox] : 0.0, sut = 0.0;
  double zi = 0, yi = 0, wi = 0, loi = 0, upi = 0;
  if (pos >= 0) { zi = d.b_z[oj]; yi = d.b_y[oj]; wi = d.b_wh[ow]; loi = d.b_l[oj]; upi = d.b_u[oj]; }
  bool cmine[2];
  size_t oc[2];
  double zc[2], yc[2], wc[2], loc[2], upc[2];
#pragma unroll
  for (int t = 0; t < 2; t++) {
    const int row = 16 * (m + KBP_MEMBERS * t) + o.row;
    cmine[t] = row < whm;
    oc[t] = (size_t)row * Bs + b;  // general rows: wh sits at its own row index
    zc[t] = yc[t] = wc[t] = loc[t] = upc[t] = 0.0;
    if (cmine[t]) { zc[t] = d.b_z[oc[t]]; yc[t] = d.b_y[oc[t]]; wc[t] = d.b_wh[oc[t]]; loc[t] = d.b_l[oc[t]]; upc[t] = d.b_u[oc[t]]; }
  }
  const unsigned rowbytes = (unsigned)(Bs * sizeof(double));
  const __amdgpu_buffer_rsrc_t rs_wh = __builtin_amdgcn_make_buffer_rsrc((void *)d.b_wh, 0, (int)((unsigned)(d.M + n + 16) * rowbytes), 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_ut = __builtin_amdgcn_make_buffer_rsrc((void *)d.b_ut, 0, (int)((unsigned)(n + 16) * rowbytes), 0x00020000);
  const unsigned lane_off = (unsigned)(4 * j) * rowbytes + (unsigned)(2 * r + col0) * (unsigned)sizeof(double);
  const int nch_f = kbp_nch(0, kend_f, w), nch_x = kbp_nch(row0, n, w), nch_c = kbp_nch(0, n, w);
  // byte offsets of this thread's elements in the two exchanged arrays (b_rx = b_wh + wh_m rows)
  const unsigned so_ut = (unsigned)(ox * sizeof(double)), so_rx = (unsigned)(((size_t)(whm + xrow) * Bs + b) * sizeof(double));
  const unsigned so_wi = (unsigned)(ow * sizeof(double));
  const unsigned so_c0 = (unsigned)(oc[0] * sizeof(double)), so_c1 = (unsigned)(oc[1] * sizeof(double));
  unsigned long long *ctr = ka.bar + 16 * g;
  unsigned long long target = 0;
  __syncthreads();

  long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  long long tc = PROF ? clock64() : 0;
#define KBP_PH(k)                                   \
  if (PROF) {                                       \
    const long long now = clock64();                \
    ph[k] += now - tc;                              \
    tc = now;                                       \
  }
  for (int it = 0; it < ka.iters; it++) {
    const bool last = it + 1 == ka.iters;
    double4_t acc[2];
    // ================= forward: ut = D22^-1 ( r~ + [ -G | strict_lower(Linv) ] [wh ; r~] ), row block m =================
    kbp_sweep<KBP_FC>([&](int c, int q) { return af[c][q]; }, rs_wh, lane_off, rowbytes, 0, nch_f, w, acc);
    KBP_PH(0)
    {
      const double s = kbp_reduce(acc, lds, o);
      sut = di * (srx + s);
      kbp_st_pair(rs_ut, so_ut, sut, xmine);
    }
    KBP_PH(1)
    target += KBP_MEMBERS;
    if (kbp_barrier(ctr, target, s_flag, d.ctrl, 2)) return;
    KBP_PH(2)
    // ================= backward: x~ = ut + strict_upper(Linv^T) ut; nu = -rho wh + (-G)^T ut; the vector updates =================
    kbp_sweep<KBP_BC>([&](int c, int q) { return ab[c][q]; }, rs_ut, lane_off, rowbytes, row0, nch_x, w, acc);
    KBP_PH(3)
    {
      const double s = kbp_reduce(acc, lds, o);
      const double xt = sut + s;
      if (last && xmine) d.b_xt[ox] = xt;
      if (xmine && live) {
        const double xn = alpha * xt + (1.0 - alpha) * sx;
        if (last) {
          d.b_x[ox] = xn;
          d.b_dx[ox] = xn - sx;
        }
        sx = xn;
        double rx = sigma * xn - qx;
        if (pos >= 0) {
          const double nu = -rho * wi + aj * xt;  // aj = rho a_j
          const double zt = zi + rinv * (nu - yi);
          const double zr = alpha * zt + (1.0 - alpha) * zi;
          const double v = zr + rinv * yi;
          const double zn = fmin(fmax(v, loi), upi);
          const double dy = rho * (zr - zn);
          const double yn = yi + dy;
          const double whn = zn - rinv * yn;
          if (last) {
            d.b_z[oj] = zn;
            d.b_y[oj] = yn;
            d.b_dy[oj] = dy;
          }
          zi = zn;
          yi = yn;
          wi = whn;
          rx += aj * whn;  // r~ = rx + t
        }
        srx = rx;
      }
      // (a frozen column stores what it holds: the same bits again; bound rows are scattered, their pairs share the row)
      kbp_st_pair(rs_wh, so_wi, wi, pos >= 0);
      kbp_st_pair(rs_wh, so_rx, srx, xmine);
    }
    KBP_PH(4)
#pragma unroll
    for (int t = 0; t < 2; t++) {
      if (16 * (m + KBP_MEMBERS * t) >= whm) continue;  // (uniform over the workgroup)
      kbp_sweep<KBP_BC>([&](int c, int q) { return la[((t * KBP_BC + c) * 4 + q) * 512 + threadIdx.x]; }, rs_ut, lane_off, rowbytes, 0,
                        nch_c, w, acc);
      const double s = kbp_reduce(acc, lds, o);
      if (cmine[t] && live) {
        const double nu = -rho * wc[t] + s;
        const double zt = zc[t] + rinv * (nu - yc[t]);
        const double zr = alpha * zt + (1.0 - alpha) * zc[t];
        const double v = zr + rinv * yc[t];
        const double zn = fmin(fmax(v, loc[t]), upc[t]);
        const double dy = rho * (zr - zn);
        const double yn = yc[t] + dy;
        if (last) {
          d.b_z[oc[t]] = zn;
          d.b_y[oc[t]] = yn;
          d.b_dy[oc[t]] = dy;
        }
        zc[t] = zn;
        yc[t] = yn;
        wc[t] = zn - rinv * yn;
      }
      kbp_st_pair(rs_wh, t == 0 ? so_c0 : so_c1, wc[t], cmine[t]);
    }
    KBP_PH(5)
    target += KBP_MEMBERS;
    if (kbp_barrier(ctr, target, s_flag, d.ctrl, 3)) return;
    KBP_PH(6)
  }
#undef KBP_PH
  if (PROF && d.prof && threadIdx.x == 0) {
    for (int k = 0; k < 7; k++) d.prof[16 * blockIdx.x + k] = (unsigned long long)ph[k];
    d.prof[16 * blockIdx.x + 7] = (unsigned long long)ka.iters;
  }
}
