// part of engine.hip (included there, not compiled alone): cooperative register-resident solver (k_coop) and its in-kernel termination test
// ------------------------------------------------------------------------------------------
// cooperative register-resident solver: the same iteration as ONE exchange per step.
//   [nu + rho wh ; x~] = W [wh ; rx],  W = K^-1 restricted as in dense_setup.hip (ks_kkt_inverse).
// Workgroup b keeps rows [b RW, (b+1) RW) of W in registers for the whole launch (thread t holds
// columns t + k*COOP_B, COOP_B = 512 threads per workgroup), owns the iterates of those rows, and
// after every step publishes its RW new entries of [wh ; rx]; every workgroup then gathers the whole
// vector.  The exchange needs no barrier and no flag: a value travels as its bare 8 bytes (8-byte stores are
// single-copy atomic), written at agent scope into the buffer of the round, one of a ring of four whose slots
// say "not yet written" by a sentinel no iterate can equal ("pair units" below: two columns per 16-byte poll); a
// reader sleeps through the first part of the hand-off (an early poll would only pull the stale line back into
// its XCD's L2 and slow the writer down; the length is calibrated at setup) and then polls its own CPT columns
// until none holds the sentinel.  A workgroup can only reach round k+1 after it has seen every value of round k;
// why that makes four buffers enough, and three too few, is written down at the ring's definition.
// (Everything off the per-iteration path -- the test's operands, the mailbox, the record, the epilogue -- keeps
// tagged 16-byte entries {lo, tag, hi, tag}: ll_publish / ll_peek.)
// The termination test runs inside the same launch (every `check_every` iterations): the owners
// also publish [y ; x] and [proj(dy) ; dx], every workgroup applies ITS rows of
//   Kc = [ 0  Abar ; Abar^T  Pbar ]   (read from HBM, only at a test)
// to both, reduces the 17 norms / sums of sec. 3.4 over its rows, publishes them, gathers those of
// all workgroups and takes the decision itself -- identical arithmetic in identical order
// everywhere, so all workgroups agree without a further exchange.
// All workgroups must be co-resident: the grid never exceeds the CU count and one workgroup fits
// per CU next to anything else this engine launches.  Polling is bounded; on expiry ctrl->pad is
// set and the host reports MIOSQP_EHIP.
// ------------------------------------------------------------------------------------------
// Bounded polling by wall clock (100 MHz counter, read only every 4096 polls).  Two limits: the start-up
// registration gives up after ~100 ms -- if the whole grid is not resident by then something else is using
// the device, nothing has been modified yet and the host redoes the solve in the two-kernel form at once --
// while a wait INSIDE the loop, where every workgroup is known to be resident, only expires after ~2 s
// (a hung device, reported as an error).
constexpr unsigned long long COOP_LIMIT_REGISTER = 10000000ull, COOP_LIMIT_EXCHANGE = 200000000ull;
__device__ __forceinline__ bool coop_expired(unsigned &spins, unsigned long long &since,
                                             unsigned long long limit = COOP_LIMIT_EXCHANGE) {
  if ((++spins & 4095u) != 0u) return false;
  const unsigned long long now = wall_clock64();
  if (spins == 4096u) {
    since = now;
    return false;
  }
  return now - since > limit;
}

typedef unsigned ll_u4 __attribute__((ext_vector_type(4)));
// one 16-byte agent-scope store / load per entry ({lo, tag, hi, tag}); the tags in BOTH 8-byte halves
// keep the hand-off correct even if the 16 bytes were ever observed torn
__device__ __forceinline__ void ll_publish(unsigned long long *slot, double v, unsigned tag) {
  ll_u4 w;
  w.x = (unsigned)__double2loint(v); w.y = tag; w.z = (unsigned)__double2hiint(v); w.w = tag;
  // (s_nop 1: the store reads its data registers a few cycles after it issues, and the compiler, which does not
  //  model the instruction, may reuse them at once -- a clobbered tag is an entry that never arrives)
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(slot), "v"(w) : "memory");
}
__device__ __forceinline__ ll_u4 ll_peek(const unsigned long long *slot) {
  ll_u4 w;
  asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(w) : "v"(slot) : "memory");
  return w;
}

// ---- the exchange ring of the iteration (coop_grid): pair units.  A value travels as its bare 8 bytes; column
// c = t + k COOP_B of a buffer lives in 16-byte unit (k / 2) COOP_B + t, half k & 1, so a thread polls its columns
// k = 0, 1 with ONE 16-byte load and k = 2, 3 with a second one (the halves of a unit are written by two workgroups, 8
// bytes each: byte enables keep them apart, and an 8-byte store is single-copy atomic).
// "Not yet written" is COOP_SENTINEL, a signalling NaN (exponent all ones, quiet bit clear, payload non-zero): no IEEE
// operation RETURNS a signalling NaN -- every arithmetic result that is a NaN is quiet -- so no iterate can equal it,
// those of a diverged solve included, and the host validates what the user passes in.
// FOUR buffers, indexed by round & 3 (the running tag).  In round k an owner stores its value into buffer k & 3 and
// then the sentinel into ITS OWN slot of buffer (k + 2) & 3.  Invariant: an owner that computes round k has gathered all
// of round k - 1, so every workgroup has published k - 1 -- which it does behind its barrier, reached by every wave
// after its gather of k - 2: nobody reads buffer (k + 2) & 3 = (k - 2) & 3 any more.  The reset is acknowledged before
// the same lane publishes round k + 1 (its gather of round k ends in s_waitcnt vmcnt(0), and stores count in vmcnt on
// gfx9), and a reader polls buffer (k + 2) & 3 only after it has seen this owner's value of round k + 1.  THREE
// buffers are not enough: the reset would hit buffer (k - 1) % 3 while slower workgroups still gather round k - 1.
// A launch leaves the ring in phase for the next one (every workgroup publishes the same rounds; a launch that is
// called off publishes none); the host refills it when the layout changes or a launch timed out (k_coop_ring_fill).
// The testers' decision (column NR of the round it is picked up in) has no owner that could reset it in step: it
// travels as {status, tag of that round} in the same 8 bytes and is accepted by its tag.
constexpr unsigned long long COOP_SENTINEL = 0x7FF0000000005EA7ull;
constexpr unsigned COOP_SENT_LO = 0x00005EA7u, COOP_SENT_HI = 0x7FF00000u;
constexpr size_t COOP_RING_WORDS = 4096;  // 8-byte words per buffer of the ring: 2 x 512 units, column 2048 and a margin
template <int COOP_B>
__host__ __device__ __forceinline__ size_t coop_ring_slot(int c) {  // 8-byte word of column c in a buffer
  return 2 * (size_t)((c / (2 * COOP_B)) * COOP_B + c % COOP_B) + (size_t)((c / COOP_B) & 1);
}
__device__ __forceinline__ unsigned long long *coop_ring_buf(unsigned long long *ring, unsigned round) {
  return ring + (size_t)(round & 3u) * COOP_RING_WORDS;
}
__device__ __forceinline__ void ll_publish8(unsigned long long *slot, unsigned long long bits) {
  // (s_nop 1: see ll_publish)
  asm volatile("global_store_dwordx2 %0, %1, off sc1\n\ts_nop 1" ::"v"(slot), "v"(bits) : "memory");
}
// (the same with the buffer in scalar registers and a 32-bit byte offset per lane: no 64-bit address arithmetic in the loop)
__device__ __forceinline__ void ll_publish8(unsigned long long *buf, unsigned byte_off, unsigned long long bits) {
  asm volatile("global_store_dwordx2 %0, %1, %2 sc1\n\ts_nop 1" ::"v"(byte_off), "v"(bits), "s"(buf) : "memory");
}
__device__ __forceinline__ ll_u4 ll_peek(const unsigned long long *buf, unsigned byte_off) {
  ll_u4 w;
  asm volatile("global_load_dwordx4 %0, %1, %2 sc1" : "=v"(w) : "v"(byte_off), "s"(buf) : "memory");
  return w;
}
__global__ void k_coop_ring_fill(unsigned long long *ring) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < 4 * COOP_RING_WORDS; i += (size_t)gridDim.x * blockDim.x)
    ring[i] = COOP_SENTINEL;
}

// The loads above are asynchronous and the compiler does not know it: between an ll_peek and the s_waitcnt that
// follows it may not touch the destination registers -- true as long as it does not SPILL them (a spill stores the
// register before the data has arrived).  The exchange loop has no spills (checked in the ISA); code under more
// register pressure uses these, where the loads and the wait are ONE statement.
__device__ __forceinline__ ll_u4 ll_peek_wait(const unsigned long long *slot) {
  ll_u4 w;
  asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(w) : "v"(slot) : "memory");
  return w;
}
__device__ __forceinline__ void ll_peek_wait2(const unsigned long long *p0, const unsigned long long *p1, ll_u4 &w0,
                                              ll_u4 &w1) {
  asm volatile("global_load_dwordx4 %0, %2, off sc1\n\tglobal_load_dwordx4 %1, %3, off sc1\n\ts_waitcnt vmcnt(0)"
               : "=&v"(w0), "=&v"(w1) : "v"(p0), "v"(p1) : "memory");
}
__device__ __forceinline__ void ll_peek_wait3x1(const unsigned long long *p0, const unsigned long long *p1, const unsigned long long *p2,
                                                ll_u4 &w0, ll_u4 &w1, ll_u4 &w2) {
  asm volatile("global_load_dwordx4 %0, %3, off sc1\n\tglobal_load_dwordx4 %1, %4, off sc1\n\tglobal_load_dwordx4 %2, %5, off sc1\n\t"
               "s_waitcnt vmcnt(0)"
               : "=&v"(w0), "=&v"(w1), "=&v"(w2) : "v"(p0), "v"(p1), "v"(p2) : "memory");
}
__device__ __forceinline__ void ll_peek_wait5(const unsigned long long *(&p)[5], ll_u4 (&w)[5]) {
  asm volatile("global_load_dwordx4 %0, %5, off sc1\n\tglobal_load_dwordx4 %1, %6, off sc1\n\t"
               "global_load_dwordx4 %2, %7, off sc1\n\tglobal_load_dwordx4 %3, %8, off sc1\n\t"
               "global_load_dwordx4 %4, %9, off sc1\n\ts_waitcnt vmcnt(0)"
               : "=&v"(w[0]), "=&v"(w[1]), "=&v"(w[2]), "=&v"(w[3]), "=&v"(w[4])
               : "v"(p[0]), "v"(p[1]), "v"(p[2]), "v"(p[3]), "v"(p[4])
               : "memory");
}
template <int CPT>
__device__ __forceinline__ void ll_peek_wait3(const unsigned long long *(&p)[3 * CPT], ll_u4 (&w)[3 * CPT]) {
  static_assert(CPT == 2 || CPT == 4, "columns per thread");
  if constexpr (CPT == 2) {
    asm volatile(
        "global_load_dwordx4 %0, %6, off sc1\n\tglobal_load_dwordx4 %1, %7, off sc1\n\t"
        "global_load_dwordx4 %2, %8, off sc1\n\tglobal_load_dwordx4 %3, %9, off sc1\n\t"
        "global_load_dwordx4 %4, %10, off sc1\n\tglobal_load_dwordx4 %5, %11, off sc1\n\ts_waitcnt vmcnt(0)"
        : "=&v"(w[0]), "=&v"(w[1]), "=&v"(w[2]), "=&v"(w[3]), "=&v"(w[4]), "=&v"(w[5])
        : "v"(p[0]), "v"(p[1]), "v"(p[2]), "v"(p[3]), "v"(p[4]), "v"(p[5])
        : "memory");
  } else {
    asm volatile(
        "global_load_dwordx4 %0, %12, off sc1\n\tglobal_load_dwordx4 %1, %13, off sc1\n\t"
        "global_load_dwordx4 %2, %14, off sc1\n\tglobal_load_dwordx4 %3, %15, off sc1\n\t"
        "global_load_dwordx4 %4, %16, off sc1\n\tglobal_load_dwordx4 %5, %17, off sc1\n\t"
        "global_load_dwordx4 %6, %18, off sc1\n\tglobal_load_dwordx4 %7, %19, off sc1\n\t"
        "global_load_dwordx4 %8, %20, off sc1\n\tglobal_load_dwordx4 %9, %21, off sc1\n\t"
        "global_load_dwordx4 %10, %22, off sc1\n\tglobal_load_dwordx4 %11, %23, off sc1\n\ts_waitcnt vmcnt(0)"
        : "=&v"(w[0]), "=&v"(w[1]), "=&v"(w[2]), "=&v"(w[3]), "=&v"(w[4]), "=&v"(w[5]), "=&v"(w[6]), "=&v"(w[7]),
          "=&v"(w[8]), "=&v"(w[9]), "=&v"(w[10]), "=&v"(w[11])
        : "v"(p[0]), "v"(p[1]), "v"(p[2]), "v"(p[3]), "v"(p[4]), "v"(p[5]), "v"(p[6]), "v"(p[7]), "v"(p[8]), "v"(p[9]),
          "v"(p[10]), "v"(p[11])
        : "memory");
  }
}

template <int CPT>
__device__ __forceinline__ void ll_peek_waitn(const unsigned long long *(&p)[CPT], ll_u4 (&w)[CPT]) {
  static_assert(CPT >= 1 && CPT <= 4, "loads per thread");
  if constexpr (CPT == 1) {
    asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(w[0]) : "v"(p[0]) : "memory");
  } else if constexpr (CPT == 2) {
    asm volatile("global_load_dwordx4 %0, %2, off sc1\n\tglobal_load_dwordx4 %1, %3, off sc1\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(w[0]), "=&v"(w[1]) : "v"(p[0]), "v"(p[1]) : "memory");
  } else if constexpr (CPT == 3) {
    asm volatile("global_load_dwordx4 %0, %3, off sc1\n\tglobal_load_dwordx4 %1, %4, off sc1\n\t"
                 "global_load_dwordx4 %2, %5, off sc1\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(w[0]), "=&v"(w[1]), "=&v"(w[2]) : "v"(p[0]), "v"(p[1]), "v"(p[2]) : "memory");
  } else {
    asm volatile("global_load_dwordx4 %0, %4, off sc1\n\tglobal_load_dwordx4 %1, %5, off sc1\n\t"
                 "global_load_dwordx4 %2, %6, off sc1\n\tglobal_load_dwordx4 %3, %7, off sc1\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(w[0]), "=&v"(w[1]), "=&v"(w[2]), "=&v"(w[3]) : "v"(p[0]), "v"(p[1]), "v"(p[2]), "v"(p[3]) : "memory");
  }
}

// transposed butterfly: RW values per lane in, the sum over the wave of ONE row per lane out
// (row coop_row<RW>(lane)); halves the live values at every exchange instead of reducing each
// row separately.  Partners: xor 1, xor 2 (quad_perm), 7 - i (row_half_mirror), 15 - i (row_mirror);
// the keep/send choice of a stage must differ between partners of that stage and agree between
// partners of every later stage, hence the mixed bits.
template <int RW>
__device__ __forceinline__ int coop_row(int lane) {
  const int cA = (lane ^ (lane >> 2)) & 1, cB = ((lane >> 1) ^ (lane >> 2)) & 1, cC = ((lane >> 2) ^ (lane >> 3)) & 1,
            cD = (lane >> 3) & 1;
  return RW == 16 ? 8 * cA + 4 * cB + 2 * cC + cD : 4 * cA + 2 * cB + cC;
}
template <int RW>
__device__ __forceinline__ double wave_tsum(double (&v)[RW], int lane) {
  static_assert(RW == 8 || RW == 16, "rows per workgroup");
  const bool cA = (lane ^ (lane >> 2)) & 1, cB = ((lane >> 1) ^ (lane >> 2)) & 1, cC = ((lane >> 2) ^ (lane >> 3)) & 1,
             cD = (lane >> 3) & 1;
#define HALVE(H, C, CTRL)                                        \
  _Pragma("unroll") for (int k = 0; k < (H) / 2; k++) {          \
    const double keep = (C) ? v[k + (H) / 2] : v[k];             \
    const double send = (C) ? v[k] : v[k + (H) / 2];             \
    v[k] = keep + dpp_get<CTRL>(send);                           \
  }
  if constexpr (RW == 16) {
    HALVE(16, cA, 0xB1) HALVE(8, cB, 0x4E) HALVE(4, cC, 0x141) HALVE(2, cD, 0x140)
  } else {
    (void)cD;
    HALVE(8, cA, 0xB1) HALVE(4, cB, 0x4E) HALVE(2, cC, 0x141)
    v[0] += dpp_get<0x140>(v[0]);
  }
#undef HALVE
  return add_xor32(add_xor16(v[0]));
}

// Pointers into LDS that were handed to a `noinline` function arrive as generic pointers: every access through one is a
// FLAT load (the address decides at run time whether it goes to LDS or to memory) that the compiler must wait for with
// both counters at zero -- serialised, ~0.5 us apiece behind the polls' traffic.  The tester's operand reads were 14 of
// its 15 us per test that way.  Cast back to the LDS address space, they are ds_read again.
typedef __attribute__((address_space(3))) double lds_f64;
typedef double coop_v2d __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) coop_v2d lds_v2d;
__device__ __forceinline__ lds_f64 *to_lds(double *p) { return (lds_f64 *)p; }
// a workgroup-uniform 4- or 8-byte value read from LDS, moved to scalar registers (the compiler cannot know it is uniform)
template <class T>
__device__ __forceinline__ T coop_uni(T v) {
  static_assert(sizeof(T) == 8 || sizeof(T) == 4, "coop_uni");
  if constexpr (sizeof(T) == 8) {
    unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b >> 32));
    b = ((unsigned long long)hi << 32) | lo;
    return __builtin_bit_cast(T, b);
  } else {
    return __builtin_bit_cast(T, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
  }
}
__device__ __forceinline__ const lds_f64 *to_lds(const double *p) { return (const lds_f64 *)p; }

constexpr int COOP_QS = 48;  // 8-byte words per workgroup in the norm exchange (NQ entries of 2 words, padded)

// ------------------------------------------------------------------------------------------
// Row layout of the exchange ("reduced" indices).  The p integer-bound rows of A_ext have one entry each (data.py:5-33
// appends I[i_idx, :]): for such a row j of variable i
//     (nu + rho wh)_j = rho a_j x~_i            -- no row of W is needed for it, the owner of x~_i has the number --
//     its column of W only ever multiplies wh_j  -- and K^-1's x-block sees it as rho a_j wh_j added to rx_i.
// So once miosqp_qp_set_integer_rows has found every bound row to be of that kind, the exchange runs on
//     W' = W restricted to { general rows 0 .. mg-1 } + { variables },  NR = mg + n  (config 2: 1500 instead of 1750),
// the exchanged vector is [ wh(general) ; rx + rho a wh(bound row) ], and the owner of variable i also owns the
// iterates of its bound row (z, y, l, u, wh, dy) and updates them from x~_i on the spot: 14 % fewer rows in the
// all-to-all, a quarter fewer products per thread.  Before set_integer_rows (and for problems whose bound rows are
// not identity rows) mg = M and every variable's bound row is -1: the same code is the full layout.
// The termination test keeps FULL indices (constraint rows 0 .. M-1, then variables): its operand buffers hold an
// entry per full index, published by whoever owns the iterate.
// ------------------------------------------------------------------------------------------
struct CoopOwner {  // the iterates one owner thread keeps in registers for the whole launch
  // constraint part (a general row, or the bound row of this thread's variable): z, y, l, u, wh, dy
  double z, y, lo, up, sw, dy;
  // variable part: x, q, dx, and rho * (scaled entry of the variable's bound row) -- 0 without one
  double x, q, dx, aint;
  int rowc;  // FULL index of the constraint row of the constraint part, -1: none
  int var;   // index of the variable of the variable part, -1: none
};

// The termination test of the cooperative solver inside the exchange grid (once per `check_every` iterations; used when
// the device has no CUs to spare for testers).  Returns the status (0 = keep iterating); identical in every workgroup.
// Must stay inlined: as a real call it broke at 512 threads per workgroup (ROCm 7.2), and it takes what it reads of Dev
// by value.
struct CoopTest {  // what the test reads of Dev, by value (a reference would pin Dev to the stack)
  unsigned long long *coop_chk, *coop_q;
  const double *Kc, *Einv, *E, *Dinv, *D, *aj;
  Ctrl *ctrl;
  int n, M, mg, ldw;
  double c, cinv, eps_abs, eps_rel, eps_pinf, eps_dinf;
};

__device__ __forceinline__ double coop_vproj(double dy, double lo, double up) {
  const bool uinf = up > QP_INFTY * QP_MIN_SCALING, linf = lo < -QP_INFTY * QP_MIN_SCALING;
  double v = dy;
  if (uinf && linf) v = 0.0;
  else if (uinf) v = fmin(v, 0.0);
  else if (linf) v = fmax(v, 0.0);
  return v;
}

template <int COOP_B, int RW, int CPTF>
__device__ __forceinline__ int coop_test(const CoopTest d, unsigned tag, int it, bool own, const CoopOwner o, int *s_fail) {
  constexpr int NW = COOP_B / 64;
  static_assert(NQ <= 32, "norm gather layout");
  // scratch with two uses that never overlap in time: the operands lv[2][2048] (N <= 2048), then the
  // gathered partial results qall[member][NQ]
  __shared__ __attribute__((aligned(16))) double tsc[256 * NQ];
  static_assert(256 * NQ >= 4096, "operand staging");
  double *const qall = tsc;
  double(*const lv)[2048] = reinterpret_cast<double(*)[2048]>(tsc);
  __shared__ double cpart[4][1][RW];
  __shared__ double qrow[RW][NQ];
  __shared__ double qres[NQ];
  __shared__ int s_status;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int M = d.M, N = d.n + d.M, NR = d.mg + d.n, T = gridDim.x;
  const int r0 = blockIdx.x * RW;
  const bool con = own && o.rowc >= 0, var = own && o.var >= 0;
  // the owner's scaling entries, requested now and used after the rows (their latency hides behind the wait)
  const double e_inv = con ? d.Einv[o.rowc] : 0.0, e_dir = con ? d.E[o.rowc] : 0.0;
  const double d_inv = var ? d.Dinv[o.var] : 0.0, d_dir = var ? d.D[o.var] : 0.0;
  const double vproj = con ? coop_vproj(o.dy, o.lo, o.up) : 0.0;
  const double a_j = (con && var && d.aj) ? d.aj[o.var] : 0.0;  // the scaled entry of the variable's bound row
  // both operands go to LDS (FULL indices); wave w then applies rows RPW w .. of this workgroup's block of Kc to
  // them (rows are read once, 16 bytes per lane; a constraint row only has its Abar part).
  // Columns < M of a variable row are Abar^T, the others Pbar.
  {
    // both operands of a column sit next to each other: {y | x, proj(dy) | dx}, polled together
    bool have[CPTF];
#pragma unroll
    for (int k = 0; k < CPTF; k++) have[k] = t + k * COOP_B >= N;
    unsigned spins = 0;
    unsigned long long since = 0;
    for (;;) {
      // (loads and wait as ONE statement per column, see ll_peek_wait: this function is under register pressure;
      //  a column beyond the problem reads entry 0)
      ll_u4 w1[CPTF], w2[CPTF];
#pragma unroll
      for (int k = 0; k < CPTF; k++) {
        const unsigned long long *p1 = d.coop_chk + (have[k] ? 0 : 4 * (size_t)(t + k * COOP_B));
        if (!have[k]) ll_peek_wait2(p1, p1 + 2, w1[k], w2[k]);
      }
      bool all = true;
#pragma unroll
      for (int k = 0; k < CPTF; k++)
        if (!have[k]) {
          if (w1[k].y == tag && w1[k].w == tag && w2[k].y == tag && w2[k].w == tag) {
            lv[0][t + k * COOP_B] = __hiloint2double((int)w1[k].z, (int)w1[k].x);
            lv[1][t + k * COOP_B] = __hiloint2double((int)w2[k].z, (int)w2[k].x);
            have[k] = true;
          } else {
            all = false;
          }
        }
      if (all) break;
      if (coop_expired(spins, since)) {
        *s_fail = 1;
        d.ctrl->pad = 3;
        break;
      }
    }
  }
  __syncthreads();
  if (*s_fail) return 0;
  {
    constexpr int RPW = RW / NW;  // rows per wave
    static_assert(RPW * NW == RW && (RPW == 1 || RPW == 2), "rows per wave");
    double a8[8];  // per row: A^T y, A^T proj(dy), P x (A x), P dx (A dx)
#pragma unroll
    for (int k = 0; k < 8; k++) a8[k] = 0.0;
    const int Ne = N & ~1;
#pragma unroll
    for (int h = 0; h < RPW; h++) {
      const int rred = r0 + RPW * wave + h;
      if (rred >= NR) continue;
      const int rr = rred < d.mg ? rred : rred + (M - d.mg);  // the row of Kc (full index)
      const double *row = d.Kc + (size_t)rr * d.ldw;
      double sA1 = 0.0, sA2 = 0.0, sP1 = 0.0, sP2 = 0.0;
      // all 16-byte pieces of the row are requested before the first is used (N <= 2048: at most 16)
      constexpr int NCH = 16;
      const int cbeg = (rr < M ? (M & ~1) : 0) + 2 * lane;
      double2 a[NCH];
#pragma unroll
      for (int j = 0; j < NCH; j++) {
        const int c = cbeg + 128 * j;
        a[j] = c < Ne ? *reinterpret_cast<const double2 *>(row + c) : make_double2(0.0, 0.0);
      }
#pragma unroll
      for (int j = 0; j < NCH; j++) {
        const int c = cbeg + 128 * j;
        if (c >= Ne) continue;
        const double2 p = *reinterpret_cast<const double2 *>(&lv[0][c]);
        const double2 s2 = *reinterpret_cast<const double2 *>(&lv[1][c]);
        if (c < M) { sA1 = fma(a[j].x, p.x, sA1); sA2 = fma(a[j].x, s2.x, sA2); }
        else { sP1 = fma(a[j].x, p.x, sP1); sP2 = fma(a[j].x, s2.x, sP2); }
        if (c + 1 < M) { sA1 = fma(a[j].y, p.y, sA1); sA2 = fma(a[j].y, s2.y, sA2); }
        else { sP1 = fma(a[j].y, p.y, sP1); sP2 = fma(a[j].y, s2.y, sP2); }
      }
      if ((N & 1) && lane == 0) {  // last column of an odd width (always a variable column)
        const double a1 = row[N - 1];
        sP1 = fma(a1, lv[0][N - 1], sP1);
        sP2 = fma(a1, lv[1][N - 1], sP2);
      }
      a8[4 * h] = sA1; a8[4 * h + 1] = sA2; a8[4 * h + 2] = sP1; a8[4 * h + 3] = sP2;
    }
    const double ws8 = wave_tsum<8>(a8, lane);
    if (lane < 8) {
      const int e = coop_row<8>(lane);  // = 4 h + quantity
      if ((e >> 2) < RPW) cpart[e & 3][0][RPW * wave + (e >> 2)] = ws8;
    }
  }
  __syncthreads();
  if (*s_fail) return 0;
  if (t < RW) {
#pragma unroll
    for (int k = 0; k < NQ; k++) qrow[t][k] = (k == 4 || k == 5) ? -1.7e308 : 0.0;
    if (own) {
      const double sA1 = cpart[0][0][t], sA2 = cpart[1][0][t], sP1 = cpart[2][0][t], sP2 = cpart[3][0][t];
      if (con) {
        // a general row: its products come from its row of Kc; the bound row of a variable: (Abar x)_j = a_j x_i
        const double ax = var ? a_j * o.x : sP1, adx0 = var ? a_j * o.dx : sP2;
        const bool uinf = o.up > QP_INFTY * QP_MIN_SCALING, linf = o.lo < -QP_INFTY * QP_MIN_SCALING;
        const double adx = e_inv * adx0;
        qrow[t][0] = fabs(e_inv * (ax - o.z));
        qrow[t][1] = fabs(e_inv * ax);
        qrow[t][2] = fabs(e_inv * o.z);
        qrow[t][3] = fabs(e_dir * vproj);
        qrow[t][4] = uinf ? -1.7e308 : adx;
        qrow[t][5] = -(linf ? 1.7e308 : adx);
        qrow[t][13] = o.up * fmax(vproj, 0.0) + o.lo * fmin(vproj, 0.0);
      }
      if (var) {
        const double px = sP1, aty = sA1;
        qrow[t][6] = fabs(d_inv * (px + o.q + aty));
        qrow[t][7] = fabs(d_inv * px);
        qrow[t][8] = fabs(d_inv * aty);
        qrow[t][9] = fabs(d_inv * o.q);
        qrow[t][10] = fabs(d_inv * sP2);
        qrow[t][11] = fabs(d_inv * sA2);
        qrow[t][12] = fabs(d_dir * o.dx);
        qrow[t][14] = o.q * o.dx;
        qrow[t][15] = o.x * px;
        qrow[t][16] = o.q * o.x;
      }
    }
  }
  __syncthreads();
  if (t < NQ) {
    double rq = qrow[0][t];
    for (int w = 1; w < RW; w++) rq = t < NQ_MAX ? fmax(rq, qrow[w][t]) : rq + qrow[w][t];
    ll_publish(d.coop_q + (size_t)blockIdx.x * COOP_QS + 2 * t, rq, tag);
  }
  // Two hops instead of one wide all-gather (an exchange costs by the cache line): workgroup g < NL
  // reduces the partial results of workgroups g, g + NL, g + 2 NL, ... and publishes the group's;
  // then everybody gathers the NL group results.  Fixed order, same arithmetic in every workgroup.
  constexpr int NL = 16, NMEM = 256 / NL;  // at most 256 workgroups
  auto collect = [&](const unsigned long long *src, int first, int step, int count) {
    // entries (member m, quantity q), m < count: source workgroup first + m * step; result in qall[m * NQ + q]
    constexpr int KC = (NMEM * NQ + COOP_B - 1) / COOP_B;
    ll_u4 w[KC];
    bool have[KC];
    const unsigned long long *ptr[KC];
#pragma unroll
    for (int k = 0; k < KC; k++) {
      const int e = t + k * COOP_B;
      have[k] = e >= count * NQ;
      ptr[k] = src + (size_t)(first + (e / NQ) * step) * COOP_QS + 2 * (e % NQ);
    }
    unsigned spins = 0;
    unsigned long long since = 0;
    for (;;) {
#pragma unroll
      for (int k = 0; k < KC; k++)
        if (!have[k]) w[k] = ll_peek_wait(ptr[k]);  // (load and wait as one statement, see ll_peek_wait)
      bool all = true;
#pragma unroll
      for (int k = 0; k < KC; k++)
        if (!have[k]) {
          if (w[k].y == tag && w[k].w == tag) {
            qall[t + k * COOP_B] = __hiloint2double((int)w[k].z, (int)w[k].x);
            have[k] = true;
          } else {
            all = false;
          }
        }
      if (all) break;
      if (coop_expired(spins, since)) {
        *s_fail = 1;
        d.ctrl->pad = 4 + (src != d.coop_q);
        break;
      }
    }
  };
  const int nl = T < NL ? T : NL;
  if ((int)blockIdx.x < nl) {
    const int count = (T - (int)blockIdx.x + nl - 1) / nl;
    collect(d.coop_q, blockIdx.x, nl, count);
    __syncthreads();
    if (t < NQ) {
      double rq = qall[t];
      for (int m = 1; m < count; m++) rq = t < NQ_MAX ? fmax(rq, qall[m * NQ + t]) : rq + qall[m * NQ + t];
      ll_publish(d.coop_q + (size_t)(256 + blockIdx.x) * COOP_QS + 2 * t, rq, tag);
    }
    __syncthreads();  // qall is reused below
  }
  collect(d.coop_q + (size_t)256 * COOP_QS, 0, 1, nl);
  __syncthreads();
  if (*s_fail) return 0;
  if (t < NQ) {
    double rq = qall[t];
    for (int g = 1; g < nl; g++) rq = t < NQ_MAX ? fmax(rq, qall[g * NQ + t]) : rq + qall[g * NQ + t];
    qres[t] = rq;
  }
  __syncthreads();
  if (t == 0) {
    Norms nm{qres[0], qres[1], qres[2], qres[3], qres[4], -qres[5], qres[6] * d.cinv, qres[7], qres[8], qres[9],
             qres[10], qres[11], qres[12], qres[13], qres[14], qres[15], qres[16]};
    double obj;
    const int st = decide_status(d, nm, obj);
    if (blockIdx.x == 0) {
      Ctrl *c = d.ctrl;
      c->iter = it;
      c->pri_res = nm.pri;
      c->dua_res = nm.dua;
      c->obj_val = obj;
      if (st) {
        c->status = st;
        c->done = 1;
      }
    }
    s_status = st;
  }
  __syncthreads();
  return s_status;
}

// ------------------------------------------------------------------------------------------
// The termination test on workgroups of its own (k_coop<..., TST = true>).  The CUs the exchange grid leaves free
// run NT "tester" workgroups in the same launch.  At a test iteration k the owners publish, next to the round's
// entries, the test's operands {y | x}, {proj(dy) | dx} and z (full indices); the exchange grid goes on iterating.  The
// testers gather the operands, apply the rows of Kc (tester j: rows j, j + NT, ...; read from memory), reduce the 17
// norms / sums (tester 0 gathers the NT partial results and decides) and publish the decision, which the exchange grid
// picks up `lag` iterations later: when it says stop, the iterates of iteration k -- kept by their owners -- are the
// result and k the reported count; the iterations in between were speculative.  The test leaves the critical
// path: it cost 8.7 us of every 25 iterations inside the grid (config 2).
// ------------------------------------------------------------------------------------------
constexpr int COOP_NT_MAX = 64;
__device__ __forceinline__ double coop_wsum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

struct CoopTesterArgs {  // what a tester reads of Dev, by value (Dev itself must not have its address taken)
  unsigned long long *coop_chk, *coop_chz, *coop_q, *coop_dec, *prof;
  const double *Kc, *Einv, *E, *Dinv, *D, *l, *u, *q;
  Ctrl *ctrl;
  int n, M, ldw;
  double c, cinv, eps_abs, eps_rel, eps_pinf, eps_dinf;
  int epi;                     // node mode: the epilogue follows a decision that leaves a solution (coop_epi_*)
  unsigned long long *stamps;  // debug timeline of the node, or nullptr
  int res;                     // the testers keep their rows of Kc in registers for the whole launch (coop_tester<.., true>)
  int run;                     // a node of k_coop_run: the bounds of the resident rows are read again at the node's first test
  // where the decision goes for the grid: entry NR of the exchange round it is picked up in (see coop_grid)
  unsigned long long *coop_buf, coop_half;
  int NR, lag;
};
// debug timeline of a node (CoopNode.stamps): who writes which word
//   grid workgroup 0: 0 entry, 1 released by the registration, 2 round 0 gathered, 6 decision picked up / loop left,
//                     7 iterates written back
//   tester 0:         4 operands gathered (last test), 3 its rows of the test done, 5 decision published, 13 epilogue entered,
//                     11 x unscaled / rounded, 12 its epilogue rows done, 8 commit entered, 9 row values gathered,
//                     14 sums and digest, 15 slot / children / incumbent written, 10 record written
#define COOP_STAMP(ptr, k)                                          \
  do {                                                              \
    if ((ptr) != nullptr && threadIdx.x == 0) (ptr)[k] = wall_clock64(); \
  } while (0)

// one padded sparse row by a group of `tpr` consecutive threads (prow_dot / prow_dot2 of kernels_iter.inc with the
// group size at run time: the same entries per lane, the same order -- the same bits as the launches' rows)
__device__ __forceinline__ double coop_prow(const int *__restrict__ idx, const double *__restrict__ val, int s, int e, int t, int tpr,
                                            const lds_f64 *v) {
  double a0 = 0.0, a1 = 0.0;
  for (int k = s + 2 * t; k < e; k += 2 * tpr) {
    const double2 a = *reinterpret_cast<const double2 *>(val + k);
    const int2 j = *reinterpret_cast<const int2 *>(idx + k);
    a0 = fma(a.x, v[j.x], a0);
    a1 = fma(a.y, v[j.y], a1);
  }
  return a0 + a1;
}
__device__ __forceinline__ void coop_prow2(const int *__restrict__ idx, const double *__restrict__ val, int s, int e, int t, int tpr,
                                           const lds_f64 *v, const lds_f64 *w, double &rv, double &rw) {
  double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
  for (int k = s + 2 * t; k < e; k += 2 * tpr) {
    const double2 a = *reinterpret_cast<const double2 *>(val + k);
    const int2 j = *reinterpret_cast<const int2 *>(idx + k);
    a0 = fma(a.x, v[j.x], a0);
    a1 = fma(a.y, v[j.y], a1);
    b0 = fma(a.x, w[j.x], b0);
    b1 = fma(a.y, w[j.y], b1);
  }
  rv = a0 + a1;
  rw = b0 + b1;
}
// row_reduce<TPR, NV> for groups of `tpr` threads of a 512-thread workgroup (every thread of the workgroup calls it);
// lds: NV x 8 doubles
template <int NV>
__device__ __forceinline__ void coop_row_reduce(double (&v)[NV], int tpr, double *lds) {
  group_sum<NV>(v, tpr < 64 ? tpr : 64);
  if (tpr > 64) {  // (workgroup-uniform)
    const int wpr = tpr / 64, wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int k = 0; k < NV; k++) lds[k * 8 + wave] = v[k];
    }
    __syncthreads();
    const int base = (wave / wpr) * wpr;
#pragma unroll
    for (int k = 0; k < NV; k++) {
      double s = lds[k * 8 + base];
      for (int w = 1; w < wpr; w++) s += lds[k * 8 + base + w];
      v[k] = s;
    }
    __syncthreads();
  }
}
// block_sum / block_max of kernels_test.inc as a 1024-thread workgroup computes them over elements 0 .. cnt-1 of `src`
// (virtual thread tid adds elements tid, tid + 1024, ...), evaluated by the 512 threads of this workgroup in two
// passes: the same order, the same bits.  lds: 16 doubles.  Every thread returns the result.
__device__ __forceinline__ double coop_block_sum1024(const lds_f64 *src, int cnt, double *lds) {
  __syncthreads();
#pragma unroll
  for (int pass = 0; pass < 2; pass++) {
    const int tid = threadIdx.x + 512 * pass;
    double s = 0;
    for (int i = tid; i < cnt; i += 1024) s += src[i];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) == 0) lds[tid >> 6] = s;
  }
  __syncthreads();
  double r = lds[0];
  for (int w = 1; w < 16; w++) r += lds[w];
  return r;
}

// The epilogue of a node inside the launch (node mode, status SOLVED or MAX_ITER_REACHED): what k_finish,
// ks_heur_obj_rows and ks_commit do in three launches behind k_coop.  It starts the moment the decision exists and
// runs on the WHOLE chip: the testers hold the iterates the decision was taken on, the workgroups of the exchange grid
// -- idle once they have left the loop -- fetch x~ of the test iteration from the test's operand buffer (nobody has
// published into it since).  Every workgroup unscales, clamps and rounds all of x for itself (n values), takes its share
// of the heuristic rows (Abar xi) and of the objective rows (P x, P xi) -- the sparse rows with the launches' threads per
// row: the same bits -- and publishes the row values; the first tester gathers them, sums in the launches' order and
// commits (slot, children, incumbent, record).  x~: lv0[M ..]; scratch: ox | xi in s1 (2 x 1024), xis in s2.
// Sizes of the in-launch epilogue, tied together here: the exchange buffer (engine.hip: coop_epi), the first tester's LDS
// staging (k_coop: lzs) and the per-thread gather count (coop_epi_commit: KE) all hold 2 n + G tagged values, n <=
// COOP_EPI_NMAX variables and G <= COOP_EPI_GMAX workgroups in the launch; host_search.inc gates `nd.epi` on both.
constexpr int COOP_EPI_NMAX = 1024, COOP_EPI_GMAX = 256, COOP_EPI_ENTRIES = 2 * COOP_EPI_NMAX + COOP_EPI_GMAX;
struct CoopEpi {  // what the epilogue reads of Dev / CoopNode, by value
  const double *D, *Dinv, *E, *Einv, *pc_A, *pr_val, *qraw, *root_l, *root_u;
  const int *int_pos, *i_idx, *pc_ptr, *pc_idx, *pr_ptr, *pr_idx;
  Ctrl *ctrl;
  int n, M, n_int, tpr_h, tpr_o;
  double cinv, eps_int, eps_lin;
  SearchArgs a;
  unsigned long long *epi_buf, *stamps;
  int coh;  // a node of k_coop_run: the slot store is read / written at agent scope (other nodes of the same launch wrote / will read it)
  unsigned long long t_node;  // wall clock when this workgroup took the node up (the record carries the first tester's)
};
__device__ __forceinline__ double epi_ld(const double *p, int coh) {
  return coh ? __hip_atomic_load((const __attribute__((address_space(1))) double *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *p;
}
__device__ __forceinline__ void epi_st(double *p, double v, int coh) {
  if (coh) __hip_atomic_store((__attribute__((address_space(1))) double *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *p = v;
}
// The node's record (coherent host memory), by one thread: every field written through to the host, acknowledged, then the
// sequence number the host polls.  (A release store at system scope would put a write-back of this XCD's whole L2 in front
// of the sequence number; nothing the host reads of a node lies in that L2 -- the record's fields go out here, the slot
// store is device memory the host does not read.)
__device__ __forceinline__ void coop_record(SearchDigest *g, int status, int iter, int int_inf, int nextvar, int action, int branched,
                                            double lower, double hviol, double hobj, double pri, double dua, double obj,
                                            unsigned long long t0, unsigned long long seq) {
#define REC_ST(f, v) __hip_atomic_store(&g->f, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)
  REC_ST(status, status); REC_ST(iter, iter); REC_ST(int_inf, int_inf); REC_ST(nextvar, nextvar);
  REC_ST(action, action); REC_ST(branched, branched); REC_ST(pad, 0); REC_ST(todo, 0);
  REC_ST(lower, lower); REC_ST(heur_viol, hviol); REC_ST(heur_obj, hobj);
  REC_ST(pri_res, pri); REC_ST(dua_res, dua); REC_ST(obj_val, obj);
  REC_ST(t0, t0); REC_ST(t1, (unsigned long long)wall_clock64());
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  REC_ST(seq, seq);
#undef REC_ST
}
// workgroup w of G: its rows.  Entries of epi_buf: [0, n) t_i = x_i (0.5 (P x)_i + q_i), [n, 2n) the same for xi,
// [2n, 2n + G) every workgroup's worst violation of the root bounds by A xi
template <int COOP_B>
__device__ __attribute__((noinline)) void coop_epi_rows(const CoopEpi *dp, unsigned long long *stamps, const int w, const int G,
                                              const unsigned tag, const double *lv0, double *s1, double *s2, double *red) {
  // (the parameter block lives in LDS: passed by value it would be a per-lane copy in scratch memory, and every field a
  //  dependent scratch load -- that alone was 30 us of a 40 us epilogue)
  const CoopEpi &d = *dp;
  const int t = threadIdx.x, n = d.n, M = d.M;
  lds_f64 *const ox = to_lds(s1), *const xi = to_lds(s1) + 1024, *const xis = to_lds(s2);  // (LDS pointers again: see to_lds)
  const lds_f64 *const lx = to_lds(lv0);
  // ---- k_finish: unscale, clamp the integer variables to the node's bounds, round
  for (int i = t; i < n; i += COOP_B) {
    double o = d.D[i] * lx[M + i];
    const int k = d.int_pos[i];
    if (k >= 0) o = fmin(fmax(o, epi_ld(d.a.lo_s + k, d.coh)), epi_ld(d.a.hi_s + k, d.coh));
    ox[i] = o;
    const double r = k >= 0 ? rint(o) : o;
    xi[i] = r;
    xis[i] = d.Dinv[i] * r;
  }
  __syncthreads();
  COOP_STAMP(stamps, 11);
  // ---- ks_heur_obj_rows: chunks of COOP_B / tpr rows, heuristic rows first; chunk c goes to workgroup c % G
  double vmax = -1.7e308;
  const int Gh = COOP_B / d.tpr_h, Go = COOP_B / d.tpr_o;
  const int CH = (M + Gh - 1) / Gh, CO = (n + Go - 1) / Go;
  for (int c = w; c < CH + CO; c += G) {  // (workgroup-uniform)
    if (c < CH) {
      const int tpr = d.tpr_h, g = t / tpr, tr = t % tpr;
      const int row_raw = c * Gh + g;
      const bool live = row_raw < M;
      const int row = live ? row_raw : M - 1;
      // (what the row's result is combined with is requested before the row, not behind it)
      const double ei = d.Einv[row], rl = d.root_l[row], ru = d.root_u[row];
      double acc[1];
      acc[0] = coop_prow(d.pc_idx, d.pc_A, d.pc_ptr[row], d.pc_ptr[row + 1], tr, tpr, xis);
      coop_row_reduce<1>(acc, tpr, red);
      if (live && tr == 0) {
        const double z = ei * acc[0];
        vmax = fmax(vmax, fmax(rl - d.eps_lin - z, z - ru - d.eps_lin));
      }
    } else {
      const int tpr = d.tpr_o, g = t / tpr, tr = t % tpr;
      const int row_raw = (c - CH) * Go + g;
      const bool live = row_raw < n;
      const int row = live ? row_raw : n - 1;
      const double qr = d.qraw[row];
      double acc[2];
      coop_prow2(d.pr_idx, d.pr_val, d.pr_ptr[row], d.pr_ptr[row + 1], tr, tpr, ox, xi, acc[0], acc[1]);
      coop_row_reduce<2>(acc, tpr, red);
      if (live && tr == 0) {
        ll_publish(d.epi_buf + 2 * (size_t)row, ox[row] * (0.5 * acc[0] + qr), tag);
        ll_publish(d.epi_buf + 2 * (size_t)(n + row), xi[row] * (0.5 * acc[1] + qr), tag);
      }
    }
  }
  COOP_STAMP(stamps, 12);
  {  // the workgroup's worst violation (max: exact whatever the order)
    for (int off = 32; off > 0; off >>= 1) vmax = fmax(vmax, __shfl_xor(vmax, off, 64));
    __syncthreads();
    if ((t & 63) == 0) red[t >> 6] = vmax;
    __syncthreads();
    if (t == 0) {
      double r = red[0];
      for (int k = 1; k < COOP_B / 64; k++) r = fmax(r, red[k]);
      ll_publish(d.epi_buf + 2 * (size_t)(2 * n + w), r, tag);
    }
    __syncthreads();
  }
}
// the first tester: every row value, the sums in the launches' order, ks_commit
template <int COOP_B>
__device__ __attribute__((noinline)) void coop_epi_commit(const CoopEpi *dp, unsigned long long *stamps, const int G, const unsigned tag,
                                                const int st, const int it, const double *lv0, double *s1, double *s2, double *red,
                                                const double *rec, int *s_fail) {
  const CoopEpi &d = *dp;
  const int t = threadIdx.x, n = d.n, M = d.M, p = d.n_int;
  lds_f64 *const ox = to_lds(s1), *const xi = to_lds(s1) + 1024;
  lds_f64 *const vals = to_lds(s2);  // xis is done with: sn | sn2 | maxima
  const lds_f64 *const ly = to_lds(lv0);
  COOP_STAMP(stamps, 8);
  // what does not depend on the row values first -- the digest of x, the slot's own solution -- while they travel
  // digest: is_int_feas + pick_nextvar (first largest fractional part)
  int cnt = 0, bestk = 0x7fffffff;
  double best = -1.0;
  for (int k = t; k < p; k += COOP_B) {
    const double v = ox[d.i_idx[k]], f = fabs(v - rint(v));
    cnt += f > d.eps_int;
    if (f > best) { best = f; bestk = k; }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double ob = __shfl_xor(best, off, 64);
    const int ok2 = __shfl_xor(bestk, off, 64);
    cnt += __shfl_xor(cnt, off, 64);
    if (ob > best || (ob == best && ok2 < bestk)) { best = ob; bestk = ok2; }
  }
  __shared__ double sb[COOP_B / 64];
  __shared__ int sk[COOP_B / 64], sc[COOP_B / 64], s_dig[2];
  if ((t & 63) == 0) { sb[t >> 6] = best; sk[t >> 6] = bestk; sc[t >> 6] = cnt; }
  __syncthreads();
  if (t == 0) {
    for (int k = 1; k < COOP_B / 64; k++) {
      cnt += sc[k];
      if (sb[k] > best || (sb[k] == best && sk[k] < bestk)) { best = sb[k]; bestk = sk[k]; }
    }
    s_dig[0] = cnt;
    s_dig[1] = bestk == 0x7fffffff ? -1 : bestk;
  }
  __syncthreads();
  const int int_inf = s_dig[0], nv = s_dig[1];
  for (int i = t; i < n; i += COOP_B) epi_st(d.a.x_s + i, ox[i], d.coh);
  for (int r = t; r < M; r += COOP_B) epi_st(d.a.y_s + r, d.cinv * d.E[r] * ly[r], d.coh);
  {
    const int ne = 2 * n + G;
    constexpr int KE = (COOP_EPI_ENTRIES + COOP_B - 1) / COOP_B;  // 5 (vals = lzs holds COOP_EPI_ENTRIES doubles)
    bool have[KE];
#pragma unroll
    for (int k = 0; k < KE; k++) have[k] = t + k * COOP_B >= ne;
    unsigned spins = 0;
    unsigned long long since = 0;
    static_assert(KE == 5, "ll_peek_wait5");
    for (;;) {
      // (all of the thread's entries are requested together -- one round trip per poll, not one per entry; an entry that
      //  has arrived, or lies beyond the end, reads entry 0 instead)
      const unsigned long long *ptr[KE];
      ll_u4 w[KE];
#pragma unroll
      for (int k = 0; k < KE; k++) ptr[k] = d.epi_buf + (have[k] ? 0 : 2 * (size_t)(t + k * COOP_B));
      ll_peek_wait5(ptr, w);
      bool all = true;
#pragma unroll
      for (int k = 0; k < KE; k++) {
        if (have[k]) continue;
        if (w[k].y == tag && w[k].w == tag) {
          vals[t + k * COOP_B] = __hiloint2double((int)w[k].z, (int)w[k].x);
          have[k] = true;
        } else {
          all = false;
        }
      }
      if (__syncthreads_and(all)) break;
      if (coop_expired(spins, since)) {
        *s_fail = 1;
        d.ctrl->pad = 12;
      }
      if (__syncthreads_or(*s_fail)) break;
    }
  }
  __syncthreads();
  if (*s_fail) return;
  COOP_STAMP(stamps, 9);
  // ---- ks_commit: sums in the launches' order, the x-only decisions of bound_and_branch, children, incumbent, record
  const double lower = coop_block_sum1024(vals, n, red);
  const double hobj = coop_block_sum1024(vals + n, n, red);
  __syncthreads();
  // (max: exact whatever the order -- spread over the threads: a serial walk through LDS behind a generic pointer was 14 us)
  double hviol = -1.7e308;
  for (int k = t; k < G; k += COOP_B) hviol = fmax(hviol, vals[2 * n + k]);
  for (int off = 32; off > 0; off >>= 1) hviol = fmax(hviol, __shfl_xor(hviol, off, 64));
  if ((t & 63) == 0) red[t >> 6] = hviol;
  __syncthreads();
  hviol = red[0];
  for (int k = 1; k < COOP_B / 64; k++) hviol = fmax(hviol, red[k]);
  __syncthreads();
  COOP_STAMP(stamps, 14);
  int action = 0, branched = 0;
  if (!(lower > d.a.upper)) {
    if (int_inf == 0) {
      action = 1;
    } else {
      if (hviol <= 0.0 && hobj < d.a.upper) action = 2;
      if (nv >= 0) {
        branched = 1;
        const double xv = ox[d.i_idx[nv]];
        for (int q = t; q < p; q += COOP_B) {
          const double lo = epi_ld(d.a.lo_s + q, d.coh), hi = epi_ld(d.a.hi_s + q, d.coh);
          epi_st(d.a.lo0 + q, lo, d.coh);
          epi_st(d.a.hi0 + q, q == nv ? floor(xv) : hi, d.coh);
          epi_st(d.a.lo1 + q, q == nv ? ceil(xv) : lo, d.coh);
          epi_st(d.a.hi1 + q, hi, d.coh);
        }
      }
    }
  }
  if (action) {
    const lds_f64 *src = action == 1 ? ox : xi;
    for (int i = t; i < n; i += COOP_B) epi_st(d.a.inc_x + i, src[i], d.coh);
  }
  // (what the other threads stored is read by later launches, behind this kernel's end; the record below is
  //  thread 0's own stores, released by its last one.  In a run the next node of the SAME launch reads them: written
  //  through at agent scope, and acknowledged before the record goes out)
  if (d.coh) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  COOP_STAMP(stamps, 15);
  if (t == 0) {
    Ctrl *c = d.ctrl;
    c->status = st;
    c->done = 1;
    c->int_inf = int_inf;
    c->nextvar = nv;
    c->lower = lower;
    c->heur_obj = hobj;
    c->heur_viol = hviol;
    // (residuals and objective of the deciding test: kept in LDS by this thread at the decision -- read back from the
    //  control block they would be three round trips to memory in front of the record)
    const lds_f64 *const rc = to_lds(rec);
    coop_record(d.a.dg, st, it, int_inf, nv, action, branched, lower, hviol, hobj, rc[0], rc[1], rc[2], d.t_node, d.a.seq);
    COOP_STAMP(stamps, 10);
  }
}

// (a real call, not inlined: inlined, its register demand moved spills into the exchange loop of the grid)
// RES: this wave's rows of Kc -- at most COOP_RC_R constraint rows of COOP_RC_S 16-byte pieces per lane and COOP_RV_R
// variable rows of COOP_RV_S -- and what their results are combined with (scalings, bounds, q) are loaded ONCE per launch
// and stay in registers: a test then touches memory for its operands only.  From memory every test, the rows took
// 17-21 us at config 2 whether they hit L2 or not (the loads queue behind the grid's polls); the decision is what the
// last iterations of every node wait for.  The host sets it when the rows fit (config 2 with 64 testers: 3 x 4 + 1 x 14
// pieces = 52 doubles per lane, + 20 for the scalars).  Same arithmetic in the same order as the rows from memory.
constexpr int COOP_RC_R = 3, COOP_RC_S = 4, COOP_RV_R = 1, COOP_RV_S = 16;
template <int COOP_B, int CPTF, bool RES>
__device__ __attribute__((noinline)) void coop_tester(const CoopTesterArgs *dp, const CoopEpi *ep, const int T, const int max_iter,
                                            const int check_every, const int final_check, const unsigned base, int *s_fail,
                                            double *lvp, double *lz) {
  // (both parameter blocks live in LDS, written once by the kernel: by value they are per-lane copies in scratch memory.
  //  Read through the LDS address space -- through the generic pointer every field access is a flat load -- and moved to
  //  scalar registers.)
  CoopTesterArgs d;
  {
    const auto *l = (const __attribute__((address_space(3))) CoopTesterArgs *)dp;
    d.coop_chk = coop_uni(l->coop_chk); d.coop_chz = coop_uni(l->coop_chz); d.coop_q = coop_uni(l->coop_q);
    d.coop_dec = coop_uni(l->coop_dec); d.prof = coop_uni(l->prof); d.Kc = coop_uni(l->Kc); d.Einv = coop_uni(l->Einv);
    d.E = coop_uni(l->E); d.Dinv = coop_uni(l->Dinv); d.D = coop_uni(l->D); d.l = coop_uni(l->l); d.u = coop_uni(l->u);
    d.q = coop_uni(l->q); d.ctrl = coop_uni(l->ctrl); d.n = coop_uni(l->n); d.M = coop_uni(l->M); d.ldw = coop_uni(l->ldw);
    d.c = coop_uni(l->c); d.cinv = coop_uni(l->cinv); d.eps_abs = coop_uni(l->eps_abs); d.eps_rel = coop_uni(l->eps_rel);
    d.eps_pinf = coop_uni(l->eps_pinf); d.eps_dinf = coop_uni(l->eps_dinf); d.epi = coop_uni(l->epi);
    d.stamps = coop_uni(l->stamps); d.res = coop_uni(l->res); d.run = coop_uni(l->run);
    d.coop_buf = coop_uni(l->coop_buf); d.coop_half = coop_uni(l->coop_half); d.NR = coop_uni(l->NR); d.lag = coop_uni(l->lag);
  }
  constexpr int NW = COOP_B / 64;
  // the kernel's arrays (the grid uses them in the epilogue), as LDS pointers again
  lds_f64 *const lv0 = to_lds(lvp), *const lv1 = to_lds(lvp) + 2048, *const lzl = to_lds(lz);
  __shared__ double qw[NW][NQ];
  __shared__ double qall[COOP_NT_MAX * NQ];
  __shared__ double qres[NQ];
  __shared__ int s_status;
  __shared__ double s_rec[3];  // the deciding test's residuals and objective (they go into the node's record)
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int M = d.M, N = d.n + d.M;
  const int j = (int)blockIdx.x - T, NT = (int)gridDim.x - T;
  // a wave's rows of Kc: loading them (with what their results are combined with), and applying them to the operands in
  // LDS -- the row's contribution to the 17 quantities.  lane q < 17 carries quantity q of this wave's rows (a row's values
  // are wave-uniform after the sums; each lane picks its own: seventeen accumulators per lane would not fit next to the
  // rows in flight)
  const double NEUTRAL = -1.7e308;
  const int Ne = N & ~1;
  auto rows_load = [&](auto RC, auto SC, const bool con, const int first, const int step, const int end, auto &a, auto &sc_inv,
                       auto &sc_dir, auto &lo, auto &up, auto &qv) {
    constexpr int R = decltype(RC)::value, S = decltype(SC)::value;
    const int cbeg = (con ? (M & ~1) : 0) + 2 * lane;
#pragma unroll
    for (int i = 0; i < R; i++) {
      const int rr = first + i * step;
      const int rc = rr < end ? rr : end - 1;  // clamped: no branch around the loads
      const double *row = d.Kc + (size_t)rc * d.ldw;
#pragma unroll
      for (int q = 0; q < S; q++) {
        const int c = cbeg + 128 * q;
        a[i][q] = c < Ne ? *reinterpret_cast<const double2 *>(row + c) : make_double2(0.0, 0.0);
      }
      sc_inv[i] = con ? d.Einv[rc] : d.Dinv[rc - M];
      sc_dir[i] = con ? d.E[rc] : d.D[rc - M];
      // (agent scope: in node mode the scaled bounds were written by their owners earlier in this launch)
      lo[i] = con ? __hip_atomic_load(d.l + rc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
      up[i] = con ? __hip_atomic_load(d.u + rc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
      qv[i] = con ? 0.0 : d.q[rc - M];
    }
  };
  auto rows_apply = [&](auto RC, auto SC, const bool con, const int first, const int step, const int end, const auto &a,
                        const auto &sc_inv, const auto &sc_dir, const auto &lo, const auto &up, const auto &qv, double &acc) {
    constexpr int R = decltype(RC)::value, S = decltype(SC)::value;
    const int cbeg = (con ? (M & ~1) : 0) + 2 * lane;
#pragma unroll
    for (int i = 0; i < R; i++) {
      const int rr = first + i * step;
      if (rr >= end) break;
      double sA1 = 0.0, sA2 = 0.0, sP1 = 0.0, sP2 = 0.0;
#pragma unroll
      for (int q = 0; q < S; q++) {
        const int c = cbeg + 128 * q;
        if (c >= Ne) continue;
        const coop_v2d p = *reinterpret_cast<const lds_v2d *>(lv0 + c);
        const coop_v2d s2 = *reinterpret_cast<const lds_v2d *>(lv1 + c);
        if (c < M) { sA1 = fma(a[i][q].x, p.x, sA1); sA2 = fma(a[i][q].x, s2.x, sA2); }
        else { sP1 = fma(a[i][q].x, p.x, sP1); sP2 = fma(a[i][q].x, s2.x, sP2); }
        if (c + 1 < M) { sA1 = fma(a[i][q].y, p.y, sA1); sA2 = fma(a[i][q].y, s2.y, sA2); }
        else { sP1 = fma(a[i][q].y, p.y, sP1); sP2 = fma(a[i][q].y, s2.y, sP2); }
      }
      if ((N & 1) && lane == 0) {  // last column of an odd width (always a variable column)
        const double a1 = d.Kc[(size_t)rr * d.ldw + N - 1];
        sP1 = fma(a1, lv0[N - 1], sP1);
        sP2 = fma(a1, lv1[N - 1], sP2);
      }
      sP1 = coop_wsum(sP1);
      sP2 = coop_wsum(sP2);
      const double si = sc_inv[i], sd = sc_dir[i];
      if (con) {
        const double z = lzl[rr], vproj = lv1[rr];
        const bool uinf = up[i] > QP_INFTY * QP_MIN_SCALING, linf = lo[i] < -QP_INFTY * QP_MIN_SCALING;
        const double adx = si * sP2;
        double val = NEUTRAL;
        val = lane == 0 ? fabs(si * (sP1 - z)) : val;
        val = lane == 1 ? fabs(si * sP1) : val;
        val = lane == 2 ? fabs(si * z) : val;
        val = lane == 3 ? fabs(sd * vproj) : val;
        val = lane == 4 ? (uinf ? -1.7e308 : adx) : val;
        val = lane == 5 ? -(linf ? 1.7e308 : adx) : val;
        acc = fmax(acc, val);
        if (lane == 13) acc += up[i] * fmax(vproj, 0.0) + lo[i] * fmin(vproj, 0.0);
      } else {
        sA1 = coop_wsum(sA1);
        sA2 = coop_wsum(sA2);
        const double x = lv0[rr], dx = lv1[rr];
        double val = NEUTRAL;
        val = lane == 6 ? fabs(si * (sP1 + qv[i] + sA1)) : val;
        val = lane == 7 ? fabs(si * sP1) : val;
        val = lane == 8 ? fabs(si * sA1) : val;
        val = lane == 9 ? fabs(si * qv[i]) : val;
        val = lane == 10 ? fabs(si * sP2) : val;
        val = lane == 11 ? fabs(si * sA2) : val;
        val = lane == 12 ? fabs(sd * dx) : val;
        if (lane < NQ_MAX) acc = fmax(acc, val);
        double add = 0.0;
        add = lane == 14 ? qv[i] * dx : add;
        add = lane == 15 ? x * sP1 : add;
        add = lane == 16 ? qv[i] * x : add;
        if (lane >= NQ_MAX) acc += add;
      }
    }
  };
  // RES: this wave's rows, once per launch (the bounds were written by their owners before the registration completed)
  double2 rca[COOP_RC_R][COOP_RC_S], rva[COOP_RV_R][COOP_RV_S];
  // (the scalars that go with the rows -- scalings, bounds, q: wave-uniform -- wait in LDS, not in registers)
  __shared__ double s_rsc[NW][5][COOP_RC_R], s_rsv[NW][5][COOP_RV_R];
  if constexpr (RES) {
    using std::integral_constant;
    const int step = NT * NW, fc = j + NT * wave, fv = M + j + NT * wave;
    double rc_si[COOP_RC_R], rc_sd[COOP_RC_R], rc_lo[COOP_RC_R], rc_up[COOP_RC_R], rc_q[COOP_RC_R];
    double rv_si[COOP_RV_R], rv_sd[COOP_RV_R], rv_lo[COOP_RV_R], rv_up[COOP_RV_R], rv_q[COOP_RV_R];
    rows_load(integral_constant<int, COOP_RC_R>{}, integral_constant<int, COOP_RC_S>{}, true, fc, step, M, rca, rc_si, rc_sd, rc_lo,
              rc_up, rc_q);
    rows_load(integral_constant<int, COOP_RV_R>{}, integral_constant<int, COOP_RV_S>{}, false, fv, step, N, rva, rv_si, rv_sd, rv_lo,
              rv_up, rv_q);
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < COOP_RC_R; i++) {
        s_rsc[wave][0][i] = rc_si[i]; s_rsc[wave][1][i] = rc_sd[i]; s_rsc[wave][2][i] = rc_lo[i]; s_rsc[wave][3][i] = rc_up[i];
        s_rsc[wave][4][i] = rc_q[i];
      }
#pragma unroll
      for (int i = 0; i < COOP_RV_R; i++) {
        s_rsv[wave][0][i] = rv_si[i]; s_rsv[wave][1][i] = rv_sd[i]; s_rsv[wave][2][i] = rv_lo[i]; s_rsv[wave][3][i] = rv_up[i];
        s_rsv[wave][4][i] = rv_q[i];
      }
    }
    __syncthreads();
  }
  int to_test = check_every > 0 ? check_every : -1;
  bool bounds_fresh = false;
  for (int it = 1; it <= max_iter; it++) {
    bool chk = final_check && it == max_iter;
    if (--to_test == 0) {
      chk = true;
      to_test = check_every;
    }
    if (!chk) continue;
    const unsigned tag = base + 1u + (unsigned)it;  // (round 0 of a launch carries its starting vector)
    const bool stamp = d.prof != nullptr && it == 75 && t == 0;  // debug timeline of the third test (100 MHz wall clock)
    unsigned long long *const st = d.prof + 8 * blockIdx.x;
    // ---- the operands: wait for the first entry with long naps (the grid is 25 iterations away from it most of
    //      the time), then gather everything
    {
      unsigned spins = 0;
      unsigned long long since = 0;
      for (;;) {
        const ll_u4 w = ll_peek_wait(d.coop_chk);
        if (w.y == tag && w.w == tag) break;
        if (__hip_atomic_load(&d.ctrl->pad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) *s_fail = 1;  // the grid gave up
        if (*s_fail) break;
        if (coop_expired(spins, since)) {
          *s_fail = 1;
          d.ctrl->pad = 7;
          break;
        }
        __builtin_amdgcn_s_sleep(8);
      }
    }
    if (*s_fail) return;
    if (stamp) st[0] = wall_clock64();
    if constexpr (RES) {
      // one column of the thread at a time (three entries: {y | x}, {proj(dy) | dx}, z): with the rows resident the twelve
      // results of an all-at-once poll would not fit next to them
      unsigned spins = 0;
      unsigned long long since = 0;
#pragma unroll 1
      for (int k = 0; k < CPTF; k++) {
        const int c = t + k * COOP_B;
        const unsigned long long *p0 = d.coop_chk + (c < N ? 4 * (size_t)c : 0), *p1 = p0 + (c < N ? 2 : 0),
                                 *p2 = c < M ? d.coop_chz + 2 * (size_t)c : d.coop_chk;
        for (;;) {
          ll_u4 w0, w1, w2;
          ll_peek_wait3x1(p0, p1, p2, w0, w1, w2);
          bool ok = c >= N || (w0.y == tag && w0.w == tag && w1.y == tag && w1.w == tag);
          if (c < M) ok = ok && w2.y == tag && w2.w == tag;
          if (ok) {
            if (c < N) {
              lv0[c] = __hiloint2double((int)w0.z, (int)w0.x);
              lv1[c] = __hiloint2double((int)w1.z, (int)w1.x);
            }
            if (c < M) lzl[c] = __hiloint2double((int)w2.z, (int)w2.x);
            break;
          }
          if (*s_fail) break;
          if (coop_expired(spins, since)) {
            *s_fail = 1;
            d.ctrl->pad = 8;
            break;
          }
        }
      }
    } else {
      // (all 3 CPTF entries are requested at every poll, also those that have arrived: the loads and the wait are one
      //  statement, see ll_peek_wait3; a column beyond the problem or a z of a variable row reads entry 0 instead)
      const unsigned long long *ptr[3 * CPTF];
#pragma unroll
      for (int k = 0; k < CPTF; k++) {
        const int c = t + k * COOP_B;
        ptr[3 * k] = d.coop_chk + (c < N ? 4 * (size_t)c : 0);
        ptr[3 * k + 1] = d.coop_chk + (c < N ? 4 * (size_t)c + 2 : 0);
        ptr[3 * k + 2] = c < M ? d.coop_chz + 2 * (size_t)c : d.coop_chk;
      }
      unsigned spins = 0;
      unsigned long long since = 0;
      for (;;) {
        ll_u4 w[3 * CPTF];
        ll_peek_wait3<CPTF>(ptr, w);
        bool all = true;
#pragma unroll
        for (int k = 0; k < CPTF; k++) {
          const int c = t + k * COOP_B;
          if (c >= N) continue;
          bool ok = w[3 * k].y == tag && w[3 * k].w == tag && w[3 * k + 1].y == tag && w[3 * k + 1].w == tag;
          if (c < M) ok = ok && w[3 * k + 2].y == tag && w[3 * k + 2].w == tag;
          if (ok) {
            lv0[c] = __hiloint2double((int)w[3 * k].z, (int)w[3 * k].x);
            lv1[c] = __hiloint2double((int)w[3 * k + 1].z, (int)w[3 * k + 1].x);
            if (c < M) lzl[c] = __hiloint2double((int)w[3 * k + 2].z, (int)w[3 * k + 2].x);
          } else {
            all = false;
          }
        }
        if (all) break;
        if (coop_expired(spins, since)) {
          *s_fail = 1;
          d.ctrl->pad = 8;
          break;
        }
      }
    }
    __syncthreads();
    if (*s_fail) return;
    if (stamp) st[1] = wall_clock64();
    if (j == 0) COOP_STAMP(d.stamps, 4);
    if constexpr (RES) {
      if (d.run && !bounds_fresh) {  // (workgroup-uniform)
        // a node of a run: rows_load above ran while the owners were still taking the node up.  They wrote its bounds before
        // they published anything under the node's tags, so behind the operands' arrival the bounds are there.
        if (lane == 0) {
          const int step = NT * NW, fc = j + NT * wave;
#pragma unroll
          for (int i = 0; i < COOP_RC_R; i++) {
            const int rr = fc + i * step, rc = rr < M ? rr : M - 1;
            s_rsc[wave][2][i] = __hip_atomic_load(d.l + rc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_rsc[wave][3][i] = __hip_atomic_load(d.u + rc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        bounds_fresh = true;
      }
    }
    // ---- this wave's rows of Kc on both operands: constraint rows j + NT (wave + NW i), variable rows M + the same;
    //      a row's pieces are 16 bytes per lane, and the pieces of R rows are requested before the first is used (the
    //      rows come from memory: one latency per batch, not per row).  Then the row's contribution to the 17 quantities.
    // lane q < 17 carries quantity q of this wave's rows (a row's values are wave-uniform after the sums; each lane
    // picks its own: seventeen accumulators per lane would not fit next to the rows in flight)
    double acc = (lane == 4 || lane == 5) ? -1.7e308 : 0.0;
    auto batch = [&](auto RC, auto SC, const bool con, int first, const int step, const int end) {
      constexpr int R = decltype(RC)::value, S = decltype(SC)::value;
      for (; first < end; first += R * step) {
        double2 a[R][S];
        double sc_inv[R], sc_dir[R], lo[R], up[R], qv[R];
        rows_load(RC, SC, con, first, step, end, a, sc_inv, sc_dir, lo, up, qv);
        rows_apply(RC, SC, con, first, step, end, a, sc_inv, sc_dir, lo, up, qv, acc);
      }
    };
    {
      using std::integral_constant;
      const int step = NT * NW, fc = j + NT * wave, fv = M + j + NT * wave;
      if constexpr (RES) {
        rows_apply(integral_constant<int, COOP_RC_R>{}, integral_constant<int, COOP_RC_S>{}, true, fc, step, M, rca, s_rsc[wave][0],
                   s_rsc[wave][1], s_rsc[wave][2], s_rsc[wave][3], s_rsc[wave][4], acc);
        rows_apply(integral_constant<int, COOP_RV_R>{}, integral_constant<int, COOP_RV_S>{}, false, fv, step, N, rva, s_rsv[wave][0],
                   s_rsv[wave][1], s_rsv[wave][2], s_rsv[wave][3], s_rsv[wave][4], acc);
      } else {
      const int n_cols = N - (M & ~1);  // width of a constraint row's Abar part
      if (n_cols <= 512) batch(integral_constant<int, 6>{}, integral_constant<int, 4>{}, true, fc, step, M);
      else if (n_cols <= 1024) batch(integral_constant<int, 3>{}, integral_constant<int, 8>{}, true, fc, step, M);
      else batch(integral_constant<int, 2>{}, integral_constant<int, 16>{}, true, fc, step, M);
      if (N <= 1024) batch(integral_constant<int, 4>{}, integral_constant<int, 8>{}, false, fv, step, N);
      else batch(integral_constant<int, 2>{}, integral_constant<int, 16>{}, false, fv, step, N);
      }
    }
    if (lane < NQ) qw[wave][lane] = acc;
    if (stamp) st[2] = wall_clock64();
    __syncthreads();
    if (j == 0) COOP_STAMP(d.stamps, 3);
    if (stamp) st[3] = wall_clock64();
    if (t < NQ) {
      double rq = qw[0][t];
      for (int w = 1; w < NW; w++) rq = t < NQ_MAX ? fmax(rq, qw[w][t]) : rq + qw[w][t];
      ll_publish(d.coop_q + (size_t)j * COOP_QS + 2 * t, rq, tag);
    }
    if (j == 0) {
      // tester 0: the NT partial results (fixed order), the decision, the record, the decision published
      {
        constexpr int KC = (COOP_NT_MAX * NQ + COOP_B - 1) / COOP_B;
        const int ne = NT * NQ;
        bool have[KC];
#pragma unroll
        for (int k = 0; k < KC; k++) have[k] = t + k * COOP_B >= ne;
        unsigned spins = 0;
        unsigned long long since = 0;
        static_assert(KC == 3, "ll_peek_waitn<3>");
        for (;;) {
          // (the thread's entries are requested together: one round trip per poll; one that has arrived reads entry 0)
          const unsigned long long *ptr[KC];
          ll_u4 w[KC];
#pragma unroll
          for (int k = 0; k < KC; k++) {
            const int e0 = t + k * COOP_B;
            ptr[k] = d.coop_q + (have[k] ? 0 : (size_t)(e0 / NQ) * COOP_QS + 2 * (e0 % NQ));
          }
          ll_peek_waitn<KC>(ptr, w);
          bool all = true;
#pragma unroll
          for (int k = 0; k < KC; k++) {
            if (have[k]) continue;  // (per lane)
            const int e0 = t + k * COOP_B;
            if (w[k].y == tag && w[k].w == tag) {
              qall[e0] = __hiloint2double((int)w[k].z, (int)w[k].x);
              have[k] = true;
            } else {
              all = false;
            }
          }
          if (all) break;
          if (coop_expired(spins, since)) {
            *s_fail = 1;
            d.ctrl->pad = 9;
            break;
          }
        }
      }
      __syncthreads();
      if (*s_fail) return;
      if (t < NQ) {
        double rq = qall[t];
        for (int m = 1; m < NT; m++) rq = t < NQ_MAX ? fmax(rq, qall[m * NQ + t]) : rq + qall[m * NQ + t];
        qres[t] = rq;
      }
      __syncthreads();
      if (t == 0) {
        Norms nm{qres[0], qres[1], qres[2], qres[3], qres[4], -qres[5], qres[6] * d.cinv, qres[7], qres[8], qres[9],
                 qres[10], qres[11], qres[12], qres[13], qres[14], qres[15], qres[16]};
        double obj;
        const int st = decide_status(d, nm, obj);
        // the decision first (what the grid's last iterations wait for); the control block -- read inside the launch only by
        // workgroup 0 behind the decision, at agent scope -- is written through at agent scope (a fence here is a write-back
        // of this XCD's whole L2 in front of the decision)
        {
          const int last_free = final_check ? max_iter - 1 : max_iter;
          const int pick = it + d.lag < last_free ? it + d.lag : (it > last_free ? it : last_free);
          const unsigned ptag = base + 1u + (unsigned)pick;
          // ({status, tag}: accepted by its tag, see the ring's description)
          ll_publish8(coop_ring_buf(d.coop_buf, ptag) + coop_ring_slot<COOP_B>(d.NR), ((unsigned long long)ptag << 32) | (unsigned)st);
        }
        ll_publish(d.coop_dec, (double)st, tag);
        Ctrl *c = d.ctrl;
        __hip_atomic_store(&c->iter, it, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&c->pri_res, nm.pri, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&c->dua_res, nm.dua, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&c->obj_val, obj, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (st) {
          __hip_atomic_store(&c->status, st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(&c->done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        COOP_STAMP(d.stamps, 5);
        s_rec[0] = nm.pri; s_rec[1] = nm.dua; s_rec[2] = obj;
        s_status = st;
      }
      __syncthreads();
    } else {
      // the other testers learn the outcome like the grid does
      if (t == 0) {
        unsigned spins = 0;
        unsigned long long since = 0;
        for (;;) {
          const ll_u4 w = ll_peek_wait(d.coop_dec);
          if (w.y == tag && w.w == tag) {
            s_status = (int)__hiloint2double((int)w.z, (int)w.x);
            break;
          }
          if (coop_expired(spins, since)) {
            *s_fail = 1;
            d.ctrl->pad = 10;
            s_status = -1;
            break;
          }
          __builtin_amdgcn_s_sleep(4);
        }
      }
      __syncthreads();
    }
    if (stamp) st[4] = wall_clock64();
    if (*s_fail) return;
    {
      // node mode: a relaxation that ends here with a solution (solved, or the iteration limit at the final test)
      // gets its epilogue at once, on the testers; anything else is left to the host's kernels (the grid says so)
      const int stn = s_status;
      const bool last = final_check && it == max_iter;
      if (d.epi && (stn == MIOSQP_QP_SOLVED || (stn == 0 && last))) {
        __syncthreads();
        unsigned long long *const stp = j == 0 ? d.stamps : nullptr;
        COOP_STAMP(stp, 13);
        coop_epi_rows<COOP_B>(ep, stp, (int)blockIdx.x, (int)gridDim.x, tag, lvp, lvp + 2048, lz, &qw[0][0]);
        if (j == 0)
          coop_epi_commit<COOP_B>(ep, stp, (int)gridDim.x, tag, stn == 0 ? MIOSQP_QP_MAX_ITER_REACHED : stn, it, lvp, lvp + 2048, lz,
                                  &qw[0][0], s_rec, s_fail);
        return;
      }
      if (d.epi && stn != 0) {
        // a certificate of infeasibility: the node has no solution, no children, nothing for the incumbent -- its
        // record is all there is (ks_commit with ok == false; the slot of such a node is never read)
        if (j == 0 && t == 0) {
          Ctrl *c = d.ctrl;
          const double nan = __builtin_nan("");
          c->int_inf = -1;
          c->nextvar = -1;
          c->lower = c->heur_obj = c->heur_viol = nan;
          coop_record(ep->a.dg, stn, it, -1, -1, 0, 0, nan, nan, nan, s_rec[0], s_rec[1], s_rec[2], ep->t_node, ep->a.seq);
          COOP_STAMP(d.stamps, 10);
        }
        return;
      }
    }
    if (s_status) return;
    __syncthreads();  // s_status and the scratch are rewritten by the next test
  }
}

// Start-up of a cooperative launch: every workgroup registers; workgroup 0 waits until the whole grid has (the proof that
// it is resident before anybody starts to depend on it) and releases everybody through a `go` word -- or, when that takes
// longer than ~100 ms, calls the launch off through an `abort` word.  ONE party decides, so a workgroup that shows up
// late cannot start a launch the others have already given up on.  The counter is never reset between launches of one
// grid size: launches of one engine are serialised and every workgroup of a launch registers exactly once (a late one
// too), so a launch's target is the next multiple of the grid size and identifies the launch (the host zeroes the words
// when the grid changes: reset_registration).  Words: [0] counter, [16] go, [32] abort (separate cache lines).
// Called by the first thread of every workgroup; *s_fail != 0 afterwards: the launch was called off.
__device__ __forceinline__ void coop_register(unsigned long long *reg, Ctrl *ctrl, int *s_fail) {
  *s_fail = 0;
  const unsigned G = gridDim.x;
  const unsigned long long old = __hip_atomic_fetch_add(reg, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned long long target = (old / G + 1ull) * G;
  unsigned spins = 0;
  unsigned long long since = 0;
  if (blockIdx.x == 0) {
    for (;;) {
      if (__hip_atomic_load(reg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= target) {
        __hip_atomic_store(reg + 16, target, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
      if (coop_expired(spins, since, COOP_LIMIT_REGISTER)) {
        __hip_atomic_store(reg + 32, target, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *s_fail = 1;
        ctrl->pad = 1;
        break;
      }
    }
  } else {
    for (;;) {
      if (__hip_atomic_load(reg + 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == target) break;
      if (__hip_atomic_load(reg + 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == target) {
        *s_fail = 1;
        break;
      }
      if (coop_expired(spins, since)) {  // workgroup 0 itself never ran: a hard error
        *s_fail = 1;
        ctrl->pad = 6;
        break;
      }
    }
  }
}

// TST: the termination test runs on d.coop_nt tester workgroups behind the exchange grid (blockIdx.x >= T), see above;
// otherwise inside the grid (coop_test).  RW rows of W' per workgroup, CPT columns per thread (NR <= COOP_B CPT),
// CPTF columns per thread in the gathers of the test's operands (N <= COOP_B CPTF).
//
// The workgroups of the exchange grid are coop_grid below; two kernels call it:
//   k_coop      one launch per relaxation (solve, solve_node, a node of the hosted search): the arguments are the kernel's;
//   k_coop_run  ONE launch per miosqp_qp_search_run (RUN): the grid stays resident, registers once, and takes node after node
//               from a mailbox the host writes (coop_mail_wait); coop_grid is then a real call per node (its register
//               allocation is the one of k_coop: a loop over nodes around the inlined body pushed the exchange loop's values
//               into scratch memory, r04) and reads Dev through the constant address space.
// ------------------------------------------------------------------------------------------
// The mailbox of k_coop_run.  The host writes a node as CM_HOST_WORDS tagged 16-byte entries {lo, tag, hi, tag} into coherent
// host memory (each 8-byte half is one atomic store; tag = the low 32 bits of the engine's mail counter); wave 0 of workgroup
// 0 polls them across PCIe, one entry per lane, and republishes them -- plus the exchange's tag base -- into device memory,
// where every other workgroup's wave 0 polls.  What a node reads of an earlier node's stores (slot store: bounds, warm start)
// goes through agent-scope stores / loads: the XCDs' L2s are not coherent with each other inside a launch.
enum {
  CM_LO_S = 0, CM_HI_S, CM_X_W, CM_Y_W, CM_X_S, CM_Y_S, CM_LO0, CM_HI0, CM_LO1, CM_HI1, CM_UPPER, CM_SEQ, CM_FLAGS, CM_STAMPS,
  CM_HOST_WORDS,              // what the host sends
  CM_BASE = CM_HOST_WORDS,    // added by workgroup 0: tag of the last exchange round that completed
  CM_WORDS
};
constexpr unsigned long long CM_FLAG_STOP = 1ull;
// what the run reports in coherent host memory next to the mailbox (word 0; word 1: wall clock at the kernel's entry)
enum { CR_RUNNING = 0, CR_STOPPED = 1, CR_CALLED_OFF = 2, CR_MAIL_TIMEOUT = 3, CR_FAILED = 4 };
constexpr unsigned long long COOP_LIMIT_MAIL = 100000000ull;  // ~1 s without a node from the host: the run ends by itself

struct CoopRun {  // device memory, constant while a run is resident; read through the constant address space
  Dev d;
  int max_iter, check_every, final_check, tpr_h, tpr_o, pad;
  unsigned long long *epi_buf;
  double *inc_x;
  SearchDigest *dg;
  const unsigned long long *mail_host;  // coherent host memory: CM_HOST_WORDS entries of two words
  unsigned long long *mail_dev;         // device memory: CM_WORDS entries
  unsigned long long *status_host;      // coherent host memory: CR_* | wall clock at entry
};
typedef const __attribute__((address_space(4))) CoopRun *coop_crun;
typedef const __attribute__((address_space(3))) CoopNode lds_node;

__device__ __forceinline__ ll_u4 ll_peek_sys_wait(const unsigned long long *slot) {  // host memory, across PCIe
  ll_u4 w;
  asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(w) : "v"(slot) : "memory");
  return w;
}
// the two flag words (s_fail, s_dec: 8 bytes at LDS address a_flags) and a row of eight partial sums (64 bytes at a_row),
// requested together and waited for once
typedef double coop_d2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void coop_flags_and_row(unsigned a_flags, unsigned a_row, long long &fl, coop_d2 &p0, coop_d2 &p1, coop_d2 &p2,
                                                   coop_d2 &p3) {
  asm volatile("ds_read_b64 %0, %5\n\tds_read_b128 %1, %6\n\tds_read_b128 %2, %6 offset:16\n\tds_read_b128 %3, %6 offset:32\n\t"
               "ds_read_b128 %4, %6 offset:48\n\ts_waitcnt lgkmcnt(0)"
               : "=&v"(fl), "=&v"(p0), "=&v"(p1), "=&v"(p2), "=&v"(p3) : "v"(a_flags), "v"(a_row) : "memory");
}
// slot-store accesses: plain in a launch per node (the data were written before the launch), agent scope in a run
template <bool RUN>
__device__ __forceinline__ double coop_ld(const double *p) {
  // (the pointer came out of LDS: said to be global memory, the load is a global_load, not a flat one)
  if constexpr (RUN) return __hip_atomic_load((const __attribute__((address_space(1))) double *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else return *p;
}

// Every thread of the workgroup calls it; wave 0 does the work.  POLLER: workgroup 0 of the grid.  Returns false when the wait
// expired (*s_fail set).  s_mail: CM_WORDS words of LDS, valid behind the barrier at the end.
template <bool POLLER>
__device__ __forceinline__ bool coop_mail_wait(const unsigned long long *mail_host, unsigned long long *mail_dev, const unsigned mtag,
                                               const unsigned base, unsigned long long *s_mail, int *s_fail) {
  if (threadIdx.x < 64) {
    const int k = threadIdx.x;
    unsigned long long val = 0;
    bool have;
    unsigned spins = 0;
    unsigned long long since = 0;
    if constexpr (POLLER) {
      have = k >= CM_HOST_WORDS;
      for (;;) {
        if (!have) {
          const ll_u4 w = ll_peek_sys_wait(mail_host + 2 * k);
          if (w.y == mtag && w.w == mtag) {
            val = ((unsigned long long)w.z << 32) | w.x;
            have = true;
          }
        }
        if (__all(have)) break;
        if (coop_expired(spins, since, COOP_LIMIT_MAIL)) { *s_fail = 2; break; }
      }
      if (k == CM_BASE) val = base;
      // (on expiry the others are told to stop: they would wait for their own second otherwise)
      if (*s_fail && k == CM_FLAGS) val = CM_FLAG_STOP;
      if (k < CM_WORDS) ll_publish(mail_dev + 2 * k, __longlong_as_double((long long)val), mtag);
    } else {
      have = k >= CM_WORDS;
      for (;;) {
        if (!have) {
          const ll_u4 w = ll_peek_wait(mail_dev + 2 * k);
          if (w.y == mtag && w.w == mtag) {
            val = ((unsigned long long)w.z << 32) | w.x;
            have = true;
          }
        }
        if (__all(have)) break;
        if (coop_expired(spins, since, 2 * COOP_LIMIT_MAIL)) { *s_fail = 2; break; }
        __builtin_amdgcn_s_sleep(16);
      }
    }
    if (k < CM_WORDS) s_mail[k] = val;
  }
  __syncthreads();
  return *s_fail == 0;
}
// the node of a run from its mail (one thread)
__device__ __forceinline__ void coop_node_from_mail(CoopNode *nd, const unsigned long long *s_mail, coop_crun blk) {
  nd->on = 1;
  nd->epi = 1;
  nd->tpr_h = blk->tpr_h;
  nd->tpr_o = blk->tpr_o;
  SearchArgs &a = nd->a;
  a.lo_s = (const double *)s_mail[CM_LO_S]; a.hi_s = (const double *)s_mail[CM_HI_S];
  a.x_w = (const double *)s_mail[CM_X_W]; a.y_w = (const double *)s_mail[CM_Y_W];
  a.x_s = (double *)s_mail[CM_X_S]; a.y_s = (double *)s_mail[CM_Y_S];
  a.lo0 = (double *)s_mail[CM_LO0]; a.hi0 = (double *)s_mail[CM_HI0];
  a.lo1 = (double *)s_mail[CM_LO1]; a.hi1 = (double *)s_mail[CM_HI1];
  a.inc_x = blk->inc_x;
  a.upper = __longlong_as_double((long long)s_mail[CM_UPPER]);
  a.dg = blk->dg;
  a.seq = s_mail[CM_SEQ];
  nd->epi_buf = blk->epi_buf;
  nd->stamps = (unsigned long long *)s_mail[CM_STAMPS];
}

template <class DV, class NV>
__device__ __forceinline__ void coop_fill_epi(CoopEpi *ep, const DV &d, const NV &nd, const int coh) {
  // (by one thread, where it is needed: the ~60 values it moves are not to be live anywhere else)
  *ep = CoopEpi{d.D, d.Dinv, d.E, d.Einv, d.pc_A, d.pr_val, d.qraw, d.root_l, d.root_u, d.int_pos, d.i_idx,
                d.pc_ptr, d.pc_idx, d.pr_ptr, d.pr_idx, d.ctrl, d.n, d.M, d.n_int, nd.tpr_h, nd.tpr_o, d.cinv,
                d.eps_int, d.eps_lin, SearchArgs{nd.a.lo_s, nd.a.hi_s, nd.a.x_w, nd.a.y_w, nd.a.x_s, nd.a.y_s, nd.a.lo0, nd.a.hi0,
                                                 nd.a.lo1, nd.a.hi1, nd.a.inc_x, nd.a.upper, nd.a.dg, nd.a.seq},
                nd.epi_buf, nullptr, coh, (unsigned long long)wall_clock64()};
}
template <class DV, class NV>
__device__ __forceinline__ void coop_fill_tester(CoopTesterArgs *ta, const DV &d, const NV &nd, const int run) {
  *ta = CoopTesterArgs{d.coop_chk, d.coop_chz, d.coop_q, d.coop_dec, d.prof, d.Kc, d.Einv, d.E, d.Dinv, d.D, d.l,
                       d.u, d.q, d.ctrl, d.n, d.M, d.ldw, d.c, d.cinv, d.eps_abs, d.eps_rel,
                       d.eps_pinf, d.eps_dinf, nd.on && nd.epi, nd.on ? nd.stamps : nullptr, d.coop_tres, run,
                       d.coop_buf, (unsigned long long)d.coop_half, d.coop_mg + d.n, d.coop_lag};
}
__device__ __forceinline__ void coop_ctrl_reset(Ctrl *c) {
  c->done = 0;
  c->pad = 0;
  c->status = MIOSQP_QP_UNSOLVED;
  c->iter = 0;
  c->pri_res = c->dua_res = c->obj_val = 0.0;
  c->lower = __builtin_nan("");
}

// LDS of the exchange grid and of the testers (one block per kernel; the testers' function gets pointers into it)
template <int RW, int NW, bool TST>
struct CoopLds {
  __attribute__((aligned(16))) double part[2][RW][NW];
  double s_ko[RW][6];  // the owners' iterates of the test iteration (restored when the test says stop)
  // the testers' operand staging; in node mode the grid's workgroups use it too (the epilogue's x, rounded x, scaled x)
  __attribute__((aligned(16))) double lvs[TST ? 2 * 2048 : 2];
  // (z operands of the test: M <= 2048; the epilogue's 2 n + G row values on the first tester: COOP_EPI_ENTRIES)
  __attribute__((aligned(16))) double lzs[TST ? COOP_EPI_ENTRIES : 2];
  // parameter blocks of the testers and of the in-launch epilogue (read through pointers: see coop_tester)
  CoopTesterArgs s_ta;
  CoopEpi s_ep;
  __attribute__((aligned(8))) int s_fail;  // (the exchange loop reads the two with one load: s_dec follows s_fail)
  int s_dec;
  // a run (k_coop_run): the node's mail and the node made of it
  unsigned long long s_mail[CM_WORDS];
  CoopNode s_nd;
};
static_assert(COOP_EPI_ENTRIES >= 2048, "lzs also stages the test's z operands (M <= 2048)");

// One relaxation on a workgroup of the exchange grid.  RUN: a node of k_coop_run -- `blk` / `mtag` / `base_in` describe the
// run, the node arrives by mail (after this workgroup's rows of W' have been requested: their latency hides behind the
// host's turn-around).  Returns the iterations carried out (the exchange tags go on from there), -1: the run ends here
// (a stop from the host, an expired wait).
template <int COOP_B, int RW, int CPT, int CPTF, bool TST, bool RUN, class DV, class NV, class LD>
__device__ __forceinline__ int coop_grid(const DV &d, const NV &nd, const int max_iter, const int check_every, const int final_check,
                                         LD &L, coop_crun blk, const unsigned mtag, const unsigned base_in) {
  // (debug stamps: nothing of them may live across the exchange loop -- its registers are spoken for)
#define GRID_STAMP(k) COOP_STAMP((nd.on && blockIdx.x == 0) ? nd.stamps : nullptr, k)
  if constexpr (!RUN) GRID_STAMP(0);
  constexpr int NW = COOP_B / 64;
  auto &part = L.part;
  auto &s_ko = L.s_ko;
  auto &lvs = L.lvs;
  auto &lzs = L.lzs;
  int &s_fail = L.s_fail;
  int &s_dec = L.s_dec;
  CoopEpi &s_ep = L.s_ep;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int M = d.M, mg = d.coop_mg, NR = mg + d.n;
  const int r0 = blockIdx.x * RW;
  auto fill_epi = [&]() { coop_fill_epi(&s_ep, d, nd, RUN ? 1 : 0); };
  // (debug phase clocks: only in the instantiations without testers -- in the others they would cost the exchange loop
  //  fourteen registers and a clock read per iteration)
  const bool prof = !TST && d.prof != nullptr;
  double Kr[RW][CPT], v[CPT];
#pragma unroll
  for (int k = 0; k < CPT; k++) {
    const int c = t + k * COOP_B;
    // unconditional loads from clamped addresses (a guarded load is a branch: RW x CPT dependent round
    // trips to HBM instead of one), masked afterwards
    const int cc = c < NR ? c : NR - 1;
    v[k] = 0.0;
#pragma unroll
    for (int rw = 0; rw < RW; rw++) {
      const int rc = r0 + rw < NR ? r0 + rw : NR - 1;
      const double w = d.coop_W[(size_t)rc * d.coop_ldw + cc];
      Kr[rw][k] = (c < NR && r0 + rw < NR) ? w : 0.0;
    }
  }
  // iterates of the row this thread owns (threads 0..RW-1): a general row, or a variable and its bound row
  const int r = r0 + t;
  const bool own = t < RW && r < NR;
  CoopOwner o{};
  o.rowc = -1;
  o.var = -1;
  if (own) {
    if (r < mg) {
      o.rowc = r;
    } else {
      o.var = r - mg;
      o.rowc = d.coop_brow ? d.coop_brow[o.var] : -1;
      o.aint = d.coop_aj ? d.rho * d.coop_aj[o.var] : 0.0;
      o.q = d.q[o.var];
    }
  }
  unsigned base;
  if constexpr (RUN) {
    // ---- a node of a run: the host's mail (the rows of W' requested above arrive meanwhile)
    if (t == 0) s_fail = 0;
    __syncthreads();  // (the previous node's readers of the node block are done)
    const bool ok = blockIdx.x == 0 ? coop_mail_wait<true>(blk->mail_host, blk->mail_dev, mtag, base_in, L.s_mail, &s_fail)
                                    : coop_mail_wait<false>(blk->mail_host, blk->mail_dev, mtag, base_in, L.s_mail, &s_fail);
    if (!ok || (L.s_mail[CM_FLAGS] & CM_FLAG_STOP) != 0) return -1;
    base = (unsigned)L.s_mail[CM_BASE];
    if (t == 0) {
      coop_node_from_mail(&L.s_nd, L.s_mail, blk);
      s_dec = 0;  // (every wave has read the previous node's behind the barriers above)
    }
    __syncthreads();
    GRID_STAMP(0);
  } else {
    base = *d.coop_tag;
  }
  if (!RUN && !nd.on) {
    if (own) {
      if (o.var >= 0) o.x = d.x[o.var];
      if (o.rowc >= 0) { o.z = d.z[o.rowc]; o.y = d.y[o.rowc]; o.lo = d.l[o.rowc]; o.up = d.u[o.rowc]; o.sw = d.wh[o.rowc]; }
    }
  } else {
    // ---- node mode: the prologue of the node (kernels_node.inc: ks_node_begin) by the owners themselves.  Bounds =
    // root bounds with the slot's integer rows, warm start = the parent's solution, scaled; z = Abar x for this
    // workgroup's general rows through the sparse rows with the launches' threads per row (the same bits); the bound
    // row of a variable has the one entry a_j: z_j = a_j x_i.
    __shared__ double s_z[RW];
    __shared__ double s_red[8];
    // (with testers in the launch their operand staging is free now: the scaled warm start D^-1 x goes there once, one
    //  coalesced load, and the rows below gather from LDS instead of chasing two global gathers per entry)
    if constexpr (TST) {
      if (r0 < mg) {
        for (int i = t; i < d.n; i += COOP_B) lvs[i] = d.Dinv[i] * coop_ld<RUN>(nd.a.x_w + i);
        __syncthreads();
      }
    }
    if (r0 < mg) {  // (workgroup-uniform) this workgroup owns general rows
      const int tpr = nd.tpr_h, G = COOP_B / tpr, g = t / tpr, tr = t % tpr;
      for (int c0 = 0; c0 < RW; c0 += G) {
        const int lr = c0 + g, row_raw = r0 + lr;
        const bool live = lr < RW && row_raw < mg;
        const int row = live ? row_raw : 0;
        double a0 = 0.0, a1 = 0.0;
        {
          const int *__restrict__ idx = d.pc_idx;
          const double *__restrict__ val = d.pc_A;
          const int s0 = d.pc_ptr[row], e0 = d.pc_ptr[row + 1];
          for (int k = s0 + 2 * tr; k < e0; k += 2 * tpr) {
            const double2 av = *reinterpret_cast<const double2 *>(val + k);
            const int2 jj = *reinterpret_cast<const int2 *>(idx + k);
            if constexpr (TST) {
              a0 = fma(av.x, lvs[jj.x], a0);
              a1 = fma(av.y, lvs[jj.y], a1);
            } else {
              a0 = fma(av.x, d.Dinv[jj.x] * coop_ld<RUN>(nd.a.x_w + jj.x), a0);
              a1 = fma(av.y, d.Dinv[jj.y] * coop_ld<RUN>(nd.a.x_w + jj.y), a1);
            }
          }
        }
        double acc[1] = {a0 + a1};
        coop_row_reduce<1>(acc, tpr, s_red);
        if (live && tr == 0) s_z[lr] = acc[0];
      }
      __syncthreads();
    }
    if (own) {
      if (o.var >= 0) o.x = d.Dinv[o.var] * coop_ld<RUN>(nd.a.x_w + o.var);
      if (o.rowc >= 0) {
        const int row = o.rowc;
        const double rl = row < d.m_orig ? d.root_l[row] : coop_ld<RUN>(nd.a.lo_s + (row - d.m_orig));
        const double ru = row < d.m_orig ? d.root_u[row] : coop_ld<RUN>(nd.a.hi_s + (row - d.m_orig));
        const double e = d.E[row];
        o.y = d.c * d.Einv[row] * coop_ld<RUN>(nd.a.y_w + row);
        o.lo = e * fmax(rl, -QP_INFTY);
        o.up = e * fmin(ru, QP_INFTY);
        o.z = o.var >= 0 ? d.coop_aj[o.var] * o.x : s_z[t];
        o.sw = o.z - d.rho_inv * o.y;
        // what the testers (and the host's epilogue kernels, when they are needed) read from memory
        __hip_atomic_store(d.l + row, o.lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(d.u + row, o.up, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        d.raw_l[row] = rl;
        d.raw_u[row] = ru;
      }
    }
    // (acknowledged before this workgroup registers: the testers read the bounds of their rows once, right behind the
    //  registration -- coop_tester<.., RES>)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // the control block starts afresh; written by the workgroup that will write it again when the test decides (the
    // first tester, or workgroup 0 when the test runs inside the grid): one line, one writer
    if (!TST && t == 0 && blockIdx.x == 0) coop_ctrl_reset(d.ctrl);
  }
  const bool con = own && o.rowc >= 0, var = own && o.var >= 0;
  if constexpr (!RUN) {
    if ((d.coop_dbg & 64) && blockIdx.x == 1) return 0;  // fault injection (tests): one workgroup never shows up
    // start-up: every workgroup registers (coop_register); the launches with testers count on words of their own, +64:
    // their grid is larger
    if (t == 0) {
      coop_register(d.coop_reg + (TST ? 64 : 0), d.ctrl, &s_fail);
      s_dec = 0;
    }
    __syncthreads();
  }
  GRID_STAMP(1);
  // (a run registered once, at its start)
  const bool called_off = RUN ? false : s_fail != 0;  // nothing has been modified: the iterates stay as they are
  // the loop's own scalars, each made a value of its own: as members of the wide kernel-argument loads they get
  // spilled to vector lanes and restored sixteen at a time in the middle of the publish path
  double rho = d.rho, rinv = d.rho_inv, alpha = d.alpha, sigma = d.sigma;
  asm volatile("" : "+s"(rho), "+s"(rinv), "+s"(alpha), "+s"(sigma));
  unsigned long long *ring = d.coop_buf;
  asm volatile("" : "+s"(ring));
  int nap = d.coop_nap;
  asm volatile("" : "+s"(nap));
  const unsigned my_slot = 8u * (unsigned)coop_ring_slot<COOP_B>(own ? r : 0);  // exchange ring: reduced index (bytes)
  const unsigned my_unit = 16u * (unsigned)t;
  const size_t chk_c = 4 * (size_t)(con ? o.rowc : 0), chk_v = 4 * (size_t)(var ? M + o.var : 0);  // test operands: full index

  // all CPT values of this thread's columns from one buffer of the ring: (CPT + 1) / 2 units of two columns
  // cnt: values of the round -- NR, or NR + 1 in the round a decision of the testers is picked up (see the loop):
  // column NR then holds {status, tag} and is accepted by its tag; it leaves as those bits (the caller takes the status)
  auto gather = [&](const unsigned long long *buf, unsigned tag, double (&out)[CPT], const int cnt) {
    constexpr int NU = (CPT + 1) / 2;
    bool have[2 * NU];
#pragma unroll
    for (int k = 0; k < 2 * NU; k++) have[k] = k >= CPT || t + k * COOP_B >= cnt;  // (a padding half is never waited for)
    // the decision's column, when it is one of this thread's: its high word must EQUAL the tag, where a value's 64 bits
    // must differ from the sentinel -- one comparison against eh[k] either way, the sense turned by isd[k]
    bool isd[CPT];
    unsigned eh[CPT];
#pragma unroll
    for (int k = 0; k < CPT; k++) {
      isd[k] = TST && cnt > NR && t + k * COOP_B == NR;
      eh[k] = isd[k] ? tag : COOP_SENT_HI;
    }
    unsigned spins = 0;
    unsigned long long since = 0;
    for (;;) {
      ll_u4 w[NU];
      if constexpr (TST) {
        // (loads whose completion the compiler cannot see, then the wait: nothing may be spilled in between --
        //  tools/check_coop_isa.py checks these instantiations)
#pragma unroll
        for (int u = 0; u < NU; u++)
          if (!(have[2 * u] && have[2 * u + 1])) w[u] = ll_peek(buf + 2 * (size_t)(u * COOP_B), my_unit);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      } else {
        // the in-grid test shares this function's registers: loads and wait as ONE statement (see ll_peek_wait);
        // a unit that has arrived, or lies beyond the problem, reads unit 0 of the buffer instead
        const unsigned long long *ptr[NU];
#pragma unroll
        for (int u = 0; u < NU; u++) ptr[u] = buf + ((have[2 * u] && have[2 * u + 1]) ? 0 : 2 * (size_t)(t + u * COOP_B));
        ll_peek_waitn<NU>(ptr, w);
      }
      bool all = true;
#pragma unroll
      for (int k = 0; k < CPT; k++)
        if (!have[k]) {
          const unsigned lo = (k & 1) ? w[k / 2].z : w[k / 2].x, hi = (k & 1) ? w[k / 2].w : w[k / 2].y;
          const bool c1 = hi != eh[k], c2 = lo != COOP_SENT_LO;
          if ((c1 | (c2 & !isd[k])) ^ isd[k]) {
            out[k] = __hiloint2double((int)hi, (int)lo);
            have[k] = true;
          } else {
            all = false;
          }
        }
      if (all) break;
      if (coop_expired(spins, since)) {
        s_fail = 1;
        d.ctrl->pad = 2;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
  };

  // round 0: the starting vector -- wh of a general row, rx_i + rho a_i wh(bound row) of a variable -- travels like every
  // later round (no workgroup reads another's iterates from memory: in node mode they were only just computed)
  if (!called_off) {
    const unsigned tag0 = base + 1u;
    if (own) {
      const double rx0 = var ? sigma * o.x - o.q : 0.0;
      const double pub0 = var ? (con ? fma(o.aint, o.sw, rx0) : rx0) : o.sw;
      ll_publish8(coop_ring_buf(ring, tag0), my_slot, (unsigned long long)__double_as_longlong(pub0));
      ll_publish8(coop_ring_buf(ring, tag0 + 2u), my_slot, COOP_SENTINEL);
    }
    for (int k = 0; k < nap; k++) __builtin_amdgcn_s_sleep(1);
    gather(coop_ring_buf(ring, tag0), tag0, v, NR);
    GRID_STAMP(2);
  }

  // TST: the test under way (0: none), its owner's iterates, the iteration the result belongs to (-1: the last one)
  // TST: the testers' decision on the test of iteration `pend` comes back THROUGH THE EXCHANGE: the first tester publishes
  // it as entry NR of the round `pick` = max(pend, min(pend + lag, last_free)) -- an entry nobody owns, polled in that round
  // only, by the thread whose columns it falls into -- so picking it up costs the loop neither a round trip of its own nor
  // a barrier: the thread leaves a decision that ends the node in s_dec, and every workgroup finds it behind the barrier
  // of iteration pick + 1 (or behind the loop) and drops the iterations after `pend`.  A decision that is late simply
  // holds that round's gather.  `last`: the test whose decision was picked up in the previous round.
  int pend = 0, it_rep = -1, last = 0, pick = -1;
  int lag = d.coop_lag, last_free = final_check ? max_iter - 1 : max_iter;
  // (values of their own, like the loop's other scalars: read from the constant block where they are used, they are a
  //  scalar load and its wait between the nap and the first poll of every iteration)
  asm volatile("" : "+s"(lag), "+s"(last_free));
  long long ph0 = 0, ph1 = 0, ph2 = 0, ph3 = 0, ph4 = 0, ph5 = 0, nchk = 0;  // debug phase clocks (thread 0, d.prof set)
  int it = 0, status = 0, to_test = check_every > 0 ? check_every : -1;
  for (it = 1; it <= max_iter && !called_off; it++) {
    const unsigned tag = base + 1u + (unsigned)it;
    bool chk = final_check && it == max_iter;
    if (--to_test == 0) {
      chk = true;
      to_test = check_every;
    }
    const long long c0 = prof ? clock64() : 0;
    double acc[RW];
#pragma unroll
    for (int rw = 0; rw < RW; rw++) {
      double a = Kr[rw][0] * v[0];
#pragma unroll
      for (int k = 1; k < CPT; k++) a = fma(Kr[rw][k], v[k], a);
      acc[rw] = a;
    }
    const double ws = wave_tsum<RW>(acc, lane);
    if (lane < RW) part[it & 1][coop_row<RW>(lane)][wave] = ws;
    __syncthreads();
    // ONE round trip to LDS behind the barrier, on the path every workgroup's publish waits for: the two flag words as one
    // load and, requested with them by every lane (no branch in front: a lane that owns nothing reads row 0), the row's
    // partial sums -- a flag tested first costs a round trip of its own
    // (one statement: written as plain loads the compiler splits the flag load in two and sinks the sums' loads behind
    //  the branches again)
    long long flags_v;
    double s;
    {
      static_assert(NW == 8, "coop_flags_and_row reads a row of eight partial sums");
      coop_d2 p0, p1, p2, p3;
      coop_flags_and_row((unsigned)(size_t)(__attribute__((address_space(3))) int *)&L.s_fail,
                         (unsigned)(size_t)(__attribute__((address_space(3))) double *)&part[it & 1][own ? t : 0][0], flags_v, p0, p1, p2, p3);
      s = p0.x + p0.y;
      s += p1.x; s += p1.y; s += p2.x; s += p2.y; s += p3.x; s += p3.y;
    }
    // (the same in every lane: kept in scalar registers, or the loop counter becomes a vector)
    const int f_fail = __builtin_amdgcn_readfirstlane((int)flags_v), f_dec = __builtin_amdgcn_readfirstlane((int)(flags_v >> 32));
    if (f_fail) break;
    if constexpr (TST) {
      if (f_dec) {  // this iteration and the ones after `last` are dropped (below); nothing of this one has been published
        it--;
        break;
      }
    }
    const long long c1 = prof ? clock64() : 0;
    unsigned long long *buf = coop_ring_buf(ring, tag);
    if (own) {
      double pub = 0.0, sc = s;  // sc: (nu + rho wh) of the constraint part
      if (var) {
        // x = alpha x~ + (1 - alpha) x; the variable's own entry of the next right-hand side, rx = sigma x - q
        const double xn = alpha * s + (1.0 - alpha) * o.x;
        pub = sigma * xn - o.q;
        o.dx = xn - o.x;
        o.x = xn;
        sc = o.aint * s;  // its bound row: rho a_j x~_i
      }
      if (con) {
        // z~ = z + (nu - y) / rho with nu = -rho wh + sc, relaxed and projected; the entry to publish,
        // wh+ = z+ - y+ / rho = 2 z+ - (z_r + y / rho), is formed before y+ (shortest path to the store)
        const double zt = o.z + rinv * ((sc - rho * o.sw) - o.y);
        const double zr = alpha * zt + (1.0 - alpha) * o.z;
        const double vv = zr + rinv * o.y;
        const double zn = fmin(fmax(vv, o.lo), o.up);
        const double whn = 2.0 * zn - vv;
        pub = var ? fma(o.aint, whn, pub) : whn;
        ll_publish8(buf, my_slot, (unsigned long long)__double_as_longlong(pub));
        o.dy = rho * (zr - zn);
        o.z = zn;
        o.y += o.dy;
        o.sw = whn;
      } else {
        ll_publish8(buf, my_slot, (unsigned long long)__double_as_longlong(pub));
      }
      // (this owner's slot two rounds on: nobody reads that buffer any more, see the ring's description)
      ll_publish8(coop_ring_buf(ring, tag + 2u), my_slot, COOP_SENTINEL);
      if (chk) {  // the test's operands travel with the same round: [y ; x] and [proj(dy) ; dx], full indices
        if (con) {
          ll_publish(d.coop_chk + chk_c, o.y, tag);
          ll_publish(d.coop_chk + chk_c + 2, coop_vproj(o.dy, o.lo, o.up), tag);
        }
        if (var) {
          ll_publish(d.coop_chk + chk_v, o.x, tag);
          ll_publish(d.coop_chk + chk_v + 2, o.dx, tag);
        }
        if constexpr (TST) {  // the testers have no iterates of their own: z travels too; the owner keeps iteration k
          if (con) ll_publish(d.coop_chz + (chk_c >> 1), o.z, tag);
          // (kept in LDS, not in registers: every thread would carry the copy, eight use it, once per test)
          s_ko[t][0] = o.z; s_ko[t][1] = o.y; s_ko[t][2] = o.dy; s_ko[t][3] = o.sw; s_ko[t][4] = o.x; s_ko[t][5] = o.dx;
          if (prof && it == 75) ph4 = (long long)wall_clock64();
        }
      }
    }
    const long long c2 = prof ? clock64() : 0;
    // nothing can have arrived yet, and polling now would only pull stale lines back into this XCD's L2
    // (each then costs its writer an invalidation): sleep through the first part of the hand-off latency.
    // The length (64-clock units) is calibrated at setup: the optimum is sharp (config 2: 2.05 us per
    // iteration at 16, 2.2 at 12 or 20, 2.45 at 0) and moves with the problem size and the code around it.
    for (int k = 0; k < nap; k++) __builtin_amdgcn_s_sleep(1);
    if constexpr (TST) {
      // a test is never started while another one is awaited (check_every > lag)
      if (chk) {
        pend = it;
        pick = it + lag < last_free ? it + lag : (it > last_free ? it : last_free);
      }
      const bool picking = it == pick;
      if (!(d.coop_dbg & 1)) gather(buf, tag, v, picking ? NR + 1 : NR);
      if (picking) {
#pragma unroll
        for (int k = 0; k < CPT; k++)
          if (t + k * COOP_B == NR) {
            const int dv = __double2loint(v[k]);  // {status, tag}
            if (dv) s_dec = dv;
            v[k] = 0.0;  // (its column of W' is zero, but the bits could be a NaN's)
          }
        last = pend;
        pend = 0;
        pick = -1;
      }
    } else {
      if (!(d.coop_dbg & 1)) gather(buf, tag, v, NR);
    }
    if (prof) {
      ph0 += c1 - c0; ph1 += c2 - c1; ph2 += clock64() - c2;
    }
    if constexpr (TST) {
      continue;
    } else {
    if (!chk) continue;

    // ---- termination test ----
    const long long k0 = prof ? clock64() : 0;
    {
      const CoopTest ta{d.coop_chk, d.coop_q, d.Kc, d.Einv, d.E, d.Dinv, d.D, d.coop_aj, d.ctrl, d.n, d.M, mg, d.ldw,
                        d.c, d.cinv, d.eps_abs, d.eps_rel, d.eps_pinf, d.eps_dinf};
      status = coop_test<COOP_B, RW, CPTF>(ta, tag, it, own, o, &s_fail);
    }
    if (prof) {
      ph3 += clock64() - k0;
      nchk++;
    }
    if (s_fail) break;
    if (status) break;
    }
  }
  if constexpr (TST) {
    // a decision that ends the node: found behind a barrier of the loop, or -- picked up in the last round (the final test
    // at the iteration limit; a test `lag` iterations before it) -- here.  The owners go back to the iterates of the test.
    if (!called_off) {
      if (it > max_iter) __syncthreads();
      const int dv = s_fail ? 0 : s_dec;
      if (dv) {
        status = dv;
        if (own) { o.z = s_ko[t][0]; o.y = s_ko[t][1]; o.dy = s_ko[t][2]; o.sw = s_ko[t][3]; o.x = s_ko[t][4]; o.dx = s_ko[t][5]; }
        it_rep = last;
      }
    }
  }
  GRID_STAMP(6);
  if (it > max_iter) it = max_iter;
  const int it_done = it;        // iterations carried out: the exchange tags go on from here
  if (it_rep >= 0) it = it_rep;  // iterations the result is made of
  if (prof && t == 0) {
    unsigned long long *out = d.prof + 8 * blockIdx.x;
    out[0] = ph0; out[1] = ph1; out[2] = ph2; out[3] = it; out[4] = ph3; out[5] = ph4; out[6] = nchk; out[7] = ph5;
  }
  if (own && !called_off) {
    if (con) { d.z[o.rowc] = o.z; d.y[o.rowc] = o.y; d.dy[o.rowc] = o.dy; d.wh[o.rowc] = o.sw; }
    if (var) { d.x[o.var] = o.x; d.dx[o.var] = o.dx; d.rx[o.var] = sigma * o.x - o.q; }
  }
  GRID_STAMP(7);
  // node mode: does the epilogue run inside this launch?  (the same answer in every workgroup, testers included: the
  // decision that ended the loop left a solution, or the final test at the iteration limit did not decide)
  const bool epi_here = TST && nd.on && nd.epi && !called_off && !s_fail &&
                        (status == MIOSQP_QP_SOLVED || (status == 0 && final_check && it_rep < 0));
  // (a certificate: the first tester writes the record by itself, there is no epilogue to run)
  const bool rec_here = epi_here || (TST && nd.on && nd.epi && !called_off && !s_fail && status != 0);
  if constexpr (TST) {
    if (epi_here) {
      // x~ of the test iteration from the test's operand buffer (entry {y | x} of full index M + i; published at that
      // iteration, untouched since: the next test would have been `check_every` > lag iterations later)
      if (t == 0) fill_epi();  // (read by coop_epi_rows behind the barrier below)
      const unsigned etag = base + 1u + (unsigned)it;
      const int n = d.n;
      for (int i0 = 0; i0 < n; i0 += COOP_B) {
        const int i = i0 + t;
        const unsigned long long *ptr = d.coop_chk + 4 * (size_t)(M + (i < n ? i : 0));
        unsigned spins = 0;
        unsigned long long since = 0;
        for (;;) {
          const ll_u4 w = ll_peek_wait(ptr);
          if (w.y == etag && w.w == etag) {
            if (i < n) lvs[M + i] = __hiloint2double((int)w.z, (int)w.x);
            break;
          }
          if (coop_expired(spins, since)) {  // (cannot happen: the entries were there when the testers decided)
            d.ctrl->pad = 13;
            break;
          }
        }
      }
      __syncthreads();
      coop_epi_rows<COOP_B>(&s_ep, nullptr, (int)blockIdx.x, (int)gridDim.x, etag, lvs, lvs + 2048, lzs, &part[0][0][0]);
    }
  }
  if (blockIdx.x == 0 && t == 0) {
    if (!called_off) *d.coop_tag = base + 1u + (unsigned)it_done;
    if (!final_check) d.ctrl->iter = it;
    if (nd.on) {
      // node mode: the host waits for a record.  The testers write it when they ran the epilogue; in every other case
      // (no testers, a certificate, a launch that was called off or timed out) this one tells the host to launch the
      // epilogue kernels -- or to redo the node -- itself.  (s_fail != 0 here also covers a time-out inside the loop.)
      if (!rec_here) {
        SearchDigest *g = nd.a.dg;
        // (a decision that ended the loop is this workgroup's own knowledge; the control block may still be on its way)
        g->status = status != 0 ? status : __hip_atomic_load(&d.ctrl->status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        g->iter = it;
        g->pad = __hip_atomic_load(&d.ctrl->pad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        g->todo = 1;
        g->t0 = g->t1 = 0;
        __hip_atomic_store(&g->seq, nd.a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
  }
  return (called_off || s_fail) ? -1 : it_done;
}

#undef GRID_STAMP

// TST: the termination test runs on d.coop_nt tester workgroups behind the exchange grid (blockIdx.x >= T), see above;
// otherwise inside the grid (coop_test).  RW rows of W' per workgroup, CPT columns per thread (NR <= COOP_B CPT),
// CPTF columns per thread in the gathers of the test's operands (N <= COOP_B CPTF).
// The exchange grid of a launch with testers, as a real call: like a node of k_coop_run (coop_grid_run below) the function has
// its own registers and schedule -- inlined into the kernel next to the testers' branch, the exchange loop of one
// instantiation or another came out with scratch accesses and 0.1 us per iteration slower (r06).  Dev is read where the
// launch put it, in the kernel-argument segment, through the constant address space; the node waits in LDS.
template <int COOP_B, int RW, int CPT, int CPTF>
__device__ __attribute__((noinline)) int coop_grid_one(const Dev *d_in, CoopLds<RW, COOP_B / 64, true> *Lp, const int max_iter,
                                                       const int check_every, const int final_check) {
  using LD = CoopLds<RW, COOP_B / 64, true>;
  typedef const __attribute__((address_space(4))) Dev *coop_cdev;
  const coop_cdev dp = (coop_cdev)coop_uni((unsigned long long)d_in);
  LD &L = *(LD *)(__attribute__((address_space(3))) LD *)Lp;
  // (arguments of a real call arrive in vector registers: the loop wants them in scalar ones)
  return coop_grid<COOP_B, RW, CPT, CPTF, true, false>(*dp, L.s_nd, coop_uni(max_iter), coop_uni(check_every), coop_uni(final_check), L,
                                                       (coop_crun) nullptr, 0u, 0u);
}

template <int COOP_B, int RW, int CPT, int CPTF, bool TST>
__global__ __launch_bounds__(COOP_B) void k_coop(Dev d, CoopNode nd, int max_iter, int check_every, int final_check) {
  if (!nd.on && d.ctrl->done) return;
  __shared__ CoopLds<RW, COOP_B / 64, TST> L;
  if constexpr (TST) {
    const int T = (int)gridDim.x - d.coop_nt;
    if ((int)blockIdx.x >= T) {
      // ---- a tester: its parameter blocks, the control block of the node (one line, one writer: the first tester writes
      //      it again when the test decides), the registration, then the tests of the whole launch
      const unsigned base = *d.coop_tag;
      if (threadIdx.x == 0) {
        coop_fill_tester(&L.s_ta, d, nd, 0);
        coop_fill_epi(&L.s_ep, d, nd, 0);
        if (nd.on && (int)blockIdx.x == T) coop_ctrl_reset(d.ctrl);
        coop_register(d.coop_reg + 64, d.ctrl, &L.s_fail);
      }
      __syncthreads();
      if (L.s_fail) return;
      if (L.s_ta.res) coop_tester<COOP_B, CPTF, true>(&L.s_ta, &L.s_ep, T, max_iter, check_every, final_check, base, &L.s_fail, L.lvs, L.lzs);
      else coop_tester<COOP_B, CPTF, false>(&L.s_ta, &L.s_ep, T, max_iter, check_every, final_check, base, &L.s_fail, L.lvs, L.lzs);
      return;
    }
  }
  if constexpr (TST) {
    // (Dev is the kernel's first argument: the segment's start)
    static_assert(alignof(Dev) <= 16, "Dev at offset 0 of the kernel-argument segment");
    if (threadIdx.x == 0) L.s_nd = nd;
    __syncthreads();
    coop_grid_one<COOP_B, RW, CPT, CPTF>((const Dev *)(const void *)__builtin_amdgcn_kernarg_segment_ptr(), &L, max_iter, check_every,
                                         final_check);
  } else {
    coop_grid<COOP_B, RW, CPT, CPTF, TST, false>(d, nd, max_iter, check_every, final_check, L, (coop_crun) nullptr, 0u, 0u);
  }
}

// ---- ONE launch per miosqp_qp_search_run: the grid and the testers stay resident and take node after node from the mailbox
// a node of the run on a workgroup of the exchange grid: a real call, see above.  The LDS block arrives as a generic pointer;
// cast to the LDS address space and back, the accesses through it are ds_* again (the compiler infers the address space;
// through the plain generic pointer every one of them would be a flat access, see to_lds)
template <int COOP_B, int RW, int CPT, int CPTF>
__device__ __attribute__((noinline)) int coop_grid_run(const CoopRun *blk_in, CoopLds<RW, COOP_B / 64, true> *Lp, const unsigned mtag,
                                                       const unsigned base) {
  using LD = CoopLds<RW, COOP_B / 64, true>;
  const coop_crun blk = (coop_crun)coop_uni((unsigned long long)blk_in);
  LD &L = *(LD *)(__attribute__((address_space(3))) LD *)Lp;
  return coop_grid<COOP_B, RW, CPT, CPTF, true, true>(blk->d, L.s_nd, blk->max_iter, blk->check_every, blk->final_check, L, blk, mtag,
                                                      base);
}

template <int COOP_B, int RW, int CPT, int CPTF>
__global__ __launch_bounds__(COOP_B) void k_coop_run(const CoopRun *blk_in, const unsigned mtag0) {
  __shared__ CoopLds<RW, COOP_B / 64, true> L;
  const coop_crun blk = (coop_crun)blk_in;
  const auto &d = blk->d;
  const int t = threadIdx.x;
  const int T = (int)gridDim.x - d.coop_nt;
  if ((d.coop_dbg & 64) && blockIdx.x == 1) return;  // fault injection (tests): one workgroup never shows up
  // the whole grid registers ONCE (coop_register: the proof that it is resident); called off, nothing has been touched
  if (t == 0) coop_register(d.coop_reg + 64, d.ctrl, &L.s_fail);
  __syncthreads();
  if (L.s_fail) {
    if (blockIdx.x == 0 && t == 0)
      __hip_atomic_store(blk->status_host, (unsigned long long)CR_CALLED_OFF, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    return;
  }
  unsigned mtag = mtag0;
  if ((int)blockIdx.x >= T) {
    // ---- a tester: node after node
    for (;;) {
      if (t == 0) L.s_fail = 0;
      __syncthreads();
      if (!coop_mail_wait<false>(blk->mail_host, blk->mail_dev, mtag, 0u, L.s_mail, &L.s_fail)) return;
      if ((L.s_mail[CM_FLAGS] & CM_FLAG_STOP) != 0) return;
      const unsigned base = (unsigned)L.s_mail[CM_BASE];
      if (t == 0) {
        coop_node_from_mail(&L.s_nd, L.s_mail, blk);
        coop_fill_tester(&L.s_ta, d, L.s_nd, 1);
        coop_fill_epi(&L.s_ep, d, L.s_nd, 1);
        if ((int)blockIdx.x == T) coop_ctrl_reset(d.ctrl);
      }
      __syncthreads();
      if (L.s_ta.res)
        coop_tester<COOP_B, CPTF, true>(&L.s_ta, &L.s_ep, T, blk->max_iter, blk->check_every, blk->final_check, base, &L.s_fail, L.lvs, L.lzs);
      else
        coop_tester<COOP_B, CPTF, false>(&L.s_ta, &L.s_ep, T, blk->max_iter, blk->check_every, blk->final_check, base, &L.s_fail, L.lvs, L.lzs);
      __syncthreads();
      if (L.s_fail) return;
      mtag++;
    }
  }
  unsigned base = *d.coop_tag;
  for (;;) {
    const int it_done = coop_grid_run<COOP_B, RW, CPT, CPTF>(blk_in, &L, mtag, base);
    if (it_done < 0) break;
    base += 1u + (unsigned)it_done;
    mtag++;
  }
  if (blockIdx.x == 0 && t == 0) {
    const int f = L.s_fail;
    const unsigned long long st = f == 0 ? CR_STOPPED : f == 2 ? CR_MAIL_TIMEOUT : CR_FAILED;
    __hip_atomic_store(blk->status_host, st, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// W' = W restricted to the rows and columns the exchange keeps (general rows 0 .. mg-1 and the variables, see above)
__global__ void k_coop_reduce_w(const double *__restrict__ W, int ldw, double *__restrict__ Wr, int ldr, int mg, int drop, int NR) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
  if (c >= ldr) return;
  const int rf = r < mg ? r : r + drop, cf = c < mg ? c : c + drop;
  Wr[(size_t)r * ldr + c] = c < NR ? W[(size_t)rf * ldw + cf] : 0.0;
}

// Kc = [ 0  Abar ; Abar^T  Pbar ] dense, N x ldw, from the dense copies of the scaled matrices
__global__ void k_build_kc(Dev d, double *Kc) {
  const int N = d.n + d.M, M = d.M;
  const int rr = blockIdx.y, c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= N) return;
  double a;
  if (rr < M) a = c < M ? 0.0 : d.f_Ad[(size_t)rr * d.ldn + (c - M)];
  else a = c < M ? d.f_Atd[(size_t)(rr - M) * d.ldm + c] : d.f_Pd[(size_t)(rr - M) * d.ldn + (c - M)];
  Kc[(size_t)rr * d.ldw + c] = a;
}
