// part of engine.hip (included there, not compiled alone): residual check of the explicit KKT inverse at set-up
// ------------------------------------------------------------------------------------------
// The register-resident solvers (k_coop, res_admm_w, k_tree_w) iterate on W = K^-1 formed explicitly
// (dense_setup.hip: ks_kkt_inverse) with sigma = 1e-6.  Applying an explicit inverse is not backward
// stable: the residual of  u = W r  grows with the conditioning of K, where the factor forms (sweeps with
// L, D) keep it at rounding level.  So the inverse is CHECKED before it is used: for NP probe vectors r
// (fixed pseudo-random entries in [-1, 1]) the device forms  u = W r  and the residual of the KKT system it
// claims to solve, from the scaled matrices themselves (Kc = [0 Abar ; Abar^T Pbar]):
//     [ wh ; rx ] = r,   [ nu + rho wh ; x~ ] = W r
//     res_c = Abar x~ - nu / rho - wh          (constraint rows)
//     res_x = Pbar x~ + sigma x~ + Abar^T nu - rx   (variable rows)
// and reports  max |res| / max |r|.  Above COOP_GUARD_TOL the engine does not use W: it falls back to the
// factor / product form (sweeps) and says so (miosqp_qp_get_inverse_guard, factor_stats).
// ------------------------------------------------------------------------------------------
constexpr int GUARD_NP = 3;
constexpr double COOP_GUARD_TOL = 1e-9;

// (the entries themselves: guard_probe.hpp, shared with the one-launch set-up of many models)
__device__ __forceinline__ double guard_probe(int p, int c) { return miosqp::guard_probe_value(p, c); }

// u[p][row] for every row of W: one wavefront per row, lanes stride the row, fixed-order butterfly
__global__ __launch_bounds__(256) void kg_apply(const double *__restrict__ W, int ldw, int N, int M, double rho,
                                                double *__restrict__ u) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  double acc[GUARD_NP] = {};
  const double *w = W + (size_t)row * ldw;
  for (int c = lane; c < N; c += 64) {
    const double a = w[c];
#pragma unroll
    for (int p = 0; p < GUARD_NP; p++) acc[p] = fma(a, guard_probe(p, c), acc[p]);
  }
#pragma unroll
  for (int p = 0; p < GUARD_NP; p++) {
    double s = acc[p];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) u[(size_t)p * N + row] = row < M ? s - rho * guard_probe(p, row) : s;  // nu | x~
  }
}

// residual of the KKT system on every row; out[0] = max |res| (as the bit pattern of a non-negative double)
__global__ __launch_bounds__(256) void kg_resid(const double *__restrict__ Kc, int ldw, int N, int M, double rho_inv,
                                                double sigma, const double *__restrict__ u,
                                                unsigned long long *__restrict__ out) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  double acc[GUARD_NP] = {};
  const double *k = Kc + (size_t)row * ldw;
  for (int c = lane; c < N; c += 64) {
    const double a = k[c];
#pragma unroll
    for (int p = 0; p < GUARD_NP; p++) acc[p] = fma(a, u[(size_t)p * N + c], acc[p]);
  }
  double worst = 0.0;
#pragma unroll
  for (int p = 0; p < GUARD_NP; p++) {
    double s = acc[p];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    const double ur = u[(size_t)p * N + row], r = guard_probe(p, row);
    const double res = row < M ? s - rho_inv * ur - r : s + sigma * ur - r;
    worst = fmax(worst, fabs(res));
  }
  if (lane == 0 && worst == worst) atomicMax(out, (unsigned long long)__double_as_longlong(worst));
  if (lane == 0 && worst != worst) atomicMax(out, 0x7FF0000000000000ull);  // NaN counts as infinite
}
