// Polishing of MANY small instances in one launch (C entry miosqp_qp_polish_many, engine.hip): instance b of the call
// -- its own q, l, u and (x, y) on the engine's P and A -- belongs to workgroup b from start to finish.  What
// miosqp_qp_polish_repair does for one large problem with about twenty launches per round and one host decision per
// round happens here inside the launch, for problems whose reduced system fits one workgroup's LDS (n + M <= 192):
//
//   1. the unscaled A, expanded to a dense M x n image in LDS, and the instance's vectors
//   2. z = A x and every row's class by OSQP's rule (k_pol_classify's), the input's two residual norms
//   3. per round: S = P + delta I + A_act^T A_act / delta as the packed lower triangle in LDS -- P's entries, delta on
//      the diagonal, then the active rows in ascending order, one fused multiply-add per entry (ks_schur_row's order: a
//      row that does not hold the variable adds an exact zero) --, a textbook right-looking LDL^T in place, and
//      1 + refine_iter solves by forward and back substitution against the residuals of the UNregularised system
//   4. the revision of the set from the polished point (k_pol_revise's rule, tol 1e-10), the next round from
//      xh = yh = 0 on the revised set, the stops 0 / 1 / 2 with the kept point of the round before a bad pivot
//   5. the acceptance test (k_pol_decide's), the record, and the polished point or the input bit for bit
//
// Stages are separated by workgroup barriers only.  Every sum has a fixed order that depends on (n, M) and the
// instance's data alone (a thread sums its row or column in ascending order; the four wavefronts' partial results meet
// in a fixed order), the counters are integer: an instance's answer has the same bits whatever B is and wherever it
// sits in the batch.  Plain fp64 HIP C++.
//
// Two entries share the body (polish_many_body.inc, included as text in both): k_pol_many, B instances on ONE engine's P
// and A from the kernel's arguments, and k_pol_many_m (C entry miosqp_qp_polish_models), workgroup b on model b of a table
// in device memory -- its own sizes, LDS carve-up, settings, P, A and vectors.
#include <hip/hip_runtime.h>

#include "polish_many.hpp"

namespace miosqp {
namespace {

constexpr double POLM_INFTY = 1e30;  // the engine's infinite bound
constexpr double POLM_TOL = 1e-10;   // the revision's tolerance: the floor of the acceptance test

__device__ __forceinline__ double polm_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
// maximum that keeps a NaN (fmax would drop it and a broken point would pass the acceptance test)
__device__ __forceinline__ double polm_max(double m, double v) { return (v > m || v != v) ? v : m; }
__device__ __forceinline__ int polm_tri(int i) { return (i * (i + 1)) >> 1; }

// maximum / sum over the workgroup of one value per thread: a butterfly per wavefront, the four results in order
__device__ __forceinline__ double polm_block_max(double v, double *red, int tid) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = polm_max(v, __shfl_xor(v, off, 64));
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  const double m = polm_max(polm_max(polm_max(red[0], red[1]), red[2]), red[3]);
  __syncthreads();
  return m;
}
__device__ __forceinline__ double polm_block_sum(double v, double *red, int tid) {
  v = polm_wave_sum(v);
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  const double s = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return s;
}

__device__ __forceinline__ int polm_block_count(bool on, double *red, int tid) {
  const int c = __popcll(__ballot(on));
  int *ri = (int *)red;
  if ((tid & 63) == 0) ri[tid >> 6] = c;
  __syncthreads();
  const int s = ri[0] + ri[1] + ri[2] + ri[3];
  __syncthreads();
  return s;
}

__global__ __launch_bounds__(256) void k_pol_many(PolManyArgs a) {
  extern __shared__ double polm_lds[];
  const size_t inst = blockIdx.x;
  constexpr bool POLM_TABLE = false;
  constexpr double polm_tau = 0.0;
#include "polish_many_body.inc"  // the body, shared with k_pol_many_m
}

// ------------------------------------------------------------------------------------------
// Polishes of DIFFERENT models in one launch (miosqp_qp_polish_models, host_polish_models.inc): workgroup b runs entry b
// of a table in device memory.  The host has written final pointers into every entry (the model's own patterns and P,
// its rows of A, vectors and output record in the call's arena), so nothing is offset here; sizes, the LDS carve-up,
// delta and the round limits are per workgroup.  The entry is read-only and its address depends on blockIdx.x alone:
// its fields arrive by scalar loads where they are used.  The body is k_pol_many's, so model b's answer has the bits
// of a one-instance launch on its own engine; only here a missing y is guessed from z (a.y NULL, tau > 0).
__global__ __launch_bounds__(256) void k_pol_many_m(const PolManyModel *__restrict__ tab) {
  extern __shared__ double polm_lds[];
  const PolManyArgs &a = tab[blockIdx.x].a;
  constexpr size_t inst = 0;
  constexpr bool POLM_TABLE = true;
  const double polm_tau = tab[blockIdx.x].tau;
#include "polish_many_body.inc"  // the body of k_pol_many
}

}  // namespace

size_t polish_many_lds_bytes(int n, int M) {
  return polm_lds_bytes(n, M);
}

int polish_many_launch(const PolManyArgs &a, void *stream) {
  static bool raised[64] = {};  // the dynamic-LDS ceiling is a property of (process, device, kernel)
  int dev = 0;
  hipError_t rc = hipGetDevice(&dev);
  if (rc != hipSuccess) return (int)rc;
  if (dev < 0 || dev >= 64 || !raised[dev]) {
    rc = hipFuncSetAttribute((const void *)k_pol_many, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (rc != hipSuccess) return (int)rc;
    if (dev >= 0 && dev < 64) raised[dev] = true;
  }
  hipLaunchKernelGGL(k_pol_many, dim3((unsigned)a.B), dim3(256), polish_many_lds_bytes(a.n, a.M), (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int polish_models_launch(const PolManyModel *table, int B, size_t lds_bytes, void *stream) {
  static bool raised[64] = {};
  int dev = 0;
  hipError_t rc = hipGetDevice(&dev);
  if (rc != hipSuccess) return (int)rc;
  if (dev < 0 || dev >= 64 || !raised[dev]) {
    rc = hipFuncSetAttribute((const void *)k_pol_many_m, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (rc != hipSuccess) return (int)rc;
    if (dev >= 0 && dev < 64) raised[dev] = true;
  }
  hipLaunchKernelGGL(k_pol_many_m, dim3((unsigned)B), dim3(256), lds_bytes, (hipStream_t)stream, table);
  return (int)hipGetLastError();
}

}  // namespace miosqp
