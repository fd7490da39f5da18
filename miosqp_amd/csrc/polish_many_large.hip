// Polishing of MANY instances in one launch beyond one workgroup's LDS (C entry miosqp_qp_polish_many_large,
// engine.hip).  k_pol_many (polish_many.hip) keeps an instance's reduced matrix S and a dense image of A in LDS and ends
// at n + M = 192; here S (n x ld, lower triangle) and the work vectors live in a slab of device scratch that belongs to
// ONE workgroup, and LDS holds only what a blocked algorithm stages there.  Workgroup w of the W launched takes
// instances w, w + W, .. one after the other, each from classification to record; no workgroup waits for another.
//
//   1. z = A x from the sparse rows (pc_*), every row's class by OSQP's rule, the input's two residual norms
//   2. per round: S = P + delta I, then the active rows in ascending order in chunks of 32 -- a chunk's rows are
//      scattered to a dense 32 x n image in the slab and added as one rank-32 update by 64 x 64 tiles staged in LDS --;
//      a blocked right-looking LDL^T (panels of 32: the diagonal block is factorised in LDS, a thread per row solves
//      the panel against it, the trailing update streams S through the same tile code); 1 + refine_iter solves by
//      blocked substitution (a block's rows gather their dot products with lanes striding S, the 32 x 32 diagonal block
//      is solved in LDS by one wavefront) against the residuals of the UNregularised system
//   3. the revision (tol 1e-10), the next round from xh = yh = 0, the stops 0 / 1 / 2 with the kept point of the round
//      before a bad pivot
//   4. the acceptance test, the record, the polished point or the input bit for bit
//
// Stages are separated by workgroup barriers only.  Every sum has a fixed order that depends on (n, M) and the
// instance's data alone (lanes stride a sparse row and meet in an xor butterfly; a tile entry sums its 32 terms in
// ascending order; partial sums of different threads meet in a fixed order), the counters are integer and there are no
// floating-point atomics: an instance's answer has the same bits whatever B is, wherever it sits in the batch and
// whichever slab it lands in.  Plain fp64 HIP C++.
//
// Two entries share the body (polish_many_large_body.inc, included as text in both): k_pol_many_g, B instances on ONE
// engine's P and A from the kernel's arguments, and k_pol_many_gm (C entry miosqp_qp_polish_models_large), the entries
// of a table in device memory -- each its own sizes, slab carve-up, settings, P, A and vectors.
#include <hip/hip_runtime.h>

#include "polish_many_large.hpp"

namespace miosqp {
namespace {

constexpr double POLG_INFTY = 1e30;  // the engine's infinite bound
constexpr double POLG_TOL = 1e-10;   // the revision's tolerance: the floor of the acceptance test
constexpr int NB = POLG_NB;          // panel width of the factorisation, block of the substitutions, rows of a chunk
constexpr int TS = 64;               // tile of the rank-32 updates
constexpr int TP = TS + 1;           // padded tile row in LDS
constexpr int TD = NB + 1;           // padded row of the diagonal block in LDS

__device__ __forceinline__ double polg_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
// maximum that keeps a NaN (fmax would drop it and a broken point would pass the acceptance test)
__device__ __forceinline__ double polg_max(double m, double v) { return (v > m || v != v) ? v : m; }

// maximum / sum of arr[0 .. len): thread t takes entries t, t + 256, .. in order, a butterfly per wavefront, the four
// results in order
__device__ __forceinline__ double polg_block_max(const double *arr, int len, double *red, int tid) {
  double v = 0.0;
  for (int i = tid; i < len; i += 256) v = polg_max(v, arr[i]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = polg_max(v, __shfl_xor(v, off, 64));
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  const double m = polg_max(polg_max(polg_max(red[0], red[1]), red[2]), red[3]);
  __syncthreads();
  return m;
}
__device__ __forceinline__ double polg_block_sum(const double *arr, int len, double *red, int tid) {
  double v = 0.0;
  for (int i = tid; i < len; i += 256) v += arr[i];
  v = polg_wave_sum(v);
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  const double s = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return s;
}
__device__ __forceinline__ int polg_block_count(int c, double *red, int tid) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
  int *ri = (int *)red;
  if ((tid & 63) == 0) ri[tid >> 6] = c;
  __syncthreads();
  const int s = ri[0] + ri[1] + ri[2] + ri[3];
  __syncthreads();
  return s;
}

// S[i][j] += sign * sum over c < 32 of (wscale * Wsrc[c][i]) * Lsrc[c][j] for r0 <= j <= i < n, by 64 x 64 tiles: both
// operands of a tile are staged in LDS (k-major, as they lie in the slab), thread (ty, tx) holds the 4 x 4 entries
// (ty + 16 a, tx + 16 b) and sums c in ascending order.  Ends behind a barrier.  ENTRY: the kernel that calls it (each
// of the two entries has its own copy with one caller, as before there were two: a copy shared by both kernels is
// compiled against the general calling convention, 924 bytes of scratch per lane instead of 92).
template <bool ENTRY>
__device__ __noinline__ void polg_rank_update(double *S, int ld, int n, int r0, const double *Wsrc, const double *Lsrc,
                                                 int ldw, double wscale, double sign, double *Wt, double *Lt, int tid) {
  const int ty = tid >> 4, tx = tid & 15;
  const int nt = (n - r0 + TS - 1) / TS;
  for (int ti = 0; ti < nt; ti++)
    for (int tj = 0; tj <= ti; tj++) {
      const int i0 = r0 + TS * ti, j0 = r0 + TS * tj;
      for (int e = tid; e < NB * TS; e += 256) {
        const int c = e >> 6, r = e & 63;
        Wt[c * TP + r] = i0 + r < n ? wscale * Wsrc[(size_t)c * ldw + i0 + r] : 0.0;
        Lt[c * TP + r] = j0 + r < n ? Lsrc[(size_t)c * ldw + j0 + r] : 0.0;
      }
      __syncthreads();
      double acc[4][4];
#pragma unroll
      for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) acc[a][b] = 0.0;
#pragma unroll 4
      for (int c = 0; c < NB; c++) {
        double wv[4], lv[4];
#pragma unroll
        for (int a = 0; a < 4; a++) wv[a] = Wt[c * TP + ty + 16 * a];
#pragma unroll
        for (int b = 0; b < 4; b++) lv[b] = Lt[c * TP + tx + 16 * b];
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
          for (int b = 0; b < 4; b++) acc[a][b] = fma(wv[a], lv[b], acc[a][b]);
      }
#pragma unroll
      for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) {
          const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
          if (i < n && j <= i) S[(size_t)i * ld + j] = fma(sign, acc[a][b], S[(size_t)i * ld + j]);
        }
      __syncthreads();
    }
}

// The panel below a factorised diagonal block T (32 x 32 in LDS: L_kk below its diagonal, the pivots on it), a thread per
// row i >= j0 + 32: W = S_ik L_kk^-T (= L D) and L = W D^-1, columns in ascending order; both go to the slab k-major for
// the trailing update, L also into S.  A function of its own: its 32 + 32 live values are not the kernel's.
template <bool ENTRY>
__device__ __noinline__ void polg_panel_solve(double *S, int ld, int n, int j0, double *Wp, double *Lp, int ldw,
                                              const double *T, int tid) {
  for (int i = j0 + NB + tid; i < n; i += 256) {
    double w[NB];
    double *row = S + (size_t)i * ld + j0;
    asm volatile("" ::: "memory");  // (the block in LDS is read where it is used, not held in 496 registers)
#pragma unroll
    for (int c = 0; c < NB; c++) w[c] = row[c];
#pragma unroll
    for (int c = 1; c < NB; c++) {
      double acc = w[c];
#pragma unroll
      for (int c2 = 0; c2 < c; c2++) acc = fma(-w[c2], T[c * TD + c2], acc);
      w[c] = acc;
    }
#pragma unroll
    for (int c = 0; c < NB; c++) {
      const double l = w[c] / T[c * TD + c];
      row[c] = l;
      Wp[(size_t)c * ldw + i] = w[c];
      Lp[(size_t)c * ldw + i] = l;
    }
  }
}

__global__ __launch_bounds__(256, 2) void k_pol_many_g(PolManyLargeArgs g) {
  __shared__ double sh_w[NB * TP], sh_l[NB * TP], sh_t[NB * TD], sh_c[NB], sh_red[8];
  double *slab = g.slab + (size_t)blockIdx.x * g.slab_doubles;
  constexpr bool POLG_TABLE = false;
  constexpr double polg_tau = 0.0;
  for (size_t inst = blockIdx.x; inst < (size_t)g.a.B; inst += gridDim.x) {
#include "polish_many_large_body.inc"  // the body, shared with k_pol_many_gm
  }
}

// ------------------------------------------------------------------------------------------
// Polishes of DIFFERENT larger models in one launch (miosqp_qp_polish_models_large, host_polish_models_large.inc):
// workgroup w of the W launched runs entries w, w + W, .. of a table in device memory, one after the other, each from
// classification to record in slab w, which is sized for the largest model of the call.  The host has written final
// pointers into every entry (the model's own patterns and P, its rows of A both ways, vectors and output record in the
// call's arena), so nothing is offset here; sizes, the slab's carve-up, delta and the round limits are per entry.  An
// entry is read-only and its address is uniform over the workgroup: its fields arrive by scalar loads where they are
// used.  The body is k_pol_many_g's, so an entry's answer has the bits of a one-instance launch on its own engine
// whatever B and W are and wherever the entry sits; only here a missing y is guessed from z (a.y NULL, tau > 0).
__global__ __launch_bounds__(256, 2) void k_pol_many_gm(const PolManyLargeModel *__restrict__ tab, int B, double *slabs,
                                                       size_t slab_doubles) {
  __shared__ double sh_w[NB * TP], sh_l[NB * TP], sh_t[NB * TD], sh_c[NB], sh_red[8];
  double *slab = slabs + (size_t)blockIdx.x * slab_doubles;
  constexpr bool POLG_TABLE = true;
  constexpr size_t inst = 0;
  for (int ent = blockIdx.x; ent < B; ent += gridDim.x) {
    const PolManyLargeArgs &g = tab[ent].g;
    const double polg_tau = tab[ent].tau;
#include "polish_many_large_body.inc"  // the body of k_pol_many_g
  }
}

}  // namespace

int polish_many_large_launch(const PolManyLargeArgs &g, int W, void *stream) {
  hipLaunchKernelGGL(k_pol_many_g, dim3((unsigned)W), dim3(256), 0, (hipStream_t)stream, g);
  return (int)hipGetLastError();
}

int polish_models_large_launch(const PolManyLargeModel *table, int B, int W, double *slabs, size_t slab_doubles, void *stream) {
  hipLaunchKernelGGL(k_pol_many_gm, dim3((unsigned)W), dim3(256), 0, (hipStream_t)stream, table, B, slabs, slab_doubles);
  return (int)hipGetLastError();
}

}  // namespace miosqp
