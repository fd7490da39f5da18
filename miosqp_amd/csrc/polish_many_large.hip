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
#include <hip/hip_runtime.h>

#include "polish_many_large.hpp"

namespace miosqp {
namespace {

constexpr double POLG_INFTY = 1e30;  // the engine's infinite bound
constexpr double POLG_TOL = 1e-10;   // the revision's tolerance: the floor of the acceptance test
constexpr int NB = 32;               // panel width of the factorisation, block of the substitutions, rows of a chunk
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

// one workgroup's slab, in doubles from its start
struct PolgSlab {
  int ld, ldw;
  size_t S, Wp, Lp, xh, t, v, xk, dd, ocol, dcol, yh, r2, yk, prow, act, cls, total;
};
__host__ __device__ inline PolgSlab polg_layout(int n, int M) {
  PolgSlab o;
  o.ld = (n + 7) & ~7;
  o.ldw = o.ld;
  const size_t nn = (size_t)o.ld, mm = ((size_t)M + 7) & ~(size_t)7;
  size_t c = 0;
  o.S = c; c += (size_t)n * nn;
  o.Wp = c; c += NB * nn;
  o.Lp = c; c += NB * nn;
  o.xh = c; c += nn;
  o.t = c; c += nn;
  o.v = c; c += nn;
  o.xk = c; c += nn;
  o.dd = c; c += nn;
  o.ocol = c; c += nn;
  o.dcol = c; c += nn;
  o.yh = c; c += mm;
  o.r2 = c; c += mm;
  o.yk = c; c += mm;
  o.prow = c; c += mm;
  o.act = c; c += mm / 2 + 8;  // M ints
  o.cls = c; c += mm / 4 + 8;  // two class arrays of M bytes
  o.total = (c + 31) & ~(size_t)31;
  return o;
}

// S[i][j] += sign * sum over c < 32 of (wscale * Wsrc[c][i]) * Lsrc[c][j] for r0 <= j <= i < n, by 64 x 64 tiles: both
// operands of a tile are staged in LDS (k-major, as they lie in the slab), thread (ty, tx) holds the 4 x 4 entries
// (ty + 16 a, tx + 16 b) and sums c in ascending order.  Ends behind a barrier.
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
  const PolManyArgs &a = g.a;
  const int n = a.n, M = a.M, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const PolgSlab o = polg_layout(n, M);
  const int ld = o.ld, ldw = o.ldw;
  double *slab = g.slab + (size_t)blockIdx.x * g.slab_doubles;
  double *S = slab + o.S, *Wp = slab + o.Wp, *Lp = slab + o.Lp, *xh = slab + o.xh, *t = slab + o.t, *v = slab + o.v;
  double *xk = slab + o.xk, *dd = slab + o.dd, *ocol = slab + o.ocol, *dcol = slab + o.dcol, *yh = slab + o.yh;
  double *r2 = slab + o.r2, *yk = slab + o.yk, *prow = slab + o.prow, *red = sh_red;
  int *act = (int *)(slab + o.act);
  signed char *clsbuf[2] = {(signed char *)(slab + o.cls), (signed char *)(slab + o.cls) + M};
  const double delta = a.delta, inv_delta = a.inv_delta;

  // sparse dot products by one wavefront (every lane returns them): row r of A, row i of P, column i of A (unrolled so
  // that four index / value / gather loads are in flight; a lane's terms keep their order)
  auto a_row = [&](int r, const double *vec) {
    double acc = 0.0;
#pragma unroll 4
    for (int k = a.pc_ptr[r] + lane; k < a.pc_ptr[r + 1]; k += 64) acc = fma(a.A[k], vec[a.pc_idx[k]], acc);
    return polg_wave_sum(acc);
  };
  auto p_row = [&](int i, const double *vec) {
    double acc = 0.0;
#pragma unroll 4
    for (int k = a.pr_ptr[i] + lane; k < a.pr_ptr[i + 1]; k += 64) acc = fma(a.pr_val[k], vec[a.pr_idx[k]], acc);
    return polg_wave_sum(acc);
  };
  auto a_col = [&](int i, const double *vec) {
    double acc = 0.0;
#pragma unroll 4
    for (int k = g.pv_ptr[i] + lane; k < g.pv_ptr[i + 1]; k += 64) acc = fma(g.At[k], vec[g.pv_idx[k]], acc);
    return polg_wave_sum(acc);
  };

  for (size_t inst = blockIdx.x; inst < (size_t)a.B; inst += gridDim.x) {
    const double *qg = a.q ? a.q + inst * n : a.q_engine;
    const double *lg = a.l + inst * M, *ug = a.u + inst * M, *xg = a.x + inst * n, *yg = a.y + inst * M;

    // the residuals and the objective of a point (X, Y), over ALL rows (every thread gets them)
    double j_pri = 0.0, j_dua = 0.0, j_obj = 0.0;
    auto judge_norms = [&](const double *X, const double *Y) {
      for (int r = wv; r < M; r += 4) {
        const double z = a_row(r, X);
        if (lane == 0) prow[r] = polg_max(polg_max(0.0, lg[r] - z), z - ug[r]);
      }
      for (int i = wv; i < n; i += 4) {
        const double px = p_row(i, X), aty = a_col(i, Y);
        if (lane == 0) {
          dcol[i] = fabs((px + qg[i]) + aty);
          ocol[i] = X[i] * fma(0.5, px, qg[i]);
        }
      }
      __syncthreads();
      j_pri = polg_block_max(prow, M, red, tid);
      j_dua = polg_block_max(dcol, n, red, tid);
      j_obj = polg_block_sum(ocol, n, red, tid);
    };

    // ---- 1. the set guessed from (x, y) and the input's residuals
    for (int i = tid; i < n; i += 256) xh[i] = 0.0;
    for (int r = tid; r < M; r += 256) yh[r] = 0.0;
    for (int r = wv; r < M; r += 4) {
      const double z = a_row(r, xg);
      if (lane == 0) {
        const double l = lg[r], u = ug[r], y = yg[r];
        signed char c = 0;
        if (l > -POLG_INFTY && (l == u || z - l < -y)) c = -1;
        else if (u < POLG_INFTY && u - z < y) c = 1;
        clsbuf[0][r] = c;
      }
    }
    judge_norms(xg, yg);
    const double pri0 = j_pri, dua0 = j_dua;
    auto judge = [&](const double *X, const double *Y) {
      judge_norms(X, Y);
      return !(j_pri <= fmax(pri0, 1e-10)) ? 2 : !(j_dua <= fmax(dua0, 1e-10)) ? 3 : 0;
    };

    // ---- 2, 3. the rounds
    int k = 0, judged = 0, stop = 0, added = 0, dropped = 0, reason0 = 1;
    bool broke0 = false;
    double pri_r0 = 0.0, dua_r0 = 0.0, obj_r0 = 0.0;
    for (;;) {
      const signed char *cur = clsbuf[k & 1];
      signed char *nxt = clsbuf[(k + 1) & 1];
      // the active rows in ascending order, by the first wavefront (every wavefront counts them)
      int na = 0;
      for (int c0 = 0; c0 < M; c0 += 64) {
        const int r = c0 + lane;
        const bool on = r < M && cur[r] != 0;
        const unsigned long long mask = __ballot(on);
        if (wv == 0 && on) act[na + __popcll(mask & ((1ull << lane) - 1ull))] = r;
        na += __popcll(mask);
      }
      // S = P + delta I on the lower triangle (the entries of a row of P are distinct columns; a pad repeats the last)
      for (int i = wv; i < n; i += 4)
        for (int c = lane; c <= i; c += 64) S[(size_t)i * ld + c] = 0.0;
      __syncthreads();
      for (int i1 = wv; i1 < n; i1 += 4) {
        const int k0 = a.pr_ptr[i1], k1 = a.pr_ptr[i1 + 1];
        for (int kk = k0 + lane; kk < k1; kk += 64) {
          const int i2 = a.pr_idx[kk];
          if (i2 > i1 || (kk > k0 && a.pr_idx[kk - 1] == i2)) continue;
          S[(size_t)i1 * ld + i2] = a.pr_val[kk];
        }
      }
      __syncthreads();
      for (int i = tid; i < n; i += 256) S[(size_t)i * ld + i] += delta;
      // ... plus A_act^T A_act / delta, 32 active rows at a time: their dense image (k-major) in the slab, then one
      // rank-32 update of the whole triangle; the rows a last chunk lacks are zeros
      for (int s0 = 0; s0 < na; s0 += NB) {
        for (int e = tid; e < NB * ldw; e += 256) Lp[e] = 0.0;
        __syncthreads();
        for (int c = wv; c < NB && s0 + c < na; c += 4) {
          const int r = act[s0 + c], k0 = a.pc_ptr[r], k1 = a.pc_ptr[r + 1];
          for (int kk = k0 + lane; kk < k1; kk += 64) {
            const int i = a.pc_idx[kk];
            if (kk > k0 && a.pc_idx[kk - 1] == i) continue;
            Lp[(size_t)c * ldw + i] = a.A[kk];
          }
        }
        __syncthreads();
        polg_rank_update(S, ld, n, 0, Lp, Lp, ldw, inv_delta, 1.0, sh_w, sh_l, tid);
      }
      __syncthreads();

      // blocked right-looking LDL^T in place: L below the diagonal, the pivots on it and in dd
      bool broke = false;
      for (int j0 = 0; j0 < n; j0 += NB) {
        const int nb = min(NB, n - j0), r0 = j0 + nb;
        for (int e = tid; e < NB * NB; e += 256) {
          const int r = e >> 5, c = e & 31;
          sh_t[r * TD + c] = (r < nb && c <= r) ? S[(size_t)(j0 + r) * ld + j0 + c] : 0.0;
        }
        __syncthreads();
        for (int j = 0; j < nb; j++) {
          const double d = sh_t[j * TD + j];
          if (!(d > 0.0)) {  // (uniform: every thread reads the same pivot)
            broke = true;
            break;
          }
          if (tid > j && tid < nb) sh_c[tid] = sh_t[tid * TD + j] / d;
          __syncthreads();
          for (int e = tid; e < NB * NB; e += 256) {
            const int i = e >> 5, c = e & 31;
            if (c > j && c <= i && i < nb) sh_t[i * TD + c] = fma(-sh_t[i * TD + j], sh_c[c], sh_t[i * TD + c]);
          }
          __syncthreads();
          if (tid > j && tid < nb) sh_t[tid * TD + j] = sh_c[tid];
        }
        if (broke) break;
        __syncthreads();
        for (int e = tid; e < NB * NB; e += 256) {
          const int r = e >> 5, c = e & 31;
          if (r < nb && c <= r) S[(size_t)(j0 + r) * ld + j0 + c] = sh_t[r * TD + c];
        }
        if (tid < nb) dd[j0 + tid] = sh_t[tid * TD + tid];
        if (r0 < n) {
          // the panel below (nb == 32 here), then the trailing update with it
          polg_panel_solve(S, ld, n, j0, Wp, Lp, ldw, sh_t, tid);
          __syncthreads();
          polg_rank_update(S, ld, n, r0, Wp, Lp, ldw, 1.0, -1.0, sh_w, sh_l, tid);
        }
        __syncthreads();
      }
      if (broke) {
        if (k == 0) broke0 = true;
        else stop = 2;  // the point and the set of the round before are judged
        break;
      }

      // 1 + refine_iter solves: with xh = yh = 0 the first pass's residuals are exactly (-q, b)
      for (int it = 0; it <= a.refine_iter; it++) {
        for (int r = wv; r < M; r += 4) {
          const signed char c = cur[r];
          double rr = 0.0;
          if (c != 0) rr = (c < 0 ? lg[r] : ug[r]) - (it > 0 ? a_row(r, xh) : 0.0);  // (uniform over the wavefront)
          if (lane == 0) r2[r] = rr;
        }
        __syncthreads();
        // t = (-q - P xh - A^T yh) + A^T r2 / delta; yh and r2 are zero on the inactive rows
        for (int i = wv; i < n; i += 4) {
          const double px = it > 0 ? p_row(i, xh) : 0.0;
          double aty = 0.0, atr = 0.0;
#pragma unroll 4
          for (int kk = g.pv_ptr[i] + lane; kk < g.pv_ptr[i + 1]; kk += 64) {
            const int r = g.pv_idx[kk];
            const double av = g.At[kk];
            aty = fma(av, yh[r], aty);
            atr = fma(av, inv_delta * r2[r], atr);
          }
          aty = polg_wave_sum(aty);
          atr = polg_wave_sum(atr);
          if (lane == 0) t[i] = ((-qg[i] - px) - aty) + atr;
        }
        __syncthreads();
        // forward, L w = t, a block of 32 at a time: each row of the block takes its dot product with the w before
        // the block (one wavefront per row, lanes striding the row of S), then the diagonal block is solved in LDS by
        // the first wavefront; w goes to v
        for (int j0 = 0; j0 < n; j0 += NB) {
          const int nb = min(NB, n - j0);
          for (int e = tid; e < NB * NB; e += 256) {
            const int r = e >> 5, c = e & 31;
            sh_t[r * TD + c] = (r < nb && c < r) ? S[(size_t)(j0 + r) * ld + j0 + c] : 0.0;
          }
          for (int r = wv; r < nb; r += 4) {
            const double *row = S + (size_t)(j0 + r) * ld;
            double acc = 0.0;
#pragma unroll 4
            for (int j = lane; j < j0; j += 64) acc = fma(row[j], v[j], acc);
            acc = polg_wave_sum(acc);
            if (lane == 0) sh_c[r] = t[j0 + r] - acc;
          }
          __syncthreads();
          if (wv == 0) {
            double reg = lane < nb ? sh_c[lane] : 0.0;
            for (int j = 0; j < nb; j++) {
              const double vj = __shfl(reg, j, 64);
              if (lane > j && lane < nb) reg = fma(-sh_t[lane * TD + j], vj, reg);
            }
            if (lane < nb) v[j0 + lane] = reg;
          }
          __syncthreads();
        }
        // the pivots and backward, L^T dx = w / d, from the last block: column c of the block gathers L[i][c] dx[i] over
        // the rows below the block (eight threads per column, each its rows in ascending order, the eight in order),
        // then the diagonal block by the first wavefront; dx replaces w in v
        for (int j0 = ((n - 1) / NB) * NB; j0 >= 0; j0 -= NB) {
          const int nb = min(NB, n - j0), r0 = j0 + nb;
          for (int e = tid; e < NB * NB; e += 256) {
            const int r = e >> 5, c = e & 31;
            sh_t[r * TD + c] = (r < nb && c < r) ? S[(size_t)(j0 + r) * ld + j0 + c] : 0.0;
          }
          {
            const int c = tid & 31, rg = tid >> 5;
            double acc = 0.0;
            if (c < nb)
#pragma unroll 4
              for (int i = r0 + rg; i < n; i += 8) acc = fma(S[(size_t)i * ld + j0 + c], v[i], acc);
            sh_w[rg * NB + c] = acc;
          }
          __syncthreads();
          if (wv == 0) {
            double reg = 0.0;
            if (lane < nb) {
              double acc = sh_w[lane];
#pragma unroll
              for (int rg = 1; rg < 8; rg++) acc += sh_w[rg * NB + lane];
              reg = v[j0 + lane] / dd[j0 + lane] - acc;
            }
            for (int j = nb - 1; j > 0; j--) {
              const double xj = __shfl(reg, j, 64);
              if (lane < j) reg = fma(-sh_t[j * TD + lane], xj, reg);
            }
            if (lane < nb) v[j0 + lane] = reg;
          }
          __syncthreads();
        }
        for (int i = tid; i < n; i += 256) xh[i] += v[i];
        for (int r = wv; r < M; r += 4) {
          if (cur[r] == 0) continue;  // (uniform over the wavefront)
          const double av = a_row(r, v);
          if (lane == 0) yh[r] += inv_delta * (av - r2[r]);
        }
        __syncthreads();
      }
      if (k == 0) {
        reason0 = judge(xh, yh);
        pri_r0 = j_pri;
        dua_r0 = j_dua;
        obj_r0 = j_obj;
      }
      // the revision: an equality row stays; an active row whose multiplier has the wrong sign leaves; an inactive row
      // violated by more than the tolerance joins on that side
      judged = k;
      for (int r = wv; r < M; r += 4) {
        const signed char c = cur[r];
        const double z = c == 0 ? a_row(r, xh) : 0.0;  // (uniform over the wavefront)
        if (lane == 0) {
          const double l = lg[r], u = ug[r], y = yh[r];
          signed char cn = c;
          if (l != u) {
            if (c < 0) cn = y > POLG_TOL ? 0 : c;
            else if (c > 0) cn = y < -POLG_TOL ? 0 : c;
            else if (l > -POLG_INFTY && l - z > POLG_TOL) cn = -1;
            else if (u < POLG_INFTY && z - u > POLG_TOL) cn = 1;
          }
          nxt[r] = cn;
        }
      }
      __syncthreads();
      int c4 = 0, c5 = 0;
      for (int r = tid; r < M; r += 256) {
        const signed char c = cur[r], cn = nxt[r];
        c4 += cn != c && c == 0;
        c5 += cn != c && c != 0;
      }
      c4 = polg_block_count(c4, red, tid);
      c5 = polg_block_count(c5, red, tid);
      added += c4;
      dropped += c5;
      if (c4 + c5 == 0) break;
      if (k == a.repair_iter) {
        stop = 1;
        break;
      }
      // the next round on the revised set from xh = yh = 0; this round's point is kept
      for (int i = tid; i < n; i += 256) {
        xk[i] = xh[i];
        xh[i] = 0.0;
      }
      for (int r = tid; r < M; r += 256) {
        yk[r] = yh[r];
        yh[r] = 0.0;
      }
      k++;
      __syncthreads();
    }
    const int rounds = k;

    // ---- 4. the point the loop ended with, the decision, the record
    const double *X = stop == 2 ? xk : xh, *Y = stop == 2 ? yk : yh;
    int reason = reason0;
    double pri1 = pri_r0, dua1 = dua_r0, obj = obj_r0;
    if (broke0) {
      reason = 1;
      pri1 = dua1 = obj = __builtin_nan("");
    } else if (rounds > 0) {
      reason = judge(X, Y);
      pri1 = j_pri;
      dua1 = j_dua;
      obj = j_obj;
    }
    const signed char *fin = clsbuf[judged & 1];
    int c_lo = 0, c_up = 0;
    for (int r = tid; r < M; r += 256) {
      c_lo += fin[r] < 0;
      c_up += fin[r] > 0;
    }
    const int n_lower = polg_block_count(c_lo, red, tid), n_upper = polg_block_count(c_up, red, tid);
    double *out = a.out + inst * polm_out_stride(n, M);
    if (tid == 0) {
      PolManyRec r;
      r.accepted = reason == 0;
      r.reason = reason;
      r.n_lower = n_lower;
      r.n_upper = n_upper;
      r.rounds = rounds;
      r.stop = stop;
      r.n_added = added;
      r.n_dropped = dropped;
      r.accepted0 = reason0 == 0;
      r.reason0 = reason0;
      r.pad[0] = r.pad[1] = 0;
      r.pri_before = pri0;
      r.dua_before = dua0;
      r.pri_after = pri1;
      r.dua_after = dua1;
      r.obj = obj;
      *(PolManyRec *)out = r;
    }
    double *xo = out + POLM_REC_DOUBLES, *yo = xo + n;
    signed char *co = (signed char *)(yo + M);
    const bool take = reason == 0;
    for (int i = tid; i < n; i += 256) xo[i] = take ? X[i] : xg[i];
    for (int r = tid; r < M; r += 256) {
      yo[r] = take ? Y[r] : yg[r];
      co[r] = fin[r];
    }
    __syncthreads();  // (the slab is the next instance's)
  }
}

}  // namespace

size_t polish_many_large_slab_doubles(int n, int M) {
  if (n < 1 || M < 0 || n > POLG_NMAX || M > POLG_MMAX) return (size_t)-1;
  return polg_layout(n, M).total;
}

int polish_many_large_launch(const PolManyLargeArgs &g, int W, void *stream) {
  hipLaunchKernelGGL(k_pol_many_g, dim3((unsigned)W), dim3(256), 0, (hipStream_t)stream, g);
  return (int)hipGetLastError();
}

}  // namespace miosqp
