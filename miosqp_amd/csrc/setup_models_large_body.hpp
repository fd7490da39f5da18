// The dense set-up of ONE model beyond n + M = 192 by ONE workgroup (k_setup_models_large, kernels_setup_models.inc):
// what miosqp_qp_setup(..., coop = 0, resident = 0, fold = 1, pers = 0) builds for it -- the Schur complement, its
// LDL^T, the triangular inverse, the product form, the dense copies and the scaled bounds; no explicit inverse, no Kc, no
// guard (the engine that comes out iterates with the sweeps of the product form, and k_tree_r_m reads nothing else).
// Written as PHASES like setup_models_body.hpp, whose ldl_inverse it calls: the same text runs on the CPU under tests/.
// body_large_auto (k_setup_models_large_auto) adds, for a model that asks for it, the choice of rho between the first
// factor and the products, with setup_models_body.hpp's probe_rule.
//
// setup_models_body.hpp keeps a dense copy of Abar in LDS beside the packed triangle, which is what stops it at n + M =
// 192.  Here only the packed triangle, the two row buffers and d are in LDS; Abar is written to memory first (f_Ad,
// f_Atd) and read back from there (L2).
//
// Plain C++; the HIP qualifiers appear only under hipcc.  Vector stores only, no inline assembly.
#pragma once
#include "setup_models_body.hpp"

namespace miosqp {
namespace setup_models {

constexpr int MAX_NM_LARGE = 2048;  // beyond that miosqp_qp_setup builds the persistent form

// LDS of the kernel for one model, in doubles: triangle of S | two rows | d (lds_layout's Lp, tmp, dv without Ad between)
MIOSQP_HD inline size_t lds_doubles_large(int n, int /*M*/) { return tri((size_t)n) + 3 * (size_t)n + 8; }
// the size rule of the launch: a model the small launch does not take, whose triangle one workgroup holds (n <= 198)
MIOSQP_HD inline bool eligible_shape_large(int n, int M) {
  return n >= 1 && M >= 1 && !eligible_shape(n, M) && n + M <= MAX_NM_LARGE &&
         lds_doubles_large(n, M) * sizeof(double) <= LDS_LIMIT;
}

// LDS of the launch that chooses rho (k_setup_models_large_auto): the probing iterations' x | z | y | Abar x | scalars
// behind d, in the layout of the small body (probe_doubles).  Within LDS_LIMIT up to n = 197; every shape beyond the
// small launch that the reduced trees solve (tree_reduced::lds_doubles(n, M, 256)) is inside (the stand-alone program
// under tests/ walks them), so the vectors need no other home.
MIOSQP_HD inline size_t lds_doubles_large_auto(int n, int M) { return lds_doubles_large(n, M) + probe_doubles(n, M); }
MIOSQP_HD inline bool eligible_shape_large_auto(int n, int M) {
  return eligible_shape_large(n, M) && lds_doubles_large_auto(n, M) * sizeof(double) <= LDS_LIMIT;
}

// phases 1 and 2: the dense copies, then S at `rho` on the packed triangle at the start of `lds`.  The arena is
// zero-filled: only the entries that are not zero are written (build_folded tests the same values).  FIRST = false is
// the second factor of body_large_auto: the copies stand, the triangle is cleared and S is formed again with the same
// terms in the same order.
template <bool FIRST, class X>
MIOSQP_HD inline void large_schur_at(const IO &io, double *lds, X &x, double rho) {
  const int n = io.n, M = io.M, NT = THREADS;
  const size_t t_all = tri((size_t)n);
  double *const Lp = lds;
  const double sigma = io.sigma;
  // ---- phase 1: f_Ad, f_Atd and f_Pd from the packed rows; the triangle cleared ----
  x.par([&](int tid) {
    if constexpr (FIRST)
      for (int r = tid; r < M; r += NT)
        for (int t = io.pc_ptr[r]; t < io.pc_ptr[r + 1]; t++) {
          const double v = io.pc_A[t];
          if (v != 0.0) {
            io.f_Ad[(size_t)r * io.ldn + io.pc_idx[t]] = v;
            io.f_Atd[(size_t)io.pc_idx[t] * io.ldm + r] = v;
          }
        }
    for (size_t k = tid; k < t_all; k += NT) Lp[k] = 0.0;
  });
  // ---- phase 2a: S = Pbar (lower part of row i: its own column of the upper triangle) + sigma I ----
  x.par([&](int tid) {
    for (int i = tid; i < n; i += NT) {
      double *Si = Lp + tri((size_t)i);
      for (int t = io.pb_ptr[i]; t < io.pb_ptr[i + 1]; t++) {
        const int c = io.pb_idx[t];
        const double v = io.pb_val[t];
        if (c <= i) Si[c] += v;
        if (FIRST && v != 0.0) io.f_Pd[(size_t)i * io.ldn + c] = v;
      }
      Si[i] += sigma;
    }
  });
  // ---- phase 2b: S += rho Abar^T Abar: entry (i1, i2) is one fused sum over the constraint rows in ascending order
  //      (schur_add_rho's and factor.cpp's terms in their order), read from rows i1 and i2 of f_Atd, contiguous in r ----
  x.par([&](int tid) {
    for (int i1 = tid / LANES; i1 < n; i1 += NT / LANES) {
      const double *A1 = io.f_Atd + (size_t)i1 * io.ldm;
      for (int i2 = tid % LANES; i2 <= i1; i2 += LANES) {
        const double *A2 = io.f_Atd + (size_t)i2 * io.ldm;
        double s = Lp[tri((size_t)i1) + i2];
        for (int r = 0; r < M; r++) s = fma(rho * A1[r], A2[r], s);
        Lp[tri((size_t)i1) + i2] = s;
      }
    }
  });
}
template <class X>
MIOSQP_HD inline void large_schur(const IO &io, double *lds, X &x) {
  large_schur_at<true>(io, lds, x, io.rho);
}

// phases 4 and 5: everything that is read off the triangle once it holds L^-1, at the rho the factor was built with
template <class X>
MIOSQP_HD inline void large_read_off(const IO &io, double *lds, X &x, double rho) {
  const int n = io.n, M = io.M, NT = THREADS;
  double *const Lp = lds;
  // ---- phase 4: Linv, LinvT, the rows of the product form ----
  x.par([&](int tid) {
    const int ld = io.ld, ldf = io.ldf, ldm = io.ldm;
    for (size_t e = tid; e < (size_t)n * ld; e += NT) {
      const int i = (int)(e / ld), c = (int)(e % ld);
      io.Linv[e] = c < i ? Lp[tri((size_t)i) + c] : 0.0;
      io.LinvT[e] = (c > i && c < n) ? Lp[tri((size_t)c) + i] : 0.0;
    }
    // row i: [ -G[i][0..M) | X[i][0..i) | 0 .. ],  -G[i][r] = rho (Abar[r][i] + sum_{j<i} X[i][j] Abar[r][j]), the sum of
    // setup_models_body.hpp term for term.  Abar[r][j] is read as f_Atd[j][r]: the lanes of a wavefront walk r, so the
    // loads of one j are contiguous.
    for (size_t e = tid; e < (size_t)n * ldf; e += NT) {
      const int i = (int)(e / ldf), c = (int)(e % ldf);
      double v = 0.0;
      if (c < M) {
        const double *Ac = io.f_Atd + c, *Xi = Lp + tri((size_t)i);
        v = rho * Ac[(size_t)i * ldm];
        for (int j = 0; j < i; j++) v = fma(Xi[j], rho * Ac[(size_t)j * ldm], v);
      } else if (c - M < i) {
        v = Lp[tri((size_t)i) + (c - M)];
      }
      io.f_rows[e] = v;
    }
  });
  // ---- phase 5: f_GmT (the transpose of -G, read back), the scaled bounds (k_scale_bounds), the record ----
  x.par([&](int tid) {
    const int ldf = io.ldf, ldn = io.ldn;
    for (size_t e = tid; e < (size_t)M * ldn; e += NT) {
      const int r = (int)(e / ldn), i = (int)(e % ldn);
      io.f_GmT[e] = i < n ? io.f_rows[(size_t)i * ldf + r] : 0.0;
    }
    for (int j = tid; j < M; j += NT) {
      io.l[j] = io.E[j] * fmax(io.raw_l[j], -INFTY);
      io.u[j] = io.E[j] * fmin(io.raw_u[j], INFTY);
    }
    if (tid == 0) {
      io.rec->bad_pivot = 0;
      io.rec->pivot = -1;
      io.rec->guard = -1.0;  // (no explicit inverse, no guard)
    }
  });
}

// phases 3 to 5: the LDL^T and the inverse (ldl_inverse: the function the small launch calls), then the products
template <class X>
MIOSQP_HD inline void large_products(const IO &io, double *lds, X &x) {
  double *const tmp = lds + tri((size_t)io.n);
  if (!ldl_inverse(io, lds, tmp, tmp + 2 * (size_t)io.n, x, 1)) return;
  large_read_off(io, lds, x, io.rho);
}

// k_setup_models_large
template <class X>
MIOSQP_HD inline void body_large(const IO &io, double *lds, X &x) {
  large_schur(io, lds, x);
  large_products(io, lds, x);
}

// How the probing iterations read Abar in the large launch: out of memory (L2), where phase 1 wrote it.  A thread that
// owns variable i and walks r reads f_Ad[r][i], one that owns row r and walks i reads f_Atd[i][r]: either way the lanes
// of a wavefront load contiguous doubles at every step of the walk.
struct AbarMem {
  const double *f_Ad, *f_Atd;
  int ldn, ldm;
  MIOSQP_HD double by_var(int r, int i) const { return f_Ad[(size_t)r * ldn + i]; }
  MIOSQP_HD double by_con(int r, int i) const { return f_Atd[(size_t)i * ldm + r]; }
};

// k_setup_models_large_auto: body_large, and for a model with au.on the choice of rho between the first factor and the
// products -- probe_rule (the function the small launch calls: every sum on one thread in ascending order, so the result
// does not depend on the list around the model) with L^-1 and 1 / d on the triangle in LDS and Abar from L2, its vectors
// behind d; where the rule moves rho, S and the factor again at the chosen value and the panel's values.  A row's sum is
// not split over lanes: the LDS rule leaves no room for partial sums.
template <class X>
MIOSQP_HD inline void body_large_auto(const IO &io, const Auto &au, double *lds, X &x) {
  if (!au.on) {
    body_large(io, lds, x);
    return;
  }
  const int n = io.n, NT = THREADS;
  double *const tmp = lds + tri((size_t)n), *const dv = tmp + 2 * (size_t)n, *const pv = dv + (size_t)n + 8;
  large_schur(io, lds, x);
  if (!ldl_inverse(io, lds, tmp, dv, x, 1)) return;
  const double rho = probe_rule(io, au, AbarMem{io.f_Ad, io.f_Atd, io.ldn, io.ldm}, lds, tmp, dv, pv, x);
  if (rho == io.rho) {  // the first factor stands
    large_read_off(io, lds, x, rho);
    return;
  }
  large_schur_at<false>(io, lds, x, rho);
  if (!ldl_inverse(io, lds, tmp, dv, x, 2)) return;
  // the panel's values at the chosen rho: the expression of build_factor(reuse_rows): padding stays +0.0, never -0.0
  x.par([&](int tid) {
    for (int k = tid; k < au.nv; k += NT) au.pv_L[k] = au.pv_At[k] == 0.0 ? 0.0 : -rho * au.pv_At[k];
    for (int k = tid; k < au.nc; k += NT) au.pc_L[k] = io.pc_A[k] == 0.0 ? 0.0 : -rho * io.pc_A[k];
  });
  large_read_off(io, lds, x, rho);
}

}  // namespace setup_models
}  // namespace miosqp
