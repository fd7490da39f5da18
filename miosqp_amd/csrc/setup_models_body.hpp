// The dense set-up of ONE small model by ONE workgroup (k_setup_models, kernels_setup_models.inc): what miosqp_qp_setup
// builds for the LDS-resident form with the explicit inverse -- the Schur complement, its LDL^T, the triangular inverse,
// the product form, W, Kc, the guard residual and the scaled bounds -- written as a sequence of PHASES.  A phase is a
// function of the thread index that reads what earlier phases wrote and keeps nothing in registers across its end; the
// executor `X` runs a phase on every thread and puts a barrier behind it.  On the device X is {f(threadIdx.x);
// __syncthreads()}; the stand-alone CPU program under tests/ runs the same phases with a loop over the thread index, so
// the arithmetic below is checked against the long-double reference without a GPU.  Code outside a phase only READS
// values that are the same for every thread (a pivot, a loop bound).
//
// body is k_setup_models: a fixed rho.  body_auto (k_setup_models_auto) adds, for a model that asks for it, the
// choice of rho as further phases between the first factor and the products: the probing iterations of the rho-once
// recipe (engine.hip: miosqp_qp_setup with rho_auto; the CPU restatement under the tests: rho_once) on what the
// workgroup holds in LDS, the rule, and -- where the rule moves rho -- the factor again at the chosen value.
//
// Plain C++; the HIP qualifiers appear only under hipcc.  Vector stores only, no inline assembly.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "guard_probe.hpp"

namespace miosqp {
namespace setup_models {

constexpr int THREADS = 256;       // one workgroup per model
constexpr int MAX_NM = 192;        // n + M of a model in the launch (RES_W_MAX: the form the engines are built for)
constexpr int GUARD_PROBES = 3;    // GUARD_NP of kernels_guard.inc
constexpr int LANES = 16;          // lanes per row where a phase strides rows (THREADS / LANES rows at a time)
constexpr size_t LDS_LIMIT = 160 * 1024;
constexpr double INFTY = 1e30;     // QP_INFTY

// one model's outcome: all records of a call come back in one copy
struct Record {
  int32_t bad_pivot;   // not 0: the pivot at index `pivot` was not positive or not finite (nothing behind the LDL^T was
  int32_t pivot;       // built); the value names the factor: 1 at the starting rho, 2 at the rho the rule chose
  double guard;        // max |K W r - r| over the probes (infinite for a NaN), as inverse_guard reads it
  double rho_est;      // rho chosen in the launch: the rule's value before it is rounded to two digits (else untouched)
  double rho;          // ... and the rho every product of the model was built with
};
static_assert(sizeof(Record) == 32, "the records of a call are laid out by this size");

constexpr int RHO_ONCE_ITERS = 50;  // probing iterations (engine.hip and the CPU restatement: same name, same value)

// what body_auto needs beyond IO for a model whose rho it chooses (on == 0: the model keeps io.rho)
struct Auto {
  int on;
  int nv, nc;            // lengths of pv_L / pc_L as stored (padding included)
  double alpha;
  const double *q;       // the scaled cost
  const double *pv_At;   // Abar^T by variable, plain values (pc_A of IO is its counterpart by constraint)
  double *pv_L, *pc_L;   // the panel's values, uploaded at the starting rho: -rho Abar
};

// what a workgroup reads and writes: final pointers into the call's arena
struct IO {
  int n, M, ld, ldf, ldn, ldm, ldw;
  double rho, sigma;
  const int *pc_ptr, *pc_idx;   // rows of Abar, packed (factor.hpp: PCsr), with the plain values
  const double *pc_A;
  const int *pb_ptr, *pb_idx;   // rows of the full symmetric Pbar, packed
  const double *pb_val;
  const double *E, *raw_l, *raw_u;
  double *l, *u;
  double *d2inv, *Linv, *LinvT, *f_rows, *f_GmT, *f_Ad, *f_Atd, *f_Pd, *W, *Kc;
  Record *rec;
};

MIOSQP_HD inline size_t tri(size_t i) { return i * (i + 1) / 2; }  // start of row i of a packed lower triangle

// doubles of scratch the guard phases use in place of the (then dead) triangle
MIOSQP_HD inline size_t guard_doubles(int n, int M) {
  return (size_t)GUARD_PROBES * (size_t)(n + M) + (size_t)THREADS * GUARD_PROBES + (size_t)(n + M) + 8;
}
// LDS of the kernel for one model, in doubles: [ triangle of S | guard scratch ] | dense Abar (M x (n | 1)) | two rows | d
MIOSQP_HD inline size_t lds_doubles(int n, int M) {
  const size_t t = tri((size_t)n), g = guard_doubles(n, M);
  return (t > g ? t : g) + (size_t)M * (size_t)(n | 1) + 3 * (size_t)n + 8;
}
// the probing iterations keep x (n), z, y and Abar x (M each) and eight scalars behind that, in LDS as well: at n + M <=
// MAX_NM the sum stays below LDS_LIMIT wherever lds_doubles does (largest at n = 191: 19 310 of 20 480 doubles), so the
// launch that chooses rho takes every shape the fixed-rho launch takes
MIOSQP_HD inline size_t probe_doubles(int n, int M) { return (size_t)n + 3 * (size_t)M + 8; }
MIOSQP_HD inline size_t lds_doubles_auto(int n, int M) { return lds_doubles(n, M) + probe_doubles(n, M); }
// the size rule of the launch: one workgroup holds the model
MIOSQP_HD inline bool eligible_shape(int n, int M) {
  return n >= 1 && M >= 1 && n + M <= MAX_NM && lds_doubles(n, M) * sizeof(double) <= LDS_LIMIT;
}

// where the parts lie in the LDS of one model
struct Lds {
  double *Lp;   // packed lower triangle: S, then L (diagonal: d), then L^-1; the guard's scratch at the end
  double *Ad;   // dense Abar, row r at r * (n | 1)
  double *tmp;  // two rows of L (the triangular inverse works in place); vectors of the probing iterations
  double *dv;   // d, then 1 / d
  double *pv;   // body_auto: x | z | y | Abar x | scalars (probe_doubles)
};
MIOSQP_HD inline Lds lds_layout(double *lds, int n, int M) {
  const size_t t_all = tri((size_t)n), g_all = guard_doubles(n, M);
  Lds w;
  w.Lp = lds;
  w.Ad = lds + (t_all > g_all ? t_all : g_all);
  w.tmp = w.Ad + (size_t)M * (size_t)(n | 1);
  w.dv = w.tmp + 2 * (size_t)n;
  w.pv = w.dv + (size_t)n + 8;
  return w;
}

// entry (i, c) of F = [ -G | L22^-1 ] with the unit diagonal restored (dense_setup.hip: ks_kkt_inverse reads the same)
// -G comes from memory (it was never in LDS: the dense Abar holds that room), the triangular part from the triangle Xp in LDS
MIOSQP_HD inline double f_entry(const double *F, int ldf, const double *Xp, int M, int N, int i, int c) {
  if (c >= N) return 0.0;
  if (c < M) return F[(size_t)i * ldf + c];
  return c == M + i ? 1.0 : (c > M + i ? 0.0 : Xp[tri((size_t)i) + (c - M)]);
}

// rho_round2 of engine.hip and of the CPU restatement: two significant digits
MIOSQP_HD inline double rho_round2(double r) {
  if (!(r > 0)) return r;
  const double e = floor(log10(r)), p = pow(10.0, e);
  return floor(r / p * 10.0 + 0.5) / 10.0 * p;
}

// S += rho Abar^T Abar on the lower triangle, constraint rows ascending, fused (factor.cpp adds the same terms in this
// order): the part of phase 2 that depends on rho
MIOSQP_HD inline void schur_add_rho(int tid, double *Lp, const double *Ad, int n, int M, int lda, double rho) {
  for (int i1 = tid / LANES; i1 < n; i1 += THREADS / LANES)
    for (int i2 = tid % LANES; i2 <= i1; i2 += LANES) {
      double s = Lp[tri((size_t)i1) + i2];
      for (int r = 0; r < M; r++) s = fma(rho * Ad[(size_t)r * lda + i1], Ad[(size_t)r * lda + i2], s);
      Lp[tri((size_t)i1) + i2] = s;
    }
}

// phases 3, 4 and 5a: the triangle holds S on entry; on return L^-1 (strict lower part; the diagonal keeps d) with 1 / d
// in dv and io.d2inv.  false: a pivot was not positive or not finite, reported as factor `which`.
template <class X>
MIOSQP_HD inline bool ldl_inverse(const IO &io, double *Lp, double *tmp, double *dv, X &x, int which) {
  const int n = io.n, NT = THREADS;
  // ---- phase 3: right-looking LDL^T in place, one column per step (the order of the textbook algorithm) ----
  for (int j = 0; j < n; j++) {
    const double dj = Lp[tri((size_t)j) + j];  // (the same value on every thread: written before the last barrier)
    if (!(dj > 0.0) || !std::isfinite(dj)) {   // the test of the host factorisation
      x.par([&](int tid) {
        if (tid == 0) {
          io.rec->bad_pivot = which;
          io.rec->pivot = j;
          io.rec->guard = -1.0;
        }
      });
      return false;
    }
    x.par([&](int tid) {
      if (tid == 0) dv[j] = dj;
      for (int i = j + 1 + tid; i < n; i += NT) Lp[tri((size_t)i) + j] /= dj;
    });
    if (j + 1 < n)
      x.par([&](int tid) {
        for (int i = j + 1 + tid / LANES; i < n; i += NT / LANES) {
          double *Si = Lp + tri((size_t)i);
          const double w = Si[j] * dj;
          for (int k = j + 1 + tid % LANES; k <= i; k += LANES) Si[k] = fma(-w, Lp[tri((size_t)k) + j], Si[k]);
        }
      });
  }
  // ---- phase 4: X = L^-1 in place, one row per step: X[i][j] = -L[i][j] - sum_{j < k < i} L[i][k] X[k][j]; row i of L is
  //      read from a copy (two buffers: the copy of row i + 1 is made while row i is computed) ----
  x.par([&](int tid) {
    if (n > 1 && tid == 0) tmp[(size_t)n] = Lp[tri(1)];  // row 1 has one entry; buffer (1 & 1)
  });
  for (int i = 1; i < n; i++) {
    const double *Li = tmp + (size_t)(i & 1) * n;
    double *Ln = tmp + (size_t)((i + 1) & 1) * n;
    x.par([&](int tid) {
      if (i + 1 < n)
        for (int c = tid; c <= i; c += NT) Ln[c] = Lp[tri((size_t)i + 1) + c];
      for (int j = tid; j < i; j += NT) {
        double acc = 0.0;
        for (int k = j + 1; k < i; k++) acc = fma(Li[k], Lp[tri((size_t)k) + j], acc);
        Lp[tri((size_t)i) + j] = -Li[j] - acc;
      }
    });
  }
  // ---- phase 5a: d2inv ----
  x.par([&](int tid) {
    for (int j = tid; j < n; j += NT) {
      const double v = 1.0 / dv[j];
      dv[j] = v;
      io.d2inv[j] = v;
    }
  });
  return true;
}

// The second factor (body_auto): the triangle (L^-1 of the first factor by now) is cleared and S is formed again at
// `rho` from the rows of Pbar, sigma and the dense Abar, which is still in LDS; the LDL^T and the inverse again; the
// panel's values at `rho`.  false: a bad pivot, reported as factor 2.
template <class X>
MIOSQP_HD inline bool refactor(const IO &io, const Auto &au, double *Lp, const double *Ad, double *tmp, double *dv, X &x,
                               double rho) {
  const int n = io.n, M = io.M, NT = THREADS, lda = n | 1;
  const size_t t_all = tri((size_t)n);
  const double sigma = io.sigma;
  x.par([&](int tid) {
    for (size_t k = tid; k < t_all; k += NT) Lp[k] = 0.0;
  });
  x.par([&](int tid) {
    for (int i = tid; i < n; i += NT) {
      double *Si = Lp + tri((size_t)i);
      for (int t = io.pb_ptr[i]; t < io.pb_ptr[i + 1]; t++)
        if (io.pb_idx[t] <= i) Si[io.pb_idx[t]] += io.pb_val[t];
      Si[i] += sigma;
    }
  });
  x.par([&](int tid) { schur_add_rho(tid, Lp, Ad, n, M, lda, rho); });
  if (!ldl_inverse(io, Lp, tmp, dv, x, 2)) return false;
  // the expression of build_factor(reuse_rows): padding stays +0.0, never -0.0
  x.par([&](int tid) {
    for (int k = tid; k < au.nv; k += NT) au.pv_L[k] = au.pv_At[k] == 0.0 ? 0.0 : -rho * au.pv_At[k];
    for (int k = tid; k < au.nc; k += NT) au.pc_L[k] = io.pc_A[k] == 0.0 ? 0.0 : -rho * io.pc_A[k];
  });
  return true;
}

// How the probing iterations read Abar.  by_var(r, i) is the read of a thread that owns variable i and walks the
// constraint rows r, by_con(r, i) that of a thread that owns row r and walks the variables: the same value either way.
// Here both come from the dense copy in LDS; the large launch (setup_models_large_body.hpp) reads f_Ad and f_Atd.
struct AbarLds {
  const double *Ad;
  int lda;
  MIOSQP_HD double by_var(int r, int i) const { return Ad[(size_t)r * lda + i]; }
  MIOSQP_HD double by_con(int r, int i) const { return Ad[(size_t)r * lda + i]; }
};

// The probe and the rule of the choice of rho: RHO_ONCE_ITERS iterations of the CPU restatement's admm_step from
// x = z = y = 0 on the first factor (L^-1 on the triangle, 1 / d in dv), then the rule of rho_estimate.  Returns the
// chosen rho (the same value on every thread) and fills Record::rho_est and Record::rho.
//   The KKT solve in reduced form: with S = Pbar + sigma I + rho Abar^T Abar = L D L^T,
//     x~ = L^-T D^-1 L^-1 (sigma x - q + Abar^T (rho z - y)),   nu = rho (Abar x~ - z) + y,
//   and admm_step's z~ = z + (nu - y) / rho is, with that nu, Abar x~: THAT identity is used, z~ = Abar x~ is formed
//   directly and nu never is.  Every sum runs on one thread in ascending index order.
template <class AB, class X>
MIOSQP_HD inline double probe_rule(const IO &io, const Auto &au, const AB &Ab, double *Lp, double *tmp, double *dv, double *pv,
                                   X &x) {
  const int n = io.n, M = io.M, NT = THREADS;
  const double rho0 = io.rho, rho0_inv = 1.0 / rho0, sigma = io.sigma, alpha = au.alpha;
  double *xs = pv, *zs = xs + n, *ys = zs + M, *ax = ys + M, *sc = ax + M;  // x, z, y, Abar x, scalars
  double *rhs = tmp, *w = tmp + n, *xt = tmp;  // (the two row buffers of phase 4 are free; x~ takes the place of the rhs)
  // ---- the scaled set-up bounds (phase 6 forms the same values again), the iterates at zero ----
  x.par([&](int tid) {
    for (int j = tid; j < M; j += NT) {
      io.l[j] = io.E[j] * fmax(io.raw_l[j], -INFTY);
      io.u[j] = io.E[j] * fmin(io.raw_u[j], INFTY);
      zs[j] = 0.0;
      ys[j] = 0.0;
    }
    for (int i = tid; i < n; i += NT) xs[i] = 0.0;
  });
  for (int it = 0; it < RHO_ONCE_ITERS; it++) {
    // rhs = sigma x - q + Abar^T (rho z - y)
    x.par([&](int tid) {
      for (int i = tid; i < n; i += NT) {
        double acc = sigma * xs[i] - au.q[i];
        for (int r = 0; r < M; r++) acc = fma(Ab.by_var(r, i), rho0 * zs[r] - ys[r], acc);
        rhs[i] = acc;
      }
    });
    // w = D^-1 L^-1 rhs (unit diagonal implied)
    x.par([&](int tid) {
      for (int i = tid; i < n; i += NT) {
        const double *Xi = Lp + tri((size_t)i);
        double acc = rhs[i];
        for (int j = 0; j < i; j++) acc = fma(Xi[j], rhs[j], acc);
        w[i] = acc * dv[i];
      }
    });
    // x~ = L^-T w
    x.par([&](int tid) {
      for (int j = tid; j < n; j += NT) {
        double acc = w[j];
        for (int i = j + 1; i < n; i++) acc = fma(Lp[tri((size_t)i) + j], w[i], acc);
        xt[j] = acc;
      }
    });
    // z~ = Abar x~; relaxation, projection and the dual step of admm_step (row r and variable i belong to one thread)
    x.par([&](int tid) {
      for (int r = tid; r < M; r += NT) {
        double zt = 0.0;
        for (int i = 0; i < n; i++) zt = fma(Ab.by_con(r, i), xt[i], zt);
        const double zr = alpha * zt + (1.0 - alpha) * zs[r];
        const double v = zr + rho0_inv * ys[r];
        const double zn = fmin(fmax(v, io.l[r]), io.u[r]);
        ys[r] += rho0 * (zr - zn);
        zs[r] = zn;
      }
      for (int i = tid; i < n; i += NT) xs[i] = alpha * xt[i] + (1.0 - alpha) * xs[i];
    });
  }
  // ---- the rule: Abar x, Pbar x (packed symmetric rows, stored order) and Abar^T y; then one thread ----
  double *Px = tmp, *Aty = tmp + n;
  x.par([&](int tid) {
    for (int r = tid; r < M; r += NT) {
      double s = 0.0;
      for (int i = 0; i < n; i++) s = fma(Ab.by_con(r, i), xs[i], s);
      ax[r] = s;
    }
    for (int i = tid; i < n; i += NT) {
      double s = 0.0;
      for (int t = io.pb_ptr[i]; t < io.pb_ptr[i + 1]; t++) s = fma(io.pb_val[t], xs[io.pb_idx[t]], s);
      Px[i] = s;
      double a = 0.0;
      for (int r = 0; r < M; r++) a = fma(Ab.by_var(r, i), ys[r], a);
      Aty[i] = a;
    }
  });
  x.par([&](int tid) {
    if (tid != 0) return;
    double pri = 0, dua = 0, nz = 0, nax = 0, nq = 0, naty = 0, npx = 0;  // (maxima: no order to fix)
    for (int r = 0; r < M; r++) {
      pri = fmax(pri, fabs(ax[r] - zs[r]));
      nz = fmax(nz, fabs(zs[r]));
      nax = fmax(nax, fabs(ax[r]));
    }
    for (int i = 0; i < n; i++) {
      dua = fmax(dua, fabs(Px[i] + au.q[i] + Aty[i]));
      nq = fmax(nq, fabs(au.q[i]));
      naty = fmax(naty, fabs(Aty[i]));
      npx = fmax(npx, fabs(Px[i]));
    }
    pri /= (fmax(nz, nax) + 1e-10);
    dua /= (fmax(nq, fmax(naty, npx)) + 1e-10);
    double r = rho0 * sqrt(pri / (dua + 1e-10));
    r = fmin(fmax(r, 1e-6), 1e6);
    const double chosen = rho_round2(r);
    sc[0] = r;
    sc[1] = (chosen > 0) ? chosen : rho0;
    io.rec->rho_est = r;
    io.rec->rho = sc[1];
  });
  return sc[1];
}

// The choice of rho (body_auto, a model with au.on): probe_rule on the dense Abar in LDS, and where the rule moves rho
// the factor again.  Returns false after a bad pivot of the second factor; `rho` is the rho in use afterwards.
template <class X>
MIOSQP_HD inline bool choose_rho(const IO &io, const Auto &au, double *Lp, const double *Ad, double *tmp, double *dv,
                                 double *pv, X &x, double &rho) {
  const double rho0 = io.rho;
  rho = probe_rule(io, au, AbarLds{Ad, io.n | 1}, Lp, tmp, dv, pv, x);
  if (rho == rho0) return true;  // the first factor stands
  return refactor(io, au, Lp, Ad, tmp, dv, x, rho);
}

template <bool AUTO, class X>
MIOSQP_HD inline void body_phases(const IO &io, const Auto *au, double *lds, X &x) {
  const int n = io.n, M = io.M, N = n + M, NT = THREADS;
  const int lda = n | 1;
  const size_t t_all = tri((size_t)n);
  const Lds at = lds_layout(lds, n, M);
  double *const Lp = at.Lp, *const Ad = at.Ad, *const tmp = at.tmp, *const dv = at.dv;
  double rho = io.rho;                               // (body_auto may choose another one below)
  const double sigma = io.sigma;

  // ---- phase 0: clear the triangle and the dense copy of Abar ----
  x.par([&](int tid) {
    for (size_t k = tid; k < t_all; k += NT) Lp[k] = 0.0;
    for (size_t k = tid; k < (size_t)M * lda; k += NT) Ad[k] = 0.0;
  });
  // ---- phase 1: Abar dense; S = Pbar (lower part of row i: its own column of the upper triangle) + sigma I; f_Pd ----
  x.par([&](int tid) {
    for (int r = tid; r < M; r += NT)
      for (int t = io.pc_ptr[r]; t < io.pc_ptr[r + 1]; t++)
        if (io.pc_A[t] != 0.0) Ad[(size_t)r * lda + io.pc_idx[t]] = io.pc_A[t];
    for (int i = tid; i < n; i += NT) {
      double *Si = Lp + tri((size_t)i);
      for (int t = io.pb_ptr[i]; t < io.pb_ptr[i + 1]; t++) {
        const int c = io.pb_idx[t];
        const double v = io.pb_val[t];
        if (c <= i) Si[c] += v;
        if (v != 0.0) io.f_Pd[(size_t)i * io.ldn + c] = v;
      }
      Si[i] += sigma;
    }
  });
  // ---- phase 2: S += rho Abar^T Abar, constraint rows ascending, fused (factor.cpp adds the same terms in this order);
  //      the dense copies of Abar and Abar^T ----
  x.par([&](int tid) {
    schur_add_rho(tid, Lp, Ad, n, M, lda, rho);
    for (size_t e = tid; e < (size_t)M * io.ldn; e += NT) {
      const int r = (int)(e / io.ldn), c = (int)(e % io.ldn);
      io.f_Ad[e] = c < n ? Ad[(size_t)r * lda + c] : 0.0;
    }
    for (size_t e = tid; e < (size_t)n * io.ldm; e += NT) {
      const int i = (int)(e / io.ldm), r = (int)(e % io.ldm);
      io.f_Atd[e] = r < M ? Ad[(size_t)r * lda + i] : 0.0;
    }
  });
  // ---- phases 3, 4, 5a: the LDL^T, X = L^-1 in place, d2inv ----
  if (!ldl_inverse(io, Lp, tmp, dv, x, 1)) return;
  if constexpr (AUTO) {  // ---- rho chosen in the launch: the probing iterations, the rule, the factor again ----
    if (au->on && !choose_rho(io, *au, Lp, Ad, tmp, dv, at.pv, x, rho)) return;
  }
  // ---- phase 5b: everything that is read off the triangle: Linv, LinvT, the rows of the product form ----
  x.par([&](int tid) {
    const int ld = io.ld, ldf = io.ldf;
    for (size_t e = tid; e < (size_t)n * ld; e += NT) {
      const int i = (int)(e / ld), c = (int)(e % ld);
      io.Linv[e] = c < i ? Lp[tri((size_t)i) + c] : 0.0;            // strict lower, padding zero
      io.LinvT[e] = (c > i && c < n) ? Lp[tri((size_t)c) + i] : 0.0;  // its transpose, lanes along the row
    }
    // row i of the product form: [ -G[i][0..M) | X[i][0..i) | 0 .. ],  -G[i][r] = rho (Abar[r][i] + sum_{j<i} X[i][j] Abar[r][j])
    for (size_t e = tid; e < (size_t)n * ldf; e += NT) {
      const int i = (int)(e / ldf), c = (int)(e % ldf);
      double v = 0.0;
      if (c < M) {
        const double *Ar = Ad + (size_t)c * lda, *Xi = Lp + tri((size_t)i);
        v = rho * Ar[i];
        for (int j = 0; j < i; j++) v = fma(Xi[j], rho * Ar[j], v);
      } else if (c - M < i) {
        v = Lp[tri((size_t)i) + (c - M)];
      }
      io.f_rows[e] = v;
    }
  });
  // ---- phase 6: f_GmT (the transpose of -G, read back), W = F^T D22^-1 F in 64 x 64 tiles with the sums of
  //      ks_kkt_inverse (4 x 4 per thread, factor rows ascending), Kc = [ 0 Abar ; Abar^T Pbar ] ----
  x.par([&](int tid) {
    const int ldf = io.ldf, ldn = io.ldn, ldw = io.ldw;
    for (size_t e = tid; e < (size_t)M * ldn; e += NT) {
      const int r = (int)(e / ldn), i = (int)(e % ldn);
      io.f_GmT[e] = i < n ? io.f_rows[(size_t)i * ldf + r] : 0.0;
    }
    const int tx = tid & 15, ty = tid >> 4, nt = (N + 63) / 64;
    for (int ta = 0; ta < nt; ta++)
      for (int tb = 0; tb < nt; tb++) {
        const int a0 = ta * 64, b0 = tb * 64;
        double acc[4][4] = {};
        const int lo = a0 > b0 ? a0 : b0;  // column c >= M of F is zero above row c - M
        for (int i = lo > M ? ((lo - M) & ~15) : 0; i < n; i++) {
          const double di = dv[i];
          double a[4], b[4];
          for (int p = 0; p < 4; p++) {
            a[p] = f_entry(io.f_rows, ldf, Lp, M, N, i, a0 + ty + 16 * p) * di;
            b[p] = f_entry(io.f_rows, ldf, Lp, M, N, i, b0 + tx + 16 * p);
          }
          for (int p = 0; p < 4; p++)
            for (int q = 0; q < 4; q++) acc[p][q] = fma(a[p], b[q], acc[p][q]);
        }
        for (int p = 0; p < 4; p++)
          for (int q = 0; q < 4; q++) {
            const int a = a0 + ty + 16 * p, b = b0 + tx + 16 * q;
            if (a < N && b < N) io.W[(size_t)a * ldw + b] = acc[p][q];
          }
      }
    for (size_t e = tid; e < (size_t)N * N; e += NT) {
      const int rr = (int)(e / N), c = (int)(e % N);
      double v;
      if (rr < M) v = c < M ? 0.0 : Ad[(size_t)rr * lda + (c - M)];
      else v = c < M ? Ad[(size_t)c * lda + (rr - M)] : io.f_Pd[(size_t)(rr - M) * ldn + (c - M)];
      io.Kc[(size_t)rr * ldw + c] = v;
    }
    // the scaled bounds (k_scale_bounds)
    for (int j = tid; j < M; j += NT) {
      io.l[j] = io.E[j] * fmax(io.raw_l[j], -INFTY);
      io.u[j] = io.E[j] * fmin(io.raw_u[j], INFTY);
    }
  });
  // ---- phase 7: the guard of kernels_guard.inc: u = W r for the probes, then the residual of the KKT system from Kc.
  //      LANES lanes stride a row, their partial sums meet in LDS in lane order. ----
  double *gu = lds;                                   // GUARD_PROBES x N (over the triangle, which is dead now)
  double *part = gu + (size_t)GUARD_PROBES * N;       // THREADS x GUARD_PROBES
  double *worst = part + (size_t)THREADS * GUARD_PROBES;  // N
  const int RB = NT / LANES;
  for (int pass = 0; pass < 2; pass++) {
    const double *Mx = pass == 0 ? io.W : io.Kc;
    for (int rb = 0; rb < N; rb += RB) {
      x.par([&](int tid) {
        const int row = rb + tid / LANES, lane = tid % LANES;
        double acc[GUARD_PROBES] = {};
        if (row < N) {
          const double *w = Mx + (size_t)row * io.ldw;
          for (int c = lane; c < N; c += LANES) {
            const double a = w[c];
            for (int p = 0; p < GUARD_PROBES; p++)
              acc[p] = fma(a, pass == 0 ? guard_probe_value(p, c) : gu[(size_t)p * N + c], acc[p]);
          }
        }
        for (int p = 0; p < GUARD_PROBES; p++) part[(size_t)tid * GUARD_PROBES + p] = acc[p];
      });
      x.par([&](int tid) {
        const int row = rb + tid;
        if (tid >= RB || row >= N) return;
        double wr = 0.0;
        for (int p = 0; p < GUARD_PROBES; p++) {
          double s = 0.0;
          for (int lane = 0; lane < LANES; lane++) s += part[((size_t)tid * LANES + lane) * GUARD_PROBES + p];
          const double r = guard_probe_value(p, row);
          if (pass == 0) {
            gu[(size_t)p * N + row] = row < M ? s - rho * r : s;  // nu | x~ (pass 0 reads the probes, never u)
          } else {
            const double ur = gu[(size_t)p * N + row];
            const double res = row < M ? s - (1.0 / rho) * ur - r : s + sigma * ur - r;
            const double a = fabs(res);
            wr = (a != a) ? HUGE_VAL : (a > wr ? a : wr);  // NaN counts as infinite
          }
        }
        if (pass == 1) worst[row] = wr;
      });
    }
  }
  x.par([&](int tid) {
    if (tid != 0) return;
    double m = 0.0;
    for (int r = 0; r < N; r++) m = worst[r] > m ? worst[r] : m;
    io.rec->bad_pivot = 0;
    io.rec->pivot = -1;
    io.rec->guard = m;
  });
}

// the fixed-rho set-up (k_setup_models)
template <class X>
MIOSQP_HD inline void body(const IO &io, double *lds, X &x) {
  body_phases<false>(io, nullptr, lds, x);
}
// ... and the one that chooses rho for a model with au.on (k_setup_models_auto)
template <class X>
MIOSQP_HD inline void body_auto(const IO &io, const Auto &au, double *lds, X &x) {
  body_phases<true>(io, &au, lds, x);
}

}  // namespace setup_models
}  // namespace miosqp
