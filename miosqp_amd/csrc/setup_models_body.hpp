// The dense set-up of ONE small model by ONE workgroup (k_setup_models, kernels_setup_models.inc): what miosqp_qp_setup
// builds for the LDS-resident form with the explicit inverse -- the Schur complement, its LDL^T, the triangular inverse,
// the product form, W, Kc, the guard residual and the scaled bounds -- written as a sequence of PHASES.  A phase is a
// function of the thread index that reads what earlier phases wrote and keeps nothing in registers across its end; the
// executor `X` runs a phase on every thread and puts a barrier behind it.  On the device X is {f(threadIdx.x);
// __syncthreads()}; the stand-alone CPU program under tests/ runs the same phases with a loop over the thread index, so
// the arithmetic below is checked against the long-double reference without a GPU.  Code outside a phase only READS
// values that are the same for every thread (a pivot, a loop bound).
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
  int32_t bad_pivot;   // 1: the pivot at index `pivot` was not positive or not finite (nothing behind the LDL^T was built)
  int32_t pivot;
  double guard;        // max |K W r - r| over the probes (infinite for a NaN), as inverse_guard reads it
  double reserved[2];
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
// the size rule of the launch: one workgroup holds the model
MIOSQP_HD inline bool eligible_shape(int n, int M) {
  return n >= 1 && M >= 1 && n + M <= MAX_NM && lds_doubles(n, M) * sizeof(double) <= LDS_LIMIT;
}

// entry (i, c) of F = [ -G | L22^-1 ] with the unit diagonal restored (dense_setup.hip: ks_kkt_inverse reads the same)
// -G comes from memory (it was never in LDS: the dense Abar holds that room), the triangular part from the triangle Xp in LDS
MIOSQP_HD inline double f_entry(const double *F, int ldf, const double *Xp, int M, int N, int i, int c) {
  if (c >= N) return 0.0;
  if (c < M) return F[(size_t)i * ldf + c];
  return c == M + i ? 1.0 : (c > M + i ? 0.0 : Xp[tri((size_t)i) + (c - M)]);
}

template <class X>
MIOSQP_HD inline void body(const IO &io, double *lds, X &x) {
  const int n = io.n, M = io.M, N = n + M, NT = THREADS;
  const int lda = n | 1;
  const size_t t_all = tri((size_t)n), g_all = guard_doubles(n, M);
  double *Lp = lds;                                  // packed lower triangle: S, then L (diagonal: d), then L^-1
  double *Ad = lds + (t_all > g_all ? t_all : g_all);  // dense Abar, row r at r * lda
  double *tmp = Ad + (size_t)M * lda;                // two rows of L (the triangular inverse works in place)
  double *dv = tmp + 2 * (size_t)n;                  // d, then 1 / d
  const double rho = io.rho, sigma = io.sigma;

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
    for (int i1 = tid / LANES; i1 < n; i1 += NT / LANES)
      for (int i2 = tid % LANES; i2 <= i1; i2 += LANES) {
        double s = Lp[tri((size_t)i1) + i2];
        for (int r = 0; r < M; r++) s = fma(rho * Ad[(size_t)r * lda + i1], Ad[(size_t)r * lda + i2], s);
        Lp[tri((size_t)i1) + i2] = s;
      }
    for (size_t e = tid; e < (size_t)M * io.ldn; e += NT) {
      const int r = (int)(e / io.ldn), c = (int)(e % io.ldn);
      io.f_Ad[e] = c < n ? Ad[(size_t)r * lda + c] : 0.0;
    }
    for (size_t e = tid; e < (size_t)n * io.ldm; e += NT) {
      const int i = (int)(e / io.ldm), r = (int)(e % io.ldm);
      io.f_Atd[e] = r < M ? Ad[(size_t)r * lda + i] : 0.0;
    }
  });
  // ---- phase 3: right-looking LDL^T in place, one column per step (the order of the textbook algorithm) ----
  for (int j = 0; j < n; j++) {
    const double dj = Lp[tri((size_t)j) + j];  // (the same value on every thread: written before the last barrier)
    if (!(dj > 0.0) || !std::isfinite(dj)) {   // the test of the host factorisation
      x.par([&](int tid) {
        if (tid == 0) {
          io.rec->bad_pivot = 1;
          io.rec->pivot = j;
          io.rec->guard = -1.0;
        }
      });
      return;
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
  // ---- phase 5: d2inv; then everything that is read off the triangle: Linv, LinvT, the rows of the product form ----
  x.par([&](int tid) {
    for (int j = tid; j < n; j += NT) {
      const double v = 1.0 / dv[j];
      dv[j] = v;
      io.d2inv[j] = v;
    }
  });
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

}  // namespace setup_models
}  // namespace miosqp
