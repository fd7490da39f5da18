// The preparation of ONE model by ONE workgroup (k_prepare_models, kernels_prepare_models.inc): what the host builds
// with scale_problem and pack_factor_rows (factor.cpp) -- the packed rows of the panel by variable and by constraint,
// the two symmetric matrices by row, the Ruiz equilibration with the cost normalisation, D, E, c, their inverses, the
// scaled q and the panel's values -rho Abar -- from the RAW problem (CSC of P as given, CSC of A, q), bit for bit.
// Written as setup_models_body.hpp is: a sequence of PHASES, each a function of the thread index that reads what earlier
// phases wrote and keeps nothing in registers across its end; the executor `X` runs a phase on every thread and puts a
// barrier behind it.  The stand-alone CPU program under tests/ runs the same phases with a loop over the thread index.
//
// Why the bits are the host's: an equilibration pass consists of maxima (any order gives the same value), 1 / sqrt(.)
// (both operations correctly rounded), products of a value with the product of two scalings (no sum, so nothing to
// contract; a product commutes) and ONE sum, the mean of Pbar's norms, which one thread forms in ascending order.
//
// The host hands over the four pointer arrays of the packed structures (prepare_pointers below: histograms of Ai / Pi,
// O(nnz) integer work) -- the plan of the arena needs their last entries anyway.
//
// Plain C++; the HIP qualifiers appear only under hipcc.  Vector stores only, no inline assembly, no floating-point
// atomic: the one atomic is an unsigned integer maximum on LDS (the bit pattern of a non-negative double orders as the
// double does), on the CPU a plain maximum.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "guard_probe.hpp"  // MIOSQP_HD

namespace miosqp {
namespace prepare_models {

constexpr int THREADS = 256;  // one workgroup per model
constexpr int LANES = 16;     // lanes per row where a phase strides rows (THREADS / LANES rows at a time)
constexpr double MIN_SCALING = 1e-4, MAX_SCALING = 1e4;  // kMinScaling, kMaxScaling of factor.cpp

// the scalars of one model's equilibration: they come back with the download
struct Scalars {
  double c, cinv;
};

// what a workgroup reads and writes: final pointers into the call's arena
struct IO {
  int n, M, passes;
  double rho;
  const int *Pp, *Pi;  // P as given (CSC; only row <= column is read), A (CSC), q: the raw problem
  const double *Px;
  const int *Ap, *Ai;
  const double *Ax;
  const double *qraw;
  const int *pv_ptr, *pc_ptr, *pb_ptr, *pr_ptr;  // made by the host (prepare_pointers)
  int *pv_idx, *pc_idx, *pb_idx, *pr_idx;
  double *pv_L, *pv_At, *pc_L, *pc_A, *pb_val, *pr_val;
  double *D, *Dinv, *E, *Einv, *q;
  Scalars *sc;
};

// LDS of the kernel for one model, in doubles: dt | et | D | E | q | 4 scalars | cursors by constraint | cursors of P
MIOSQP_HD inline size_t lds_doubles(int n, int M) {
  return 3 * (size_t)n + 2 * (size_t)M + 4 + ((size_t)n + (size_t)M + 1) / 2;
}

struct Lds {
  double *dt, *et, *D, *E, *q, *s;  // s[0]: c, s[1]: the cost scaling of the pass
  int *cc, *cp;                     // entries written so far to a row by constraint / to a row of the symmetric matrices
};
MIOSQP_HD inline Lds lds_layout(double *lds, int n, int M) {
  Lds w;
  w.dt = lds;
  w.et = w.dt + n;
  w.D = w.et + M;
  w.E = w.D + n;
  w.q = w.E + M;
  w.s = w.q + n;
  w.cc = reinterpret_cast<int *>(w.s + 4);
  w.cp = w.cc + M;
  return w;
}

MIOSQP_HD inline double clamp_scaling(double v) {  // factor.cpp
  if (v < MIN_SCALING) v = 1.0;
  if (v > MAX_SCALING) v = MAX_SCALING;
  return v;
}

// *slot = max(*slot, a) for a >= 0 (an absolute value), from several threads of a phase at once
MIOSQP_HD inline void absmax_to(double *slot, double a) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMax(reinterpret_cast<unsigned long long *>(slot), (unsigned long long)__double_as_longlong(a));
#else
  if (*slot < a) *slot = a;
#endif
}

// max |val| over the packed rows (pads are zeros) into norm[row]; with `cols`, into cols[idx] as well
MIOSQP_HD inline void row_norms(int tid, int rows, const int *ptr, const int *idx, const double *val, double *norm, double *cols) {
  for (int r = tid / LANES; r < rows; r += THREADS / LANES) {
    double m = 0.0;
    for (int k = ptr[r] + tid % LANES; k < ptr[r + 1]; k += LANES) {
      const double a = fabs(val[k]);
      if (m < a) m = a;
      if (cols) absmax_to(&cols[idx[k]], a);
    }
    absmax_to(&norm[r], m);
  }
}

// val[k] *= sr[row] * sc[idx[k]] over the packed rows
MIOSQP_HD inline void row_scale(int tid, int rows, const int *ptr, const int *idx, double *val, const double *sr, const double *sc) {
  for (int r = tid / LANES; r < rows; r += THREADS / LANES)
    for (int k = ptr[r] + tid % LANES; k < ptr[r + 1]; k += LANES) val[k] *= sr[r] * sc[idx[k]];
}

// the panel's values of the packed rows: -rho a for an entry (an explicit zero gives -0.0), 0.0 for the pad
MIOSQP_HD inline void panel_values(int tid, int rows, const int *ptr, const double *a, double *L, double rho, const int *Ap, const int *cnt) {
  for (int r = tid / LANES; r < rows; r += THREADS / LANES) {
    const int c = Ap ? Ap[r + 1] - Ap[r] : cnt[r];
    for (int k = tid % LANES; k < ptr[r + 1] - ptr[r]; k += LANES) L[ptr[r] + k] = k < c ? -rho * a[ptr[r] + k] : 0.0;
  }
}

template <class X>
MIOSQP_HD inline void body(const IO &io, double *lds, X &x) {
  const int n = io.n, M = io.M, NT = THREADS;
  const Lds w = lds_layout(lds, n, M);
  // ---- phase 1: rows by variable (the CSC columns of A, ascending already) with their pad; the first part of every row
  //      of the two symmetric matrices (column r of the upper triangle); the cursors; D = E = 1, q, c = 1 ----
  x.par([&](int tid) {
    for (int j = tid / LANES; j < n; j += NT / LANES) {
      const int a0 = io.Ap[j], cnt = io.Ap[j + 1] - a0, base = io.pv_ptr[j];
      for (int k = tid % LANES; k < cnt; k += LANES) {
        io.pv_idx[base + k] = io.Ai[a0 + k];
        io.pv_At[base + k] = io.Ax[a0 + k];
      }
      if (tid % LANES == 0 && (cnt & 1)) {
        io.pv_idx[base + cnt] = io.Ai[a0 + cnt - 1];
        io.pv_At[base + cnt] = 0.0;
      }
    }
    for (int j = tid; j < n; j += NT) {
      int wr = io.pb_ptr[j], cnt = 0;
      for (int p = io.Pp[j]; p < io.Pp[j + 1]; p++) {
        const int i = io.Pi[p];
        if (i > j) continue;  // only the upper triangle is read
        const double v = io.Px[p];
        io.pb_idx[wr] = i;
        io.pr_idx[wr] = i;
        io.pb_val[wr] = v;
        io.pr_val[wr] = v;
        wr++;
        cnt++;
      }
      w.cp[j] = cnt;
      w.D[j] = 1.0;
      w.q[j] = io.qraw[j];
    }
    for (int i = tid; i < M; i += NT) {
      w.cc[i] = 0;
      w.E[i] = 1.0;
    }
    if (tid == 0) w.s[0] = 1.0;
  });
  // ---- phase 2: the transposes, one column per step: rows by constraint, and the second part of the symmetric rows (row
  //      i of the strict upper triangle).  Row indices ascend strictly within a column, so no two threads of a step meet
  //      at a cursor; the steps follow the columns, so every row comes out ascending ----
  for (int j = 0; j < n; j++)
    x.par([&](int tid) {
      for (int p = io.Ap[j] + tid; p < io.Ap[j + 1]; p += NT) {
        const int i = io.Ai[p], k = io.pc_ptr[i] + w.cc[i];
        w.cc[i]++;
        io.pc_idx[k] = j;
        io.pc_A[k] = io.Ax[p];
      }
      for (int p = io.Pp[j] + tid; p < io.Pp[j + 1]; p += NT) {
        const int i = io.Pi[p];
        if (i >= j) continue;
        const int k = io.pb_ptr[i] + w.cp[i];
        w.cp[i]++;
        const double v = io.Px[p];
        io.pb_idx[k] = j;
        io.pr_idx[k] = j;
        io.pb_val[k] = v;
        io.pr_val[k] = v;
      }
    });
  // ---- phase 3: the pads of those rows (zero value, the last valid column); the norms of the first pass start at 0 ----
  x.par([&](int tid) {
    for (int i = tid; i < M; i += NT) {
      const int cnt = w.cc[i], e = io.pc_ptr[i] + cnt;
      if (cnt & 1) {
        io.pc_idx[e] = io.pc_idx[e - 1];
        io.pc_A[e] = 0.0;
      }
      w.et[i] = 0.0;
    }
    for (int i = tid; i < n; i += NT) {
      const int cnt = w.cp[i], e = io.pb_ptr[i] + cnt;
      if (cnt & 1) {
        io.pb_idx[e] = io.pb_idx[e - 1];
        io.pr_idx[e] = io.pb_idx[e - 1];
        io.pb_val[e] = 0.0;
        io.pr_val[e] = 0.0;
      }
      w.dt[i] = 0.0;
    }
  });
  // ---- phase 4: the equilibration passes, in place on Abar^T by variable, Abar by constraint and Pbar by row ----
  for (int pass = 0; pass < io.passes; pass++) {
    // column norms of [P A^T; A 0]: a row of the full symmetric Pbar and a row by variable give dt, the latter's columns et
    x.par([&](int tid) {
      row_norms(tid, n, io.pb_ptr, io.pb_idx, io.pb_val, w.dt, nullptr);
      row_norms(tid, n, io.pv_ptr, io.pv_idx, io.pv_At, w.dt, w.et);
    });
    x.par([&](int tid) {
      for (int j = tid; j < n; j += NT) w.dt[j] = 1.0 / sqrt(clamp_scaling(w.dt[j]));
      for (int i = tid; i < M; i += NT) w.et[i] = 1.0 / sqrt(clamp_scaling(w.et[i]));
    });
    x.par([&](int tid) {
      row_scale(tid, n, io.pb_ptr, io.pb_idx, io.pb_val, w.dt, w.dt);
      row_scale(tid, n, io.pv_ptr, io.pv_idx, io.pv_At, w.dt, w.et);
      row_scale(tid, M, io.pc_ptr, io.pc_idx, io.pc_A, w.et, w.dt);
      for (int j = tid; j < n; j += NT) {
        w.q[j] *= w.dt[j];
        w.D[j] *= w.dt[j];
      }
      for (int i = tid; i < M; i += NT) w.E[i] *= w.et[i];
    });
    // cost normalisation: the mean of Pbar's norms (one thread, ascending) against max |q|
    x.par([&](int tid) {
      for (int j = tid; j < n; j += NT) w.dt[j] = 0.0;
    });
    x.par([&](int tid) { row_norms(tid, n, io.pb_ptr, io.pb_idx, io.pb_val, w.dt, nullptr); });
    x.par([&](int tid) {
      if (tid != 0) return;
      double mean = 0;
      for (int j = 0; j < n; j++) mean += w.dt[j];
      mean /= n;
      double nq = 0;
      for (int j = 0; j < n; j++) {
        const double a = fabs(w.q[j]);
        if (nq < a) nq = a;
      }
      const double cq = clamp_scaling(nq);
      const double ct = 1.0 / clamp_scaling(mean < cq ? cq : mean);
      w.s[1] = ct;
      w.s[0] *= ct;
    });
    x.par([&](int tid) {
      const double ct = w.s[1];
      for (int r = tid / LANES; r < n; r += NT / LANES)
        for (int k = io.pb_ptr[r] + tid % LANES; k < io.pb_ptr[r + 1]; k += LANES) io.pb_val[k] *= ct;
      for (int j = tid; j < n; j += NT) {
        w.q[j] *= ct;
        w.dt[j] = 0.0;
      }
      for (int i = tid; i < M; i += NT) w.et[i] = 0.0;
    });
  }
  // ---- phase 5: what remains: D, E, their inverses, the scaled q, c; the panel's values ----
  x.par([&](int tid) {
    for (int j = tid; j < n; j += NT) {
      io.D[j] = w.D[j];
      io.Dinv[j] = 1.0 / w.D[j];
      io.q[j] = w.q[j];
    }
    for (int i = tid; i < M; i += NT) {
      io.E[i] = w.E[i];
      io.Einv[i] = 1.0 / w.E[i];
    }
    if (tid == 0) {
      io.sc->c = w.s[0];
      io.sc->cinv = 1.0 / w.s[0];
    }
    panel_values(tid, n, io.pv_ptr, io.pv_At, io.pv_L, io.rho, io.Ap, nullptr);
    panel_values(tid, M, io.pc_ptr, io.pc_A, io.pc_L, io.rho, nullptr, w.cc);
  });
}

// ---- host: the pointer arrays of the four packed structures from histograms of Ai / Pi (every row padded to an even
//      count), and how many entries of P lie in the upper triangle.  pb_ptr serves Pbar and Praw: the same pattern. ----
inline void prepare_pointers(int n, int M, const int32_t *Pp, const int32_t *Pi, const int32_t *Ap, const int32_t *Ai, int32_t *pv_ptr,
                             int32_t *pc_ptr, int32_t *pb_ptr, int64_t *nnz_upper) {
  pv_ptr[0] = 0;
  for (int j = 0; j < n; j++) pv_ptr[j + 1] = pv_ptr[j] + ((Ap[j + 1] - Ap[j] + 1) & ~1);
  for (int i = 0; i <= M; i++) pc_ptr[i] = 0;
  for (int32_t p = 0; p < Ap[n]; p++) pc_ptr[Ai[p] + 1]++;
  for (int i = 0; i < M; i++) pc_ptr[i + 1] = pc_ptr[i] + ((pc_ptr[i + 1] + 1) & ~1);
  for (int i = 0; i <= n; i++) pb_ptr[i] = 0;
  int64_t up = 0;
  for (int j = 0; j < n; j++)
    for (int32_t p = Pp[j]; p < Pp[j + 1]; p++) {
      const int i = Pi[p];
      if (i > j) continue;
      up++;
      pb_ptr[j + 1]++;
      if (i != j) pb_ptr[i + 1]++;
    }
  for (int i = 0; i < n; i++) pb_ptr[i + 1] = pb_ptr[i] + ((pb_ptr[i + 1] + 1) & ~1);
  *nnz_upper = up;
}

}  // namespace prepare_models
}  // namespace miosqp
