// The relaxation of the one-launch trees in REDUCED form (k_tree_r_m, kernels_tree.inc): models whose product form
// [ -G | strict_lower(Linv) ] (n x (M + n) doubles) no workgroup's LDS holds.  With
//     S = Pbar + sigma I + rho Abar^T Abar = L D L^T,   Linv = L^-1 (unit lower),   d2 = 1 / D,
// the KKT solve of an iteration is
//     x~ = Linv^T d2 Linv (rx + rho Abar^T wh),   nu = rho (Abar x~ - wh),      rx = sigma x - q,  wh = z - y / rho,
// which is what the two sweeps of res_admm compute with -G = rho Linv Abar^T multiplied out.  Only the strict lower
// triangle of Linv is kept in LDS (n (n - 1) / 2 doubles: 89 KB at n = 150); Abar is read by variable and by constraint
// from the engine's own rows (LDS copies where they fit, else L2).
//
// Written as PHASES, as setup_models_body.hpp is: a phase is a function of the thread index that reads what earlier
// phases wrote and keeps nothing in registers across its end; the executor `X` runs a phase on every thread and puts a
// barrier behind it.  On the device X is {f(threadIdx.x); __syncthreads()}; the stand-alone CPU program under tests/
// runs the same phases with a loop over the thread index.  A row's sum is split over TG lanes (TG a power of two, the
// lanes of an aligned group): lane t takes the entries t, t + TG, ... in four interleaved chains, and the executor's
// lane_sum adds the TG partial sums as a butterfly, small strides first -- ((p0 + p1) + (p2 + p3)) + ... -- on the
// device through lane exchanges, on the CPU by lane 0 of the group, which forms the other lanes' partial sums itself.
// Every sum is therefore in one fixed order that depends on the model alone.
//
// Plain C++; the HIP qualifiers appear only under hipcc.  Vector loads and stores only, no inline assembly.
#pragma once
#include <cmath>
#include <cstddef>

#include "guard_probe.hpp"  // MIOSQP_HD

namespace miosqp {
namespace tree_reduced {

constexpr int THREADS = 512, WAVES = THREADS / 64;  // RES_THREADS, RES_WAVES
constexpr int NQ = 17;                              // the termination test's norms and sums (kernels_test.inc)
constexpr int TGB = 4;    // lanes per row of Linv (phase B)
constexpr int TGC = 8;    // lanes per column of Linv (phase C): TGB * TGC = 32, see tri_ld
constexpr int TGR = 16;   // lanes per row of Abar^T (phase A) and of Abar (phase D)
constexpr int LEAF_CAP_DEFAULT = 256;
constexpr size_t LDS_LIMIT = 160 * 1024;

// ---- the packed triangle ----------------------------------------------------------------------------------
// Rows i and n - 1 - i of the strict lower triangle hold n - 1 entries together: they share one row of a rectangle of
// ceil(n / 2) rows.  The long row (i >= n / 2) lies forwards from column 0 of rectangle row n - 1 - i, the short one
// backwards from the last column of rectangle row i.  Neighbouring rows of the triangle are one rectangle row apart
// (ld doubles), neighbouring entries of a row one double.  A 32-lane half of a wavefront reads LDS in one cycle when its
// lanes hit 32 different 8-byte banks.  Phase B gives TGB lanes to a row and 32 / TGB consecutive rows to the half:
// banks t - g ld; phase C gives TGC lanes to a column (consecutive rows) and 32 / TGC consecutive columns to the
// half: banks g - t ld.  With ld = -TGB = 28 (mod 32) these are 4 g + t and 4 t + g: all 32 banks once, in both
// walks.  (Only a half that straddles row n / 2, where the direction turns, can meet a conflict.)
MIOSQP_HD inline int tri_ld(int n) {
  const int w = n > 1 ? n - 1 : 1;
  return w + ((32 - TGB) - w % 32 + 32) % 32;
}
MIOSQP_HD inline int tri_rows(int n) { return (n + 1) / 2; }
MIOSQP_HD inline size_t tri_doubles(int n) { return (size_t)tri_rows(n) * (size_t)tri_ld(n); }
// entry (i, j), j < i, and the step from it to (i, j + 1)
MIOSQP_HD inline size_t tri_at(int n, int ld, int i, int j) {
  return i >= n / 2 ? (size_t)(n - 1 - i) * ld + j : (size_t)i * ld + (ld - 1 - j);
}
MIOSQP_HD inline int tri_step(int n, int i) { return i >= n / 2 ? 1 : -1; }

// ---- the LDS of one model ---------------------------------------------------------------------------------
// Offsets in doubles.  There is no product-form matrix and nothing of the register-resident loop (wr2, tv).  The
// termination test's scratch (vp, smc, snc) and the vectors of a node's epilogue (xf, xi, prow, yf, rowbuf) are never
// live together -- the test's last answer is consumed before the epilogue starts, and the epilogue's vectors are dead
// once the children are stored -- so they share `scr`.  The leaf list has `cap` places (TreeArgs.leaf_cap).
struct Carve {
  size_t tri, d2, wr, x, q, ut, dx, tx, z, y, l, u, dy;
  size_t scr;                       // vp (M) | smc (8 M) | snc (4 n)   or   xf | xi | prow (2 n) | yf | rowbuf
  size_t part, res;                 // NQ x WAVES, NQ + 8
  size_t lf_lower, order;           // cap doubles; order, depth, freelist: 3 cap ints
  size_t sc, iiL;                   // 32 doubles of scalars and per-wavefront pairs; n ints
  size_t end;
};
MIOSQP_HD inline Carve carve(int n_, int M_, int cap_) {
  const size_t n = (size_t)n_, M = (size_t)M_, cap = (size_t)cap_;
  Carve c;
  size_t at = 0;
  c.tri = at; at += tri_doubles(n_);
  c.d2 = at; at += n;
  c.wr = at; at += M + n;
  c.x = at; at += n;
  c.q = at; at += n;
  c.ut = at; at += n;
  c.dx = at; at += n;
  c.tx = at; at += n;   // t of phases A / B, then x~ of phases C / D
  c.z = at; at += M;
  c.y = at; at += M;
  c.l = at; at += M;
  c.u = at; at += M;
  c.dy = at; at += M;
  c.scr = at; at += 9 * M + 4 * n;   // (the epilogue's 4 n + 2 M is the smaller of the two)
  c.part = at; at += (size_t)NQ * WAVES;
  c.res = at; at += NQ + 8;
  c.lf_lower = at; at += cap;
  c.order = at; at += (3 * cap + 1) / 2;
  c.sc = at; at += 32;
  c.iiL = at; at += (n + 1) / 2;
  c.end = at + 1;
  return c;
}
MIOSQP_HD inline size_t lds_doubles(int n, int M, int leaf_cap) { return carve(n, M, leaf_cap).end; }
// LDS copies of Abar behind everything else: the rows the test walks (res_sp_doubles counts them) and the rows of
// Abar^T -- values, then column indices and row pointers as ints
MIOSQP_HD inline size_t pv_doubles(size_t nnzV, int n) { return nnzV + (nnzV + (size_t)n + 1 + 1) / 2 + 1; }

// ---- what the phases work on ------------------------------------------------------------------------------
struct State {
  int n, M, ld;
  double *tri, *d2, *wr, *x, *q, *ut, *dx, *tx, *z, *y, *l, *u, *dy;
};
MIOSQP_HD inline State state(double *lds, int n, int M, int cap) {
  const Carve c = carve(n, M, cap);
  return State{n,          M,          tri_ld(n),  lds + c.tri, lds + c.d2, lds + c.wr, lds + c.x, lds + c.q,
               lds + c.ut, lds + c.dx, lds + c.tx, lds + c.z,   lds + c.y,  lds + c.l,  lds + c.u, lds + c.dy};
}
// Abar twice: by variable (rows of Abar^T) and by constraint, each as packed rows (PCsr: padding is a zero value on a
// valid index) or as a dense copy (f_Atd: n x ldm, f_Ad: M x ldn)
struct Abar {
  const int *pv_ptr, *pv_idx;
  const double *pv_At;
  const int *pc_ptr, *pc_idx;
  const double *pc_A;
  const double *Atd, *Ad;
  int ldm, ldn;
  int dense;
};
struct Par {
  double rho, rinv, sigma, alpha;
};

// lane `lane` of `TG`: its share of sum_k val[k] * vec[idx[k]], k in [k0, k1), four chains (the loads of a step are
// independent: a chain of round trips to L2 is what bounds these rows)
MIOSQP_HD inline double packed_dot(const double *val, const int *idx, const double *vec, int k0, int k1, int lane, int TG) {
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int k = k0 + lane;
  for (; k + 3 * TG < k1; k += 4 * TG) {
    const double a0 = val[k], a1 = val[k + TG], a2 = val[k + 2 * TG], a3 = val[k + 3 * TG];
    const int c0 = idx[k], c1 = idx[k + TG], c2 = idx[k + 2 * TG], c3 = idx[k + 3 * TG];
    s0 = fma(a0, vec[c0], s0);
    s1 = fma(a1, vec[c1], s1);
    s2 = fma(a2, vec[c2], s2);
    s3 = fma(a3, vec[c3], s3);
  }
  for (; k < k1; k += TG) s0 = fma(val[k], vec[idx[k]], s0);
  return (s0 + s1) + (s2 + s3);
}
// ... of sum_k a[k * step] * vec[k], k in [0, len)
MIOSQP_HD inline double dense_dot(const double *a, int step, const double *vec, int len, int lane, int TG) {
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int k = lane;
  for (; k + 3 * TG < len; k += 4 * TG) {
    const double a0 = a[(ptrdiff_t)k * step], a1 = a[(ptrdiff_t)(k + TG) * step], a2 = a[(ptrdiff_t)(k + 2 * TG) * step],
                 a3 = a[(ptrdiff_t)(k + 3 * TG) * step];
    s0 = fma(a0, vec[k], s0);
    s1 = fma(a1, vec[k + TG], s1);
    s2 = fma(a2, vec[k + 2 * TG], s2);
    s3 = fma(a3, vec[k + 3 * TG], s3);
  }
  for (; k < len; k += TG) s0 = fma(a[(ptrdiff_t)k * step], vec[k], s0);
  return (s0 + s1) + (s2 + s3);
}

// the triangle and d2 into LDS, once per launch: row i of f_rows holds Linv[i][0 .. i) in columns M .. M + i - 1 (the unit
// diagonal is implied); a wavefront per row, lanes along it
template <class X>
MIOSQP_HD inline void load_triangle(X &x, const State &s, const double *f_rows, int ldf, const double *d2inv) {
  x.par([&](int tid) {
    const int n = s.n;
    for (int i = tid >> 6; i < n; i += WAVES) {
      const double *src = f_rows + (size_t)i * ldf + s.M;
      for (int j = tid & 63; j < i; j += 64) s.tri[tri_at(n, s.ld, i, j)] = src[j];
    }
    for (int i = tid; i < n; i += THREADS) s.d2[i] = d2inv[i];
  });
}

// one ADMM iteration on s (x, z, y, l, u, q, dx, dy, wr = [wh | rx] as res_admm keeps them): four phases
template <class X>
MIOSQP_HD inline void iterate(X &x, const State &s, const Abar &A, const Par &p) {
  const int n = s.n, M = s.M, ld = s.ld;
  // ---- (A) t = rx + rho Abar^T wh, by variable ----
  x.par([&](int tid) {
    const int g = tid / TGR, t = tid % TGR;
    for (int i = g; i < n; i += THREADS / TGR) {
      const double acc = x.lane_sum(TGR, t, [&](int lane) {
        return A.dense ? dense_dot(A.Atd + (size_t)i * A.ldm, 1, s.wr, M, lane, TGR)
                       : packed_dot(A.pv_At, A.pv_idx, s.wr, A.pv_ptr[i], A.pv_ptr[i + 1], lane, TGR);
      });
      if (t == 0) s.tx[i] = fma(p.rho, acc, s.wr[M + i]);
    }
  });
  // ---- (B) ut = d2 (t + strict_lower(Linv) t), by row ----
  x.par([&](int tid) {
    const int g = tid / TGB, t = tid % TGB;
    for (int i = g; i < n; i += THREADS / TGB) {
      const double acc = x.lane_sum(TGB, t, [&](int lane) {
        return dense_dot(s.tri + tri_at(n, ld, i, 0), tri_step(n, i), s.tx, i, lane, TGB);
      });
      if (t == 0) s.ut[i] = s.d2[i] * (s.tx[i] + acc);
    }
  });
  // ---- (C) x~ = ut + strict_lower(Linv)^T ut, by column (rows descending from n - 1: every column's lanes start on the
  //      same rows); the x update of res_admm ----
  x.par([&](int tid) {
    const int g = tid / TGC, t = tid % TGC;
    for (int j = g; j < n; j += THREADS / TGC) {
      const double acc = x.lane_sum(TGC, t, [&](int lane) {
        double s0 = 0.0, s1 = 0.0;
        int i = n - 1 - lane;
        for (; i - TGC > j; i -= 2 * TGC) {
          s0 = fma(s.tri[tri_at(n, ld, i, j)], s.ut[i], s0);
          s1 = fma(s.tri[tri_at(n, ld, i - TGC, j)], s.ut[i - TGC], s1);
        }
        if (i > j) s0 = fma(s.tri[tri_at(n, ld, i, j)], s.ut[i], s0);
        return s0 + s1;
      });
      if (t == 0) {
        const double xt = s.ut[j] + acc, xp = s.x[j];
        const double xn = p.alpha * xt + (1.0 - p.alpha) * xp;
        s.x[j] = xn;
        s.dx[j] = xn - xp;
        s.wr[M + j] = p.sigma * xn - s.q[j];
        s.tx[j] = xt;
      }
    }
  });
  // ---- (D) nu = rho (Abar x~ - wh), by constraint; the z / y / dy / wh update of res_admm ----
  x.par([&](int tid) {
    const int g = tid / TGR, t = tid % TGR;
    for (int j = g; j < M; j += THREADS / TGR) {
      const double acc = x.lane_sum(TGR, t, [&](int lane) {
        return A.dense ? dense_dot(A.Ad + (size_t)j * A.ldn, 1, s.tx, n, lane, TGR)
                       : packed_dot(A.pc_A, A.pc_idx, s.tx, A.pc_ptr[j], A.pc_ptr[j + 1], lane, TGR);
      });
      if (t == 0) {
        const double zp = s.z[j], yp = s.y[j];
        const double nu = p.rho * (acc - s.wr[j]);
        const double zt = zp + p.rinv * (nu - yp);
        const double zr = p.alpha * zt + (1.0 - p.alpha) * zp;
        const double v = zr + p.rinv * yp;
        const double zn = fmin(fmax(v, s.l[j]), s.u[j]);
        const double dyj = p.rho * (zr - zn);
        const double yn = yp + dyj;
        s.z[j] = zn;
        s.y[j] = yn;
        s.dy[j] = dyj;
        s.wr[j] = zn - p.rinv * yn;
      }
    }
  });
}

}  // namespace tree_reduced
}  // namespace miosqp
