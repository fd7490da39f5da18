// Polishing of many LARGER instances in one launch (polish_many_large.hip; C entries miosqp_qp_polish_many_large and
// miosqp_qp_polish_models_large in engine.hip): what the translation units share.  The records, the output layout and the
// pinned blocks are those of polish_many.hpp; an instance's reduced matrix and work vectors live in a slab of device
// scratch per workgroup.  Plain C++ outside the launchers' declarations: polish_models_large_plan.hpp brings this header
// into a stand-alone program.
#pragma once

#include "polish_many.hpp"

namespace miosqp {

constexpr int POLG_NMAX = 512;              // the widest reduced system (config 2 has n = 500; nothing larger was tried)
constexpr int POLG_MMAX = 1 << 16;          // rows of A
constexpr size_t POLG_BUDGET = (size_t)1 << 30;  // bytes of slabs one engine may hold (2.4 MB each at n = 512)
constexpr int POLG_NB = 32;                 // panel width of the factorisation, block of the substitutions, rows of a chunk

struct PolManyLargeArgs {
  PolManyArgs a;            // as for k_pol_many (a.A: rows of A by constraint, pc_*)
  const int *pv_ptr, *pv_idx;
  const double *At;         // rows of A^T (by variable, pv_*), unscaled, pads zero
  double *slab;             // gridDim.x slabs of slab_doubles each
  size_t slab_doubles;
};

// one entry of the table of k_pol_many_gm (miosqp_qp_polish_models_large): a model's own sizes, settings and FINAL
// pointers (g.a.B is 1, nothing is offset by the workgroup's index; g.slab and g.slab_doubles are unused: the slabs are
// the launch's); g.a.y may be nullptr when tau > 0: the kernel guesses y from z
struct PolManyLargeModel {
  PolManyLargeArgs g;
  double tau;
};

// one workgroup's slab, in doubles from its start
struct PolgSlab {
  int ld, ldw;
  size_t S, Wp, Lp, xh, t, v, xk, dd, ocol, dcol, yh, r2, yk, prow, act, cls, total;
};
POLM_HD inline PolgSlab polg_layout(int n, int M) {
  PolgSlab o;
  o.ld = (n + 7) & ~7;
  o.ldw = o.ld;
  const size_t nn = (size_t)o.ld, mm = ((size_t)M + 7) & ~(size_t)7;
  size_t c = 0;
  o.S = c; c += (size_t)n * nn;
  o.Wp = c; c += POLG_NB * nn;
  o.Lp = c; c += POLG_NB * nn;
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

// doubles of one workgroup's slab; (size_t)-1 beyond the limits
inline size_t polish_many_large_slab_doubles(int n, int M) {
  if (n < 1 || M < 0 || n > POLG_NMAX || M > POLG_MMAX) return (size_t)-1;
  return polg_layout(n, M).total;
}
// queues the one launch of `W` workgroups on `stream`; returns the hipError_t of the launch as an int (0: queued)
int polish_many_large_launch(const PolManyLargeArgs &g, int W, void *stream);
// ... the launch of `W` workgroups over a table of B entries in device memory, on W slabs of slab_doubles each
int polish_models_large_launch(const PolManyLargeModel *table, int B, int W, double *slabs, size_t slab_doubles, void *stream);

}  // namespace miosqp
