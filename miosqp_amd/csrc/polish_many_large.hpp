// Polishing of many LARGER instances in one launch (polish_many_large.hip; C entry miosqp_qp_polish_many_large in
// engine.hip): what the two translation units share.  The records, the output layout and the pinned blocks are those of
// polish_many.hpp; an instance's reduced matrix and work vectors live in a slab of device scratch per workgroup.
#pragma once

#include "polish_many.hpp"

namespace miosqp {

constexpr int POLG_NMAX = 512;              // the widest reduced system (config 2 has n = 500; nothing larger was tried)
constexpr int POLG_MMAX = 1 << 16;          // rows of A
constexpr size_t POLG_BUDGET = (size_t)1 << 30;  // bytes of slabs one engine may hold (2.4 MB each at n = 512)

struct PolManyLargeArgs {
  PolManyArgs a;            // as for k_pol_many (a.A: rows of A by constraint, pc_*)
  const int *pv_ptr, *pv_idx;
  const double *At;         // rows of A^T (by variable, pv_*), unscaled, pads zero
  double *slab;             // gridDim.x slabs of slab_doubles each
  size_t slab_doubles;
};

// doubles of one workgroup's slab; (size_t)-1 beyond the limits
size_t polish_many_large_slab_doubles(int n, int M);
// queues the one launch of `W` workgroups on `stream`; returns the hipError_t of the launch as an int (0: queued)
int polish_many_large_launch(const PolManyLargeArgs &g, int W, void *stream);

}  // namespace miosqp
