// Polishing of many small instances in one launch (polish_many.hip; C entry miosqp_qp_polish_many in engine.hip):
// what the two translation units share -- the kernel's argument block, the record an instance writes, the host's scratch.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define POLM_HD __host__ __device__
#else
#define POLM_HD  // (polish_models_plan.hpp brings this header into a plain C++ program)
#endif

namespace miosqp {

// one instance's answer on the device and in the pinned block: this record, then x (n), y (M), then the class of every
// row in the final set (M bytes, padded to doubles)
struct PolManyRec {
  int accepted, reason, n_lower, n_upper;
  int rounds, stop, n_added, n_dropped, accepted0, reason0, pad[2];
  double pri_before, dua_before, pri_after, dua_after, obj;
};
constexpr size_t POLM_REC_DOUBLES = (sizeof(PolManyRec) + 7) / 8;
constexpr size_t polm_out_stride(int n, int M) { return POLM_REC_DOUBLES + (size_t)n + (size_t)M + ((size_t)M + 7) / 8; }

// raw device pointers and sizes: the unscaled problem as the single polish keeps it (rows of A by constraint with the
// engine's padded pattern, rows of the full symmetric P), the call's inputs (instance-major) and where the answers go
struct PolManyArgs {
  int n, M, B, refine_iter, repair_iter;
  double delta, inv_delta;
  const int *pc_ptr, *pc_idx, *pr_ptr, *pr_idx;
  const double *A, *pr_val;
  const double *q;         // B x n, or nullptr: q_engine (n) for every instance
  const double *q_engine;
  const double *l, *u, *x, *y;  // B x M, B x M, B x n, B x M
  double *out;             // B x polm_out_stride(n, M)
};

// one entry of the table of k_pol_many_m (miosqp_qp_polish_models): a model's own sizes, settings and FINAL pointers (B
// is 1, nothing is offset by the workgroup's index); a.y may be nullptr when tau > 0: the kernel guesses y from z
struct PolManyModel {
  PolManyArgs a;
  double tau;
};

// the LDS image of one instance, in doubles from the start of the dynamic block
struct PolmLds {
  int S, Ad, q, xh, t, v, px, xk, l, u, yh, r2, yk, red, act, cls, total;
};
POLM_HD inline PolmLds polm_layout(int n, int M) {
  PolmLds o;
  const int lda = n | 1;  // odd: the threads of a wavefront, one per row, fall on different banks
  int c = 0;
  o.S = c; c += (n * (n + 1)) / 2;
  o.Ad = c; c += M * lda;
  o.q = c; c += n;
  o.xh = c; c += n;
  o.t = c; c += n;
  o.v = c; c += n;
  o.px = c; c += n;
  o.xk = c; c += n;
  o.l = c; c += M;
  o.u = c; c += M;
  o.yh = c; c += M;
  o.r2 = c; c += M;
  o.yk = c; c += M;
  o.red = c; c += 8;
  o.act = c; c += (M + 1) / 2;      // M ints
  o.cls = c; c += (2 * M + 7) / 8;  // two class arrays of M bytes
  o.total = c;
  return o;
}
constexpr int POLM_NMAX = 192;  // three entries per lane of the wavefront that runs the substitutions
// bytes of LDS one instance's workgroup needs, (size_t)-1 beyond one thread per row and three entries per lane
inline size_t polm_lds_bytes(int n, int M) {
  if (n < 1 || M < 0 || n > POLM_NMAX || M > 256) return (size_t)-1;
  return (size_t)polm_layout(n, M).total * sizeof(double);
}

// host scratch of one engine: the pinned blocks of both directions and their device copies (grown with B on demand),
// the events around a call; the last call's answers stay in h_out for the class getter
struct PolManyScratch {
  double *h_in = nullptr, *h_out = nullptr, *d_in = nullptr, *d_out = nullptr;
  size_t cap_in = 0, cap_out = 0;  // doubles
  void *ev[2] = {nullptr, nullptr};
  int last_B = 0;
  double *slab = nullptr;  // miosqp_qp_polish_many_large only: the workgroups' slabs (polish_many_large.hpp)
  size_t cap_slab = 0;     // doubles
};

// bytes of LDS one instance's workgroup needs (the caller compares with the chip's 160 KB)
size_t polish_many_lds_bytes(int n, int M);
// queues the one launch on `stream` (a hipStream_t); returns the hipError_t of the launch as an int (0: queued)
int polish_many_launch(const PolManyArgs &a, void *stream);
// ... the launch over a table of B entries in device memory, with `lds_bytes` of dynamic LDS (the largest need among them)
int polish_models_launch(const PolManyModel *table, int B, size_t lds_bytes, void *stream);

}  // namespace miosqp
