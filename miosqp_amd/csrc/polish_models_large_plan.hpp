// Polishes of different LARGER models in one launch (miosqp_qp_polish_models_large): the host logic that needs neither an
// engine nor the device -- the fit rule, the number of workgroups, and the layout of the call's arena.  The argument
// checks are those of polish_models_plan.hpp (check_args with this entry's name).  Plain C++ (no HIP): engine.hip
// includes it, and so does the stand-alone sanitized program under tests/.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "polish_many_large.hpp"
#include "polish_models_plan.hpp"

namespace miosqp {
namespace polish_models_large {

using polish_models::ERR_ARG;
using polish_models::ERR_BOUNDS;
using polish_models::ERR_UNSUPPORTED;
using polish_models::NONE;
using polish_models::round_up;

constexpr const char *ENTRY = "polish_models_large";

// the fit rule: within the slab limits (n <= 512, M <= 65536) and one slab within the budget
inline bool fits(int n, int M) {
  const size_t slab = polish_many_large_slab_doubles(n, M);
  return slab != (size_t)-1 && slab * sizeof(double) <= POLG_BUDGET;
}

struct Shape {
  int n, M;
  size_t rows_con, rows_var;  // doubles of the unscaled rows of A to stage, by constraint and by variable (the patterns'
                              // entries); both 0: the engine lends the copies of its single polish's scratch
  bool has_q, has_y;          // q[b] / y[b] given (otherwise the engine's cost / the device's guess: no room is taken)
};

// the models beyond the slabs: MIOSQP_EUNSUPPORTED naming the first, 0 when all fit
inline int check_fit(const std::vector<Shape> &sh, std::string &err) {
  for (size_t b = 0; b < sh.size(); b++)
    if (!fits(sh[b].n, sh[b].M)) {
      err = std::string(ENTRY) + ": model " + std::to_string(b) + " is beyond the slabs (n " + std::to_string(sh[b].n) + ", M " +
            std::to_string(sh[b].M) + "; only for n <= 512 and M <= 65536): polish that model on its own";
      return ERR_UNSUPPORTED;
    }
  return 0;
}

// W = min(B, two workgroups per compute unit, what the slab budget allows); 0 when one slab exceeds the budget
inline int workgroups(size_t B, int compute_units, size_t slab_doubles) {
  if (slab_doubles == 0 || slab_doubles == (size_t)-1 || slab_doubles * sizeof(double) > POLG_BUDGET) return 0;
  const size_t fit = POLG_BUDGET / (slab_doubles * sizeof(double));
  return (int)std::min(std::min(B, (size_t)2 * (size_t)std::max(compute_units, 1)), fit);
}

// where model b's arrays lie in the arena (offsets in doubles from its base; NONE: no room taken)
struct Slot {
  size_t A, At, q, l, u, x, y;  // uploaded
  size_t out;                   // downloaded: record | x | y | classes (polm_out_stride)
};

// [ table | per model: rows of A by constraint, rows of A^T by variable, q, l, u, x, y | per model: record | W slabs ]:
// the first two parts go up in ONE copy, the records come back in ONE copy, the slabs are device-only and take no room in
// the pinned mirror.  Entry b of the table is model b's, in the caller's order; slab w is sized for the largest model.
struct Plan {
  std::vector<Slot> slot;
  size_t table_doubles = 0;
  size_t up_doubles = 0;                  // what the host stages and uploads: [0, up_doubles)
  size_t down_off = 0, down_doubles = 0;  // what comes back
  size_t pinned_doubles = 0;              // the pinned mirror: [0, down_off + down_doubles)
  size_t slab_off = 0, slab_doubles = 0;  // W slabs of slab_doubles each from slab_off
  int W = 0;                              // workgroups of the launch; 0: the largest slab exceeds the budget (refused)
  size_t total_doubles = 0;
};

inline Plan plan(const std::vector<Shape> &sh, int compute_units) {
  Plan P;
  const size_t B = sh.size();
  P.slot.resize(B);
  P.table_doubles = round_up((B * sizeof(PolManyLargeModel) + 7) / 8, 32);
  size_t at = P.table_doubles;
  for (size_t b = 0; b < B; b++) {
    const size_t n = (size_t)sh[b].n, M = (size_t)sh[b].M;
    Slot &s = P.slot[b];
    auto take = [&at](size_t doubles) { const size_t r = at; at += doubles; return r; };
    const bool staged = sh[b].rows_con || sh[b].rows_var;
    s.A = staged ? take(sh[b].rows_con) : NONE;
    s.At = staged ? take(sh[b].rows_var) : NONE;
    s.q = sh[b].has_q ? take(n) : NONE;
    s.l = take(M);
    s.u = take(M);
    s.x = take(n);
    s.y = sh[b].has_y ? take(M) : NONE;
    const size_t slab = polish_many_large_slab_doubles(sh[b].n, sh[b].M);
    if (slab != (size_t)-1 && slab > P.slab_doubles) P.slab_doubles = slab;
  }
  P.up_doubles = at;
  at = round_up(at, 2);  // (16-byte alignment of the part that comes back)
  P.down_off = at;
  for (size_t b = 0; b < B; b++) {
    P.slot[b].out = at;
    at += polm_out_stride(sh[b].n, sh[b].M);
  }
  P.down_doubles = at - P.down_off;
  P.pinned_doubles = at;
  at = round_up(at, 32);  // (a slab starts on 256 bytes; a slab's size is a multiple of 32 doubles)
  P.slab_off = at;
  P.W = workgroups(B, compute_units, P.slab_doubles);
  at += (size_t)P.W * P.slab_doubles;
  P.total_doubles = at;
  return P;
}

}  // namespace polish_models_large
}  // namespace miosqp
