// B trees of ONE model beyond one workgroup's product form in one launch (miosqp_qp_solve_trees_large, _rf, _sb): the host
// logic that needs neither an engine nor the device -- where the batch's arrays lie in the engine's arena, with every
// product in size_t and checked for overflow, and the arena against what the device can give.  Plain C++ (no HIP):
// engine.hip includes it, and so does the stand-alone sanitized program under tests/.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "tree_sb_logic.hpp"  // the size of a tree's work area under strong / reliability branching

namespace miosqp {
namespace trees_large {

constexpr int ERR_ARG = -1;        // MIOSQP_EARG
constexpr size_t OUT_DOUBLES = 6;  // one outcome record (TreeOut: 48 bytes; the kernel strides by the record itself)
constexpr size_t RF_DOUBLES = 4;   // one round-and-fix record (TreeRfOut: 32 bytes)
constexpr size_t SB_DOUBLES = 4;   // one strong-branching record (TreeSbOut: 32 bytes)

enum Variant { PLAIN = 0, RF = 1, SB = 2 };

// Offsets in doubles from the arena's base; every array holds B instances back to back, instance b at b x (its size).
// [ raw | qraw | upper | inc | out | rf | sb ] go up in ONE copy, [ inc | out | rf | sb ] come back in ONE copy; the
// scaled costs, the leaf store and the sb areas follow and never cross the bus.
struct Plan {
  size_t raw = 0;    // l | u | x0 | y0: 3 M + n per instance
  size_t qraw = 0;   // the raw cost: n
  size_t upper = 0;  // the incumbent's value: 1
  size_t inc = 0;    // the incumbent: n
  size_t out = 0;    // OUT_DOUBLES
  size_t rf = 0;     // RF_DOUBLES (variant RF; else empty, at the place of what follows)
  size_t sb = 0;     // SB_DOUBLES (variant SB; else empty)
  size_t q = 0;      // the scaled cost: n
  size_t lf_lo = 0, lf_hi = 0, lf_x = 0, lf_y = 0;  // the leaf store: leaf_cap x p, x p, x n, x M
  size_t sb_work = 0;  // tree_sb::work_doubles(p) (variant SB; else empty)
  size_t sb_pc = 0;    // leaf_cap x tree_sb::PC_DOUBLES (variant SB; else empty)
  size_t up_doubles = 0;                  // what the host stages and uploads: [0, up_doubles)
  size_t down_off = 0, down_doubles = 0;  // what comes back
  size_t total_doubles = 0;
};

// r = a * b, r = a + b: false when the result does not fit size_t
inline bool mul(size_t a, size_t b, size_t &r) { return !__builtin_mul_overflow(a, b, &r); }
inline bool add(size_t a, size_t b, size_t &r) { return !__builtin_add_overflow(a, b, &r); }

// The layout for B instances of a model with n variables, M rows (general + integer) and p integer variables, a leaf
// list of leaf_cap places.  0, or ERR_ARG with `err` naming B and leaf_cap when a size does not fit size_t (bytes
// included): nothing wraps.
inline int plan(int n_, int M_, int p_, int32_t B_, int32_t leaf_cap_, Variant v, Plan &P, std::string &err) {
  const std::string who = "solve_trees_large: ";
  if (n_ < 1 || M_ < 1 || p_ < 1 || B_ < 1 || leaf_cap_ < 2) {
    err = who + "n, M, n_int and B must be at least 1 and leaf_cap at least 2";
    return ERR_ARG;
  }
  const size_t n = (size_t)n_, M = (size_t)M_, p = (size_t)p_, B = (size_t)B_, cap = (size_t)leaf_cap_;
  P = Plan{};
  size_t at = 0;
  bool ok = true;
  // one array of B x (per x each) doubles at `at`, rounded up to 16 bytes behind it
  auto take = [&](size_t &off, size_t per, size_t each) {
    size_t one = 0, all = 0;
    off = at;
    ok = ok && mul(per, each, one) && mul(B, one, all) && add(at, all, at) && add(at, at & 1, at);
  };
  size_t blk = 0;
  ok = mul(3, M, blk) && add(blk, n, blk);
  take(P.raw, blk, 1);
  take(P.qraw, n, 1);
  take(P.upper, 1, 1);
  P.down_off = at;
  take(P.inc, n, 1);
  take(P.out, OUT_DOUBLES, 1);
  take(P.rf, v == RF ? RF_DOUBLES : 0, 1);
  take(P.sb, v == SB ? SB_DOUBLES : 0, 1);
  P.up_doubles = at;
  P.down_doubles = at - P.down_off;
  ok = ok && add(at, (32 - at % 32) % 32, at);
  take(P.q, n, 1);
  take(P.lf_lo, cap, p);
  take(P.lf_hi, cap, p);
  take(P.lf_x, cap, n);
  take(P.lf_y, cap, M);
  take(P.sb_work, v == SB ? tree_sb::work_doubles(p_) : 0, 1);
  take(P.sb_pc, v == SB ? cap : 0, (size_t)tree_sb::PC_DOUBLES);
  P.total_doubles = at;
  size_t bytes = 0;
  ok = ok && mul(at, sizeof(double), bytes) && add(bytes, 4096, bytes);
  if (!ok) {
    err = who + "the arrays of B = " + std::to_string(B_) + " instances with leaf_cap " + std::to_string(leaf_cap_) +
          " are beyond what an address can hold";
    P = Plan{};
    return ERR_ARG;
  }
  return 0;
}

// The arena against what the device can give (`limit_doubles`): 0, or ERR_ARG with `err` naming B and the bytes.
inline int check_room(const Plan &P, int32_t B, size_t limit_doubles, std::string &err) {
  if (P.total_doubles <= limit_doubles) return 0;
  err = "solve_trees_large: the arrays of B = " + std::to_string(B) + " instances (" + std::to_string(P.total_doubles * sizeof(double)) +
        " bytes) are beyond what the device can give (" + std::to_string(limit_doubles * sizeof(double)) +
        " bytes): fewer instances per call, or a smaller leaf_cap";
  return ERR_ARG;
}

}  // namespace trees_large
}  // namespace miosqp
