// Round and fix inside the one-launch trees (k_tree_rf, k_tree_rf_m, k_tree_rf_r_m: kernels_tree_body.inc under TREE_RF):
// the decisions that need neither the device nor an engine -- when the heuristic fires, the value an integer row is
// fixed to, and the running pick among the candidates.  They restate Workspace.primal_heuristic, rf_roundings and the
// pick loop of Workspace.round_and_fix (miosqp_amd/bnb.py); k_rf_candidates / k_rf_pick (kernels_derived.inc) decide the
// same way for the batched form.  Plain C++: the kernels include it, and so does the stand-alone sanitized program
// tests/tree_rf_harness.cpp.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define TREE_RF_HD __host__ __device__ __forceinline__
#else
#define TREE_RF_HD inline
#endif

namespace miosqp {
namespace tree_rf {

constexpr int MAX_K = 32;  // rf_candidates at most (RF_MAX_K of the batched form)

// `counter` fractional nodes were about to branch before this one: the heuristic runs on every `every`-th of them, the
// first included
TREE_RF_HD bool fires(int counter, int every) { return counter % every == 0; }

// theta_k = (k + 1) / (K + 1) as one double division
TREE_RF_HD double theta(int k, int K) { return (double)(k + 1) / (double)(K + 1); }

// the value candidate k fixes an integer row to: x is the node's clamped, unscaled entry, lo / hi the node's own bounds
TREE_RF_HD double fixed_value(double x, double th, double lo, double hi) { return fmin(fmax(floor(x + th), lo), hi); }

// The running pick over k = 0 .. K-1 in order.  A candidate is feasible when it has an x and the worst margin of its
// rounded point against the ROOT bounds is <= 0 (a NaN margin is not); it counts when it is feasible and its objective
// is below `upper`; the lowest objective among those that count wins, ties go to the lowest k (strict comparison).
struct Pick {
  int best = -1, feasible = 0;
  double best_obj = 0.0;
  // true when candidate k is the best so far: its rounded point is then the one to keep
  TREE_RF_HD bool take(int k, bool has_x, double viol, double obj, double upper) {
    if (!has_x || !(viol <= 0.0)) return false;
    feasible++;
    if (obj < upper && (best < 0 || obj < best_obj)) {
      best = k;
      best_obj = obj;
      return true;
    }
    return false;
  }
};

}  // namespace tree_rf
}  // namespace miosqp
