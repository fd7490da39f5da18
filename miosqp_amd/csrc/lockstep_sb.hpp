// Strong and reliability branching in the lock-step trees (host_lockstep_sb.inc drives it; tests/lockstep_sb_harness.cpp
// replays recorded trees through it): plain C++17, no HIP include, compiles with g++ alone.
//
// It restates, per tree, the branching decision of the Python mirror (miosqp_amd/bnb.py) under branching_rule 1 and 2:
// Workspace.select_branching with _most_fractional, the bookkeeping of record_gain / pseudo_costs (numpy's summation
// order for np.mean included), the scores of sb_scores, and what branch_children leaves with the two children for
// their own solves (Node.pc, read back at the top of bound_and_branch).  Tree (lockstep_trees.hpp) is used as it is: a
// node whose Tree::begin says `branch` asks here for its position between begin and end.
//
//   node_solved   the first lines of bound_and_branch: a child's own solve is an observation (rule 2)
//   ask           the fractional set and the candidates; a position when nothing has to be solved
//   decide        the 2K children's outcome -> observations (rule 2), scores, the position
//   branched      the two children remember the branching (rule 2)
#ifndef MIOSQP_LOCKSTEP_SB_HPP
#define MIOSQP_LOCKSTEP_SB_HPP

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

#include "lockstep_trees.hpp"

namespace miosqp {
namespace lockstep {

struct SbParams {
  int rule;         // 1: strong branching, 2: reliability branching
  int K;            // sb_candidates
  int reliability;  // sb_reliability
  double eps;       // sb_eps
  double eps_int;   // eps_int_feas
};

// a strong-branching child as the batch leaves it
struct SbChild {
  bool has_x;    // OSQP_SOLVED or OSQP_MAX_ITER_REACHED
  int iter;
  double lower;  // objective at the clamped x
};

// np.add.reduce over a contiguous float64 array: numpy's pairwise summation (blocks of 128, eight accumulators)
inline double np_pairwise_sum(const double *a, size_t n) {
  if (n < 8) {
    double res = 0.0;
    for (size_t i = 0; i < n; i++) res += a[i];
    return res;
  }
  if (n <= 128) {
    double r[8];
    for (int j = 0; j < 8; j++) r[j] = a[j];
    size_t i = 8;
    for (; i < n - (n % 8); i += 8)
      for (int j = 0; j < 8; j++) r[j] += a[i + (size_t)j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; i++) res += a[i];
    return res;
  }
  size_t n2 = n / 2;
  n2 -= n2 % 8;
  return np_pairwise_sum(a, n2) + np_pairwise_sum(a + n2, n - n2);
}

inline double np_mean(const double *a, size_t n) { return np_pairwise_sum(a, n) / (double)n; }

// Node.pc per slot: (parent lower, position, direction 0 down / 1 up, distance f) of the branching that made the node
struct SbSlots {
  std::vector<char> has;
  std::vector<int> pos, side;
  std::vector<double> lp, f;
  void reset(int cap) {
    const size_t c = (size_t)cap;
    has.assign(c, 0); pos.assign(c, 0); side.assign(c, 0); lp.assign(c, 0.0); f.assign(c, 0.0);
  }
  void grow(int ncap) {
    const size_t c = (size_t)ncap;
    has.resize(c, 0); pos.resize(c, 0); side.resize(c, 0); lp.resize(c, 0.0); f.resize(c, 0.0);
  }
};

struct SbTree {
  int p = 0;                    // integer positions
  std::vector<double> pc_sum;   // [2][p]: sums of gains per unit distance (Workspace.pc_sum)
  std::vector<int64_t> pc_cnt;  // [2][p]: observations (Workspace.pc_cnt)
  int64_t calls = 0, children = 0, iters = 0;  // Workspace.sb_stats
  // the node that is asking: its fractional positions, its candidates (both ascending)
  std::vector<int> frac, cand;
  std::vector<double> psi, means, score;
  std::vector<char> scored;

  void start(int n_int) {
    p = n_int;
    pc_sum.assign(2 * (size_t)p, 0.0);
    pc_cnt.assign(2 * (size_t)p, 0);
    calls = children = iters = 0;
    frac.clear();
    cand.clear();
  }

  // Workspace.record_gain
  void record_gain(int pos, int side, double delta, double f) {
    pc_sum[(size_t)side * (size_t)p + (size_t)pos] += (delta > 0.0 ? delta : 0.0) / f;
    pc_cnt[(size_t)side * (size_t)p + (size_t)pos] += 1;
  }

  // Workspace.pseudo_costs into psi [2][p]
  void pseudo_costs() {
    psi.assign(2 * (size_t)p, 1.0);
    for (int side = 0; side < 2; side++) {
      const size_t o = (size_t)side * (size_t)p;
      means.clear();
      for (int k = 0; k < p; k++)
        if (pc_cnt[o + (size_t)k] > 0) means.push_back(pc_sum[o + (size_t)k] / (double)pc_cnt[o + (size_t)k]);
      if (means.empty()) continue;
      const double rest = np_mean(means.data(), means.size());
      size_t j = 0;
      for (int k = 0; k < p; k++) psi[o + (size_t)k] = pc_cnt[o + (size_t)k] > 0 ? means[j++] : rest;
    }
  }

  // the top of bound_and_branch: the solve of a node made by a branching is an observation when it has an x
  void node_solved(const SbSlots &P, int s, bool ok, double lower) {
    if (P.has[(size_t)s] && ok) record_gain(P.pos[(size_t)s], P.side[(size_t)s], lower - P.lp[(size_t)s], P.f[(size_t)s]);
  }

  // Workspace._most_fractional: `count` positions of `from` with the largest |x - round(x)|, ties to the lower position,
  // ascending, into cand
  void most_fractional(const std::vector<int> &from, int count, const double *x) {
    cand = from;  // ascending
    std::stable_sort(cand.begin(), cand.end(), [x](int a, int b) {
      return std::fabs(x[a] - std::nearbyint(x[a])) > std::fabs(x[b] - std::nearbyint(x[b]));
    });
    if ((int)cand.size() > count) cand.resize((size_t)count);
    std::sort(cand.begin(), cand.end());
  }

  // select_branching up to strong_branch on the node's x at the integer positions (x[0 .. p-1]).  Returns the position when
  // nothing has to be solved (rule 1: one fractional position; rule 2: no unreliable one), -1 when the children of
  // `cand` have to be solved first (decide), -2 when no position is fractional (the caller's error).
  int ask(const SbParams &sp, const double *x) {
    frac.clear();
    cand.clear();
    for (int k = 0; k < p; k++)
      if (std::fabs(x[k] - std::nearbyint(x[k])) > sp.eps_int) frac.push_back(k);
    if (frac.empty()) return -2;
    if (sp.rule == 1) {
      if (frac.size() == 1) return frac[0];
      most_fractional(frac, sp.K, x);
      return -1;
    }
    std::vector<int> unrel;
    for (int c : frac)
      if (std::min(pc_cnt[(size_t)c], pc_cnt[(size_t)p + (size_t)c]) < (int64_t)sp.reliability) unrel.push_back(c);
    if (unrel.empty()) return pick(sp, x);
    most_fractional(unrel, sp.K, x);
    return -1;
  }

  // sb_scores for candidate j of K from its two children
  static double sb_score(const SbChild &dn, const SbChild &up, double node_lower, double eps) {
    double gd = dn.has_x ? dn.lower - node_lower : 1e30;
    double gu = up.has_x ? up.lower - node_lower : 1e30;
    gd = gd > 0.0 ? gd : 0.0;
    gu = gu > 0.0 ? gu : 0.0;
    return (gd > eps ? gd : eps) * (gu > eps ? gu : eps);
  }

  // strong_branch's outcome for `cand` (ch: K down children, then K up children): the counters, under rule 2 the
  // observations in candidate order, down then up, and the position.  *chosen_cand: the argmax of the scores (index
  // into cand), what strong_branch reports.
  int decide(const SbParams &sp, const double *x, double node_lower, const SbChild *ch, int *chosen_cand = nullptr) {
    const int K = (int)cand.size();
    calls++;
    children += 2 * K;
    for (int b = 0; b < 2 * K; b++) iters += ch[b].iter;
    score.assign((size_t)K, 0.0);
    int best = 0;
    for (int j = 0; j < K; j++) {
      score[(size_t)j] = sb_score(ch[j], ch[K + j], node_lower, sp.eps);
      if (score[(size_t)j] > score[(size_t)best]) best = j;
    }
    if (chosen_cand) *chosen_cand = best;
    if (sp.rule == 1) return cand[(size_t)best];
    for (int j = 0; j < K; j++) {
      const int c = cand[(size_t)j];
      const double v = x[c];
      if (ch[j].has_x) record_gain(c, 0, ch[j].lower - node_lower, v - std::floor(v));
      if (ch[K + j].has_x) record_gain(c, 1, ch[K + j].lower - node_lower, std::ceil(v) - v);
    }
    return pick(sp, x);
  }

  // the end of select_branching under rule 2: every fractional position scored, by its strong-branching score where
  // it has one (cand / score), by pseudo-costs otherwise; the first maximum in ascending position order
  int pick(const SbParams &sp, const double *x) {
    pseudo_costs();
    scored.assign((size_t)p, 0);
    std::vector<double> &by_pos = means;  // (free again after pseudo_costs)
    by_pos.assign((size_t)p, 0.0);
    for (size_t j = 0; j < cand.size(); j++) {
      scored[(size_t)cand[j]] = 1;
      by_pos[(size_t)cand[j]] = score[j];
    }
    int best = -1;
    double best_s = -std::numeric_limits<double>::infinity();
    for (int c : frac) {
      double s;
      if (scored[(size_t)c]) s = by_pos[(size_t)c];
      else {
        const double v = x[c];
        const double sd = psi[(size_t)c] * (v - std::floor(v)), su = psi[(size_t)p + (size_t)c] * (std::ceil(v) - v);
        s = (sd > sp.eps ? sd : sp.eps) * (su > sp.eps ? su : sp.eps);
      }
      if (s > best_s) {
        best = c;
        best_s = s;
      }
    }
    return best;
  }

  // branch_children: under rule 2 each child remembers what its own solve will tell the pseudo-costs; under rule 1 a
  // reused slot forgets what it held
  void branched(const SbParams &sp, SbSlots &P, int c0, int c1, int pos, const double *x, double node_lower) const {
    const double v = x[pos];
    const double f[2] = {v - std::floor(v), std::ceil(v) - v};
    const int c[2] = {c0, c1};
    for (int side = 0; side < 2; side++) {
      const size_t s = (size_t)c[side];
      P.has[s] = sp.rule == 2;
      P.pos[s] = pos;
      P.side[s] = side;
      P.lp[s] = node_lower;
      P.f[s] = f[side];
    }
  }
};

}  // namespace lockstep
}  // namespace miosqp

#endif
