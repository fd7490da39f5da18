// Strong and reliability branching inside the one-launch trees (k_tree_sb, k_tree_sb_m, k_tree_sb_r_m:
// kernels_tree_body.inc under TREE_SB): the decisions that need neither the device nor an engine -- the fractional set
// and the candidates, the scores of the 2K children, the pseudo-costs with numpy's pairwise mean, the final pick, and
// what a child remembers of its branching.  They restate Workspace.select_branching, _most_fractional, sb_scores,
// record_gain and pseudo_costs (miosqp_amd/bnb.py) as lockstep::SbTree (lockstep_sb.hpp) restates them for the
// lock-step trees; here without std::vector, on arrays the caller owns (one tree's work area in device memory, laid
// out by `view`), so that thread 0 of a tree's workgroup can run them.  Plain C++: the kernels include it, and so does
// the stand-alone sanitized program tests/tree_sb_harness.cpp, which runs it side by side with SbTree.
#pragma once
#include <cmath>
#include <cstddef>

#if defined(__HIPCC__)
#define TREE_SB_HD __host__ __device__ inline
#else
#define TREE_SB_HD inline
#endif

namespace miosqp {
namespace tree_sb {

constexpr int MAX_K = 32;        // sb_candidates at most (SB_MAX_K of the batched form)
constexpr int PC_DOUBLES = 4;    // Node.pc of one leaf-store place: parent lower, distance f, position, side (-1: none)
constexpr int SUM_DEPTH = 16;    // splits of the pairwise sum: 128 * 2^16 entries and more

struct Par {
  int rule;         // 1: strong branching, 2: reliability branching
  int K;            // sb_candidates
  int reliability;  // sb_reliability
  double eps;       // sb_eps
  double eps_int;   // eps_int_feas
};

// np.add.reduce over a contiguous float64 array (lockstep::np_pairwise_sum) without recursion: blocks of at most 128
// with eight accumulators, halves split at a multiple of 8 and added left + right
TREE_SB_HD double pairwise_block(const double *a, size_t n) {
  if (n < 8) {
    double res = 0.0;
    for (size_t i = 0; i < n; i++) res += a[i];
    return res;
  }
  double r[8];
  for (int j = 0; j < 8; j++) r[j] = a[j];
  size_t i = 8;
  for (; i < n - (n % 8); i += 8)
    for (int j = 0; j < 8; j++) r[j] += a[i + (size_t)j];
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; i++) res += a[i];
  return res;
}

TREE_SB_HD double pairwise_sum(const double *a, size_t n) {
  if (n <= 128) return pairwise_block(a, n);
  const double *fa[SUM_DEPTH];
  size_t fn[SUM_DEPTH];
  double fl[SUM_DEPTH];
  int fs[SUM_DEPTH];
  int top = 0;
  fa[0] = a; fn[0] = n; fl[0] = 0.0; fs[0] = 0;
  double ret = 0.0;
  while (top >= 0) {
    if (fn[top] <= 128 || top + 1 >= SUM_DEPTH) {  // (the last frame takes what is left as one block: beyond 128 * 2^15 entries only)
      ret = pairwise_block(fa[top], fn[top]);
      top--;
      continue;
    }
    size_t n2 = fn[top] / 2;
    n2 -= n2 % 8;
    if (fs[top] == 0) {
      fs[top] = 1;
      fa[top + 1] = fa[top]; fn[top + 1] = n2; fl[top + 1] = 0.0; fs[top + 1] = 0;
      top++;
    } else if (fs[top] == 1) {
      fl[top] = ret;
      fs[top] = 2;
      fa[top + 1] = fa[top] + n2; fn[top + 1] = fn[top] - n2; fl[top + 1] = 0.0; fs[top + 1] = 0;
      top++;
    } else {
      ret = fl[top] + ret;
      top--;
    }
  }
  return ret;
}

// One tree's work area: p integer positions.  pc_sum / pc_cnt are Workspace.pc_sum / pc_cnt as [2][p] (down, up); the
// rest is the asking node's: x at the integer positions, the fractional positions (ascending), marks, the candidates
// (ascending), their scores, and the 2K children as the solves leave them (K down, then K up).
struct View {
  int p;
  double *pc_sum;      // [2 p]
  long long *pc_cnt;   // [2 p]
  double *psi;         // [2 p]
  double *means;       // [p]   (by position once pseudo_costs is done)
  double *x;           // [p]
  double *score;       // [MAX_K]
  double *ch_lower;    // [2 MAX_K]
  int *frac;           // [p]
  int *mark;           // [p]
  int *cand;           // [MAX_K]
  int *ch_has;         // [2 MAX_K]
  int *ch_iter;        // [2 MAX_K]
  int *count;          // [2]: fractional positions, candidates
};

// doubles of a work area (even, so that areas laid back to back stay 16-byte aligned)
TREE_SB_HD size_t work_doubles(int p) {
  const size_t P = (size_t)p;
  const size_t d = 8 * P + 3 * (size_t)MAX_K, ints = 2 * P + 5 * (size_t)MAX_K + 2;
  const size_t all = d + (ints + 1) / 2;
  return (all + 1) / 2 * 2;
}

TREE_SB_HD View view(double *w, int p) {
  const size_t P = (size_t)p;
  View v;
  v.p = p;
  v.pc_sum = w;
  v.pc_cnt = reinterpret_cast<long long *>(w + 2 * P);
  v.psi = w + 4 * P;
  v.means = w + 6 * P;
  v.x = w + 7 * P;
  v.score = w + 8 * P;
  v.ch_lower = v.score + MAX_K;
  int *iw = reinterpret_cast<int *>(v.ch_lower + 2 * MAX_K);
  v.frac = iw;
  v.mark = iw + P;
  v.cand = iw + 2 * P;
  v.ch_has = v.cand + MAX_K;
  v.ch_iter = v.ch_has + 2 * MAX_K;
  v.count = v.ch_iter + 2 * MAX_K;
  return v;
}

// a tree starts: no observations
TREE_SB_HD void start(const View &v) {
  for (int k = 0; k < 2 * v.p; k++) {
    v.pc_sum[k] = 0.0;
    v.pc_cnt[k] = 0;
  }
  v.count[0] = v.count[1] = 0;
}

// Workspace.record_gain
TREE_SB_HD void record_gain(const View &v, int pos, int side, double delta, double f) {
  const size_t at = (size_t)side * (size_t)v.p + (size_t)pos;
  v.pc_sum[at] += (delta > 0.0 ? delta : 0.0) / f;
  v.pc_cnt[at] += 1;
}

// Workspace.pseudo_costs into psi [2][p]
TREE_SB_HD void pseudo_costs(const View &v) {
  const int p = v.p;
  for (int side = 0; side < 2; side++) {
    const size_t o = (size_t)side * (size_t)p;
    size_t have = 0;
    for (int k = 0; k < p; k++)
      if (v.pc_cnt[o + (size_t)k] > 0) v.means[have++] = v.pc_sum[o + (size_t)k] / (double)v.pc_cnt[o + (size_t)k];
    if (have == 0) {
      for (int k = 0; k < p; k++) v.psi[o + (size_t)k] = 1.0;
      continue;
    }
    const double rest = pairwise_sum(v.means, have) / (double)have;
    size_t j = 0;
    for (int k = 0; k < p; k++) v.psi[o + (size_t)k] = v.pc_cnt[o + (size_t)k] > 0 ? v.means[j++] : rest;
  }
}

TREE_SB_HD double fraction(double x) { return fabs(x - rint(x)); }

// Workspace._most_fractional over the positions with mark 1: the `count` largest fractions, ties to the lower position,
// ascending, into cand.  One pass per pick, the first maximum each time -- what a stable sort by falling fraction keeps.
TREE_SB_HD void most_fractional(const View &v, int count) {
  const int p = v.p;
  for (int t = 0; t < count; t++) {
    int best = -1;
    double bf = -1.0;
    for (int k = 0; k < p; k++)
      if (v.mark[k] == 1) {
        const double f = fraction(v.x[k]);
        if (f > bf) {
          bf = f;
          best = k;
        }
      }
    if (best < 0) break;
    v.mark[best] = 2;
  }
  int K = 0;
  for (int k = 0; k < p; k++)
    if (v.mark[k] == 2) v.cand[K++] = k;
  v.count[1] = K;
}

// the end of select_branching under rule 2: every fractional position scored, by its strong-branching score where it
// has one, by pseudo-costs otherwise; the first maximum in ascending position order
TREE_SB_HD int pick(const View &v, const Par &sp) {
  pseudo_costs(v);
  const int p = v.p, F = v.count[0], K = v.count[1];
  double *by_pos = v.means;  // (free again after pseudo_costs)
  for (int k = 0; k < p; k++) v.mark[k] = 0;
  for (int j = 0; j < K; j++) {
    v.mark[v.cand[j]] = 1;
    by_pos[v.cand[j]] = v.score[j];
  }
  int best = -1;
  double best_s = -HUGE_VAL;
  for (int i = 0; i < F; i++) {
    const int c = v.frac[i];
    double s;
    if (v.mark[c]) s = by_pos[c];
    else {
      const double xv = v.x[c];
      const double sd = v.psi[c] * (xv - floor(xv)), su = v.psi[(size_t)p + (size_t)c] * (ceil(xv) - xv);
      s = (sd > sp.eps ? sd : sp.eps) * (su > sp.eps ? su : sp.eps);
    }
    if (s > best_s) {
      best = c;
      best_s = s;
    }
  }
  return best;
}

// select_branching up to strong_branch on v.x.  Returns the position when nothing has to be solved (rule 1: one
// fractional position; rule 2: no unreliable one), -1 when the children of cand[0 .. count[1]) have to be solved first
// (decide), -2 when no position is fractional (the caller's error).
TREE_SB_HD int ask(const View &v, const Par &sp) {
  const int p = v.p;
  int F = 0;
  for (int k = 0; k < p; k++)
    if (fraction(v.x[k]) > sp.eps_int) v.frac[F++] = k;
  v.count[0] = F;
  v.count[1] = 0;
  if (F == 0) return -2;
  for (int k = 0; k < p; k++) v.mark[k] = 0;
  if (sp.rule == 1) {
    if (F == 1) return v.frac[0];
    for (int i = 0; i < F; i++) v.mark[v.frac[i]] = 1;
    most_fractional(v, sp.K);
    return -1;
  }
  int U = 0;
  for (int i = 0; i < F; i++) {
    const int c = v.frac[i];
    const long long a = v.pc_cnt[c], b = v.pc_cnt[(size_t)p + (size_t)c];
    if ((a < b ? a : b) < (long long)sp.reliability) {
      v.mark[c] = 1;
      U++;
    }
  }
  if (U == 0) return pick(v, sp);
  most_fractional(v, sp.K);
  return -1;
}

// sb_scores for one candidate from its two children
TREE_SB_HD double sb_score(bool dn_has, double dn_lower, bool up_has, double up_lower, double node_lower, double eps) {
  double gd = dn_has ? dn_lower - node_lower : 1e30;
  double gu = up_has ? up_lower - node_lower : 1e30;
  gd = gd > 0.0 ? gd : 0.0;
  gu = gu > 0.0 ? gu : 0.0;
  return (gd > eps ? gd : eps) * (gu > eps ? gu : eps);
}

// strong_branch's outcome for cand (ch_*: K down children, then K up children): the scores, under rule 2 the
// observations in candidate order, down then up, and the position.  *iters: the children's iterations summed.
TREE_SB_HD int decide(const View &v, const Par &sp, double node_lower, int *iters) {
  const int K = v.count[1];
  int it = 0;
  for (int b = 0; b < 2 * K; b++) it += v.ch_iter[b];
  *iters = it;
  int best = 0;
  for (int j = 0; j < K; j++) {
    v.score[j] = sb_score(v.ch_has[j] != 0, v.ch_lower[j], v.ch_has[K + j] != 0, v.ch_lower[K + j], node_lower, sp.eps);
    if (v.score[j] > v.score[best]) best = j;
  }
  if (sp.rule == 1) return v.cand[best];
  for (int j = 0; j < K; j++) {
    const int c = v.cand[j];
    const double xv = v.x[c];
    if (v.ch_has[j]) record_gain(v, c, 0, v.ch_lower[j] - node_lower, xv - floor(xv));
    if (v.ch_has[K + j]) record_gain(v, c, 1, v.ch_lower[K + j] - node_lower, ceil(xv) - xv);
  }
  return pick(v, sp);
}

// branch_children: under rule 2 each child's place remembers what its own solve will tell the pseudo-costs; under rule 1
// a reused place forgets what it held.  pc: Node.pc of every leaf-store place, PC_DOUBLES each.
TREE_SB_HD void branched(const Par &sp, double *pc, int c0, int c1, int pos, double xv, double node_lower) {
  const double f[2] = {xv - floor(xv), ceil(xv) - xv};
  const int c[2] = {c0, c1};
  for (int side = 0; side < 2; side++) {
    double *r = pc + (size_t)c[side] * PC_DOUBLES;
    r[0] = node_lower;
    r[1] = f[side];
    r[2] = (double)pos;
    r[3] = sp.rule == 2 ? (double)side : -1.0;
  }
}

// the top of bound_and_branch: the solve of a node made by a branching is an observation when it has an x
TREE_SB_HD void node_solved(const View &v, const double *pc, int slot, bool ok, double lower) {
  const double *r = pc + (size_t)slot * PC_DOUBLES;
  if (r[3] >= 0.0 && ok) record_gain(v, (int)r[2], (int)r[3], lower - r[0], r[1]);
}

}  // namespace tree_sb
}  // namespace miosqp
