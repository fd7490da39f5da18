// Test-only C wrapper over miosqp_amd/csrc/lockstep_sb.hpp beside lockstep_trees.hpp: tests/test_lockstep_sb_cpu.py
// compiles it with g++ and replays recorded sequential solves with branching_rule 1 and 2 through it.  The wave loop
// here is host_lockstep_sb.inc's without the device: choose and two child slots per column (the store doubling when the
// free list runs short), node_solved + begin for every column, ask / decide for the nodes that branch, branched + end
// for every column.
#include <cstdint>
#include <vector>

#include "../miosqp_amd/csrc/lockstep_sb.hpp"

using miosqp::lockstep::Record;
using miosqp::lockstep::SbChild;
using miosqp::lockstep::SbParams;
using miosqp::lockstep::SbSlots;
using miosqp::lockstep::SbTree;
using miosqp::lockstep::Slots;
using miosqp::lockstep::Tree;
using miosqp::lockstep::Verdict;

namespace {
struct Harness {
  Slots slots;
  SbSlots sbslots;
  std::vector<Tree> trees;
  std::vector<SbTree> sb;
  std::vector<int> cur, c0, c1;      // per tree: the node in flight and its children's slots (-1: none)
  std::vector<Verdict> verdict;      // ... what begin decided about it,
  std::vector<double> lower;         // ... its lower value
  std::vector<std::vector<double>> x;  // ... and its x at the integer positions
  SbParams sp{1, 8, 4, 1e-6, 1e-6};
  int p = 0, grown = 0;
};
}  // namespace

extern "C" {

// ntrees roots in slots 0 .. ntrees-1; upper0[t] >= 1.7e308: no incumbent
void *lbh_new(int ntrees, int capacity, const double *upper0, int p, int rule, int K, int reliability, double eps, double eps_int) {
  Harness *h = new Harness();
  int cap = capacity;
  while (cap < ntrees) {
    cap *= 2;
    h->grown++;
  }
  h->slots.reset(cap);
  h->sbslots.reset(cap);
  h->trees.assign((size_t)ntrees, Tree());
  h->sb.assign((size_t)ntrees, SbTree());
  h->cur.assign((size_t)ntrees, -1);
  h->c0.assign((size_t)ntrees, -1);
  h->c1.assign((size_t)ntrees, -1);
  h->verdict.assign((size_t)ntrees, Verdict{false, 0});
  h->lower.assign((size_t)ntrees, 0.0);
  h->x.assign((size_t)ntrees, std::vector<double>((size_t)p, 0.0));
  h->sp = SbParams{rule, K, reliability, eps, eps_int};
  h->p = p;
  for (int t = 0; t < ntrees; t++) {
    h->trees[(size_t)t].start(h->slots, h->slots.take(), upper0[t]);
    h->sb[(size_t)t].start(p);
  }
  return h;
}

void lbh_free(void *p) { delete static_cast<Harness *>(p); }

int lbh_can_continue(void *p, int t, int64_t max_iter_bb) {
  return static_cast<Harness *>(p)->trees[(size_t)t].can_continue(max_iter_bb) ? 1 : 0;
}

// choose_leaf of tree t: returns the index into its open list; the leaf leaves the list, two child slots are taken
int lbh_choose(void *p, int t, int rule) {
  Harness *h = static_cast<Harness *>(p);
  Tree &T = h->trees[(size_t)t];
  while (h->slots.free_count() < 2) {
    h->slots.grow(2 * h->slots.cap);
    h->sbslots.grow(h->slots.cap);
    h->grown++;
  }
  const int idx = (int)T.choose(h->slots, rule);
  h->cur[(size_t)t] = T.pop(h->slots, rule);
  h->c0[(size_t)t] = h->slots.take();
  h->c1[(size_t)t] = h->slots.take();
  return idx;
}

// bound_and_branch of tree t up to the branching: returns branch | incumbent << 1
int lbh_begin(void *p, int t, int ok, int iter, double lower, int int_inf, int nextvar, int heur_feasible, double heur_obj) {
  Harness *h = static_cast<Harness *>(p);
  Record r;
  r.ok = ok != 0;
  r.iter = iter;
  r.lower = lower;
  r.int_inf = int_inf;
  r.nextvar = nextvar;
  r.heur_feasible = heur_feasible != 0;
  r.heur_obj = heur_obj;
  h->sb[(size_t)t].node_solved(h->sbslots, h->cur[(size_t)t], r.ok, r.lower);
  const Verdict v = h->trees[(size_t)t].begin(h->slots, h->cur[(size_t)t], r, 0).v;
  h->verdict[(size_t)t] = v;
  h->lower[(size_t)t] = lower;
  return (v.branch ? 1 : 0) | (v.incumbent << 1);
}

// select_branching up to strong_branch on the node's x at the integer positions: the position, -1 (candidates: lbh_cand) or -2
int lbh_ask(void *p, int t, const double *x) {
  Harness *h = static_cast<Harness *>(p);
  h->x[(size_t)t].assign(x, x + h->p);
  return h->sb[(size_t)t].ask(h->sp, h->x[(size_t)t].data());
}

int lbh_ncand(void *p, int t) { return (int)static_cast<Harness *>(p)->sb[(size_t)t].cand.size(); }
int lbh_cand(void *p, int t, int j) { return static_cast<Harness *>(p)->sb[(size_t)t].cand[(size_t)j]; }

// the 2K children's outcome (K down, then K up): returns the position; *best: the argmax of the scores
int lbh_decide(void *p, int t, const int *has_x, const int *iter, const double *lower, int *best) {
  Harness *h = static_cast<Harness *>(p);
  SbTree &S = h->sb[(size_t)t];
  const int K = (int)S.cand.size();
  std::vector<SbChild> ch((size_t)(2 * K));
  for (int b = 0; b < 2 * K; b++) ch[(size_t)b] = SbChild{has_x[b] != 0, iter[b], lower[b]};
  return S.decide(h->sp, h->x[(size_t)t].data(), h->lower[(size_t)t], ch.data(), best);
}

// the children on position `pos` enter the list (or their slots go back)
void lbh_end(void *p, int t, int pos) {
  Harness *h = static_cast<Harness *>(p);
  const size_t k = (size_t)t;
  if (h->verdict[k].branch)
    h->sb[k].branched(h->sp, h->sbslots, h->c0[k], h->c1[k], pos, h->x[k].data(), h->lower[k]);
  h->trees[k].end(h->slots, h->cur[k], h->c0[k], h->c1[k], h->verdict[k]);
  h->cur[k] = h->c0[k] = h->c1[k] = -1;
}

int lbh_open(void *p, int t) { return (int)static_cast<Harness *>(p)->trees[(size_t)t].open.size(); }
int lbh_open_depth(void *p, int t, int i) {
  Harness *h = static_cast<Harness *>(p);
  return h->slots.depth[(size_t)h->trees[(size_t)t].open[(size_t)i]];
}
double lbh_open_lower(void *p, int t, int i) {
  Harness *h = static_cast<Harness *>(p);
  return h->slots.lower[(size_t)h->trees[(size_t)t].open[(size_t)i]];
}
double lbh_upper(void *p, int t) { return static_cast<Harness *>(p)->trees[(size_t)t].upper; }
int64_t lbh_nodes(void *p, int t) { return static_cast<Harness *>(p)->trees[(size_t)t].nodes; }
int64_t lbh_iters(void *p, int t) { return static_cast<Harness *>(p)->trees[(size_t)t].iters; }
// which: 0 calls, 1 children, 2 the children's iterations
int64_t lbh_sb(void *p, int t, int which) {
  const SbTree &S = static_cast<Harness *>(p)->sb[(size_t)t];
  const int64_t v[3] = {S.calls, S.children, S.iters};
  return v[which];
}
// the tree's tables, [2][p] each
void lbh_pc(void *p, int t, double *sum, int64_t *cnt) {
  const SbTree &S = static_cast<Harness *>(p)->sb[(size_t)t];
  for (size_t k = 0; k < S.pc_sum.size(); k++) {
    sum[k] = S.pc_sum[k];
    cnt[k] = S.pc_cnt[k];
  }
}
int lbh_grown(void *p) { return static_cast<Harness *>(p)->grown; }
int lbh_cap(void *p) { return static_cast<Harness *>(p)->slots.cap; }
int lbh_free_slots(void *p) { return (int)static_cast<Harness *>(p)->slots.free_count(); }

// Workspace.pseudo_costs on tables handed in: psi [2][p]
void lbh_pseudo_costs(int p, const double *sum, const int64_t *cnt, double *psi) {
  SbTree S;
  S.start(p);
  for (int k = 0; k < 2 * p; k++) {
    S.pc_sum[(size_t)k] = sum[k];
    S.pc_cnt[(size_t)k] = cnt[k];
  }
  S.pseudo_costs();
  for (int k = 0; k < 2 * p; k++) psi[k] = S.psi[(size_t)k];
}

}  // extern "C"
