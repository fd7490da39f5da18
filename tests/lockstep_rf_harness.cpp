// Test-only C wrapper over miosqp_amd/csrc/lockstep_trees.hpp with the absorb split around round and fix (Tree::begin /
// heuristic / end): tests/test_lockstep_rf_cpu.py compiles it with g++ and replays recorded sequential solves with
// primal_heuristic = 1 through it.  The wave loop here is host_lockstep.inc's without the device: choose and two child
// slots per column (the store doubling when the free list runs short), begin for every column, the heuristic's outcome
// for the trees that fired, end for every column.
#include <cstdint>
#include <vector>

#include "../miosqp_amd/csrc/lockstep_trees.hpp"

using miosqp::lockstep::Begun;
using miosqp::lockstep::Record;
using miosqp::lockstep::Slots;
using miosqp::lockstep::Tree;
using miosqp::lockstep::Verdict;

namespace {
struct Harness {
  Slots slots;
  std::vector<Tree> trees;
  std::vector<int> cur, c0, c1;  // per tree: the node in flight and its children's slots (-1: none)
  std::vector<Verdict> verdict;  // ... and what begin decided about it
  int rf_every = 1, grown = 0;
};
}  // namespace

extern "C" {

// ntrees roots in slots 0 .. ntrees-1; upper0[t] >= 1.7e308: no incumbent
void *lrh_new(int ntrees, int capacity, const double *upper0, int rf_every) {
  Harness *h = new Harness();
  int cap = capacity;
  while (cap < ntrees) {
    cap *= 2;
    h->grown++;
  }
  h->slots.reset(cap);
  h->trees.assign((size_t)ntrees, Tree());
  h->cur.assign((size_t)ntrees, -1);
  h->c0.assign((size_t)ntrees, -1);
  h->c1.assign((size_t)ntrees, -1);
  h->verdict.assign((size_t)ntrees, Verdict{false, 0});
  h->rf_every = rf_every;
  for (int t = 0; t < ntrees; t++) h->trees[(size_t)t].start(h->slots, h->slots.take(), upper0[t]);
  return h;
}

void lrh_free(void *p) { delete static_cast<Harness *>(p); }

int lrh_can_continue(void *p, int t, int64_t max_iter_bb) {
  return static_cast<Harness *>(p)->trees[(size_t)t].can_continue(max_iter_bb) ? 1 : 0;
}

// choose_leaf of tree t: returns the index into its open list; the leaf leaves the list, two child slots are taken
int lrh_choose(void *p, int t, int rule) {
  Harness *h = static_cast<Harness *>(p);
  Tree &T = h->trees[(size_t)t];
  while (h->slots.free_count() < 2) {
    h->slots.grow(2 * h->slots.cap);
    h->grown++;
  }
  const int idx = (int)T.choose(h->slots, rule);
  h->cur[(size_t)t] = T.pop(h->slots, rule);
  h->c0[(size_t)t] = h->slots.take();
  h->c1[(size_t)t] = h->slots.take();
  return idx;
}

// bound_and_branch of tree t up to the heuristic: returns branch | incumbent << 1 | fire << 3
int lrh_begin(void *p, int t, int ok, int iter, double lower, int int_inf, int nextvar, int heur_feasible, double heur_obj) {
  Harness *h = static_cast<Harness *>(p);
  Record r;
  r.ok = ok != 0;
  r.iter = iter;
  r.lower = lower;
  r.int_inf = int_inf;
  r.nextvar = nextvar;
  r.heur_feasible = heur_feasible != 0;
  r.heur_obj = heur_obj;
  const Begun g = h->trees[(size_t)t].begin(h->slots, h->cur[(size_t)t], r, h->rf_every);
  h->verdict[(size_t)t] = g.v;
  return (g.v.branch ? 1 : 0) | (g.v.incumbent << 1) | ((g.fire ? 1 : 0) << 3);
}

// the outcome of the K candidates at the node in flight; returns whether the winner became the incumbent
int lrh_heuristic(void *p, int t, int K, int counted, double obj, int feasible, int64_t iters) {
  Harness *h = static_cast<Harness *>(p);
  return h->trees[(size_t)t].heuristic(h->slots, K, counted != 0, obj, feasible, iters) ? 1 : 0;
}

// the children enter the list (or their slots go back)
void lrh_end(void *p, int t) {
  Harness *h = static_cast<Harness *>(p);
  h->trees[(size_t)t].end(h->slots, h->cur[(size_t)t], h->c0[(size_t)t], h->c1[(size_t)t], h->verdict[(size_t)t]);
  h->cur[(size_t)t] = h->c0[(size_t)t] = h->c1[(size_t)t] = -1;
}

int lrh_open(void *p, int t) { return (int)static_cast<Harness *>(p)->trees[(size_t)t].open.size(); }
double lrh_upper(void *p, int t) { return static_cast<Harness *>(p)->trees[(size_t)t].upper; }
int64_t lrh_nodes(void *p, int t) { return static_cast<Harness *>(p)->trees[(size_t)t].nodes; }
int64_t lrh_iters(void *p, int t) { return static_cast<Harness *>(p)->trees[(size_t)t].iters; }
// which: 0 calls, 1 candidates, 2 feasible, 3 improved, 4 the candidates' iterations
int64_t lrh_rf(void *p, int t, int which) {
  const Tree &T = static_cast<Harness *>(p)->trees[(size_t)t];
  const int64_t v[5] = {T.rf_calls, T.rf_candidates, T.rf_feasible, T.rf_improved, T.rf_iters};
  return v[which];
}
int lrh_grown(void *p) { return static_cast<Harness *>(p)->grown; }
int lrh_cap(void *p) { return static_cast<Harness *>(p)->slots.cap; }
int lrh_free_slots(void *p) { return (int)static_cast<Harness *>(p)->slots.free_count(); }

}  // extern "C"
