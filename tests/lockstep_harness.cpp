// Test-only C wrapper over miosqp_amd/csrc/lockstep_trees.hpp (the host logic of the lock-step trees driven in the
// library): tests/test_lockstep_trees_cpu.py compiles it with g++ and replays recorded trees through it.  The wave
// loop here is host_lockstep.inc's without the device: choose, two child slots per column (the store doubling when the
// free list runs short), absorb.
#include <cstdint>
#include <vector>

#include "../miosqp_amd/csrc/lockstep_trees.hpp"

using miosqp::lockstep::Record;
using miosqp::lockstep::Slots;
using miosqp::lockstep::Tree;
using miosqp::lockstep::Verdict;

namespace {
struct Harness {
  Slots slots;
  std::vector<Tree> trees;
  std::vector<int> cur, c0, c1;  // per tree: the node in flight and its children's slots (-1: none)
  int grown = 0;
};
}  // namespace

extern "C" {

// ntrees roots in slots 0 .. ntrees-1; upper0[t] >= 1.7e308: no incumbent
void *lsh_new(int ntrees, int capacity, const double *upper0) {
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
  for (int t = 0; t < ntrees; t++) h->trees[(size_t)t].start(h->slots, h->slots.take(), upper0[t]);
  return h;
}

void lsh_free(void *p) { delete static_cast<Harness *>(p); }

int lsh_can_continue(void *p, int t, int64_t max_iter_bb) {
  return static_cast<Harness *>(p)->trees[(size_t)t].can_continue(max_iter_bb) ? 1 : 0;
}

// choose_leaf of tree t: returns the index into its open list; the leaf leaves the list, two child slots are taken
int lsh_choose(void *p, int t, int rule) {
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

// bound_and_branch of tree t on the record of the node in flight: returns branch | incumbent << 1
int lsh_absorb(void *p, int t, int ok, int iter, double lower, int int_inf, int nextvar, int heur_feasible, double heur_obj) {
  Harness *h = static_cast<Harness *>(p);
  Record r;
  r.ok = ok != 0;
  r.iter = iter;
  r.lower = lower;
  r.int_inf = int_inf;
  r.nextvar = nextvar;
  r.heur_feasible = heur_feasible != 0;
  r.heur_obj = heur_obj;
  const Verdict v = h->trees[(size_t)t].absorb(h->slots, h->cur[(size_t)t], h->c0[(size_t)t], h->c1[(size_t)t], r);
  h->cur[(size_t)t] = h->c0[(size_t)t] = h->c1[(size_t)t] = -1;
  return (v.branch ? 1 : 0) | (v.incumbent << 1);
}

int lsh_open(void *p, int t) { return (int)static_cast<Harness *>(p)->trees[(size_t)t].open.size(); }
double lsh_upper(void *p, int t) { return static_cast<Harness *>(p)->trees[(size_t)t].upper; }
int64_t lsh_nodes(void *p, int t) { return static_cast<Harness *>(p)->trees[(size_t)t].nodes; }
int64_t lsh_iters(void *p, int t) { return static_cast<Harness *>(p)->trees[(size_t)t].iters; }
int lsh_found(void *p, int t) { return static_cast<Harness *>(p)->trees[(size_t)t].found ? 1 : 0; }
int lsh_grown(void *p) { return static_cast<Harness *>(p)->grown; }
int lsh_cap(void *p) { return static_cast<Harness *>(p)->slots.cap; }
int lsh_free_slots(void *p) { return (int)static_cast<Harness *>(p)->slots.free_count(); }

}  // extern "C"
