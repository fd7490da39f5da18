// The host logic of B branch-and-bound trees advanced in lock step (host_lockstep.inc drives it; tests/lockstep_harness.cpp
// replays recorded trees through it): plain C++17, no HIP include, compiles with g++ alone.
//
// It restates the three decisions of the Python mirror (miosqp_amd/bnb.py) with the list semantics of host_search.inc:
// list order = creation order, choose = first extremum (workspace.py:128-149 and best bound), the prune traversal that does
// not examine the element behind a removed one (workspace.py:274-280), and bound_and_branch on a node's digest
// (workspace.py:282-334), whole (absorb) or in three steps around round and fix (begin / heuristic / end: bnb.py's
// Workspace.primal_heuristic between the verdict and the children).  Every tree has its own open list, incumbent value and counters; the node slots -- the device
// store's indices -- and their free list are shared by all trees.
#ifndef MIOSQP_LOCKSTEP_TREES_HPP
#define MIOSQP_LOCKSTEP_TREES_HPP

#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

namespace miosqp {
namespace lockstep {

constexpr double NO_UPPER = 1.7e308;  // an incumbent value at or above it means "none" (the C ABI's convention)

// what the device leaves of a solved node (a column of the wave)
struct Record {
  bool ok;             // OSQP_SOLVED or OSQP_MAX_ITER_REACHED: x, lower and the digest mean something
  int iter;            // ADMM iterations
  double lower;        // objective at the clamped x
  int int_inf;         // integer entries further than eps_int_feas from an integer
  int nextvar;         // most fractional position (branching_rule 0)
  bool heur_feasible;  // the rounded point satisfies the INSTANCE's root rows
  double heur_obj;     // its objective
};

// what absorbing a record decided
struct Verdict {
  bool branch;    // the two children enter the list (their slots are kept)
  int incumbent;  // 0: unchanged, 1: the node's x is the new incumbent, 2: its rounded point is
};

// what the first step of a split absorb decided (Tree::begin)
struct Begun {
  Verdict v;
  bool fire;  // round and fix runs at this node before its children enter the list
};

// Node slots shared by all trees.  A slot stays allocated while a child may still read its solution as a warm start: the
// last child to be decided frees it (host_search.inc: search_done).
struct Slots {
  int cap = 0;
  std::vector<int> freelist, depth, parent, kids;
  std::vector<char> decided;
  std::vector<double> lower;

  void reset(int capacity) {
    cap = capacity;
    const size_t c = (size_t)capacity;
    depth.assign(c, 0); parent.assign(c, -1); kids.assign(c, 0); decided.assign(c, 0); lower.assign(c, 0.0);
    freelist.clear();
    for (int s = capacity - 1; s >= 0; s--) freelist.push_back(s);  // take() hands out slot 0 first
  }
  // the store has doubled (or more): the new slots join the free list, lowest handed out first
  void grow(int ncap) {
    const size_t c = (size_t)ncap;
    depth.resize(c, 0); parent.resize(c, -1); kids.resize(c, 0); decided.resize(c, 0); lower.resize(c, 0.0);
    for (int s = ncap - 1; s >= cap; s--) freelist.push_back(s);
    cap = ncap;
  }
  size_t free_count() const { return freelist.size(); }
  int take() {
    const int s = freelist.back();
    freelist.pop_back();
    return s;
  }
  void give_back(int s) { freelist.push_back(s); }
  // node `s` has been decided or discarded
  void done(int s) {
    decided[(size_t)s] = 1;
    if (kids[(size_t)s] == 0) freelist.push_back(s);
    const int par = parent[(size_t)s];
    if (par >= 0 && --kids[(size_t)par] == 0 && decided[(size_t)par]) freelist.push_back(par);
  }
  // the slot whose solution warm-starts node `s`: its parent's, its own for a root (x0, y0 were written there)
  int warm_slot(int s) const { return parent[(size_t)s] >= 0 ? parent[(size_t)s] : s; }
};

struct Tree {
  std::vector<int> open;  // slots of the open leaves, in creation order
  double upper = std::numeric_limits<double>::infinity();
  bool found = false;     // an incumbent was found by a node of this run
  int64_t nodes = 0, iters = 0;
  int finished_at = 0;    // the wave after which the tree was done (0: nothing to do)
  size_t max_open = 0;
  // round and fix: the fractional nodes that asked (Workspace.rf_nodes) and what Workspace.rf_stats counts
  int64_t rf_nodes = 0, rf_calls = 0, rf_candidates = 0, rf_feasible = 0, rf_improved = 0, rf_iters = 0;

  // a root with explicit bounds and warm start in slot `s`; upper0 >= NO_UPPER: no incumbent (Workspace.set_x0)
  void start(Slots &S, int s, double upper0) {
    open.clear();
    upper = upper0 < NO_UPPER ? upper0 : std::numeric_limits<double>::infinity();
    found = false;
    nodes = iters = 0;
    rf_nodes = rf_calls = rf_candidates = rf_feasible = rf_improved = rf_iters = 0;
    finished_at = 0;
    S.depth[(size_t)s] = 0;
    S.lower[(size_t)s] = -std::numeric_limits<double>::infinity();
    S.parent[(size_t)s] = -1;
    S.kids[(size_t)s] = 0;
    S.decided[(size_t)s] = 0;
    open.push_back(s);
    max_open = 1;
  }

  // workspace.py:113-126 (iter_num = nodes + 1)
  bool can_continue(int64_t max_iter_bb) const { return !open.empty() && nodes + 1 < max_iter_bb; }

  // workspace.py:128-149: index into the open list.  Rule 0: the first deepest leaf; rule 1: that until an incumbent
  // exists, then the leaf with the LARGEST inherited bound (sic), the first one; rule 2: the leaf with the SMALLEST
  // inherited bound, the first one; rule 3: like rule 0 until an incumbent exists, then like rule 2.
  size_t choose(const Slots &S, int rule) const {
    size_t best = 0;
    if (rule == 0 || (rule != 2 && !(upper < NO_UPPER))) {
      for (size_t k = 1; k < open.size(); k++)
        if (S.depth[(size_t)open[k]] > S.depth[(size_t)open[best]]) best = k;
    } else if (rule >= 2) {
      for (size_t k = 1; k < open.size(); k++)
        if (S.lower[(size_t)open[k]] < S.lower[(size_t)open[best]]) best = k;
    } else {
      for (size_t k = 1; k < open.size(); k++)
        if (S.lower[(size_t)open[k]] > S.lower[(size_t)open[best]]) best = k;
    }
    return best;
  }

  // choose_leaf: the leaf leaves the list
  int pop(const Slots &S, int rule) {
    const size_t idx = choose(S, rule);
    const int s = open[idx];
    open.erase(open.begin() + (std::ptrdiff_t)idx);
    return s;
  }

  // workspace.py:274-280 with the reference's traversal: the element following a removed one is not examined
  void prune(Slots &S) {
    size_t k = 0;
    while (k < open.size()) {
      if (S.lower[(size_t)open[k]] > upper) {
        const int s = open[k];
        open.erase(open.begin() + (std::ptrdiff_t)k);
        S.done(s);
      }
      k++;
    }
  }

  // bound_and_branch (workspace.py:282-334) on the record of node `s`, whose children would sit in slots c0 and c1
  // (taken before the wave).  Without a branching the two slots go back to the free list.
  Verdict absorb(Slots &S, int s, int c0, int c1, const Record &r) {
    const Verdict v = begin(S, s, r, 0).v;
    end(S, s, c0, c1, v);
    return v;
  }

  // absorb in three steps, for the driver that runs round and fix (Workspace.primal_heuristic / round_and_fix of
  // miosqp_amd/bnb.py) between a node's verdict and the entry of its children:
  // begin: bound_and_branch up to the point where the children would be pushed, and whether the heuristic fires at this
  // node -- only a fractional node that is about to branch asks, every rf_every-th of them, the first included
  // (rf_every < 1: the heuristic is off and nothing is counted).
  Begun begin(Slots &S, int s, const Record &r, int rf_every) {
    Begun g{{false, 0}, false};
    Verdict &v = g.v;
    nodes++;
    iters += r.iter;
    if (r.ok) {
      S.lower[(size_t)s] = r.lower;
      if (!(r.lower > upper)) {
        if (r.int_inf == 0) {
          upper = r.lower;
          found = true;
          v.incumbent = 1;
          prune(S);
        } else {
          if (r.heur_feasible && r.heur_obj < upper) {
            upper = r.heur_obj;
            found = true;
            v.incumbent = 2;
            prune(S);
          }
          v.branch = true;
          if (rf_every > 0) {
            g.fire = rf_nodes % rf_every == 0;
            rf_nodes++;
          }
        }
      }
    }
    return g;
  }

  // the outcome of the heuristic's K candidates at a node where begin said `fire`: `counted`: a candidate counts (it has
  // an x and its rounded point keeps the root's rows), `obj` the lowest objective among those, `feasible` how many count,
  // `it` the candidates' iterations.  The winner becomes the incumbent when it is better (primal_heuristic).  Returns
  // whether it did.
  bool heuristic(Slots &S, int K, bool counted, double obj, int feasible, int64_t it) {
    rf_calls++;
    rf_candidates += K;
    rf_feasible += feasible;
    rf_iters += it;
    if (!counted || !(obj < upper)) return false;
    upper = obj;
    found = true;
    rf_improved++;
    prune(S);
    return true;
  }

  // end: the children enter the list behind whatever the pruning left, or their slots go back
  void end(Slots &S, int s, int c0, int c1, const Verdict &v) {
    if (v.branch) {
      for (int c : {c0, c1}) {
        S.depth[(size_t)c] = S.depth[(size_t)s] + 1;
        S.lower[(size_t)c] = S.lower[(size_t)s];
        S.parent[(size_t)c] = s;
        S.kids[(size_t)c] = 0;
        S.decided[(size_t)c] = 0;
        open.push_back(c);
      }
      S.kids[(size_t)s] = 2;
      if (open.size() > max_open) max_open = open.size();
    } else {
      S.give_back(c1);
      S.give_back(c0);
      S.kids[(size_t)s] = 0;
    }
    S.done(s);
  }

  // workspace.py:334, reported once: the smallest bound of the open leaves (the incumbent's value on a closed tree)
  double lower_glob(const Slots &S) const {
    if (open.empty()) return upper;
    double lg = std::numeric_limits<double>::infinity();
    for (int s : open) lg = S.lower[(size_t)s] < lg ? S.lower[(size_t)s] : lg;
    return lg;
  }
};

}  // namespace lockstep
}  // namespace miosqp

#endif
