// The scheduling of B branch-and-bound trees on C columns that are refilled between chunks (host_refill.inc drives it;
// tests/refill_fuzz.cpp runs it on the CPU): plain C++17, no HIP include, compiles with g++ alone.
//
// A column holds one node of one tree; a tree has at most ONE node in flight, so its next leaf is chosen only after its
// previous node was absorbed and every tree makes the decisions of its sequential solve (solver.py:85-123: choose_leaf ->
// solve -> bound_and_branch, one node after the other) whatever the other trees do.  The trees, their open lists and the
// shared slots are those of lockstep_trees.hpp, unchanged (workspace.py:128-155, 282-334).  What is decided here:
//   * which tree goes into which free column: the lowest free column takes the lowest-numbered tree that has no node in
//     flight and can continue (so the busy columns stay at the front while trees are waiting);
//   * the in-flight flags;
//   * the two child slots a column reserves when it is filled, and their return when its node does not branch.
#ifndef MIOSQP_LOCKSTEP_REFILL_HPP
#define MIOSQP_LOCKSTEP_REFILL_HPP

#include "lockstep_trees.hpp"

namespace miosqp {
namespace lockstep {

// a column as it is filled: what the device needs to load it (the order of the upload, host_refill.inc)
struct Fill {
  int col, tree, slot, warm, child0, child1;
};

struct Refill {
  int C = 0;                   // columns
  int busy = 0;                // columns holding a node in flight
  std::vector<Fill> cols;      // per column: the node it holds (tree < 0: free)
  std::vector<char> in_flight; // per tree
  int first_tree = 0;          // no tree below this one can ever be filled again (they are done): where fill() starts looking

  void reset(int columns, int trees) {
    C = columns;
    busy = 0;
    cols.assign((size_t)columns, Fill{-1, -1, -1, -1, -1, -1});
    in_flight.assign((size_t)trees, 0);
    first_tree = 0;
  }

  // how many columns fill() would load now: min(free columns, trees without a node in flight that can continue).  The
  // caller makes sure that twice as many slots are free (the store grows) BEFORE it calls fill().
  int fillable(const std::vector<Tree> &T, int64_t max_iter_bb) const {
    const int room = C - busy;
    int k = 0;
    for (size_t b = (size_t)first_tree; b < T.size() && k < room; b++)
      if (!in_flight[b] && T[b].can_continue(max_iter_bb)) k++;
    return k;
  }

  // Fill the free columns, lowest first, with the next leaf of the waiting trees, lowest tree first; appends to `out`.
  // Returns the number of columns filled.
  int fill(Slots &S, std::vector<Tree> &T, int rule, int64_t max_iter_bb, std::vector<Fill> &out) {
    int filled = 0, c = 0;
    // trees that are done and idle never come back: skip them for good
    while ((size_t)first_tree < T.size() && !in_flight[(size_t)first_tree] && !T[(size_t)first_tree].can_continue(max_iter_bb))
      first_tree++;
    for (size_t b = (size_t)first_tree; b < T.size() && busy < C; b++) {
      if (in_flight[b] || !T[b].can_continue(max_iter_bb)) continue;
      while (cols[(size_t)c].tree >= 0) c++;  // (busy < C: there is a free one)
      Fill f;
      f.col = c;
      f.tree = (int)b;
      f.slot = T[b].pop(S, rule);
      f.warm = S.warm_slot(f.slot);
      f.child0 = S.take();
      f.child1 = S.take();
      cols[(size_t)c] = f;
      in_flight[b] = 1;
      busy++;
      filled++;
      out.push_back(f);
    }
    return filled;
  }

  // The node in column c has been decided: bound_and_branch of its tree on the record, the column becomes free and the tree
  // may be filled again.  *tree, *slot: whose node it was (for the incumbent's copy).
  Verdict absorb(Slots &S, std::vector<Tree> &T, int c, const Record &r, int *tree, int *slot) {
    Fill &f = cols[(size_t)c];
    const Verdict v = T[(size_t)f.tree].absorb(S, f.slot, f.child0, f.child1, r);
    *tree = f.tree;
    *slot = f.slot;
    in_flight[(size_t)f.tree] = 0;
    f = Fill{-1, -1, -1, -1, -1, -1};
    busy--;
    return v;
  }
};

}  // namespace lockstep
}  // namespace miosqp

#endif
