// The host logic of lock-step trees whose spare columns solve open leaves early (host_lockstep_ahead.inc drives it;
// tests/lockstep_ahead_harness.cpp replays recorded trees through it, tests/lockstep_ahead_fuzz.cpp runs random ones):
// plain C++17, no HIP include, compiles with g++ alone.  It sits on lockstep_trees.hpp and uses Tree and Slots unchanged.
//
// A wave launches whole tiles of 64 columns; with L live trees the columns behind the L mandatory ones iterate on
// padding.  A node is a pure function of (q, l, u, x0, y0), so a tree may put more than its chosen leaf into a wave:
//
//   * an AHEAD RECORD is the record of a node solved before the tree's exploration rule reached it, kept with `crossed`
//     and the two child slots reserved for its column.  A leaf of the open list that holds one stays in the list, is
//     counted as a leaf and keeps its INHERITED bound in Slots::lower: choose and prune see what the sequential solve
//     sees at that moment.
//   * the children of a node with an ahead record that is ok, fractional, not crossed and not above the tree's current
//     upper are SHADOW LEAVES: they live in the parent's reserved child slots (the device has written their lo / hi), are
//     not in the open list, and may be solved ahead as well, recursively.
//
// After a wave every tree absorbs its mandatory column and then, while it can continue and its rule chooses a leaf that
// holds an ahead record, pops that leaf and absorbs the record (a HIT): its shadow children become leaves and bring their
// own records along.  The first chosen leaf without a record is the next wave's mandatory column.  nodes, iters,
// incumbents and prunings happen at absorb time only; a record whose leaf is pruned, whose parent does not branch after
// all, or that is left when the call ends is DISCARDED with the whole shadow subtree below it, and every reserved slot
// goes back to the free list.  What is solved ahead and never reached cannot matter.
//
// The order in which ahead columns are chosen (it influences speed only, never results):
//   1. every live tree places its mandatory leaf, in tree order: columns 0 .. L-1 of the wave;
//   2. a tree's candidates are the leaves WITHOUT a record of its virtual list: the open leaves in list order, then the
//      shadow leaves in the order `end` would push them -- the list is walked front to back and the two shadow children
//      of every entry that has them are appended behind its current end (child 0, then child 1).  Shadow leaves carry the
//      depth and the inherited bound `end` would give them.  The candidates are ranked as the tree's rule would `choose`
//      them one after the other: depth descending (rule 0; rules 1 and 3 without an incumbent), inherited bound ascending
//      (rule 2; rule 3 with an incumbent) or descending (rule 1 with an incumbent), ties in virtual-list order;
//   3. the free columns are dealt round-robin over the live trees in tree order, one candidate per tree per round, until
//      a tree holds `ahead` columns, its candidates run out, or the free columns run out.
#ifndef MIOSQP_LOCKSTEP_AHEAD_HPP
#define MIOSQP_LOCKSTEP_AHEAD_HPP

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "lockstep_trees.hpp"

namespace miosqp {
namespace lockstep {

// a column of a wave: the five integers the device reads and whether the wave has to wait for it
struct AheadColumn {
  int tree, slot, warm, c0, c1;
  bool mandatory;
};

// what came back for a column.  finished == false: the wave ended before the column was decided (only an ahead column
// can be called off); nothing of it is kept, r.iter holds the iterations it had run
struct AheadOutcome {
  Record r;
  bool crossed;
  bool finished;
};

// one absorb, reported to the driver in the order the absorbs happen
struct AheadEvent {
  int tree, slot;
  Verdict v;
  bool crossed;  // with v.branch: the branching produced l > u (the driver refuses it, as the wave drivers do)
  bool hit;      // the record had been solved ahead
  int index;     // of a hit: the place `choose` gave it in the open list (-1 for a mandatory column: it was popped by plan)
};

struct AheadCounts {
  int64_t sent = 0, hits = 0, discarded = 0, called_off = 0;                 // ahead columns
  int64_t sent_iters = 0, hit_iters = 0, discarded_iters = 0, called_off_iters = 0;  // their ADMM iterations
};

struct Ahead {
  // per slot (sized like Slots): the ahead record a leaf or shadow leaf holds
  std::vector<char> has, crossed;
  std::vector<Record> rec;
  std::vector<int> c0, c1;
  // per tree: the leaves of its open list that hold a record
  std::vector<std::vector<int>> held;
  AheadCounts n;
  // scratch of plan()
  struct Cand { int slot, depth; double lower; };
  std::vector<std::vector<Cand>> cand;
  std::vector<int> virt, stack;

  void reset(int capacity, int ntrees) {
    const size_t c = (size_t)capacity;
    has.assign(c, 0); crossed.assign(c, 0); rec.assign(c, Record()); c0.assign(c, -1); c1.assign(c, -1);
    held.assign((size_t)ntrees, std::vector<int>());
    cand.assign((size_t)ntrees, std::vector<Cand>());
    n = AheadCounts();
  }
  void grow(int ncap) {
    const size_t c = (size_t)ncap;
    has.resize(c, 0); crossed.resize(c, 0); rec.resize(c, Record()); c0.resize(c, -1); c1.resize(c, -1);
  }

  // the children of the record in slot `s` are shadow leaves
  bool shadows(const Tree &T, int s) const {
    const Record &r = rec[(size_t)s];
    return has[(size_t)s] && r.ok && r.int_inf > 0 && r.nextvar >= 0 && !crossed[(size_t)s] && !(r.lower > T.upper);
  }

  // the record in slot `s` goes, with every record below it; the reserved slots return to the free list (s itself is the
  // caller's: a leaf being pruned, a child slot `end` gives back, or a leaf left at the end of the call)
  void discard(Slots &S, int s) {
    stack.clear();
    stack.push_back(s);
    while (!stack.empty()) {
      const int t = stack.back();
      stack.pop_back();
      if (!has[(size_t)t]) continue;
      has[(size_t)t] = 0;
      n.discarded++;
      n.discarded_iters += rec[(size_t)t].iter;
      for (int c : {c1[(size_t)t], c0[(size_t)t]}) {
        stack.push_back(c);  // (its own reserved slots first go back when it is popped)
        S.give_back(c);
      }
    }
  }

  // The wave: cols[0 .. L-1] the mandatory leaves of the live trees (popped from their lists), then at most `free_cols`
  // ahead columns in dealing order.  Two child slots are taken per column: the caller has made sure the free list holds
  // 2 * (live.size() + free_cols).  ahead: the most columns a tree may hold.
  void plan(Slots &S, std::vector<Tree> &T, const std::vector<int> &live, int rule, int ahead, int free_cols,
            std::vector<AheadColumn> &cols) {
    cols.clear();
    for (int b : live) {
      AheadColumn c;
      c.tree = b;
      c.slot = T[(size_t)b].pop(S, rule);
      c.warm = S.warm_slot(c.slot);
      c.c0 = S.take();
      c.c1 = S.take();
      c.mandatory = true;
      cols.push_back(c);
    }
    if (ahead <= 1 || free_cols <= 0) return;
    for (int b : live) {
      const Tree &tr = T[(size_t)b];
      std::vector<Cand> &cd = cand[(size_t)b];
      cd.clear();
      virt.assign(tr.open.begin(), tr.open.end());
      for (size_t k = 0; k < virt.size(); k++) {
        const int s = virt[k];
        if (!has[(size_t)s]) {
          cd.push_back(Cand{s, S.depth[(size_t)s], S.lower[(size_t)s]});
        } else if (shadows(tr, s)) {
          for (int c : {c0[(size_t)s], c1[(size_t)s]}) {  // what `end` will write when the record is absorbed
            S.depth[(size_t)c] = S.depth[(size_t)s] + 1;
            S.lower[(size_t)c] = rec[(size_t)s].lower;
            S.parent[(size_t)c] = s;
            virt.push_back(c);
          }
        }
      }
      const bool by_depth = rule == 0 || (rule != 2 && !(tr.upper < NO_UPPER));
      if (by_depth) std::stable_sort(cd.begin(), cd.end(), [](const Cand &a, const Cand &b2) { return a.depth > b2.depth; });
      else if (rule >= 2) std::stable_sort(cd.begin(), cd.end(), [](const Cand &a, const Cand &b2) { return a.lower < b2.lower; });
      else std::stable_sort(cd.begin(), cd.end(), [](const Cand &a, const Cand &b2) { return a.lower > b2.lower; });
    }
    int left = free_cols;
    for (int round = 0; round + 1 < ahead && left > 0; round++) {
      bool any = false;
      for (int b : live) {
        if (left == 0) break;
        const std::vector<Cand> &cd = cand[(size_t)b];
        if ((size_t)round >= cd.size()) continue;
        AheadColumn c;
        c.tree = b;
        c.slot = cd[(size_t)round].slot;
        c.warm = S.warm_slot(c.slot);
        c.c0 = S.take();
        c.c1 = S.take();
        c.mandatory = false;
        cols.push_back(c);
        left--;
        any = true;
      }
      if (!any) break;
    }
  }

  // the leaves of tree b that a pruning has just removed from its list lose their records
  void sweep(Slots &S, int b) {
    std::vector<int> &h = held[(size_t)b];
    size_t w = 0;
    for (size_t k = 0; k < h.size(); k++) {
      const int s = h[k];
      if (S.decided[(size_t)s]) discard(S, s);  // (Slots::done marked it; its own slot went back there)
      else h[w++] = s;
    }
    h.resize(w);
  }

  // bound_and_branch on the record of node `s` of tree b (Tree::absorb = begin + end), with what hangs below it
  template <class Sink>
  bool absorb_one(Slots &S, Tree &tr, int b, int s, int k0, int k1, const Record &r, bool cr, int hit_index, Sink &&sink) {
    const Verdict v = tr.begin(S, s, r, 0).v;
    if (!v.branch) {  // the children's slots go back in `end`: whatever was solved below them goes first
      discard(S, k0);
      discard(S, k1);
    }
    tr.end(S, s, k0, k1, v);
    if (v.branch)
      for (int c : {k0, k1})
        if (has[(size_t)c]) held[(size_t)b].push_back(c);
    sweep(S, b);
    return sink(AheadEvent{b, s, v, cr, hit_index >= 0, hit_index});
  }

  // After the wave `cols` with the outcomes `out` (same order): the ahead records are stored, then every tree of the wave,
  // in the order of the mandatory columns, absorbs its mandatory column and every record its rule reaches.
  // sink(const AheadEvent &) -> bool is called per absorb; false stops everything at once (the driver's error exit).
  // wave: the wave's number, for Tree::finished_at.
  template <class Sink>
  bool settle(Slots &S, std::vector<Tree> &T, const std::vector<AheadColumn> &cols, const std::vector<AheadOutcome> &out,
              int rule, int64_t max_iter_bb, int wave, Sink &&sink) {
    size_t L = 0;
    while (L < cols.size() && cols[L].mandatory) L++;
    for (size_t k = L; k < cols.size(); k++) {
      const AheadColumn &c = cols[k];
      const AheadOutcome &o = out[k];
      n.sent++;
      n.sent_iters += o.r.iter;
      if (!o.finished) {  // nothing half-done is kept: the leaf is solved again from its parent's iterate
        n.called_off++;
        n.called_off_iters += o.r.iter;
        S.give_back(c.c1);
        S.give_back(c.c0);
        continue;
      }
      const size_t s = (size_t)c.slot;
      has[s] = 1;
      rec[s] = o.r;
      crossed[s] = o.crossed;
      c0[s] = c.c0;
      c1[s] = c.c1;
      Tree &tr = T[(size_t)c.tree];
      if (std::find(tr.open.begin(), tr.open.end(), c.slot) != tr.open.end()) held[(size_t)c.tree].push_back(c.slot);
    }
    for (size_t k = 0; k < L; k++) {
      const AheadColumn &c = cols[k];
      Tree &tr = T[(size_t)c.tree];
      if (!absorb_one(S, tr, c.tree, c.slot, c.c0, c.c1, out[k].r, out[k].crossed, -1, sink)) return false;
      while (tr.can_continue(max_iter_bb)) {
        const int idx = (int)tr.choose(S, rule);
        const int s = tr.open[(size_t)idx];
        if (!has[(size_t)s]) break;  // the next wave's mandatory column
        tr.pop(S, rule);
        std::vector<int> &h = held[(size_t)c.tree];
        h.erase(std::find(h.begin(), h.end(), s));
        has[(size_t)s] = 0;
        n.hits++;
        n.hit_iters += rec[(size_t)s].iter;
        const Record r = rec[(size_t)s];
        if (!absorb_one(S, tr, c.tree, s, c0[(size_t)s], c1[(size_t)s], r, crossed[(size_t)s] != 0, idx, sink)) return false;
      }
      if (!tr.can_continue(max_iter_bb)) tr.finished_at = wave;
    }
    return true;
  }

  // the end of the call (also a failed one): every record that was never reached goes
  void finish(Slots &S) {
    for (std::vector<int> &h : held) {
      for (int s : h) discard(S, s);
      h.clear();
    }
  }
};

}  // namespace lockstep
}  // namespace miosqp

#endif
