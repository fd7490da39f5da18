// Stand-alone program over miosqp_amd/csrc/lockstep_trees.hpp with the absorb split around round and fix
// (tests/test_lockstep_rf_cpu.py builds it with g++ -fsanitize=address,undefined and runs it): several trees sharing one
// free list advance in lock step on random records and random heuristic outcomes -- begin for every column of the wave,
// the heuristic for the trees that fired, end for every column --, the store starting small so that it has to double
// several times.  Between begin and end the node in flight and its two child slots are in nobody's list; after every
// wave each slot must be exactly one of free / open in one tree / held for a child's warm start; when every tree has
// closed, every slot is free again.  A twin of every tree runs the unsplit absorb on the same records with the
// heuristic off: where the heuristic never improved, the two must be the same tree.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../miosqp_amd/csrc/lockstep_trees.hpp"

using namespace miosqp::lockstep;

static int fail(const char *what, int wave) {
  std::fprintf(stderr, "lockstep_rf_fuzz: %s (wave %d)\n", what, wave);
  return 1;
}

int main() {
  std::mt19937_64 rng(4321);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  int64_t records = 0, calls = 0, improved = 0;
  int grown_total = 0;
  for (int round = 0; round < 8; round++) {
    const int B = 3 + 2 * round, rule = round % 4, every = 1 + round % 3, K = 1 + 5 * (round % 4);
    const bool never_improves = round >= 6;  // the heuristic runs and finds nothing: the trees are those of absorb
    const int64_t max_iter_bb = round == 5 ? 40 : 100000;
    Slots S, S2;
    S.reset(B + 1);
    S2.reset(B + 1);
    std::vector<Tree> T((size_t)B), T2((size_t)B);
    for (int b = 0; b < B; b++) {
      T[(size_t)b].start(S, S.take(), b % 3 == 0 ? 50.0 : NO_UPPER);
      T2[(size_t)b].start(S2, S2.take(), b % 3 == 0 ? 50.0 : NO_UPPER);
    }
    int wave = 0;
    for (;;) {
      std::vector<int> live;
      for (int b = 0; b < B; b++)
        if (T[(size_t)b].can_continue(max_iter_bb)) live.push_back(b);
      if (never_improves)
        for (int b = 0; b < B; b++)
          if (T2[(size_t)b].can_continue(max_iter_bb) != T[(size_t)b].can_continue(max_iter_bb)) return fail("the twin stopped elsewhere", wave);
      if (live.empty()) break;
      wave++;
      while (S.free_count() < 2 * live.size()) {
        S.grow(2 * S.cap);
        grown_total++;
      }
      while (S2.free_count() < 2 * live.size()) S2.grow(2 * S2.cap);
      struct Col { int b, s, c0, c1, s2, d0, d1; Begun g; };
      std::vector<Col> cols;
      for (int b : live) {
        Col c;
        c.b = b;
        c.s = T[(size_t)b].pop(S, rule);
        const int w = S.warm_slot(c.s);
        if (w < 0 || w >= S.cap) return fail("warm-start slot out of range", wave);
        if (w != c.s && S.kids[(size_t)w] < 1) return fail("a warm-start slot was released before its child ran", wave);
        c.c0 = S.take();
        c.c1 = S.take();
        c.s2 = c.d0 = c.d1 = -1;
        if (never_improves) {
          c.s2 = T2[(size_t)b].pop(S2, rule);
          c.d0 = S2.take();
          c.d1 = S2.take();
        }
        c.g = Begun{{false, 0}, false};
        cols.push_back(c);
      }
      // begin for every column
      for (Col &c : cols) {
        Tree &tr = T[(size_t)c.b];
        const int depth = S.depth[(size_t)c.s];
        Record r;
        const double v = U(rng);
        // deeper nodes close more often, and past 300 nodes a tree only closes: the trees stay finite
        r.ok = tr.nodes < 300 && v > 0.03 + 0.01 * depth;
        r.iter = 25 + (int)(U(rng) * 400);
        const double inherited = S.lower[(size_t)c.s];
        r.lower = (inherited > -1e300 ? inherited : 0.0) + 0.5 * U(rng);
        r.int_inf = U(rng) < 0.02 + 0.01 * depth ? 0 : 1 + (int)(U(rng) * 5);
        r.nextvar = (int)(U(rng) * 20);
        r.heur_feasible = U(rng) < 0.1;
        r.heur_obj = r.lower + 20.0 * U(rng);
        const double before = tr.upper;
        const int64_t asked = tr.rf_nodes;
        c.g = tr.begin(S, c.s, r, every);
        records++;
        if (c.g.v.incumbent && !(tr.upper < before)) return fail("an incumbent that does not improve", wave);
        if (c.g.fire && !c.g.v.branch) return fail("the heuristic fired at a node that does not branch", wave);
        if (c.g.fire != (c.g.v.branch && asked % every == 0)) return fail("fired at the wrong node", wave);
        if (tr.rf_nodes != asked + (c.g.v.branch ? 1 : 0)) return fail("rf_nodes counts other nodes than the branching ones", wave);
        if (never_improves) {
          const Verdict v2 = T2[(size_t)c.b].absorb(S2, c.s2, c.d0, c.d1, r);
          if (v2.branch != c.g.v.branch || v2.incumbent != c.g.v.incumbent) return fail("the twin decided otherwise", wave);
        }
      }
      // the node in flight and its child slots are nowhere yet: not free, not open
      for (const Col &c : cols) {
        for (int s : S.freelist)
          if (s == c.s || s == c.c0 || s == c.c1) return fail("a slot of a node in flight is free before end", wave);
      }
      // the heuristic's outcome for the trees that fired
      for (Col &c : cols) {
        if (!c.g.fire) continue;
        Tree &tr = T[(size_t)c.b];
        const double before = tr.upper;
        const int feasible = never_improves ? 0 : (int)(U(rng) * (K + 1));
        const double obj = S.lower[(size_t)c.s] + 15.0 * U(rng);
        const bool imp = tr.heuristic(S, K, feasible > 0, obj, feasible, 10 * K);
        calls++;
        improved += imp;
        if (imp != (feasible > 0 && obj < before)) return fail("the heuristic's winner was judged wrongly", wave);
        if (imp && tr.upper != obj) return fail("the winner's value is not the incumbent's", wave);
        if (!imp && tr.upper != before) return fail("the incumbent moved without a winner", wave);
      }
      // end for every column
      for (const Col &c : cols) {
        T[(size_t)c.b].end(S, c.s, c.c0, c.c1, c.g.v);
        if (c.g.v.branch && (S.parent[(size_t)c.c0] != c.s || S.parent[(size_t)c.c1] != c.s)) return fail("children without their parent", wave);
        if (c.g.v.branch && T[(size_t)c.b].open.back() != c.c1) return fail("the children are not the last of the list", wave);
      }
      // every slot exactly once: free, open, or held by a decided parent whose children are still undecided
      std::vector<int> seen((size_t)S.cap, 0);
      for (int s : S.freelist) {
        if (s < 0 || s >= S.cap) return fail("free slot out of range", wave);
        seen[(size_t)s]++;
      }
      for (const Tree &tr : T)
        for (int s : tr.open) {
          if (s < 0 || s >= S.cap) return fail("open slot out of range", wave);
          seen[(size_t)s]++;
        }
      for (int s = 0; s < S.cap; s++) {
        const bool held = S.decided[(size_t)s] && S.kids[(size_t)s] > 0;
        if (seen[(size_t)s] > 1) return fail("a slot is in two places", wave);
        if (seen[(size_t)s] == 1 && held) return fail("a slot a child still reads is free or open", wave);
        if (seen[(size_t)s] == 0 && !held) return fail("a slot was lost", wave);
      }
      if (never_improves)
        for (int b = 0; b < B; b++) {
          const Tree &a = T[(size_t)b], &t2 = T2[(size_t)b];
          if (a.open.size() != t2.open.size() || a.upper != t2.upper || a.nodes != t2.nodes || a.iters != t2.iters)
            return fail("a heuristic that finds nothing changed the tree", wave);
        }
      if (wave > 200000) return fail("the trees do not end", wave);
    }
    for (const Tree &tr : T) {
      if (tr.rf_candidates != tr.rf_calls * K) return fail("candidates are not K per call", wave);
      if (tr.rf_improved > tr.rf_calls || tr.rf_feasible > tr.rf_candidates) return fail("counters out of range", wave);
      if (tr.rf_calls != (tr.rf_nodes + every - 1) / every) return fail("calls are not every rf_every-th asking node", wave);
    }
    if (max_iter_bb > 1000) {
      for (const Tree &tr : T)
        if (!tr.open.empty()) return fail("a tree ended with open leaves", wave);
      if ((int)S.free_count() != S.cap) return fail("slots were not returned when every tree had closed", wave);
    } else {
      for (const Tree &tr : T)
        if (tr.nodes > max_iter_bb - 1) return fail("a tree ran past max_iter_bb", wave);
    }
  }
  if (records < 2000) return fail("too few records for a meaningful run", 0);
  if (calls < 200 || improved < 10) return fail("the heuristic hardly ran", 0);
  if (grown_total < 6) return fail("the store never had to grow", 0);
  std::printf("lockstep_rf_fuzz ok: %lld records, %lld heuristic calls, %lld improved, %d growths\n", (long long)records,
              (long long)calls, (long long)improved, grown_total);
  return 0;
}
