// Stand-alone program over miosqp_amd/csrc/lockstep_trees.hpp (tests/test_lockstep_trees_cpu.py builds it with
// g++ -fsanitize=address,undefined and runs it): several trees sharing one free list advance in lock step on random
// records, the store starting small so that it has to double several times.  After every wave each slot must be exactly
// one of free / open in one tree / held for a child's warm start; when every tree has closed, every slot is free again.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../miosqp_amd/csrc/lockstep_trees.hpp"

using namespace miosqp::lockstep;

static int fail(const char *what, int wave) {
  std::fprintf(stderr, "lockstep_fuzz: %s (wave %d)\n", what, wave);
  return 1;
}

int main() {
  std::mt19937_64 rng(12345);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  int64_t records = 0;
  int grown_total = 0;
  for (int round = 0; round < 6; round++) {
    const int B = 3 + 2 * round, rule = round % 4;
    const int64_t max_iter_bb = round == 5 ? 40 : 100000;
    Slots S;
    S.reset(B + 1);
    std::vector<Tree> T((size_t)B);
    for (int b = 0; b < B; b++) T[(size_t)b].start(S, S.take(), b % 3 == 0 ? 50.0 : NO_UPPER);
    int wave = 0;
    for (;;) {
      std::vector<int> live;
      for (int b = 0; b < B; b++)
        if (T[(size_t)b].can_continue(max_iter_bb)) live.push_back(b);
      if (live.empty()) break;
      wave++;
      while (S.free_count() < 2 * live.size()) {
        S.grow(2 * S.cap);
        grown_total++;
      }
      struct Col { int b, s, w, c0, c1; };
      std::vector<Col> cols;
      for (int b : live) {
        Col c;
        c.b = b;
        c.s = T[(size_t)b].pop(S, rule);
        c.w = S.warm_slot(c.s);
        if (c.w < 0 || c.w >= S.cap) return fail("warm-start slot out of range", wave);
        if (c.w != c.s && S.kids[(size_t)c.w] < 1) return fail("a warm-start slot was released before its child ran", wave);
        c.c0 = S.take();
        c.c1 = S.take();
        cols.push_back(c);
      }
      for (const Col &c : cols) {
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
        r.heur_feasible = U(rng) < 0.15;
        r.heur_obj = r.lower + 20.0 * U(rng);
        const double before = tr.upper;
        const Verdict vd = tr.absorb(S, c.s, c.c0, c.c1, r);
        records++;
        if (vd.incumbent && !(tr.upper < before)) return fail("an incumbent that does not improve", wave);
        if (vd.branch && (S.parent[(size_t)c.c0] != c.s || S.parent[(size_t)c.c1] != c.s)) return fail("children without their parent", wave);
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
      if (wave > 200000) return fail("the trees do not end", wave);
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
  if (grown_total < 6) return fail("the store never had to grow", 0);
  std::printf("lockstep_fuzz ok: %lld records, %d growths\n", (long long)records, grown_total);
  return 0;
}
