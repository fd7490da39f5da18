// Stand-alone program over miosqp_amd/csrc/lockstep_ahead.hpp (tests/test_lockstep_ahead_cpu.py builds it with
// g++ -fsanitize=address,undefined and runs it): random PURE record functions -- a node's record is a hash of its tree
// and its path from the root -- through 1, 3, 64 and 70 trees sharing one free list that starts at 8 slots, with and
// without a node cap, under rules 0 - 3 and ahead 2, 4, 8.  Every run is compared with the same trees driven one node per
// wave by `Tree` alone (the loop of tests/lockstep_fuzz.cpp): the sequence of absorbed nodes (as a running hash), nodes,
// iters, upper, found, the open list's length and its largest, lower_glob.  After every wave each slot must be exactly one
// of free / open in one tree / reserved below a record / held for a child's warm start; at the end nothing reserved is
// left, and when every tree has closed every slot is free again.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../miosqp_amd/csrc/lockstep_ahead.hpp"

using namespace miosqp::lockstep;

static int fail(const char *what, int a, int b) {
  std::fprintf(stderr, "lockstep_ahead_fuzz: %s (%d, %d)\n", what, a, b);
  return 1;
}

static uint64_t mix(uint64_t x) {
  x += 0x9e3779b97f4a7c15ull;
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

static double unit(uint64_t h) { return (double)(h >> 11) * (1.0 / 9007199254740992.0); }

// the record of node `path` of tree `tree`: a pure function.  The bound grows along the path, deeper nodes close more
// often and nothing lives below depth 11: the trees are finite
static AheadOutcome node(uint64_t seed, int tree, const std::string &path) {
  uint64_t h = mix(seed ^ mix((uint64_t)tree + 1));
  double lower = unit(mix(h ^ 1));
  for (char c : path) {
    h = mix(h ^ (uint64_t)(unsigned char)c);
    lower += 0.5 * unit(mix(h ^ 1));
  }
  const int depth = (int)path.size();
  AheadOutcome o;
  o.finished = true;
  o.crossed = false;
  o.r.ok = depth < 11 && unit(mix(h ^ 2)) > 0.03 + 0.01 * depth;
  o.r.iter = 25 + (int)(unit(mix(h ^ 3)) * 400);
  o.r.lower = lower;
  o.r.int_inf = unit(mix(h ^ 4)) < 0.02 + 0.02 * depth ? 0 : 1 + (int)(unit(mix(h ^ 5)) * 5);
  o.r.nextvar = (int)(unit(mix(h ^ 6)) * 20);
  o.r.heur_feasible = unit(mix(h ^ 7)) < 0.15;
  o.r.heur_obj = lower + 6.0 * unit(mix(h ^ 8));
  return o;
}

struct End {
  uint64_t seq;
  int64_t nodes, iters;
  double upper, lower_glob;
  bool found;
  size_t open, max_open;
};

static uint64_t step(uint64_t seq, const std::string &path) {
  uint64_t h = mix(seq ^ 0xabcdefull);
  for (char c : path) h = mix(h ^ (uint64_t)(unsigned char)c);
  return h;
}

static End end_of(const Tree &t, const Slots &S, uint64_t seq) {
  return End{seq, t.nodes, t.iters, t.upper, t.lower_glob(S), t.found, t.open.size(), t.max_open};
}

static double upper0_of(int b) { return b % 3 == 0 ? 4.0 : NO_UPPER; }

// one node per wave with Tree alone
static void baseline(uint64_t seed, int B, int rule, int64_t max_iter_bb, std::vector<End> &ends, int64_t &waves) {
  Slots S;
  S.reset(8);
  while (S.cap < B) S.grow(2 * S.cap);
  std::vector<Tree> T((size_t)B);
  std::vector<std::string> path((size_t)S.cap);
  std::vector<uint64_t> seq((size_t)B, 0);
  for (int b = 0; b < B; b++) T[(size_t)b].start(S, S.take(), upper0_of(b));
  waves = 0;
  for (;;) {
    std::vector<int> live;
    for (int b = 0; b < B; b++)
      if (T[(size_t)b].can_continue(max_iter_bb)) live.push_back(b);
    if (live.empty()) break;
    waves++;
    while (S.free_count() < 2 * live.size()) {
      S.grow(2 * S.cap);
      path.resize((size_t)S.cap);
    }
    for (int b : live) {
      const int s = T[(size_t)b].pop(S, rule), c0 = S.take(), c1 = S.take();
      const std::string p = path[(size_t)s];
      path[(size_t)c0] = p + "0";
      path[(size_t)c1] = p + "1";
      seq[(size_t)b] = step(seq[(size_t)b], p);
      T[(size_t)b].absorb(S, s, c0, c1, node(seed, b, p).r);
    }
  }
  ends.clear();
  for (int b = 0; b < B; b++) ends.push_back(end_of(T[(size_t)b], S, seq[(size_t)b]));
}

int main() {
  int64_t records = 0, hits = 0, discarded = 0, called_off = 0, saved_waves = 0;
  int grown_total = 0, run = 0;
  const int Bs[4] = {1, 3, 64, 70};
  const int aheads[3] = {2, 4, 8};
  for (int bi = 0; bi < 4; bi++)
    for (int rule = 0; rule < 4; rule++)
      for (int capped = 0; capped < 2; capped++) {
        const int B = Bs[bi], ahead = aheads[(run++) % 3], ct = 25;
        const uint64_t seed = 1000 + (uint64_t)run;
        const int64_t max_iter_bb = capped ? 40 : 1000000;
        std::vector<End> want;
        int64_t waves1 = 0;
        baseline(seed, B, rule, max_iter_bb, want, waves1);
        Slots S;
        S.reset(8);
        Ahead A;
        while (S.cap < B) {
          S.grow(2 * S.cap);
          grown_total++;
        }
        A.reset(S.cap, B);
        std::vector<Tree> T((size_t)B);
        std::vector<std::string> path((size_t)S.cap);
        std::vector<uint64_t> seq((size_t)B, 0);
        for (int b = 0; b < B; b++) T[(size_t)b].start(S, S.take(), upper0_of(b));
        std::vector<int> live;
        std::vector<AheadColumn> cols;
        std::vector<AheadOutcome> out;
        int wave = 0;
        for (;;) {
          live.clear();
          for (int b = 0; b < B; b++)
            if (T[(size_t)b].can_continue(max_iter_bb)) live.push_back(b);
          if (live.empty()) break;
          wave++;
          const int L = (int)live.size(), free_cols = 64 * ((L + 63) / 64) - L;
          while (S.free_count() < 2 * (size_t)(L + free_cols)) {
            S.grow(2 * S.cap);
            A.grow(S.cap);
            path.resize((size_t)S.cap);
            grown_total++;
          }
          A.plan(S, T, live, rule, ahead, free_cols, cols);
          const int W = (int)cols.size();
          if (W > L + free_cols) return fail("a wave wider than its tiles", run, wave);
          std::vector<int> per((size_t)B, 0);
          out.resize((size_t)W);
          int chunks = 0;
          for (int c = 0; c < W; c++) {
            const AheadColumn &col = cols[(size_t)c];
            if (col.mandatory != (c < L)) return fail("the mandatory columns do not come first", run, wave);
            if (++per[(size_t)col.tree] > ahead) return fail("a tree holds more than `ahead` columns", run, wave);
            if (!col.mandatory && A.has[(size_t)col.slot]) return fail("a node with a record was sent again", run, wave);
            if (col.warm < 0 || col.warm >= S.cap) return fail("warm-start slot out of range", run, wave);
            const std::string p = path[(size_t)col.slot];
            path[(size_t)col.c0] = p + "0";
            path[(size_t)col.c1] = p + "1";
            out[(size_t)c] = node(seed, col.tree, p);
            if (col.mandatory) {
              const int k = (out[(size_t)c].r.iter + ct - 1) / ct;
              chunks = k > chunks ? k : chunks;
            }
          }
          for (int c = L; c < W; c++)
            if ((out[(size_t)c].r.iter + ct - 1) / ct > chunks) {
              out[(size_t)c].finished = false;
              out[(size_t)c].r.iter = chunks * ct;
            }
          records += W;
          A.settle(S, T, cols, out, rule, max_iter_bb, wave, [&](const AheadEvent &ev) {
            seq[(size_t)ev.tree] = step(seq[(size_t)ev.tree], path[(size_t)ev.slot]);
            return true;
          });
          std::vector<int> seen((size_t)S.cap, 0);
          for (int s : S.freelist) {
            if (s < 0 || s >= S.cap) return fail("free slot out of range", run, wave);
            seen[(size_t)s]++;
          }
          for (const Tree &tr : T)
            for (int s : tr.open) seen[(size_t)s]++;
          for (int s = 0; s < S.cap; s++)
            if (A.has[(size_t)s]) {
              seen[(size_t)A.c0[(size_t)s]]++;
              seen[(size_t)A.c1[(size_t)s]]++;
            }
          for (int s = 0; s < S.cap; s++) {
            const bool held = S.decided[(size_t)s] && S.kids[(size_t)s] > 0;
            if (seen[(size_t)s] != (held ? 0 : 1)) return fail("a slot is in two places or lost", run, wave);
          }
          if (wave > 200000) return fail("the trees do not end", run, wave);
        }
        A.finish(S);
        for (int s = 0; s < S.cap; s++)
          if (A.has[(size_t)s]) return fail("a record outlived the call", run, s);
        size_t open = 0;
        for (int b = 0; b < B; b++) {
          const End got = end_of(T[(size_t)b], S, seq[(size_t)b]), &w = want[(size_t)b];
          if (got.seq != w.seq) return fail("a tree absorbed other nodes, or in another order", run, b);
          if (got.nodes != w.nodes || got.iters != w.iters) return fail("nodes or iterations differ", run, b);
          if (got.upper != w.upper || got.found != w.found) return fail("the incumbent differs", run, b);
          if (got.lower_glob != w.lower_glob) return fail("lower_glob differs", run, b);
          if (got.open != w.open || got.max_open != w.max_open) return fail("the open list differs", run, b);
          if (capped && got.nodes > max_iter_bb - 1) return fail("a tree ran past max_iter_bb", run, b);
          open += got.open;
        }
        size_t held = 0;
        for (int s = 0; s < S.cap; s++) held += S.decided[(size_t)s] && S.kids[(size_t)s] > 0;
        if (S.free_count() + open + held != (size_t)S.cap) return fail("slots leaked", run, 0);
        if (!capped && (open != 0 || (int)S.free_count() != S.cap)) return fail("slots were not returned when every tree had closed", run, 0);
        if (wave > waves1) return fail("more waves than one node per wave", run, wave);
        if (A.n.sent != A.n.hits + A.n.discarded + A.n.called_off) return fail("the ahead columns do not add up", run, 0);
        saved_waves += waves1 - wave;
        hits += A.n.hits;
        discarded += A.n.discarded;
        called_off += A.n.called_off;
      }
  if (records < 2000) return fail("too few records for a meaningful run", 0, 0);
  if (grown_total < 6) return fail("the store never had to grow", 0, 0);
  if (hits < 100 || discarded < 10 || called_off < 10) return fail("hits, discards or call-offs were hardly exercised", (int)hits, (int)discarded);
  std::printf("lockstep_ahead_fuzz ok: %lld records, %lld hits, %lld discarded, %lld called off, %lld waves saved, %d growths\n",
              (long long)records, (long long)hits, (long long)discarded, (long long)called_off, (long long)saved_waves, grown_total);
  return 0;
}
