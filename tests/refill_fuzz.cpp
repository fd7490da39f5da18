// Stand-alone program over miosqp_amd/csrc/lockstep_refill.hpp (tests/test_lockstep_refill_cpu.py builds it with
// g++ -fsanitize=address,undefined and runs it): the scheduling of B trees on C refilled columns, without a device.
// Every node gets a duration of 1-8 chunks; the loop below is host_refill.inc's -- fill the free columns, run a chunk,
// absorb the columns whose node ended, in column order -- with the checks the device cannot make:
//   * a tree never has two nodes in flight, no column is filled while it is busy, no slot is held twice;
//   * every tree's sequence of (rank of the chosen leaf in its list, list length after the absorb) is the wave driver's
//     for the same records: the trees do not depend on the order in which the columns end;
//   * when every tree has closed, every slot is free again;
//   * with B <= C no chunk is idle: the chunks run equal the largest per-tree sum of durations.
// Without an argument the records are random (a tree draws them from a generator of its own, so that the k-th node of a
// tree gets the same record under both drivers).  With a file they are recorded ones (written by the test from the Python
// trees on the CPU backend), and the sequences must also be the recorded ones.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "../miosqp_amd/csrc/lockstep_refill.hpp"

using namespace miosqp::lockstep;

typedef std::vector<std::pair<int, int>> Trace;  // per node of a tree: (rank chosen, leaves after)

static int fail(const char *what, int a, int b) {
  std::fprintf(stderr, "refill_fuzz: %s (%d, %d)\n", what, a, b);
  return 1;
}

// where a tree's records come from: node k of tree b, given the state the tree is in when the node is chosen
struct Source {
  // recorded
  bool recorded = false;
  std::vector<std::vector<Record>> rec;
  // random
  std::vector<std::mt19937_64> rng;
  std::vector<std::mt19937_64> dur;

  void seed(int B, uint64_t s) {
    rng.clear();
    dur.clear();
    for (int b = 0; b < B; b++) {
      rng.emplace_back(s * 1000003ull + (uint64_t)b);
      dur.emplace_back(s * 7919ull + 31ull * (uint64_t)b + 5ull);
    }
  }
  bool next(int b, const Tree &tr, const Slots &S, int slot, Record *r) {
    if (recorded) {
      if ((size_t)tr.nodes >= rec[(size_t)b].size()) return false;
      *r = rec[(size_t)b][(size_t)tr.nodes];
      return true;
    }
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::mt19937_64 &g = rng[(size_t)b];
    const int depth = S.depth[(size_t)slot];
    const double v = U(g);
    r->ok = tr.nodes < 200 && v > 0.03 + 0.01 * depth;  // deeper nodes close more often; past 200 nodes a tree only closes
    r->iter = 25 * (1 + (int)(U(g) * 16));
    const double inherited = S.lower[(size_t)slot];
    r->lower = (inherited > -1e300 ? inherited : 0.0) + 0.5 * U(g);
    r->int_inf = U(g) < 0.02 + 0.01 * depth ? 0 : 1 + (int)(U(g) * 5);
    r->nextvar = (int)(U(g) * 20);
    r->heur_feasible = U(g) < 0.15;
    r->heur_obj = r->lower + 20.0 * U(g);
    return true;
  }
  int duration(int b) { return 1 + (int)(dur[(size_t)b]() % 8ull); }
};

static void start_trees(Slots &S, std::vector<Tree> &T, const std::vector<double> &upper0, int cap) {
  S.reset(cap);
  for (size_t b = 0; b < T.size(); b++) T[b].start(S, S.take(), upper0[b]);
}

// the wave driver (host_lockstep.inc without the device): one node of every unfinished tree per wave
static int run_waves(Source &src, int B, int rule, int64_t max_iter_bb, const std::vector<double> &upper0, std::vector<Trace> *trace) {
  Slots S;
  std::vector<Tree> T((size_t)B);
  start_trees(S, T, upper0, B + 1);
  trace->assign((size_t)B, Trace());
  for (;;) {
    std::vector<int> live;
    for (int b = 0; b < B; b++)
      if (T[(size_t)b].can_continue(max_iter_bb)) live.push_back(b);
    if (live.empty()) break;
    while (S.free_count() < 2 * live.size()) S.grow(2 * S.cap);
    struct Col { int b, s, c0, c1, rank; };
    std::vector<Col> cols;
    for (int b : live) {
      Col c;
      c.b = b;
      c.rank = (int)T[(size_t)b].choose(S, rule);
      c.s = T[(size_t)b].pop(S, rule);
      c.c0 = S.take();
      c.c1 = S.take();
      cols.push_back(c);
    }
    for (const Col &c : cols) {
      Record r;
      if (!src.next(c.b, T[(size_t)c.b], S, c.s, &r)) return fail("the recorded tree is shorter than the replay (waves)", c.b, (int)T[(size_t)c.b].nodes);
      if (!src.recorded) (void)src.duration(c.b);  // (keeps the two generators of a tree in step with the refill run)
      T[(size_t)c.b].absorb(S, c.s, c.c0, c.c1, r);
      (*trace)[(size_t)c.b].push_back(std::make_pair(c.rank, (int)T[(size_t)c.b].open.size()));
    }
  }
  return 0;
}

// the refill driver (host_refill.inc without the device)
static int run_refill(Source &src, int B, int C, int rule, int64_t max_iter_bb, const std::vector<double> &upper0,
                      std::vector<Trace> *trace, int *chunks_out, int64_t *longest_out, int *grown_out) {
  Slots S;
  std::vector<Tree> T((size_t)B);
  start_trees(S, T, upper0, B + 1);
  Refill R;
  R.reset(C, B);
  trace->assign((size_t)B, Trace());
  std::vector<int> remaining((size_t)C, 0), rank_of((size_t)B, -1), flying((size_t)B, 0);
  std::vector<Record> rec_of((size_t)C);
  std::vector<int64_t> dur_sum((size_t)B, 0);
  std::vector<Fill> fills;
  std::mt19937_64 drec(99);  // durations of recorded nodes: any will do, the trees must not depend on them
  int chunks = 0, grown = 0;
  for (;;) {
    const int want = R.fillable(T, max_iter_bb);
    while (S.free_count() < 2 * (size_t)want) {
      S.grow(2 * S.cap);
      grown++;
    }
    for (int b = 0; b < B; b++)
      rank_of[(size_t)b] = (!R.in_flight[(size_t)b] && T[(size_t)b].can_continue(max_iter_bb)) ? (int)T[(size_t)b].choose(S, rule) : -1;
    std::vector<char> was_busy((size_t)C);
    for (int c = 0; c < C; c++) was_busy[(size_t)c] = R.cols[(size_t)c].tree >= 0;
    fills.clear();
    const int nfill = R.fill(S, T, rule, max_iter_bb, fills);
    if (nfill != want || (int)fills.size() != nfill) return fail("fill() loaded another number of columns than fillable() announced", nfill, want);
    int last_col = -1, last_tree = -1;
    for (const Fill &f : fills) {
      if (f.col < 0 || f.col >= C || was_busy[(size_t)f.col]) return fail("a busy column was filled", f.col, f.tree);
      if (f.col <= last_col || f.tree <= last_tree) return fail("fills are not lowest column first, lowest tree first", f.col, f.tree);
      last_col = f.col;
      last_tree = f.tree;
      if (flying[(size_t)f.tree]) return fail("two nodes of a tree in flight", f.tree, f.col);
      if (rank_of[(size_t)f.tree] < 0) return fail("a tree that could not continue was filled", f.tree, f.col);
      flying[(size_t)f.tree] = 1;
      if (f.warm != S.warm_slot(f.slot)) return fail("wrong warm-start slot", f.slot, f.warm);
      if (f.warm != f.slot && S.kids[(size_t)f.warm] < 1) return fail("a warm-start slot was released before its child ran", f.warm, f.slot);
      Record r;
      if (!src.next(f.tree, T[(size_t)f.tree], S, f.slot, &r)) return fail("the recorded tree is shorter than the replay (refill)", f.tree, (int)T[(size_t)f.tree].nodes);
      rec_of[(size_t)f.col] = r;
      const int d = src.recorded ? 1 + (int)(drec() % 8ull) : src.duration(f.tree);
      remaining[(size_t)f.col] = d;
      dur_sum[(size_t)f.tree] += d;
      (*trace)[(size_t)f.tree].push_back(std::make_pair(rank_of[(size_t)f.tree], -1));
    }
    // the lowest free columns were taken: with trees still waiting, no column may be free
    if (R.fillable(T, max_iter_bb) != 0 && R.busy != C) return fail("a column stays free while a tree waits", R.busy, C);
    {
      // every slot at most once: free, open in one tree, or held by a busy column (node + two children)
      std::set<int> seen;
      size_t total = 0;
      for (int s : S.freelist) { seen.insert(s); total++; }
      for (const Tree &tr : T)
        for (int s : tr.open) { seen.insert(s); total++; }
      int busy = 0;
      for (int c = 0; c < C; c++) {
        const Fill &f = R.cols[(size_t)c];
        if (f.tree < 0) continue;
        busy++;
        if (f.col != c) return fail("a column's record names another column", c, f.col);
        for (int s : {f.slot, f.child0, f.child1}) {
          if (s < 0 || s >= S.cap) return fail("slot out of range", s, c);
          seen.insert(s);
          total++;
        }
      }
      if (seen.size() != total) return fail("a slot is held twice", (int)seen.size(), (int)total);
      if (busy != R.busy) return fail("busy count is off", busy, R.busy);
    }
    if (R.busy == 0) break;
    chunks++;
    for (int c = 0; c < C; c++) {  // the harvest list is in column order
      if (R.cols[(size_t)c].tree < 0 || --remaining[(size_t)c] > 0) continue;
      int b = -1, slot = -1;
      const int c0 = R.cols[(size_t)c].child0, c1 = R.cols[(size_t)c].child1;
      const Verdict v = R.absorb(S, T, c, rec_of[(size_t)c], &b, &slot);
      if (b < 0 || !flying[(size_t)b]) return fail("absorbed a node that was not in flight", b, c);
      flying[(size_t)b] = 0;
      if (v.branch && (S.parent[(size_t)c0] != slot || S.parent[(size_t)c1] != slot)) return fail("children without their parent", b, slot);
      (*trace)[(size_t)b].back().second = (int)T[(size_t)b].open.size();
    }
  }
  bool closed = true;
  for (const Tree &tr : T) closed = closed && tr.open.empty();
  if (closed && S.free_count() != (size_t)S.cap) return fail("slots were not returned", (int)S.free_count(), S.cap);
  if (!closed) {
    size_t open = 0;
    for (const Tree &tr : T) open += tr.open.size();
    // (the open leaves, plus decided parents still held for an open child's warm start)
    if (S.free_count() + open > (size_t)S.cap) return fail("more slots than the store has", (int)S.free_count(), (int)open);
  }
  int64_t longest = 0;
  for (int64_t d : dur_sum) longest = d > longest ? d : longest;
  *chunks_out = chunks;
  *longest_out = longest;
  *grown_out = grown;
  return 0;
}

static int compare(const std::vector<Trace> &a, const std::vector<Trace> &b, const char *what) {
  if (a.size() != b.size()) return fail(what, (int)a.size(), (int)b.size());
  for (size_t t = 0; t < a.size(); t++) {
    if (a[t].size() != b[t].size()) return fail(what, (int)t, -1);
    for (size_t k = 0; k < a[t].size(); k++)
      if (a[t][k] != b[t][k]) return fail(what, (int)t, (int)k);
  }
  return 0;
}

static int one_case(Source &src, uint64_t seed, int B, int width, int rule, int64_t max_iter_bb, const std::vector<double> &upper0,
                    const std::vector<Trace> *expect, int64_t *nodes, int *grown_total) {
  const int C = B < width ? B : width;
  std::vector<Trace> waves, refill;
  if (!src.recorded) src.seed(B, seed);
  if (int rc = run_waves(src, B, rule, max_iter_bb, upper0, &waves)) return rc;
  if (!src.recorded) src.seed(B, seed);
  int chunks = 0, grown = 0;
  int64_t longest = 0;
  if (int rc = run_refill(src, B, C, rule, max_iter_bb, upper0, &refill, &chunks, &longest, &grown)) return rc;
  if (int rc = compare(refill, waves, "the refill driver's trees differ from the wave driver's")) return rc;
  if (expect)
    if (int rc = compare(refill, *expect, "the refill driver's trees differ from the recorded ones")) return rc;
  if (B <= width && chunks != (int)longest) return fail("idle chunks with a column per tree", chunks, (int)longest);
  if (chunks < (int)longest) return fail("fewer chunks than the longest tree needs", chunks, (int)longest);
  for (const Trace &t : refill) *nodes += (int64_t)t.size();
  *grown_total += grown;
  return 0;
}

int main(int argc, char **argv) {
  int64_t nodes = 0;
  int grown = 0, cases = 0;
  const int widths[4] = {1, 3, 64, 64};
  if (argc > 1) {
    // recorded trees: B rule max_iter_bb, then per tree: upper0 count, then count lines
    //   ok iter lower int_inf nextvar heur_feasible heur_obj rank leaves_after
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) return fail("cannot open the recorded trees", 0, 0);
    int B = 0, rule = 0;
    long long cap = 0;
    if (std::fscanf(f, "%d %d %lld", &B, &rule, &cap) != 3 || B < 1) return fail("bad header", B, rule);
    Source src;
    src.recorded = true;
    src.rec.assign((size_t)B, std::vector<Record>());
    std::vector<Trace> expect((size_t)B);
    std::vector<double> upper0((size_t)B);
    for (int b = 0; b < B; b++) {
      int count = 0;
      if (std::fscanf(f, "%lf %d", &upper0[(size_t)b], &count) != 2) return fail("bad tree header", b, 0);
      for (int k = 0; k < count; k++) {
        int ok, iter, int_inf, nextvar, hf, rank, after;
        double lower, hobj;
        if (std::fscanf(f, "%d %d %lf %d %d %d %lf %d %d", &ok, &iter, &lower, &int_inf, &nextvar, &hf, &hobj, &rank, &after) != 9)
          return fail("bad record", b, k);
        Record r;
        r.ok = ok != 0; r.iter = iter; r.lower = lower; r.int_inf = int_inf; r.nextvar = nextvar;
        r.heur_feasible = hf != 0; r.heur_obj = hobj;
        src.rec[(size_t)b].push_back(r);
        expect[(size_t)b].push_back(std::make_pair(rank, after));
      }
    }
    std::fclose(f);
    for (int w = 0; w < 3; w++) {
      if (int rc = one_case(src, 0, B, widths[w], rule, (int64_t)cap, upper0, &expect, &nodes, &grown)) return rc;
      cases++;
    }
  } else {
    for (int round = 0; round < 8; round++) {
      const int rule = round % 4;
      const int64_t max_iter_bb = round == 5 ? 40 : 100000;
      // 1, 3 and 64 trees with a column each; 70 trees on 64 columns; 7 and 70 trees on 1 and 3 columns
      const int Bs[8] = {1, 3, 64, 70, 7, 70, 70, 5};
      const int Ws[8] = {widths[0], widths[1], widths[2], widths[3], 1, 3, 1, 64};
      for (int k = 0; k < 8; k++) {
        const int B = Bs[k];
        std::vector<double> upper0((size_t)B);
        for (int b = 0; b < B; b++) upper0[(size_t)b] = b % 3 == 0 ? 50.0 : NO_UPPER;
        Source src;
        if (int rc = one_case(src, (uint64_t)(round * 8 + k + 1), B, Ws[k], rule, max_iter_bb, upper0, nullptr, &nodes, &grown)) return rc;
        cases++;
      }
    }
  }
  std::printf("refill_fuzz ok: %d cases, %lld nodes, the store grew %d times\n", cases, (long long)nodes, grown);
  return 0;
}
