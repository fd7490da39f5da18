// Test-only C wrapper over miosqp_amd/csrc/lockstep_ahead.hpp (the host logic of the lock-step trees whose spare columns
// solve open leaves early): tests/test_lockstep_ahead_cpu.py compiles it with g++ and replays recorded trees through it.
// The wave loop here is host_lockstep_ahead.inc's without the device.  A node is known by its PATH from the root ('0':
// the child with the lowered upper bound, '1': the other).  The nodes a recorded tree visited answer with their recorded
// record; every other node -- it can only be solved ahead and must never be absorbed -- answers with an ADVERSARIAL record
// drawn from a seed: infeasible, integral with a tiny objective, crossed, huge iteration counts.  An ahead column is
// finished iff ceil(iter / check_termination) <= the largest such count among the wave's mandatory columns.
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../miosqp_amd/csrc/lockstep_ahead.hpp"

using namespace miosqp::lockstep;

namespace {

struct Logged {
  std::string path;
  int index, open_after, hit;  // the index `choose` gave in the open list; the list's length after the absorb
  double upper_after;
};

struct Harness {
  int B = 0;
  std::vector<double> upper0;
  std::vector<std::map<std::string, Record>> known;  // per tree: the recorded nodes
  // a run
  Slots slots;
  std::vector<Tree> trees;
  Ahead logic;
  std::vector<std::string> path;  // per slot
  std::vector<std::vector<Logged>> log;
  int waves = 0, grown = 0, error = 0;
  int64_t mandatory_chunks = 0, columns = 0;
  std::vector<int> wave_width;
};

uint64_t mix(uint64_t x) {
  x += 0x9e3779b97f4a7c15ull;
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

uint64_t hash_path(const std::string &p, uint64_t seed) {
  uint64_t h = mix(seed);
  for (char c : p) h = mix(h ^ (uint64_t)(unsigned char)c);
  return h;
}

// a record meant to do damage if it were ever absorbed
AheadOutcome adversarial(const std::string &p, uint64_t seed, int tree) {
  const uint64_t h = hash_path(p, seed + 977u * (uint64_t)tree);
  AheadOutcome o;
  o.finished = true;
  o.crossed = false;
  o.r.ok = true;
  o.r.iter = 1 + (int)(h % 37);
  o.r.lower = -1e9;
  o.r.int_inf = 3;
  o.r.nextvar = (int)((h >> 8) % 11);
  o.r.heur_feasible = false;
  o.r.heur_obj = 0.0;
  switch ((h >> 16) % 5) {
    case 0:  // infeasible
      o.r.ok = false;
      o.r.int_inf = o.r.nextvar = -1;
      break;
    case 1:  // integral with a tiny objective: it would become the incumbent and prune everything
      o.r.int_inf = 0;
      o.r.lower = -1e12;
      break;
    case 2:  // fractional and crossed: absorbing it would be an error
      o.crossed = true;
      break;
    case 3:  // fractional with a rounded point that would become the incumbent, and a huge iteration count
      o.r.heur_feasible = true;
      o.r.heur_obj = -1e12;
      o.r.iter = 1 << 28;
      break;
    default:  // fractional with a very low bound: best-bound rules would love its children
      break;
  }
  return o;
}

}  // namespace

extern "C" {

void *lah_new(int ntrees, const double *upper0) {
  Harness *h = new Harness();
  h->B = ntrees;
  h->upper0.assign(upper0, upper0 + ntrees);
  h->known.resize((size_t)ntrees);
  return h;
}

void lah_free(void *p) { delete static_cast<Harness *>(p); }

// a node the recorded tree `t` visited
void lah_add_node(void *p, int t, const char *path, int ok, int iter, double lower, int int_inf, int nextvar, int heur_feasible,
                  double heur_obj) {
  Harness *h = static_cast<Harness *>(p);
  Record r;
  r.ok = ok != 0;
  r.iter = iter;
  r.lower = lower;
  r.int_inf = int_inf;
  r.nextvar = nextvar;
  r.heur_feasible = heur_feasible != 0;
  r.heur_obj = heur_obj;
  h->known[(size_t)t][std::string(path)] = r;
}

// The whole run.  Returns 0, or: 1 a mandatory column outside the recorded set, 2 an absorbed record that was crossed,
// 3 a slot in two places or lost, 4 an ahead column on a node that holds a record already, 5 a wave wider than its tiles.
int lah_run(void *p, int rule, int64_t max_iter_bb, int ahead, int capacity, int check_termination, uint64_t seed) {
  Harness *h = static_cast<Harness *>(p);
  const int B = h->B, ct = check_termination;
  int cap = capacity;
  h->grown = 0;
  while (cap < B) {
    cap *= 2;
    h->grown++;
  }
  h->slots.reset(cap);
  h->trees.assign((size_t)B, Tree());
  h->logic.reset(cap, B);
  h->path.assign((size_t)cap, std::string());
  h->log.assign((size_t)B, std::vector<Logged>());
  h->waves = 0;
  h->mandatory_chunks = h->columns = 0;
  h->wave_width.clear();
  h->error = 0;
  for (int t = 0; t < B; t++) {
    const int s = h->slots.take();
    h->path[(size_t)s].clear();
    h->trees[(size_t)t].start(h->slots, s, h->upper0[(size_t)t]);
  }
  std::vector<int> live;
  std::vector<AheadColumn> cols;
  std::vector<AheadOutcome> out;
  for (;;) {
    live.clear();
    for (int t = 0; t < B; t++)
      if (h->trees[(size_t)t].can_continue(max_iter_bb)) live.push_back(t);
    if (live.empty()) break;
    const int L = (int)live.size();
    const int free_cols = ahead > 1 ? 64 * ((L + 63) / 64) - L : 0;
    while (h->slots.free_count() < 2 * (size_t)(L + free_cols)) {
      h->slots.grow(2 * h->slots.cap);
      h->logic.grow(h->slots.cap);
      h->path.resize((size_t)h->slots.cap);
      h->grown++;
    }
    // (the index `choose` gives the mandatory leaf, before plan pops it)
    std::vector<int> index((size_t)L);
    for (int c = 0; c < L; c++) index[(size_t)c] = (int)h->trees[(size_t)live[(size_t)c]].choose(h->slots, rule);
    h->logic.plan(h->slots, h->trees, live, rule, ahead, free_cols, cols);
    const int W = (int)cols.size();
    if (W > 64 * ((L + 63) / 64)) return h->error = 5;
    h->waves++;
    h->wave_width.push_back(W);
    h->columns += W;
    out.assign((size_t)W, AheadOutcome());
    int chunks = 0;
    for (int c = 0; c < W; c++) {
      const AheadColumn &col = cols[(size_t)c];
      const std::string &pth = h->path[(size_t)col.slot];
      h->path[(size_t)col.c0] = pth + "0";
      h->path[(size_t)col.c1] = pth + "1";
      if (!col.mandatory && h->logic.has[(size_t)col.slot]) return h->error = 4;
      const std::map<std::string, Record> &kn = h->known[(size_t)col.tree];
      const auto it = kn.find(pth);
      AheadOutcome &o = out[(size_t)c];
      if (it != kn.end()) {
        o.r = it->second;
        o.crossed = false;
        o.finished = true;
      } else if (col.mandatory) {
        return h->error = 1;
      } else {
        o = adversarial(pth, seed, col.tree);
      }
      if (col.mandatory) {
        const int k = (o.r.iter + ct - 1) / ct;
        chunks = k > chunks ? k : chunks;
      }
    }
    h->mandatory_chunks += chunks;
    for (int c = L; c < W; c++) {  // the call-off model
      AheadOutcome &o = out[(size_t)c];
      if ((o.r.iter + ct - 1) / ct > chunks) {
        o.finished = false;
        o.r.iter = chunks * ct;
      }
    }
    std::vector<Tree> &T = h->trees;
    std::vector<int> mand_index((size_t)B, -1);
    for (int c = 0; c < L; c++) mand_index[(size_t)cols[(size_t)c].tree] = index[(size_t)c];
    const bool ok = h->logic.settle(h->slots, T, cols, out, rule, max_iter_bb, h->waves, [&](const AheadEvent &ev) {
      if (ev.v.branch && ev.crossed) return false;
      Logged g;
      g.path = h->path[(size_t)ev.slot];
      g.index = ev.hit ? ev.index : mand_index[(size_t)ev.tree];
      g.open_after = (int)T[(size_t)ev.tree].open.size();
      g.hit = ev.hit ? 1 : 0;
      g.upper_after = T[(size_t)ev.tree].upper;
      h->log[(size_t)ev.tree].push_back(g);
      return true;
    });
    if (!ok) return h->error = 2;
    // every slot exactly once: free, open, reserved below a record, or held by a decided parent for its children
    std::vector<int> seen((size_t)h->slots.cap, 0);
    for (int s : h->slots.freelist) seen[(size_t)s]++;
    for (const Tree &tr : T)
      for (int s : tr.open) seen[(size_t)s]++;
    for (int s = 0; s < h->slots.cap; s++)
      if (h->logic.has[(size_t)s]) {
        seen[(size_t)h->logic.c0[(size_t)s]]++;
        seen[(size_t)h->logic.c1[(size_t)s]]++;
      }
    for (int s = 0; s < h->slots.cap; s++) {
      const bool held = h->slots.decided[(size_t)s] && h->slots.kids[(size_t)s] > 0;
      if (seen[(size_t)s] != (held ? 0 : 1)) return h->error = 3;
    }
  }
  h->logic.finish(h->slots);
  return 0;
}

// after a run: every slot is free, an open leaf, or the decided parent of an undecided child (nothing reserved is left)
int lah_slots_complete(void *p) {
  Harness *h = static_cast<Harness *>(p);
  std::vector<int> seen((size_t)h->slots.cap, 0);
  for (int s : h->slots.freelist) seen[(size_t)s]++;
  for (const Tree &tr : h->trees)
    for (int s : tr.open) seen[(size_t)s]++;
  for (int s = 0; s < h->slots.cap; s++) {
    if (h->logic.has[(size_t)s]) return 0;
    const bool held = h->slots.decided[(size_t)s] && h->slots.kids[(size_t)s] > 0;
    if (seen[(size_t)s] != (held ? 0 : 1)) return 0;
  }
  return 1;
}

int lah_waves(void *p) { return static_cast<Harness *>(p)->waves; }
int lah_grown(void *p) { return static_cast<Harness *>(p)->grown; }
int lah_wave_width(void *p, int w) { return static_cast<Harness *>(p)->wave_width[(size_t)w]; }
int64_t lah_mandatory_chunks(void *p) { return static_cast<Harness *>(p)->mandatory_chunks; }
int64_t lah_columns(void *p) { return static_cast<Harness *>(p)->columns; }
// 0 sent, 1 hits, 2 discarded, 3 called off, 4 .. 7 their iterations
int64_t lah_count(void *p, int what) {
  const AheadCounts &n = static_cast<Harness *>(p)->logic.n;
  const int64_t v[8] = {n.sent, n.hits, n.discarded, n.called_off, n.sent_iters, n.hit_iters, n.discarded_iters, n.called_off_iters};
  return v[what];
}
int lah_free_slots(void *p) { return (int)static_cast<Harness *>(p)->slots.free_count(); }
int lah_cap(void *p) { return static_cast<Harness *>(p)->slots.cap; }

int lah_log_len(void *p, int t) { return (int)static_cast<Harness *>(p)->log[(size_t)t].size(); }
// absorb k of tree t: its path into buf (room for len bytes), the other fields through the pointers
void lah_log(void *p, int t, int k, char *buf, int len, int *index, int *open_after, int *hit, double *upper_after) {
  const Logged &g = static_cast<Harness *>(p)->log[(size_t)t][(size_t)k];
  std::strncpy(buf, g.path.c_str(), (size_t)len - 1);
  buf[len - 1] = 0;
  *index = g.index;
  *open_after = g.open_after;
  *hit = g.hit;
  *upper_after = g.upper_after;
}

int lah_open(void *p, int t) { return (int)static_cast<Harness *>(p)->trees[(size_t)t].open.size(); }
int lah_max_open(void *p, int t) { return (int)static_cast<Harness *>(p)->trees[(size_t)t].max_open; }
int lah_found(void *p, int t) { return static_cast<Harness *>(p)->trees[(size_t)t].found ? 1 : 0; }
int lah_finished_at(void *p, int t) { return static_cast<Harness *>(p)->trees[(size_t)t].finished_at; }
double lah_upper(void *p, int t) { return static_cast<Harness *>(p)->trees[(size_t)t].upper; }
double lah_lower_glob(void *p, int t) {
  Harness *h = static_cast<Harness *>(p);
  return h->trees[(size_t)t].lower_glob(h->slots);
}
int64_t lah_nodes(void *p, int t) { return static_cast<Harness *>(p)->trees[(size_t)t].nodes; }
int64_t lah_iters(void *p, int t) { return static_cast<Harness *>(p)->trees[(size_t)t].iters; }

}  // extern "C"
