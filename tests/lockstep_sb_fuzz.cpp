// Stand-alone fuzz program over miosqp_amd/csrc/lockstep_sb.hpp and lockstep_trees.hpp (its own main; built by
// tests/test_lockstep_sb_cpu.py with -fsanitize=address,undefined): random records, random x at the integer positions
// and random children's outcomes through several trees sharing one free list, growth included, under both rules.
// Checked on the way: the candidates are ascending fractional positions, at most K of them; the chosen position is
// fractional; the counters add up; the observation counts only grow; every slot comes back when the trees close.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../miosqp_amd/csrc/lockstep_sb.hpp"

using namespace miosqp::lockstep;

#define CHECK(c)                                                 \
  do {                                                           \
    if (!(c)) {                                                  \
      fprintf(stderr, "check failed: %s (line %d)\n", #c, __LINE__); \
      return 1;                                                  \
    }                                                            \
  } while (0)

static int run(unsigned seed, int rule) {
  std::mt19937 rng(seed);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  const int B = 1 + (int)(rng() % 6), p = 1 + (int)(rng() % 40), K = 1 + (int)(rng() % 32);
  const int explor = (int)(rng() % 4);
  const int64_t max_iter_bb = 5 + (int64_t)(rng() % 60);
  const SbParams sp{rule, K, (int)(rng() % 5), 1e-6, 1e-6};
  Slots S;
  SbSlots P;
  int cap = 2;
  while (cap < B) cap *= 2;
  S.reset(cap);
  P.reset(cap);
  std::vector<Tree> T((size_t)B);
  std::vector<SbTree> Q((size_t)B);
  for (int b = 0; b < B; b++) {
    T[(size_t)b].start(S, S.take(), rng() % 3 == 0 ? 100.0 * U(rng) : NO_UPPER);
    Q[(size_t)b].start(p);
  }
  std::vector<double> x((size_t)p);
  std::vector<SbChild> ch;
  std::vector<int64_t> cnt_before;
  for (int wave = 0; wave < 200; wave++) {
    std::vector<int> live;
    for (int b = 0; b < B; b++)
      if (T[(size_t)b].can_continue(max_iter_bb)) live.push_back(b);
    if (live.empty()) break;
    while (S.free_count() < 2 * live.size()) {
      S.grow(2 * S.cap);
      P.grow(S.cap);
    }
    struct Col { int b, s, c0, c1; };
    std::vector<Col> cols;
    for (int b : live) {
      Col c;
      c.b = b;
      c.s = T[(size_t)b].pop(S, explor);
      c.c0 = S.take();
      c.c1 = S.take();
      cols.push_back(c);
    }
    for (const Col &c : cols) {
      Tree &t = T[(size_t)c.b];
      SbTree &q = Q[(size_t)c.b];
      Record r;
      r.ok = rng() % 8 != 0;
      r.iter = 25 * (1 + (int)(rng() % 8));
      r.lower = S.lower[(size_t)c.s] > -1e300 ? S.lower[(size_t)c.s] + U(rng) : 10.0 * U(rng);
      int nfrac = 0;
      for (int k = 0; k < p; k++) {
        x[(size_t)k] = rng() % 3 == 0 ? (double)(rng() % 3) + U(rng) : (double)(rng() % 3);
        if (std::fabs(x[(size_t)k] - std::nearbyint(x[(size_t)k])) > sp.eps_int) nfrac++;
      }
      r.int_inf = nfrac;
      r.nextvar = 0;
      r.heur_feasible = rng() % 4 == 0;
      r.heur_obj = r.lower + 2.0 * U(rng);
      cnt_before = q.pc_cnt;
      q.node_solved(P, c.s, r.ok, r.lower);
      const Verdict v = t.begin(S, c.s, r, 0).v;
      if (v.branch) {
        CHECK(nfrac > 0);
        int pos = q.ask(sp, x.data());
        CHECK(pos != -2);
        CHECK((int)q.frac.size() == nfrac);
        if (pos == -1) {
          const int Kc = (int)q.cand.size();
          CHECK(Kc >= 1 && Kc <= K);
          for (int j = 0; j < Kc; j++) {
            CHECK(j == 0 || q.cand[(size_t)j] > q.cand[(size_t)j - 1]);
            CHECK(std::fabs(x[(size_t)q.cand[(size_t)j]] - std::nearbyint(x[(size_t)q.cand[(size_t)j]])) > sp.eps_int);
          }
          ch.resize((size_t)(2 * Kc));
          const int64_t calls = q.calls, kids = q.children, its = q.iters;
          int64_t sum = 0;
          for (SbChild &k : ch) {
            k.has_x = rng() % 5 != 0;
            k.iter = 25 * (1 + (int)(rng() % 2));
            k.lower = k.has_x ? r.lower - 0.1 + U(rng) : std::nan("");
            sum += k.iter;
          }
          int best = -1;
          pos = q.decide(sp, x.data(), r.lower, ch.data(), &best);
          CHECK(best >= 0 && best < Kc);
          CHECK(q.calls == calls + 1 && q.children == kids + 2 * Kc && q.iters == its + sum);
          if (rule == 1) CHECK(pos == q.cand[(size_t)best]);
        } else if (rule == 1) {
          CHECK(nfrac == 1);
        }
        CHECK(pos >= 0 && pos < p);
        CHECK(std::fabs(x[(size_t)pos] - std::nearbyint(x[(size_t)pos])) > sp.eps_int);
        q.branched(sp, P, c.c0, c.c1, pos, x.data(), r.lower);
        CHECK(P.has[(size_t)c.c0] == (rule == 2) && P.f[(size_t)c.c0] > 0.0 && P.f[(size_t)c.c1] > 0.0);
      }
      for (size_t k = 0; k < q.pc_cnt.size(); k++) {
        CHECK(q.pc_cnt[k] >= cnt_before[k]);
        CHECK(rule == 2 || q.pc_cnt[k] == 0);
        CHECK(q.pc_sum[k] >= 0.0);
      }
      t.end(S, c.s, c.c0, c.c1, v);
    }
  }
  bool closed = true;
  for (const Tree &t : T) closed = closed && t.open.empty();
  if (closed) CHECK((int)S.free_count() == S.cap);
  return 0;
}

int main() {
  // the restated summation at the sizes where numpy's takes another branch: exact on small integers
  for (size_t n : {(size_t)1, (size_t)7, (size_t)8, (size_t)9, (size_t)127, (size_t)128, (size_t)129, (size_t)300, (size_t)1000}) {
    std::vector<double> a(n);
    for (size_t i = 0; i < n; i++) a[i] = (double)(i % 17);
    double s = 0.0;
    for (double v : a) s += v;
    CHECK(np_pairwise_sum(a.data(), n) == s);
  }
  for (unsigned seed = 0; seed < 300; seed++)
    for (int rule = 1; rule <= 2; rule++)
      if (run(seed, rule)) {
        fprintf(stderr, "seed %u rule %d\n", seed, rule);
        return 1;
      }
  printf("lockstep_sb_fuzz ok\n");
  return 0;
}
