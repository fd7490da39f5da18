// Stand-alone program (its own main; built with -fsanitize=address,undefined by tests/test_solve_trees_sb_cpu.py): the
// decisions of strong and reliability branching inside the one-launch trees -- miosqp_amd/csrc/tree_sb_logic.hpp, which
// the kernels include -- side by side with lockstep::SbTree (lockstep_sb.hpp), the restatement that recorded trees pin,
// over random sequences of asks, child outcomes and solved nodes.  Every chosen position, score, pc_sum and pc_cnt must
// be equal bit for bit.  Rules 1 and 2; K in {1, 8, 32}; p in {1, 7, 130} (130: the pairwise sum beyond 128);
// reliability 0, 1, 4; ties in fractions and in scores; children without a value.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../miosqp_amd/csrc/lockstep_sb.hpp"
#include "../miosqp_amd/csrc/tree_sb_logic.hpp"

namespace sbl = miosqp::tree_sb;
namespace ls = miosqp::lockstep;

static long g_asks = 0, g_decides = 0, g_solved = 0, g_ties_f = 0, g_ties_s = 0, g_novalue = 0, g_big_mean = 0;

static bool same(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

#define REQUIRE(cond, ...)                      \
  do {                                          \
    if (!(cond)) {                              \
      std::printf("FAILED %s: ", #cond);        \
      std::printf(__VA_ARGS__);                 \
      std::printf("\n");                        \
      return 1;                                 \
    }                                           \
  } while (0)

static int compare_state(const sbl::View &v, const ls::SbTree &t, const char *when) {
  for (int k = 0; k < 2 * v.p; k++) {
    REQUIRE(same(v.pc_sum[k], t.pc_sum[(size_t)k]), "%s pc_sum[%d] %.17g vs %.17g", when, k, v.pc_sum[k], t.pc_sum[(size_t)k]);
    REQUIRE(v.pc_cnt[k] == (long long)t.pc_cnt[(size_t)k], "%s pc_cnt[%d]", when, k);
  }
  return 0;
}

static int run(int rule, int K, int p, int reliability, unsigned seed) {
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  const int cap = 24;  // leaf-store places
  // exactly sized buffers: the sanitizer sees every step outside
  std::vector<double> work(sbl::work_doubles(p)), pc((size_t)cap * sbl::PC_DOUBLES);
  const sbl::View v = sbl::view(work.data(), p);
  const sbl::Par par{rule, K, reliability, 1e-6, 1e-6};
  const ls::SbParams lpar{rule, K, reliability, 1e-6, 1e-6};
  ls::SbTree t;
  ls::SbSlots P;
  t.start(p);
  P.reset(cap);
  sbl::start(v);
  for (int s = 0; s < cap; s++) pc[(size_t)s * sbl::PC_DOUBLES + 3] = -1.0;
  if (rule == 2 && p > 129)  // every position but the first observed downwards from the start: the first gets the mean
    for (int k = 1; k < p; k++) {  // over more than 128 of them
      const double delta = U(rng), f = 0.1 + 0.8 * U(rng);
      t.record_gain(k, 0, delta, f);
      sbl::record_gain(v, k, 0, delta, f);
    }
  std::vector<double> x((size_t)p);
  std::vector<ls::SbChild> ch;
  for (int step = 0; step < 160; step++) {
    const int slot = (int)(rng() % (unsigned)cap);
    // ---- the node's own solve is an observation (rule 2), also when the node is then pruned or infeasible ----
    const bool ok = U(rng) < 0.85;
    const double lower = 10.0 * U(rng) - 2.0;
    t.node_solved(P, slot, ok, lower);
    sbl::node_solved(v, pc.data(), slot, ok, lower);
    g_solved++;
    if (compare_state(v, t, "node_solved")) return 1;
    if (!ok || U(rng) < 0.2) continue;  // no x, or pruned: nothing is asked
    // ---- the node's x: fractions from a small set (ties), some integral, some a hair beside an integer ----
    const int mode = step % 4;
    for (int k = 0; k < p; k++) {
      const double base = (double)((int)(rng() % 7) - 3);
      double f;
      if (mode == 0) f = U(rng);
      else if (mode == 1) f = 0.125 * (double)(rng() % 8);      // exact ties, integral entries among them
      else if (mode == 2) f = (rng() % 2) ? 0.5 : 0.25;          // everything tied at two levels
      else f = (rng() % 3 == 0) ? 0.0 : U(rng);
      if (step % 11 == 3 && k % 5 == 0) f = 5e-7;                // below eps_int_feas: not fractional
      x[(size_t)k] = base + f;
    }
    if (step % 9 == 0) x[(size_t)(rng() % (unsigned)p)] += 0.5;  // at least one fractional entry now and then
    for (int k = 0; k < p; k++) v.x[k] = x[(size_t)k];
    int pos_l = t.ask(lpar, x.data());
    int pos_d = sbl::ask(v, par);
    g_asks++;
    REQUIRE(pos_l == pos_d, "ask %d vs %d (rule %d K %d p %d step %d)", pos_d, pos_l, rule, K, p, step);
    if (pos_l == -2) continue;
    REQUIRE(v.count[0] == (int)t.frac.size(), "fractional set %d vs %zu", v.count[0], t.frac.size());
    for (int i = 0; i < v.count[0]; i++) REQUIRE(v.frac[i] == t.frac[(size_t)i], "frac[%d]", i);
    {
      int tie = 0;
      for (size_t i = 1; i < t.frac.size(); i++)
        if (sbl::fraction(x[(size_t)t.frac[i]]) == sbl::fraction(x[(size_t)t.frac[i - 1]])) tie = 1;
      g_ties_f += tie;
    }
    const double node_lower = lower;
    if (pos_l == -1) {
      const int Kc = (int)t.cand.size();
      REQUIRE(v.count[1] == Kc, "candidates %d vs %d", v.count[1], Kc);
      for (int j = 0; j < Kc; j++) REQUIRE(v.cand[j] == t.cand[(size_t)j], "cand[%d] %d vs %d", j, v.cand[j], t.cand[(size_t)j]);
      ch.assign((size_t)(2 * Kc), ls::SbChild{});
      const int cmode = (int)(rng() % 4);
      for (int b = 0; b < 2 * Kc; b++) {
        ls::SbChild &c = ch[(size_t)b];
        c.has_x = U(rng) < 0.85;
        c.iter = 25 * (1 + (int)(rng() % 2));
        if (cmode == 0) c.lower = node_lower + U(rng);
        else if (cmode == 1) c.lower = node_lower + 0.25 * (double)(rng() % 3);  // ties in the scores, gains of exactly 0
        else if (cmode == 2) c.lower = node_lower - U(rng) * 0.1;               // below the node: gain 0, score eps * eps
        else c.lower = node_lower + ((rng() % 2) ? 1.0 : 0.5);
        if (!c.has_x) {
          c.lower = std::numeric_limits<double>::quiet_NaN();
          g_novalue++;
        }
        v.ch_has[b] = c.has_x ? 1 : 0;
        v.ch_iter[b] = c.iter;
        v.ch_lower[b] = c.lower;
      }
      const int64_t it0 = t.iters;
      int chosen = -1, iters = 0;
      pos_l = t.decide(lpar, x.data(), node_lower, ch.data(), &chosen);
      pos_d = sbl::decide(v, par, node_lower, &iters);
      g_decides++;
      REQUIRE(pos_l == pos_d, "decide %d vs %d (rule %d K %d p %d step %d)", pos_d, pos_l, rule, K, p, step);
      REQUIRE((int64_t)iters == t.iters - it0, "iterations %d", iters);
      int tie = 0;
      for (int j = 0; j < Kc; j++) {
        REQUIRE(same(v.score[j], t.score[(size_t)j]), "score[%d] %.17g vs %.17g", j, v.score[j], t.score[(size_t)j]);
        for (int i = 0; i < j; i++)
          if (t.score[(size_t)i] == t.score[(size_t)j]) tie = 1;
      }
      g_ties_s += tie;
      if (compare_state(v, t, "decide")) return 1;
    }
    REQUIRE(pos_l >= 0 && pos_l < p, "position %d", pos_l);
    if (rule == 2) {
      int have = 0;
      for (int k = 0; k < p; k++) have += t.pc_cnt[(size_t)k] > 0;
      if (have > 128) g_big_mean++;
    }
    // ---- the two children remember the branching ----
    int c0 = (int)(rng() % (unsigned)cap), c1 = (int)(rng() % (unsigned)cap);
    if (c1 == c0) c1 = (c0 + 1) % cap;
    t.branched(lpar, P, c0, c1, pos_l, x.data(), node_lower);
    sbl::branched(par, pc.data(), c0, c1, pos_l, x[(size_t)pos_l], node_lower);
    for (int s = 0; s < cap; s++) {
      const double *r = pc.data() + (size_t)s * sbl::PC_DOUBLES;
      REQUIRE((r[3] >= 0.0) == (P.has[(size_t)s] != 0), "Node.pc of place %d", s);
      if (P.has[(size_t)s])
        REQUIRE(same(r[0], P.lp[(size_t)s]) && same(r[1], P.f[(size_t)s]) && (int)r[2] == P.pos[(size_t)s] && (int)r[3] == P.side[(size_t)s],
                "Node.pc of place %d differs", s);
    }
  }
  return 0;
}

int main() {
  // the pairwise sum against the recursive restatement, around every split
  {
    std::mt19937_64 rng(7);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    std::vector<double> a(1500);
    for (double &d : a) d = U(rng) * 1e3;
    for (size_t n = 0; n <= a.size(); n++) {
      std::vector<double> b(a.begin(), a.begin() + (long)n);  // exactly sized
      const double want = ls::np_pairwise_sum(b.data(), n), got = sbl::pairwise_sum(b.data(), n);
      if (!same(want, got)) {
        std::printf("FAILED pairwise_sum at n = %zu: %.17g vs %.17g\n", n, got, want);
        return 1;
      }
    }
  }
  unsigned seed = 1;
  int runs = 0;
  for (int rule = 1; rule <= 2; rule++)
    for (int K : {1, 8, 32})
      for (int p : {1, 7, 130})
        for (int rel : {0, 1, 4})
          for (int rep = 0; rep < 3; rep++) {
            if (run(rule, K, p, rel, seed++)) return 1;
            runs++;
          }
  if (!(g_ties_f > 0 && g_ties_s > 0 && g_novalue > 0 && g_big_mean > 0 && g_decides > 0)) {
    std::printf("FAILED coverage: fraction ties %ld, score ties %ld, children without a value %ld, means beyond 128 %ld\n", g_ties_f,
                g_ties_s, g_novalue, g_big_mean);
    return 1;
  }
  std::printf("tree_sb ok: %d runs, %ld asks, %ld decides, %ld solved nodes; ties in fractions %ld, in scores %ld, children "
              "without a value %ld, means over more than 128 positions %ld\n",
              runs, g_asks, g_decides, g_solved, g_ties_f, g_ties_s, g_novalue, g_big_mean);
  return 0;
}
