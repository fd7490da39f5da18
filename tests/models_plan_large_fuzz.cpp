// Stand-alone program over miosqp_amd/csrc/models_plan.hpp as miosqp_qp_solve_trees_models_large drives it (built with
// -fsanitize=address,undefined by tests/test_tree_reduced_cpu.py and run as a subprocess), next to models_plan_fuzz.cpp:
// the leaf_cap check, a model listed twice, and the arena layout on random lists that MIX the three forms -- table
// entries wave, group, reduced, each in the caller's order; the leaf store of a reduced-form model with leaf_cap places,
// every other one with tree_cap; every array inside the arena, no two overlapping --, a list without a reduced-form model
// laid out exactly as the three-argument plan lays it out, and the arena refusal naming the model at which the limit is
// reached.
#include <algorithm>
#include <cstdio>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "../miosqp_amd/csrc/models_plan.hpp"

namespace mm = miosqp::models;

static int fails = 0;
#define EXPECT(c)                                            \
  do {                                                       \
    if (!(c)) {                                              \
      std::printf("line %d: %s\n", __LINE__, #c);            \
      fails++;                                               \
    }                                                        \
  } while (0)

static void checks() {
  std::string err;
  EXPECT(mm::check_leaf_cap(1, err) == mm::ERR_ARG && err.find("at least 2") != std::string::npos);
  EXPECT(mm::check_leaf_cap(0, err) == mm::ERR_ARG && mm::check_leaf_cap(-5, err) == mm::ERR_ARG);
  EXPECT(mm::check_leaf_cap(2, err) == 0 && mm::check_leaf_cap(256, err) == 0 && mm::check_leaf_cap(1024, err) == 0);
  // a model listed twice, in a call whose shapes differ per model
  const int B = 4;
  int eng[B] = {0, 0, 0, 0}, M[B] = {3, 9, 5, 7}, rule[B] = {0, 1, 2, 3}, mi[B] = {10, 10, 10, 10};
  std::vector<std::vector<double>> q, l, u, x0, y0, xo;
  std::vector<const void *> pe, pxo;
  std::vector<const double *> pq, pl, pu, px0, py0, pinc(B, nullptr);
  std::vector<double> up(B, 1e300);
  for (int b = 0; b < B; b++) {
    q.emplace_back(4 + b, 0.0); x0.emplace_back(4 + b, 0.0); xo.emplace_back(4 + b, 0.0);
    l.emplace_back(M[b], -1.0); u.emplace_back(M[b], 1.0); y0.emplace_back(M[b], 0.0);
  }
  for (int b = 0; b < B; b++) {
    pe.push_back(&eng[b]); pxo.push_back(xo[b].data()); pq.push_back(q[b].data()); pl.push_back(l[b].data());
    pu.push_back(u[b].data()); px0.push_back(x0[b].data()); py0.push_back(y0[b].data());
  }
  int info = 0, stats = 0;
  auto run = [&]() {
    return mm::check_args(B, pe.data(), M, pq.data(), pl.data(), pu.data(), px0.data(), py0.data(), up.data(), pinc.data(), rule,
                          mi, pxo.data(), &info, &stats, err);
  };
  EXPECT(run() == 0);
  pe[2] = pe[0];
  EXPECT(run() == mm::ERR_ARG && err.find("model 0") != std::string::npos && err.find("model 2") != std::string::npos);
}

static void layouts() {
  std::mt19937 rng(4711);
  const size_t caps[] = {2, 256, 1024};
  for (int trial = 0; trial < 150; trial++) {
    const int B = 1 + (int)(rng() % 30);
    const size_t entry = 8 * (1 + rng() % 200), tree_cap = 1 + rng() % 64, leaf_cap = caps[rng() % 3];
    const bool no_reduced = trial % 5 == 0;
    std::vector<mm::Shape> sh;
    for (int b = 0; b < B; b++) {
      const int n = 1 + (int)(rng() % 70), p = 1 + (int)(rng() % n), M = p + (int)(rng() % 600);
      sh.push_back(mm::Shape{n, M, p, (int)(rng() % (no_reduced ? 2 : 3)) + 1});
    }
    const mm::Plan P = mm::plan(sh, entry, tree_cap, leaf_cap);
    EXPECT((int)P.slot.size() == B && P.n1 + P.n2 + P.n3 == B);
    if (no_reduced) {  // the existing entry's layout, field by field
      const mm::Plan Q = mm::plan(sh, entry, tree_cap);
      EXPECT(Q.n1 == P.n1 && Q.n2 == P.n2 && P.n3 == 0 && Q.total_doubles == P.total_doubles && Q.up_doubles == P.up_doubles &&
             Q.down_off == P.down_off && Q.down_doubles == P.down_doubles && Q.table_doubles == P.table_doubles);
      for (int b = 0; b < B; b++) {
        const mm::Slot &s = P.slot[b], &t = Q.slot[b];
        EXPECT(s.entry == t.entry && s.raw == t.raw && s.qraw == t.qraw && s.inc == t.inc && s.out == t.out && s.q == t.q &&
               s.lf_lo == t.lf_lo && s.lf_hi == t.lf_hi && s.lf_x == t.lf_x && s.lf_y == t.lf_y);
      }
    }
    EXPECT(P.table_doubles * 8 >= (size_t)B * entry);
    EXPECT(P.down_off + P.down_doubles == P.up_doubles && P.up_doubles <= P.total_doubles && P.down_off % 2 == 0);
    std::vector<std::pair<size_t, size_t>> iv;
    iv.push_back({0, P.table_doubles});
    std::vector<int> seen(B, 0);
    int last[4] = {-1, -1, -1, -1};
    size_t leaf_total = 0;
    for (int b = 0; b < B; b++) {
      const mm::Slot &s = P.slot[b];
      const size_t n = sh[b].n, M = sh[b].M, p = sh[b].p, cap = sh[b].form == 3 ? leaf_cap : tree_cap;
      EXPECT(s.entry >= 0 && s.entry < B);
      if (s.entry >= 0 && s.entry < B) seen[s.entry]++;
      const int lo = sh[b].form == 1 ? 0 : sh[b].form == 2 ? P.n1 : P.n1 + P.n2;
      const int hi = sh[b].form == 1 ? P.n1 : sh[b].form == 2 ? P.n1 + P.n2 : B;
      EXPECT(s.entry >= lo && s.entry < hi && s.entry > last[sh[b].form]);  // the caller's order inside a form
      last[sh[b].form] = s.entry;
      iv.push_back({s.raw, s.raw + 3 * M + n});
      iv.push_back({s.qraw, s.qraw + n});
      iv.push_back({s.inc, s.inc + n});
      iv.push_back({s.out, s.out + mm::OUT_DOUBLES});
      iv.push_back({s.q, s.q + n});
      iv.push_back({s.lf_lo, s.lf_lo + cap * p});
      iv.push_back({s.lf_hi, s.lf_hi + cap * p});
      iv.push_back({s.lf_x, s.lf_x + cap * n});
      iv.push_back({s.lf_y, s.lf_y + cap * M});
      leaf_total += cap * (2 * p + n + M);
      EXPECT(s.qraw + n <= P.down_off);
      EXPECT(s.inc >= P.down_off && s.out + mm::OUT_DOUBLES <= P.up_doubles);
      EXPECT(s.q >= P.up_doubles);
    }
    for (int b = 0; b < B; b++) EXPECT(seen[b] == 1);
    EXPECT(P.total_doubles >= P.up_doubles + leaf_total);  // the arena grows with cap x (2 p + n + M) per model
    std::sort(iv.begin(), iv.end());
    for (size_t k = 0; k < iv.size(); k++) {
      EXPECT(iv[k].second <= P.total_doubles);
      if (k) EXPECT(iv[k - 1].second <= iv[k].first);
    }
    // the plan is what the host writes through: fill every array of a real buffer (the sanitizer watches the ends)
    std::vector<double> arena(P.total_doubles, 0.0);
    for (size_t k = 1; k < iv.size(); k++)
      for (size_t i = iv[k].first; i < iv[k].second; i++) arena[i] += 1.0;
    size_t twice = 0;
    for (size_t k = 1; k < iv.size(); k++)
      for (size_t i = iv[k].first; i < iv[k].second; i++) twice += arena[i] != 1.0;
    EXPECT(twice == 0);
    // the arena refusal: accepted at its own size; one double short, the last model is named; at the end of model k's
    // leaf store, model k + 1 is named
    std::string err;
    EXPECT(mm::check_arena(P, sh, tree_cap, leaf_cap, P.total_doubles, err) == 0);
    EXPECT(mm::check_arena(P, sh, tree_cap, leaf_cap, P.total_doubles - 1, err) == mm::ERR_ARG &&
           err.find("model " + std::to_string(B - 1) + ";") != std::string::npos);
    if (B >= 2) {
      const int k = (int)(rng() % (B - 1));
      const size_t cap = sh[k].form == 3 ? leaf_cap : tree_cap;
      const size_t end_k = P.slot[k].lf_y + cap * (size_t)sh[k].M;
      EXPECT(mm::check_arena(P, sh, tree_cap, leaf_cap, end_k, err) == mm::ERR_ARG &&
             err.find("model " + std::to_string(k + 1) + ";") != std::string::npos);
    }
    EXPECT(mm::check_arena(P, sh, tree_cap, leaf_cap, 0, err) == mm::ERR_ARG && err.find("model 0;") != std::string::npos);
  }
}

int main() {
  checks();
  layouts();
  if (fails) {
    std::printf("%d failures\n", fails);
    return 1;
  }
  std::printf("models_plan_large ok\n");
  return 0;
}
