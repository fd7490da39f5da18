// Stand-alone program over miosqp_amd/csrc/models_plan.hpp (built with -fsanitize=address,undefined by
// tests/test_solve_trees_rf_cpu.py and run as a subprocess), next to models_plan_fuzz.cpp and models_plan_large_fuzz.cpp:
// the two table groups and the per-model record that round and fix inside the one-launch trees adds.
//   1. with the defaulted arguments and forms 1..3 only, plan() is the layout it was before them -- restated here;
//   2. with forms 4 and 5 and a record per model: the entries are wave | group | reduced | group_rf | reduced_rf, each in
//      the caller's order; every region of the arena is where the previous one ends (up to the stated alignment), the
//      record lies in the downloaded part, and the last leaf store ends at total_doubles;
//   3. check_rf refuses what the entry documents, naming the model.
#include <algorithm>
#include <cstdio>
#include <random>

#include "../miosqp_amd/csrc/models_plan.hpp"

namespace mm = miosqp::models;

#define REQUIRE(c)                                          \
  do {                                                      \
    if (!(c)) {                                             \
      printf("FAILED %s (line %d)\n", #c, __LINE__);        \
      return 1;                                             \
    }                                                       \
  } while (0)

// the layout before the round-and-fix groups, written out again
static mm::Plan before(const std::vector<mm::Shape> &sh, size_t entry_bytes, size_t tree_cap, size_t leaf_cap_r) {
  mm::Plan P;
  const size_t B = sh.size();
  P.slot.resize(B);
  for (const mm::Shape &s : sh) (s.form == 1 ? P.n1 : s.form == 3 ? P.n3 : P.n2)++;
  int k1 = 0, k2 = P.n1, k3 = P.n1 + P.n2;
  for (size_t b = 0; b < B; b++) P.slot[b].entry = sh[b].form == 1 ? k1++ : sh[b].form == 3 ? k3++ : k2++;
  P.table_doubles = mm::round_up((B * entry_bytes + 7) / 8, 32);
  size_t at = P.table_doubles;
  for (size_t b = 0; b < B; b++) {
    P.slot[b].raw = at;
    at += 3 * (size_t)sh[b].M + (size_t)sh[b].n;
    P.slot[b].qraw = at;
    at += (size_t)sh[b].n;
  }
  at = mm::round_up(at, 2);
  P.down_off = at;
  for (size_t b = 0; b < B; b++) {
    P.slot[b].inc = at;
    at += (size_t)sh[b].n;
    P.slot[b].out = at;
    at += mm::OUT_DOUBLES;
  }
  P.down_doubles = at - P.down_off;
  P.up_doubles = at;
  at = mm::round_up(at, 32);
  for (size_t b = 0; b < B; b++) {
    const size_t n = (size_t)sh[b].n, M = (size_t)sh[b].M, p = (size_t)sh[b].p, cap = sh[b].form == 3 ? leaf_cap_r : tree_cap;
    P.slot[b].q = at;
    at += mm::round_up(n, 2);
    P.slot[b].lf_lo = at;
    at += cap * p;
    P.slot[b].lf_hi = at;
    at += cap * p;
    P.slot[b].lf_x = at;
    at += cap * n;
    P.slot[b].lf_y = at;
    at += cap * M;
  }
  P.total_doubles = at;
  return P;
}

int main() {
  std::mt19937 rng(20240917);
  auto draw = [&](int lo, int hi) { return (int)(lo + rng() % (unsigned)(hi - lo + 1)); };
  long plans = 0;
  for (int round = 0; round < 400; round++) {
    const int B = draw(1, 40);
    const size_t entry_bytes = (size_t)draw(8, 1500), tree_cap = (size_t)draw(1, 64), leaf_cap_r = (size_t)draw(2, 40);
    std::vector<mm::Shape> sh((size_t)B);
    // ---- 1. the defaults ----
    for (mm::Shape &s : sh) s = mm::Shape{draw(1, 30), draw(1, 50), draw(1, 9), draw(1, 3)};
    {
      const mm::Plan P = mm::plan(sh, entry_bytes, tree_cap, leaf_cap_r), Q = before(sh, entry_bytes, tree_cap, leaf_cap_r);
      REQUIRE(P.n1 == Q.n1 && P.n2 == Q.n2 && P.n3 == Q.n3 && P.n4 == 0 && P.n5 == 0);
      REQUIRE(P.table_doubles == Q.table_doubles && P.up_doubles == Q.up_doubles && P.down_off == Q.down_off &&
              P.down_doubles == Q.down_doubles && P.total_doubles == Q.total_doubles);
      for (size_t b = 0; b < (size_t)B; b++) {
        const mm::Slot &x = P.slot[b], &y = Q.slot[b];
        REQUIRE(x.entry == y.entry && x.raw == y.raw && x.qraw == y.qraw && x.inc == y.inc && x.out == y.out && x.q == y.q &&
                x.lf_lo == y.lf_lo && x.lf_hi == y.lf_hi && x.lf_x == y.lf_x && x.lf_y == y.lf_y && x.rf == 0);
      }
      if (P.n3 == 0) {  // ... and without leaf_cap_r, as miosqp_qp_solve_trees_models calls it
        const mm::Plan R = mm::plan(sh, entry_bytes, tree_cap);
        REQUIRE(R.total_doubles == Q.total_doubles && R.slot.back().lf_y == Q.slot.back().lf_y);
      }
    }
    // ---- 2. all five groups, a record per model ----
    for (mm::Shape &s : sh) s.form = draw(1, 5);
    const mm::Plan P = mm::plan(sh, entry_bytes, tree_cap, leaf_cap_r, mm::RF_DOUBLES);
    plans++;
    REQUIRE(P.n1 + P.n2 + P.n3 + P.n4 + P.n5 == B);
    const int first[6] = {0, 0, P.n1, P.n1 + P.n2, P.n1 + P.n2 + P.n3, P.n1 + P.n2 + P.n3 + P.n4};
    int seen[6] = {0, 0, 0, 0, 0, 0};
    for (size_t b = 0; b < (size_t)B; b++) {  // group by group, the caller's order inside a group
      const int f = sh[b].form;
      REQUIRE(P.slot[b].entry == first[f] + seen[f]);
      seen[f]++;
    }
    REQUIRE(seen[1] == P.n1 && seen[2] == P.n2 && seen[3] == P.n3 && seen[4] == P.n4 && seen[5] == P.n5);
    REQUIRE(P.table_doubles * 8 >= (size_t)B * entry_bytes && P.table_doubles % 32 == 0);
    size_t at = P.table_doubles;
    for (size_t b = 0; b < (size_t)B; b++) {
      REQUIRE(P.slot[b].raw == at);
      at += 3 * (size_t)sh[b].M + (size_t)sh[b].n;
      REQUIRE(P.slot[b].qraw == at);
      at += (size_t)sh[b].n;
    }
    REQUIRE(P.down_off >= at && P.down_off < at + 2 && P.down_off % 2 == 0);
    at = P.down_off;
    for (size_t b = 0; b < (size_t)B; b++) {
      REQUIRE(P.slot[b].inc == at);
      at += (size_t)sh[b].n;
      REQUIRE(P.slot[b].out == at);
      at += mm::OUT_DOUBLES;
      REQUIRE(P.slot[b].rf == at);  // the record: uploaded (zeroed) and downloaded with the outcome
      at += mm::RF_DOUBLES;
    }
    REQUIRE(P.up_doubles == at && P.down_doubles == at - P.down_off);
    size_t lf = mm::round_up(at, 32);
    for (size_t b = 0; b < (size_t)B; b++) {
      const size_t n = (size_t)sh[b].n, M = (size_t)sh[b].M, p = (size_t)sh[b].p;
      const size_t cap = (sh[b].form == 3 || sh[b].form == 5) ? leaf_cap_r : tree_cap;
      REQUIRE(P.slot[b].q == lf && P.slot[b].lf_lo == lf + mm::round_up(n, 2));
      REQUIRE(P.slot[b].lf_hi == P.slot[b].lf_lo + cap * p && P.slot[b].lf_x == P.slot[b].lf_hi + cap * p &&
              P.slot[b].lf_y == P.slot[b].lf_x + cap * n);
      lf = P.slot[b].lf_y + cap * M;
    }
    REQUIRE(P.total_doubles == lf);
    std::string err;
    REQUIRE(mm::check_arena(P, sh, tree_cap, leaf_cap_r, P.total_doubles, err) == 0);
    REQUIRE(mm::check_arena(P, sh, tree_cap, leaf_cap_r, P.total_doubles - 1, err) == mm::ERR_ARG &&
            err.find("model " + std::to_string(B - 1)) != std::string::npos);
  }
  // ---- 3. the settings of round and fix ----
  {
    std::string err;
    int32_t K[3] = {0, 7, 32}, it[3] = {1, 250, 5}, ev[3] = {1, 3, 10};
    int dummy = 0;
    REQUIRE(mm::check_rf(3, K, it, ev, &dummy, 0, "solve_trees_models_rf", err) == 0);
    REQUIRE(mm::check_rf(3, K, it, ev, &dummy, 1, "solve_trees_rf", err) == mm::ERR_ARG && err.find("model 0") != std::string::npos);
    REQUIRE(mm::check_rf(3, K, it, ev, nullptr, 0, "x", err) == mm::ERR_ARG);
    REQUIRE(mm::check_rf(3, nullptr, it, ev, &dummy, 0, "x", err) == mm::ERR_ARG);
    K[2] = 33;
    REQUIRE(mm::check_rf(3, K, it, ev, &dummy, 0, "x", err) == mm::ERR_ARG && err.find("model 2") != std::string::npos);
    K[2] = 32;
    K[1] = -1;
    REQUIRE(mm::check_rf(3, K, it, ev, &dummy, 0, "x", err) == mm::ERR_ARG && err.find("model 1") != std::string::npos);
    K[1] = 7;
    it[1] = 0;
    REQUIRE(mm::check_rf(3, K, it, ev, &dummy, 0, "x", err) == mm::ERR_ARG && err.find("rf_max_iter of model 1") != std::string::npos);
    it[1] = 1;
    ev[0] = 0;  // (read for every model, also where the heuristic is off)
    REQUIRE(mm::check_rf(3, K, it, ev, &dummy, 0, "x", err) == mm::ERR_ARG && err.find("rf_every of model 0") != std::string::npos);
  }
  printf("models_plan_rf ok: %ld plans\n", plans);
  return 0;
}
