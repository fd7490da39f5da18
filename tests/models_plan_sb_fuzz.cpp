// Stand-alone program over miosqp_amd/csrc/models_plan.hpp (built with -fsanitize=address,undefined by
// tests/test_solve_trees_sb_cpu.py and run as a subprocess), next to models_plan_rf_fuzz.cpp: the two table groups, the
// per-model record and the per-tree work areas that strong / reliability branching inside the one-launch trees adds.
//   1. with the defaulted argument and forms 1..5 only, plan() is the layout it was before them -- restated here, with
//      and without the round-and-fix record;
//   2. with forms 6 and 7 and a record per model: the entries are wave | group | reduced | group_rf | reduced_rf |
//      group_sb | reduced_sb, each in the caller's order; every region of the arena is where the previous one ends (up
//      to the stated alignment), the record lies in the downloaded part, a model of form 6 or 7 has its work area and
//      Node.pc behind its leaf store and no other model has one, and the last region ends at total_doubles;
//   3. check_sb refuses what the entry documents, naming the model.
#include <algorithm>
#include <cstdio>
#include <random>

#include "../miosqp_amd/csrc/models_plan.hpp"

namespace mm = miosqp::models;
namespace sbl = miosqp::tree_sb;

#define REQUIRE(c)                                          \
  do {                                                      \
    if (!(c)) {                                             \
      printf("FAILED %s (line %d)\n", #c, __LINE__);        \
      return 1;                                             \
    }                                                       \
  } while (0)

// the layout before the strong-branching groups, written out again
static mm::Plan before(const std::vector<mm::Shape> &sh, size_t entry_bytes, size_t tree_cap, size_t leaf_cap_r, size_t rf_doubles) {
  mm::Plan P;
  const size_t B = sh.size();
  P.slot.resize(B);
  for (const mm::Shape &s : sh) (s.form == 1 ? P.n1 : s.form == 3 ? P.n3 : s.form == 4 ? P.n4 : s.form == 5 ? P.n5 : P.n2)++;
  int k1 = 0, k2 = P.n1, k3 = P.n1 + P.n2, k4 = k3 + P.n3, k5 = k4 + P.n4;
  for (size_t b = 0; b < B; b++)
    P.slot[b].entry = sh[b].form == 1 ? k1++ : sh[b].form == 3 ? k3++ : sh[b].form == 4 ? k4++ : sh[b].form == 5 ? k5++ : k2++;
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
    P.slot[b].rf = rf_doubles ? at : 0;
    at += rf_doubles;
  }
  P.down_doubles = at - P.down_off;
  P.up_doubles = at;
  at = mm::round_up(at, 32);
  for (size_t b = 0; b < B; b++) {
    const size_t n = (size_t)sh[b].n, M = (size_t)sh[b].M, p = (size_t)sh[b].p;
    const size_t cap = (sh[b].form == 3 || sh[b].form == 5) ? leaf_cap_r : tree_cap;
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
  std::mt19937 rng(20241021);
  auto draw = [&](int lo, int hi) { return (int)(lo + rng() % (unsigned)(hi - lo + 1)); };
  long plans = 0;
  for (int round = 0; round < 400; round++) {
    const int B = draw(1, 40);
    const size_t entry_bytes = (size_t)draw(8, 1500), tree_cap = (size_t)draw(1, 64), leaf_cap_r = (size_t)draw(2, 40);
    std::vector<mm::Shape> sh((size_t)B);
    // ---- 1. the defaults ----
    for (mm::Shape &s : sh) s = mm::Shape{draw(1, 30), draw(1, 50), draw(1, 9), draw(1, 5)};
    for (size_t rf : {mm::RF_DOUBLES, (size_t)0}) {
      if (rf == 0)
        for (mm::Shape &s : sh) s.form = 1 + (s.form - 1) % 3;
      const mm::Plan P = mm::plan(sh, entry_bytes, tree_cap, leaf_cap_r, rf), Q = before(sh, entry_bytes, tree_cap, leaf_cap_r, rf);
      REQUIRE(P.n1 == Q.n1 && P.n2 == Q.n2 && P.n3 == Q.n3 && P.n4 == Q.n4 && P.n5 == Q.n5 && P.n6 == 0 && P.n7 == 0);
      REQUIRE(P.table_doubles == Q.table_doubles && P.up_doubles == Q.up_doubles && P.down_off == Q.down_off &&
              P.down_doubles == Q.down_doubles && P.total_doubles == Q.total_doubles);
      for (size_t b = 0; b < (size_t)B; b++) {
        const mm::Slot &x = P.slot[b], &y = Q.slot[b];
        REQUIRE(x.entry == y.entry && x.raw == y.raw && x.qraw == y.qraw && x.inc == y.inc && x.out == y.out && x.rf == y.rf &&
                x.q == y.q && x.lf_lo == y.lf_lo && x.lf_hi == y.lf_hi && x.lf_x == y.lf_x && x.lf_y == y.lf_y && x.sb == 0 &&
                x.sb_work == 0 && x.sb_pc == 0);
      }
    }
    // ---- 2. the groups of a call with rules, a record per model ----
    for (mm::Shape &s : sh) {
      const int f = draw(1, 5);
      s.form = f == 4 ? 6 : f == 5 ? 7 : f;
    }
    const mm::Plan P = mm::plan(sh, entry_bytes, tree_cap, leaf_cap_r, 0, mm::SB_DOUBLES);
    plans++;
    REQUIRE(P.n1 + P.n2 + P.n3 + P.n6 + P.n7 == B && P.n4 == 0 && P.n5 == 0);
    const int first[8] = {0, 0, P.n1, P.n1 + P.n2, 0, 0, P.n1 + P.n2 + P.n3, P.n1 + P.n2 + P.n3 + P.n6};
    int seen[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t b = 0; b < (size_t)B; b++) {  // group by group, the caller's order inside a group
      const int f = sh[b].form;
      REQUIRE(P.slot[b].entry == first[f] + seen[f]);
      seen[f]++;
    }
    REQUIRE(seen[1] == P.n1 && seen[2] == P.n2 && seen[3] == P.n3 && seen[6] == P.n6 && seen[7] == P.n7);
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
      REQUIRE(P.slot[b].rf == 0);
      REQUIRE(P.slot[b].sb == at);  // the record: uploaded (zeroed) and downloaded with the outcome
      at += mm::SB_DOUBLES;
    }
    REQUIRE(P.up_doubles == at && P.down_doubles == at - P.down_off);
    size_t lf = mm::round_up(at, 32);
    for (size_t b = 0; b < (size_t)B; b++) {
      const size_t n = (size_t)sh[b].n, M = (size_t)sh[b].M, p = (size_t)sh[b].p;
      const size_t cap = (sh[b].form == 3 || sh[b].form == 7) ? leaf_cap_r : tree_cap;
      REQUIRE(P.slot[b].q == lf && P.slot[b].lf_lo == lf + mm::round_up(n, 2));
      REQUIRE(P.slot[b].lf_hi == P.slot[b].lf_lo + cap * p && P.slot[b].lf_x == P.slot[b].lf_hi + cap * p &&
              P.slot[b].lf_y == P.slot[b].lf_x + cap * n);
      lf = P.slot[b].lf_y + cap * M;
      if (sh[b].form == 6 || sh[b].form == 7) {
        REQUIRE(P.slot[b].sb_work == mm::round_up(lf, 2) && P.slot[b].sb_work % 2 == 0);
        REQUIRE(P.slot[b].sb_pc == P.slot[b].sb_work + sbl::work_doubles(sh[b].p));
        lf = P.slot[b].sb_pc + cap * (size_t)sbl::PC_DOUBLES;
        // the work area holds what view() carves from it
        std::vector<double> w(sbl::work_doubles(sh[b].p));
        const sbl::View v = sbl::view(w.data(), sh[b].p);
        REQUIRE(reinterpret_cast<char *>(v.count + 2) <= reinterpret_cast<char *>(w.data() + w.size()));
        sbl::start(v);
      } else {
        REQUIRE(P.slot[b].sb_work == 0 && P.slot[b].sb_pc == 0);
      }
    }
    REQUIRE(P.total_doubles == lf);
    std::string err;
    REQUIRE(mm::check_arena(P, sh, tree_cap, leaf_cap_r, P.total_doubles, err) == 0);
    REQUIRE(mm::check_arena(P, sh, tree_cap, leaf_cap_r, P.total_doubles - 1, err) == mm::ERR_ARG &&
            err.find("model " + std::to_string(B - 1)) != std::string::npos);
  }
  // ---- 3. the settings of the rules ----
  {
    std::string err;
    int32_t rule[3] = {0, 1, 2}, K[3] = {-5, 8, 32}, it[3] = {0, 50, 25}, rel[3] = {-1, 0, 4};
    double eps[3] = {0.0, 1e-6, 1e-3};
    int dummy = 0;
    REQUIRE(mm::check_sb(3, rule, K, it, rel, eps, &dummy, 0, "solve_trees_models_sb", err) == 0);  // (model 0: "none", not read)
    REQUIRE(mm::check_sb(3, rule, K, it, rel, eps, &dummy, 1, "solve_trees_sb", err) == mm::ERR_ARG && err.find("model 0") != std::string::npos);
    REQUIRE(mm::check_sb(3, rule, K, it, rel, eps, nullptr, 0, "x", err) == mm::ERR_ARG);
    REQUIRE(mm::check_sb(3, nullptr, K, it, rel, eps, &dummy, 0, "x", err) == mm::ERR_ARG);
    REQUIRE(mm::check_sb(3, rule, K, it, rel, nullptr, &dummy, 0, "x", err) == mm::ERR_ARG);
    rule[2] = 3;
    REQUIRE(mm::check_sb(3, rule, K, it, rel, eps, &dummy, 0, "x", err) == mm::ERR_ARG && err.find("branching_rule 3 of model 2") != std::string::npos);
    rule[2] = 2;
    K[2] = 33;
    REQUIRE(mm::check_sb(3, rule, K, it, rel, eps, &dummy, 0, "x", err) == mm::ERR_ARG && err.find("model 2") != std::string::npos);
    K[2] = 32;
    K[1] = 0;
    REQUIRE(mm::check_sb(3, rule, K, it, rel, eps, &dummy, 0, "x", err) == mm::ERR_ARG && err.find("sb_candidates 0 of model 1") != std::string::npos);
    K[1] = 8;
    it[1] = 0;
    REQUIRE(mm::check_sb(3, rule, K, it, rel, eps, &dummy, 0, "x", err) == mm::ERR_ARG && err.find("sb_max_iter of model 1") != std::string::npos);
    it[1] = 50;
    rel[2] = -1;
    REQUIRE(mm::check_sb(3, rule, K, it, rel, eps, &dummy, 0, "x", err) == mm::ERR_ARG && err.find("sb_reliability of model 2") != std::string::npos);
    rel[2] = 4;
    eps[1] = 0.0;
    REQUIRE(mm::check_sb(3, rule, K, it, rel, eps, &dummy, 0, "x", err) == mm::ERR_ARG && err.find("sb_eps of model 1") != std::string::npos);
    eps[1] = 0.0 / 0.0;
    REQUIRE(mm::check_sb(3, rule, K, it, rel, eps, &dummy, 0, "x", err) == mm::ERR_ARG && err.find("sb_eps of model 1") != std::string::npos);
  }
  printf("models_plan_sb ok: %ld plans\n", plans);
  return 0;
}
