// Stand-alone program over miosqp_amd/csrc/models_plan.hpp (built with -fsanitize=address,undefined by
// tests/test_solve_models_cpu.py and run as a subprocess): the argument checks of miosqp_qp_solve_trees_models on
// hand-made calls, and the arena layout on random lists of shapes -- every array inside the arena, no two arrays
// overlapping, the table entries a permutation with the one-wavefront models first, the staged part in front.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
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

struct Call {
  int B;
  std::vector<int> eng, M, rule, mi;
  std::vector<std::vector<double>> q, l, u, x0, y0, xo;
  std::vector<double> up;
  std::vector<const void *> pe, pxo;
  std::vector<const double *> pq, pl, pu, px0, py0, pinc;
  Call(int B_, int n, int M_) : B(B_), eng(B_), M(B_, M_), rule(B_, 0), mi(B_, 100), up(B_, 1e300) {
    for (int b = 0; b < B; b++) {
      q.emplace_back(n, 0.0);
      x0.emplace_back(n, 0.0);
      xo.emplace_back(n, 0.0);
      l.emplace_back(M_, -1.0);
      u.emplace_back(M_, 1.0);
      y0.emplace_back(M_, 0.0);
    }
    link();
  }
  void link() {
    pe.clear(); pxo.clear(); pq.clear(); pl.clear(); pu.clear(); px0.clear(); py0.clear(); pinc.clear();
    for (int b = 0; b < B; b++) {
      pe.push_back(&eng[b]);
      pxo.push_back(xo[b].data());
      pq.push_back(q[b].data());
      pl.push_back(l[b].data());
      pu.push_back(u[b].data());
      px0.push_back(x0[b].data());
      py0.push_back(y0[b].data());
      pinc.push_back(nullptr);  // no incumbent: allowed
    }
  }
  int run(std::string &err, int B_override = -1) {
    int info = 0, stats = 0;
    return mm::check_args(B_override >= 0 ? B_override : B, pe.data(), M.data(), pq.data(), pl.data(), pu.data(), px0.data(),
                          py0.data(), up.data(), pinc.data(), rule.data(), mi.data(), pxo.data(), &info, &stats, err);
  }
};

static void checks() {
  std::string err;
  {
    Call c(3, 4, 6);
    EXPECT(c.run(err) == 0);
    EXPECT(c.run(err, 0) == mm::ERR_ARG && err.find("at least 1") != std::string::npos);
  }
  {
    Call c(3, 4, 6);
    int info = 0, stats = 0;
    EXPECT(mm::check_args(3, nullptr, c.M.data(), c.pq.data(), c.pl.data(), c.pu.data(), c.px0.data(), c.py0.data(), c.up.data(),
                          c.pinc.data(), c.rule.data(), c.mi.data(), c.pxo.data(), &info, &stats, err) == mm::ERR_ARG);
    EXPECT(mm::check_args(3, c.pe.data(), c.M.data(), c.pq.data(), c.pl.data(), c.pu.data(), c.px0.data(), c.py0.data(), c.up.data(),
                          c.pinc.data(), c.rule.data(), c.mi.data(), c.pxo.data(), nullptr, &stats, err) == mm::ERR_ARG);
    c.pl[1] = nullptr;
    EXPECT(c.run(err) == mm::ERR_ARG && err.find("model 1") != std::string::npos);
  }
  {
    Call c(4, 3, 5);
    c.pe[3] = c.pe[1];
    EXPECT(c.run(err) == mm::ERR_ARG && err.find("model 1") != std::string::npos && err.find("model 3") != std::string::npos);
  }
  {
    Call c(2, 3, 5);
    c.rule[1] = 4;
    EXPECT(c.run(err) == mm::ERR_ARG && err.find("model 1") != std::string::npos && err.find("0..3") != std::string::npos);
    c.rule[1] = -1;
    EXPECT(c.run(err) == mm::ERR_ARG);
    c.rule[1] = 3;
    c.mi[0] = 0;
    EXPECT(c.run(err) == mm::ERR_ARG && err.find("model 0") != std::string::npos);
  }
  {
    Call c(3, 3, 5);
    c.l[2][4] = 2.0;  // above u: the last row of the last model
    EXPECT(c.run(err) == mm::ERR_BOUNDS && err.find("model 2") != std::string::npos);
    c.l[2][4] = 1.0;  // equal: fine
    EXPECT(c.run(err) == 0);
  }
}

static void layouts() {
  std::mt19937 rng(12345);
  for (int trial = 0; trial < 100; trial++) {
    const int B = 1 + (int)(rng() % 40);
    const size_t entry = 8 * (1 + rng() % 200), cap = 1 + rng() % 64;
    std::vector<mm::Shape> sh;
    for (int b = 0; b < B; b++) {
      const int n = 1 + (int)(rng() % 70), p = 1 + (int)(rng() % n), M = p + (int)(rng() % 90);
      sh.push_back(mm::Shape{n, M, p, (int)(rng() % 2) + 1});
    }
    const mm::Plan P = mm::plan(sh, entry, cap);
    EXPECT((int)P.slot.size() == B && P.n1 + P.n2 == B);
    EXPECT(P.table_doubles * 8 >= (size_t)B * entry);
    EXPECT(P.down_off + P.down_doubles == P.up_doubles && P.up_doubles <= P.total_doubles && P.down_off % 2 == 0);
    std::vector<std::pair<size_t, size_t>> iv;  // [begin, end) of every array
    iv.push_back({0, P.table_doubles});
    std::vector<int> seen(B, 0);
    int last1 = -1, last2 = -1;
    for (int b = 0; b < B; b++) {
      const mm::Slot &s = P.slot[b];
      const size_t n = sh[b].n, M = sh[b].M, p = sh[b].p;
      EXPECT(s.entry >= 0 && s.entry < B);
      if (s.entry >= 0 && s.entry < B) seen[s.entry]++;
      if (sh[b].form == 1) {
        EXPECT(s.entry < P.n1 && s.entry > last1);  // the caller's order inside a form
        last1 = s.entry;
      } else {
        EXPECT(s.entry >= P.n1 && s.entry > last2);
        last2 = s.entry;
      }
      iv.push_back({s.raw, s.raw + 3 * M + n});
      iv.push_back({s.qraw, s.qraw + n});
      iv.push_back({s.inc, s.inc + n});
      iv.push_back({s.out, s.out + mm::OUT_DOUBLES});
      iv.push_back({s.q, s.q + n});
      iv.push_back({s.lf_lo, s.lf_lo + cap * p});
      iv.push_back({s.lf_hi, s.lf_hi + cap * p});
      iv.push_back({s.lf_x, s.lf_x + cap * n});
      iv.push_back({s.lf_y, s.lf_y + cap * M});
      // staged: raw, qraw in front of what comes back; inc, out inside it; the rest behind the upload
      EXPECT(s.qraw + n <= P.down_off);
      EXPECT(s.inc >= P.down_off && s.out + mm::OUT_DOUBLES <= P.up_doubles);
      EXPECT(s.q >= P.up_doubles);
    }
    for (int b = 0; b < B; b++) EXPECT(seen[b] == 1);
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
  }
}

int main() {
  checks();
  layouts();
  if (fails) {
    std::printf("%d failures\n", fails);
    return 1;
  }
  std::printf("models_plan ok\n");
  return 0;
}
