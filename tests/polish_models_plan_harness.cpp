// Stand-alone program over miosqp_amd/csrc/polish_models_plan.hpp (built with -fsanitize=address,undefined by
// tests/test_polish_models_cpu.py and run as a subprocess): every refusal of miosqp_qp_polish_models that reads only the
// caller's arrays, each naming its model; the arena layout of a twelve-model list -- parts disjoint, 8-byte aligned,
// inside `total`, the upload in front of the download --; and the launch's LDS figure, the maximum over the list.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "../miosqp_amd/csrc/polish_models_plan.hpp"

namespace pm = miosqp::polish_models;

static int fails = 0;
#define EXPECT(c)                                            \
  do {                                                       \
    if (!(c)) {                                              \
      std::printf("line %d: %s\n", __LINE__, #c);            \
      fails++;                                               \
    }                                                        \
  } while (0)

static bool names(const std::string &err, int b) { return err.find("model " + std::to_string(b)) != std::string::npos; }

struct Call {
  int B;
  double tau = 1e-2;
  std::vector<int> eng, n, M, refine, repair;
  std::vector<double> delta;
  std::vector<std::vector<double>> q, l, u, x, y, xo, yo;
  std::vector<const void *> pe, pxo, pyo;
  std::vector<const double *> pq, pl, pu, px, py;
  Call(int B_, int n_, int M_) : B(B_), eng(B_), n(B_, n_), M(B_, M_), refine(B_, 3), repair(B_, 20), delta(B_, 1e-6) {
    for (int b = 0; b < B; b++) {
      q.emplace_back(n_, 0.5);
      x.emplace_back(n_, 0.0);
      xo.emplace_back(n_, 0.0);
      l.emplace_back(M_, -1.0);
      u.emplace_back(M_, 1.0);
      y.emplace_back(M_, 0.0);
      yo.emplace_back(M_, 0.0);
    }
    for (int b = 0; b < B; b++) {
      pe.push_back(&eng[b]);
      pxo.push_back(xo[b].data());
      pyo.push_back(yo[b].data());
      pq.push_back(q[b].data());
      pl.push_back(l[b].data());
      pu.push_back(u[b].data());
      px.push_back(x[b].data());
      py.push_back(y[b].data());
    }
  }
  int run(std::string &err, int B_override = -1) {
    int info = 0, stats = 0;
    err.clear();
    return pm::check_args(B_override >= 0 ? B_override : B, pe.data(), n.data(), M.data(), pq.data(), pl.data(), pu.data(),
                          px.data(), py.data(), tau, delta.data(), refine.data(), repair.data(), pxo.data(), pyo.data(), &info,
                          &stats, err);
  }
};

static void refusals() {
  std::string err;
  const double nan = std::nan("");
  {
    Call c(3, 4, 6);
    EXPECT(c.run(err) == 0 && err.empty());
    EXPECT(c.run(err, 0) == pm::ERR_ARG && err.find("at least 1") != std::string::npos);
    c.pq[1] = nullptr;  // the engine's cost: allowed
    c.py[2] = nullptr;  // the device's guess: allowed with tau > 0
    EXPECT(c.run(err) == 0);
  }
  {
    Call c(3, 4, 6);
    int info = 0, stats = 0;
    EXPECT(pm::check_args(3, nullptr, c.n.data(), c.M.data(), c.pq.data(), c.pl.data(), c.pu.data(), c.px.data(), c.py.data(), c.tau,
                          c.delta.data(), c.refine.data(), c.repair.data(), c.pxo.data(), c.pyo.data(), &info, &stats, err) == pm::ERR_ARG);
    EXPECT(pm::check_args(3, c.pe.data(), c.n.data(), c.M.data(), c.pq.data(), c.pl.data(), c.pu.data(), c.px.data(), c.py.data(), c.tau,
                          c.delta.data(), c.refine.data(), c.repair.data(), c.pxo.data(), c.pyo.data(), &info, nullptr, err) == pm::ERR_ARG);
    EXPECT(pm::check_args(3, c.pe.data(), c.n.data(), c.M.data(), c.pq.data(), c.pl.data(), c.pu.data(), c.px.data(), c.py.data(), c.tau,
                          nullptr, c.refine.data(), c.repair.data(), c.pxo.data(), c.pyo.data(), &info, &stats, err) == pm::ERR_ARG);
    c.px[1] = nullptr;
    EXPECT(c.run(err) == pm::ERR_ARG && names(err, 1));
    c.px[1] = c.x[1].data();
    c.pyo[2] = nullptr;
    EXPECT(c.run(err) == pm::ERR_ARG && names(err, 2));
    c.pyo[2] = c.yo[2].data();
    c.pe[0] = nullptr;
    EXPECT(c.run(err) == pm::ERR_ARG && names(err, 0));
  }
  {  // an engine listed twice: both positions named
    Call c(4, 3, 5);
    c.pe[3] = c.pe[1];
    EXPECT(c.run(err) == pm::ERR_ARG && names(err, 1) && names(err, 3));
  }
  {  // delta
    Call c(3, 3, 5);
    c.delta[2] = 0.0;
    EXPECT(c.run(err) == pm::ERR_ARG && names(err, 2) && err.find("delta") != std::string::npos);
    c.delta[2] = -1e-6;
    EXPECT(c.run(err) == pm::ERR_ARG && names(err, 2));
    c.delta[2] = nan;
    EXPECT(c.run(err) == pm::ERR_ARG && names(err, 2));
    c.delta[2] = 1e-3;
    EXPECT(c.run(err) == 0);
  }
  {  // refine_iter 0..10, repair_iter 0..20
    Call c(3, 3, 5);
    c.refine[1] = 11;
    EXPECT(c.run(err) == pm::ERR_ARG && names(err, 1) && err.find("0..10") != std::string::npos);
    c.refine[1] = -1;
    EXPECT(c.run(err) == pm::ERR_ARG && names(err, 1));
    c.refine[1] = 10;
    c.repair[0] = 21;
    EXPECT(c.run(err) == pm::ERR_ARG && names(err, 0) && err.find("0..20") != std::string::npos);
    c.repair[0] = -1;
    EXPECT(c.run(err) == pm::ERR_ARG && names(err, 0));
    c.repair[0] = 0;
    c.refine[1] = 0;
    EXPECT(c.run(err) == 0);
  }
  {  // a NaN in q, l, u, x or y
    for (int which = 0; which < 5; which++) {
      Call c(3, 3, 5);
      std::vector<double> &v = which == 0 ? c.q[2] : which == 1 ? c.l[2] : which == 2 ? c.u[2] : which == 3 ? c.x[2] : c.y[2];
      v.back() = nan;  // the last entry of the last model
      EXPECT(c.run(err) == pm::ERR_ARG && names(err, 2) && err.find("NaN") != std::string::npos);
    }
  }
  {  // no y and tau not positive
    Call c(3, 3, 5);
    c.py[1] = nullptr;
    c.tau = 0.0;
    EXPECT(c.run(err) == pm::ERR_ARG && names(err, 1) && err.find("tau") != std::string::npos);
    c.tau = -1.0;
    EXPECT(c.run(err) == pm::ERR_ARG && names(err, 1));
    c.tau = nan;
    EXPECT(c.run(err) == pm::ERR_ARG && names(err, 1));
    c.py[1] = c.y[1].data();  // every y given: tau is not read
    EXPECT(c.run(err) == 0);
  }
  {  // l > u
    Call c(3, 3, 5);
    c.l[2][4] = 2.0;
    EXPECT(c.run(err) == pm::ERR_BOUNDS && names(err, 2));
    c.l[2][4] = 1.0;  // equal: fine
    EXPECT(c.run(err) == 0);
  }
  {  // a model beyond one workgroup's LDS
    std::vector<pm::Shape> sh = {{10, 7, 40, true, true}, {192, 3, 500, true, true}, {192, 4, 600, true, true}, {20, 15, 0, true, false}};
    EXPECT(pm::check_fit(sh, err) == pm::ERR_UNSUPPORTED && names(err, 2));
    sh[2] = pm::Shape{193, 1, 100, true, true};
    EXPECT(pm::check_fit(sh, err) == pm::ERR_UNSUPPORTED && names(err, 2));
    sh[2] = pm::Shape{3, 257, 100, true, true};
    EXPECT(pm::check_fit(sh, err) == pm::ERR_UNSUPPORTED && names(err, 2));
    sh.erase(sh.begin() + 2);
    EXPECT(pm::check_fit(sh, err) == 0);
  }
}

static void layout_of_twelve() {
  // twelve shapes (n, M), with and without rows to stage, q and y
  const int nM[12][2] = {{10, 7}, {20, 15}, {12, 36}, {32, 24}, {192, 3}, {150, 5}, {30, 140}, {6, 9}, {50, 60}, {7, 7}, {64, 64}, {1, 0}};
  std::vector<pm::Shape> sh;
  for (int b = 0; b < 12; b++)
    sh.push_back(pm::Shape{nM[b][0], nM[b][1], b % 4 == 3 ? (size_t)0 : (size_t)(nM[b][0] * nM[b][1] / 2 + b), b % 3 != 1, b % 5 != 2});
  const pm::Plan P = pm::plan(sh);
  EXPECT(P.slot.size() == 12);
  EXPECT(P.table_doubles * 8 >= 12 * sizeof(miosqp::PolManyModel));
  EXPECT(P.up_doubles <= P.down_off && P.down_off % 2 == 0 && P.down_off + P.down_doubles == P.total_doubles);
  std::vector<std::pair<size_t, size_t>> iv;  // [begin, end) of every part, in doubles: 8-byte aligned by construction
  iv.push_back({0, P.table_doubles});
  size_t lds_max = 0;
  for (int b = 0; b < 12; b++) {
    const pm::Slot &s = P.slot[b];
    const size_t n = sh[b].n, M = sh[b].M;
    EXPECT((s.A == pm::NONE) == (sh[b].rows == 0));
    EXPECT((s.q == pm::NONE) == !sh[b].has_q);
    EXPECT((s.y == pm::NONE) == !sh[b].has_y);
    if (s.A != pm::NONE) iv.push_back({s.A, s.A + sh[b].rows});
    if (s.q != pm::NONE) iv.push_back({s.q, s.q + n});
    iv.push_back({s.l, s.l + M});
    iv.push_back({s.u, s.u + M});
    iv.push_back({s.x, s.x + n});
    if (s.y != pm::NONE) iv.push_back({s.y, s.y + M});
    iv.push_back({s.out, s.out + miosqp::polm_out_stride(sh[b].n, sh[b].M)});
    // what goes up lies in front of what comes back
    EXPECT(s.x + n <= P.up_doubles && (s.y == pm::NONE || s.y + M <= P.up_doubles));
    EXPECT(s.out >= P.down_off);
    EXPECT(miosqp::polm_out_stride(sh[b].n, sh[b].M) * 8 >= sizeof(miosqp::PolManyRec) + 8 * (n + M) + M);
    lds_max = std::max(lds_max, miosqp::polm_lds_bytes(sh[b].n, sh[b].M));
  }
  std::sort(iv.begin(), iv.end());
  for (size_t k = 0; k < iv.size(); k++) {
    EXPECT(iv[k].first <= iv[k].second && iv[k].second <= P.total_doubles);
    if (k) EXPECT(iv[k - 1].second <= iv[k].first);
  }
  // the plan is what the host writes through: fill every part of a real buffer (the sanitizer watches the ends)
  std::vector<double> arena(P.total_doubles, 0.0);
  for (const auto &p : iv)
    for (size_t i = p.first; i < p.second; i++) arena[i] += 1.0;
  size_t twice = 0;
  for (const auto &p : iv)
    for (size_t i = p.first; i < p.second; i++) twice += arena[i] != 1.0;
  EXPECT(twice == 0);
  // the LDS of the launch: the largest need among the models -- here that of (192, 3), below the limit
  EXPECT(P.lds_bytes == lds_max && P.lds_bytes == miosqp::polm_lds_bytes(192, 3) && P.lds_bytes <= pm::LDS_LIMIT);
  EXPECT(miosqp::polm_lds_bytes(192, 4) > pm::LDS_LIMIT);
  // ... and it does not depend on the order of the list
  std::vector<pm::Shape> rev(sh.rbegin(), sh.rend());
  EXPECT(pm::plan(rev).lds_bytes == P.lds_bytes && pm::plan(rev).total_doubles == P.total_doubles);
  // a one-model list takes that model's own figure
  EXPECT(pm::plan({sh[0]}).lds_bytes == miosqp::polm_lds_bytes(10, 7));
}

int main() {
  refusals();
  layout_of_twelve();
  if (fails) {
    std::printf("%d failures\n", fails);
    return 1;
  }
  std::printf("polish_models_plan ok\n");
  return 0;
}
