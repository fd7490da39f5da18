// Stand-alone program over miosqp_amd/csrc/polish_models_large_plan.hpp (built with -fsanitize=address,undefined by
// tests/test_polish_models_large_cpu.py and run as a subprocess): every refusal of miosqp_qp_polish_models_large that
// reads only the caller's arrays, each naming its model and the entry; the fit rule at its limits; the number of
// workgroups at three list lengths; and the arena layout -- parts disjoint, 8-byte aligned, inside `total`, the upload in
// front of the records, the slabs behind both and outside the pinned size, a slab sized for the list's largest model.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "../miosqp_amd/csrc/polish_models_large_plan.hpp"

namespace pm = miosqp::polish_models;
namespace pl = miosqp::polish_models_large;

static int fails = 0;
#define EXPECT(c)                                            \
  do {                                                       \
    if (!(c)) {                                              \
      std::printf("line %d: %s\n", __LINE__, #c);            \
      fails++;                                               \
    }                                                        \
  } while (0)

static bool names(const std::string &err, int b) { return err.find("model " + std::to_string(b)) != std::string::npos; }
static bool entry(const std::string &err) { return err.rfind("polish_models_large: ", 0) == 0; }

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
                          &stats, err, pl::ENTRY);
  }
};

static void refusals() {
  std::string err;
  const double nan = std::nan("");
  {
    Call c(3, 200, 30);
    EXPECT(c.run(err) == 0 && err.empty());
    EXPECT(c.run(err, 0) == pl::ERR_ARG && err.find("at least 1") != std::string::npos && entry(err));
    c.pq[1] = nullptr;  // the engine's cost: allowed
    c.py[2] = nullptr;  // the device's guess: allowed with tau > 0
    EXPECT(c.run(err) == 0);
  }
  {
    Call c(3, 4, 6);
    int info = 0, stats = 0;
    EXPECT(pm::check_args(3, nullptr, c.n.data(), c.M.data(), c.pq.data(), c.pl.data(), c.pu.data(), c.px.data(), c.py.data(), c.tau,
                          c.delta.data(), c.refine.data(), c.repair.data(), c.pxo.data(), c.pyo.data(), &info, &stats, err,
                          pl::ENTRY) == pl::ERR_ARG && entry(err));
    EXPECT(pm::check_args(3, c.pe.data(), c.n.data(), c.M.data(), c.pq.data(), c.pl.data(), c.pu.data(), c.px.data(), c.py.data(), c.tau,
                          c.delta.data(), c.refine.data(), c.repair.data(), c.pxo.data(), c.pyo.data(), &info, nullptr, err,
                          pl::ENTRY) == pl::ERR_ARG);
    c.px[1] = nullptr;
    EXPECT(c.run(err) == pl::ERR_ARG && names(err, 1) && entry(err));
    c.px[1] = c.x[1].data();
    c.pyo[2] = nullptr;
    EXPECT(c.run(err) == pl::ERR_ARG && names(err, 2));
    c.pyo[2] = c.yo[2].data();
    c.pe[0] = nullptr;
    EXPECT(c.run(err) == pl::ERR_ARG && names(err, 0));
  }
  {  // an engine listed twice: both positions named
    Call c(4, 3, 5);
    c.pe[3] = c.pe[1];
    EXPECT(c.run(err) == pl::ERR_ARG && names(err, 1) && names(err, 3) && entry(err));
  }
  {  // delta
    Call c(3, 3, 5);
    c.delta[2] = 0.0;
    EXPECT(c.run(err) == pl::ERR_ARG && names(err, 2) && err.find("delta") != std::string::npos && entry(err));
    c.delta[2] = -1e-6;
    EXPECT(c.run(err) == pl::ERR_ARG && names(err, 2));
    c.delta[2] = nan;
    EXPECT(c.run(err) == pl::ERR_ARG && names(err, 2));
    c.delta[2] = 1e-3;
    EXPECT(c.run(err) == 0);
  }
  {  // refine_iter 0..10, repair_iter 0..20
    Call c(3, 3, 5);
    c.refine[1] = 11;
    EXPECT(c.run(err) == pl::ERR_ARG && names(err, 1) && err.find("0..10") != std::string::npos && entry(err));
    c.refine[1] = -1;
    EXPECT(c.run(err) == pl::ERR_ARG && names(err, 1));
    c.refine[1] = 10;
    c.repair[0] = 21;
    EXPECT(c.run(err) == pl::ERR_ARG && names(err, 0) && err.find("0..20") != std::string::npos && entry(err));
    c.repair[0] = -1;
    EXPECT(c.run(err) == pl::ERR_ARG && names(err, 0));
    c.repair[0] = 0;
    c.refine[1] = 0;
    EXPECT(c.run(err) == 0);
  }
  {  // a NaN in q, l, u, x or y
    for (int which = 0; which < 5; which++) {
      Call c(3, 3, 5);
      std::vector<double> &v = which == 0 ? c.q[2] : which == 1 ? c.l[2] : which == 2 ? c.u[2] : which == 3 ? c.x[2] : c.y[2];
      v.back() = nan;  // the last entry of the last model
      EXPECT(c.run(err) == pl::ERR_ARG && names(err, 2) && err.find("NaN") != std::string::npos && entry(err));
    }
  }
  {  // no y and tau not positive
    Call c(3, 3, 5);
    c.py[1] = nullptr;
    c.tau = 0.0;
    EXPECT(c.run(err) == pl::ERR_ARG && names(err, 1) && err.find("tau") != std::string::npos && entry(err));
    c.tau = -1.0;
    EXPECT(c.run(err) == pl::ERR_ARG && names(err, 1));
    c.tau = nan;
    EXPECT(c.run(err) == pl::ERR_ARG && names(err, 1));
    c.py[1] = c.y[1].data();  // every y given: tau is not read
    EXPECT(c.run(err) == 0);
  }
  {  // l > u
    Call c(3, 3, 5);
    c.l[2][4] = 2.0;
    EXPECT(c.run(err) == pl::ERR_BOUNDS && names(err, 2) && entry(err));
    c.l[2][4] = 1.0;  // equal: fine
    EXPECT(c.run(err) == 0);
  }
  {  // the order: a repeated engine before a bad delta before a NaN before a missing tau before l > u
    Call c(3, 3, 5);
    c.l[0][0] = 2.0;
    EXPECT(c.run(err) == pl::ERR_BOUNDS && names(err, 0));
    c.py[1] = nullptr;
    c.tau = 0.0;
    EXPECT(c.run(err) == pl::ERR_ARG && err.find("tau") != std::string::npos);
    c.x[2][0] = nan;
    EXPECT(c.run(err) == pl::ERR_ARG && err.find("NaN") != std::string::npos);
    c.delta[1] = 0.0;
    EXPECT(c.run(err) == pl::ERR_ARG && err.find("delta") != std::string::npos);
    c.pe[2] = c.pe[0];
    EXPECT(c.run(err) == pl::ERR_ARG && err.find("listed again") != std::string::npos);
  }
}

static void fit_rule() {
  EXPECT(pl::fits(512, 65536) && pl::fits(512, 0) && pl::fits(1, 65536) && pl::fits(10, 7));
  EXPECT(!pl::fits(513, 4) && !pl::fits(512, 65537) && !pl::fits(0, 5) && !pl::fits(5, -1));
  EXPECT(miosqp::polish_many_large_slab_doubles(512, 65536) * 8 <= miosqp::POLG_BUDGET);  // (one slab within the budget at both limits)
  EXPECT(miosqp::polish_many_large_slab_doubles(513, 4) == (size_t)-1 && miosqp::polish_many_large_slab_doubles(4, 65537) == (size_t)-1);
  std::string err;
  std::vector<pl::Shape> sh = {{10, 7, 40, 40, true, true}, {512, 65536, 500, 500, true, true}, {513, 4, 600, 600, true, true},
                               {20, 15, 0, 0, true, false}};
  EXPECT(pl::check_fit(sh, err) == pl::ERR_UNSUPPORTED && names(err, 2) && entry(err));
  sh[2] = pl::Shape{100, 65537, 100, 100, true, true};
  EXPECT(pl::check_fit(sh, err) == pl::ERR_UNSUPPORTED && names(err, 2));
  sh[0] = pl::Shape{513, 1, 10, 10, true, true};
  EXPECT(pl::check_fit(sh, err) == pl::ERR_UNSUPPORTED && names(err, 0));  // the first one is named
  sh[0] = pl::Shape{10, 7, 40, 40, true, true};
  sh.erase(sh.begin() + 2);
  EXPECT(pl::check_fit(sh, err) == 0);
}

static void workgroups() {
  const int cus = 256;
  const size_t small = miosqp::polish_many_large_slab_doubles(150, 320), big = miosqp::polish_many_large_slab_doubles(512, 100);
  // B below two workgroups per compute unit: one workgroup per model
  EXPECT(pl::workgroups(9, cus, small) == 9 && pl::workgroups(1, cus, big) == 1 && pl::workgroups(512, cus, small) == 512);
  // B above it
  EXPECT(pl::workgroups(600, cus, small) == 512 && pl::workgroups(513, cus, small) == 512 && pl::workgroups(5, 2, small) == 4);
  EXPECT(pl::workgroups(7, 0, small) == 2);  // (a device that reports no compute unit counts as one)
  // a B where the budget binds: n = 512 takes 2.4 MB a slab, 1 GiB holds fewer than 512 of them
  const size_t fit = miosqp::POLG_BUDGET / (big * 8);
  EXPECT(fit >= 1 && fit < 512 && big * 8 > 2000000 && big * 8 < 3000000);
  EXPECT(pl::workgroups(600, cus, big) == (int)fit && pl::workgroups(fit, cus, big) == (int)fit &&
         pl::workgroups(fit + 1, cus, big) == (int)fit && pl::workgroups(fit - 1, cus, big) == (int)fit - 1);
  // one slab beyond the budget: refused
  EXPECT(pl::workgroups(4, cus, miosqp::POLG_BUDGET / 8 + 1) == 0 && pl::workgroups(4, cus, (size_t)-1) == 0 &&
         pl::workgroups(4, cus, 0) == 0);
  std::vector<pl::Shape> many(600, pl::Shape{512, 100, 0, 0, false, true});
  const pl::Plan P = pl::plan(many, cus);
  EXPECT(P.W == (int)fit && (size_t)P.W * P.slab_doubles * 8 <= miosqp::POLG_BUDGET && P.slab_doubles == big);
  EXPECT(P.total_doubles == P.slab_off + (size_t)P.W * big);
}

static void layout_of_twelve() {
  // twelve shapes (n, M) on both sides of one workgroup's LDS, with and without rows to stage, q and y
  const int nM[12][2] = {{60, 133}, {20, 534}, {12, 36}, {150, 320}, {192, 3}, {150, 105}, {300, 140}, {6, 9}, {512, 60}, {7, 7},
                         {257, 45}, {1, 0}};
  const int cus = 256;
  std::vector<pl::Shape> sh;
  for (int b = 0; b < 12; b++) {
    const bool lent = b % 4 == 3;
    sh.push_back(pl::Shape{nM[b][0], nM[b][1], lent ? (size_t)0 : (size_t)(nM[b][0] * nM[b][1] / 2 + b),
                           lent ? (size_t)0 : (size_t)(nM[b][0] * nM[b][1] / 2 + 2 * b + 1), b % 3 != 1, b % 5 != 2});
  }
  const pl::Plan P = pl::plan(sh, cus);
  EXPECT(P.slot.size() == 12 && P.W == 12);
  EXPECT(P.table_doubles * 8 >= 12 * sizeof(miosqp::PolManyLargeModel));
  EXPECT(P.up_doubles <= P.down_off && P.down_off % 2 == 0 && P.down_off + P.down_doubles == P.pinned_doubles);
  // the slabs: behind the upload and the records, outside the pinned size, on 256 bytes, W of them to the end
  EXPECT(P.slab_off >= P.pinned_doubles && P.slab_off % 32 == 0 && P.slab_doubles % 32 == 0);
  EXPECT(P.slab_off + (size_t)P.W * P.slab_doubles == P.total_doubles && P.pinned_doubles < P.total_doubles);
  std::vector<std::pair<size_t, size_t>> iv;  // [begin, end) of every part, in doubles: 8-byte aligned by construction
  iv.push_back({0, P.table_doubles});
  size_t slab_max = 0;
  for (int b = 0; b < 12; b++) {
    const pl::Slot &s = P.slot[b];
    const size_t n = sh[b].n, M = sh[b].M;
    EXPECT((s.A == pl::NONE) == (sh[b].rows_con == 0) && (s.At == pl::NONE) == (sh[b].rows_var == 0));
    EXPECT((s.q == pl::NONE) == !sh[b].has_q);
    EXPECT((s.y == pl::NONE) == !sh[b].has_y);
    if (s.A != pl::NONE) iv.push_back({s.A, s.A + sh[b].rows_con});
    if (s.At != pl::NONE) iv.push_back({s.At, s.At + sh[b].rows_var});
    if (s.q != pl::NONE) iv.push_back({s.q, s.q + n});
    iv.push_back({s.l, s.l + M});
    iv.push_back({s.u, s.u + M});
    iv.push_back({s.x, s.x + n});
    if (s.y != pl::NONE) iv.push_back({s.y, s.y + M});
    iv.push_back({s.out, s.out + miosqp::polm_out_stride(sh[b].n, sh[b].M)});
    // what goes up lies in front of what comes back, and both in the pinned mirror
    EXPECT(s.x + n <= P.up_doubles && (s.y == pl::NONE || s.y + M <= P.up_doubles));
    EXPECT(s.A == pl::NONE || s.At + sh[b].rows_var <= P.up_doubles);
    EXPECT(s.out >= P.down_off && s.out + miosqp::polm_out_stride(sh[b].n, sh[b].M) <= P.pinned_doubles);
    slab_max = std::max(slab_max, miosqp::polish_many_large_slab_doubles(sh[b].n, sh[b].M));
  }
  for (int w = 0; w < P.W; w++) iv.push_back({P.slab_off + (size_t)w * P.slab_doubles, P.slab_off + (size_t)(w + 1) * P.slab_doubles});
  std::sort(iv.begin(), iv.end());
  for (size_t k = 0; k < iv.size(); k++) {
    EXPECT(iv[k].first <= iv[k].second && iv[k].second <= P.total_doubles);
    if (k) EXPECT(iv[k - 1].second <= iv[k].first);
  }
  // the plan is what the host and the workgroups write through: fill every part of a real buffer (the sanitizer watches
  // the ends)
  std::vector<double> arena(P.total_doubles, 0.0);
  for (const auto &p : iv)
    for (size_t i = p.first; i < p.second; i++) arena[i] += 1.0;
  size_t twice = 0;
  for (const auto &p : iv)
    for (size_t i = p.first; i < p.second; i++) twice += arena[i] != 1.0;
  EXPECT(twice == 0);
  // a slab is sized for the list's largest model -- here (512, 60) -- and every model's carve-up lies inside it
  EXPECT(P.slab_doubles == slab_max && P.slab_doubles == miosqp::polish_many_large_slab_doubles(512, 60));
  for (int b = 0; b < 12; b++) {
    const miosqp::PolgSlab o = miosqp::polg_layout(sh[b].n, sh[b].M);
    EXPECT(o.total <= P.slab_doubles && o.cls + ((size_t)2 * sh[b].M + 7) / 8 <= o.total && o.act + ((size_t)sh[b].M + 1) / 2 <= o.cls);
    EXPECT(o.S + (size_t)sh[b].n * o.ld <= o.Wp && o.prow + (size_t)sh[b].M <= o.act);
  }
  // ... and it does not depend on the order of the list
  std::vector<pl::Shape> rev(sh.rbegin(), sh.rend());
  EXPECT(pl::plan(rev, cus).slab_doubles == P.slab_doubles && pl::plan(rev, cus).total_doubles == P.total_doubles);
  // a one-model list takes that model's own figure and one workgroup
  EXPECT(pl::plan({sh[0]}, cus).slab_doubles == miosqp::polish_many_large_slab_doubles(60, 133) && pl::plan({sh[0]}, cus).W == 1);
}

int main() {
  refusals();
  fit_rule();
  workgroups();
  layout_of_twelve();
  if (fails) {
    std::printf("%d failures\n", fails);
    return 1;
  }
  std::printf("polish_models_large_plan ok\n");
  return 0;
}
