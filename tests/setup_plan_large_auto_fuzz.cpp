// Stand-alone check of miosqp_amd/csrc/setup_plan.hpp for the large launch that chooses rho (the host logic of
// miosqp_qp_setup_models_large_auto that needs neither an engine nor a device), built with -fsanitize=address,undefined by
// tests/test_setup_models_large_auto_cpu.py, beside setup_plan_large_fuzz.cpp: the size rule on the whole grid -- n up to
// 197, the edge shapes, one launch per model, every (n, M) the reduced trees take with 256 leaf places --; over random
// lists of small / large x fixed / auto shapes the parts of the arena never overlap and each launch gets its own LDS
// size; with the new flag off every refusal of setup_plan_large_fuzz.cpp still happens; with it on a large rho_auto
// model beyond the rule is refused with its position.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "../miosqp_amd/csrc/setup_plan.hpp"
#include "../miosqp_amd/csrc/tree_reduced_body.hpp"

namespace sm = miosqp::setup_models;

#define REQUIRE(c)                                                      \
  do {                                                                  \
    if (!(c)) {                                                         \
      fprintf(stderr, "%s:%d: REQUIRE(%s) failed\n", __FILE__, __LINE__, #c); \
      exit(1);                                                          \
    }                                                                   \
  } while (0)

static void check_size_rule() {
  namespace tr = miosqp::tree_reduced;
  int n_max = 0;
  size_t taken = 0, by_tree = 0, need_max = 0;
  int at_n = 0, at_M = 0;
  for (int n = 1; n <= 230; n++)
    for (int M = 1; M <= 2300; M++) {
      const bool s = sm::eligible_shape(n, M), l = sm::eligible_shape_large(n, M), a = sm::eligible_shape_large_auto(n, M);
      REQUIRE(!(s && l) && !(s && a));  // a model belongs to exactly one launch
      if (a) {
        REQUIRE(l);  // ... the large one, whose fixed-rho rule holds as well
        const size_t need = sm::lds_doubles_large_auto(n, M) * sizeof(double);
        REQUIRE(sm::lds_doubles_large_auto(n, M) == sm::lds_doubles_large(n, M) + sm::probe_doubles(n, M));
        REQUIRE(sm::lds_doubles_large_auto(n, M) == sm::tri((size_t)n) + 4 * (size_t)n + 3 * (size_t)M + 16);
        REQUIRE(need <= sm::LDS_LIMIT);
        if (need > need_max) need_max = need, at_n = n, at_M = M;
        n_max = std::max(n_max, n);
        taken++;
      } else if (l) {
        REQUIRE(sm::lds_doubles_large_auto(n, M) * sizeof(double) > sm::LDS_LIMIT);
      }
      // every shape the large tree launch solves (256 leaf places) beyond the small launch is taken
      if (!s && tr::lds_doubles(n, M, 256) * sizeof(double) <= tr::LDS_LIMIT) {
        REQUIRE(a);
        by_tree++;
      }
    }
  REQUIRE(n_max == 197);
  REQUIRE(need_max == 163832 && at_n == 168 && at_M == 1865);
  REQUIRE(by_tree == 131333);
  REQUIRE(taken >= by_tree);
  REQUIRE(!sm::eligible_shape_large_auto(198, 3) && sm::eligible_shape_large(198, 3));
  REQUIRE(sm::lds_doubles_large_auto(198, 3) * sizeof(double) == 164144);
  REQUIRE(sm::eligible_shape_large_auto(197, 3) && sm::lds_doubles_large_auto(197, 3) * sizeof(double) == 162528);
  const int grid[][2] = {{50, 210}, {100, 215}, {150, 105}, {150, 320}, {100, 93}, {20, 174}, {197, 3}, {20, 534}, {80, 140}};
  for (const auto &g : grid) {
    REQUIRE(sm::eligible_shape_large_auto(g[0], g[1]) && !sm::eligible_shape(g[0], g[1]));
    if (g[0] <= 150) REQUIRE(sm::lds_doubles_large_auto(g[0], g[1]) * sizeof(double) <= 103 * 1024);
  }
  REQUIRE(!sm::eligible_shape_large_auto(0, 300) && !sm::eligible_shape_large_auto(100, 0) && !sm::eligible_shape_large_auto(100, 92));
  // the settings: rho_auto = 1 only with the flag, everything else as without it
  sm::Args a;
  REQUIRE(sm::eligible_settings_large(a) && sm::eligible_settings_large(a, true));
  a.rho_auto = 1;
  REQUIRE(!sm::eligible_settings_large(a) && sm::eligible_settings_large(a, true));
  a.rho_auto = 2;
  REQUIRE(!sm::eligible_settings_large(a, true));
  for (int k = 1; k < 6; k++) {
    sm::Args b;
    b.rho_auto = 1;
    if (k == 1) b.coop = 1;
    if (k == 2) b.resident = 1;
    if (k == 3) b.fold = 0;
    if (k == 4) b.setup_on_device = 1;
    if (k == 5) b.pers = 1;
    REQUIRE(!sm::eligible_settings_large(b, true));
  }
}

static sm::Shape random_shape(std::mt19937 &rng, bool large, bool rho_auto) {
  sm::Shape s;
  s.rho_auto = rho_auto ? 1 : 0;
  if (large) {
    do {
      s.n = 1 + (int)(rng() % 198u);
      s.M = 1 + (int)(rng() % 700u);
    } while (!(rho_auto ? sm::eligible_shape_large_auto(s.n, s.M) : sm::eligible_shape_large(s.n, s.M)));
    s.form = sm::FORM_LARGE;
  } else {
    s.n = 1 + (int)(rng() % 191u);
    s.M = 1 + (int)(rng() % (unsigned)(sm::MAX_NM - s.n));
    REQUIRE(sm::eligible_shape(s.n, s.M));
  }
  const size_t n = (size_t)s.n, M = (size_t)s.M;
  s.nv = 2 * (rng() % (n * M / 2 + 2));
  s.nc = 2 * (rng() % (n * M / 2 + 2));
  s.npb = 2 * (rng() % (n * n / 2 + 2));
  s.npr = 2 * (rng() % (n * n / 2 + 2));
  return s;
}

static void check_layout(std::mt19937 &rng) {
  const int B = 1 + (int)(rng() % 24u);
  std::vector<sm::Shape> sh;
  for (int b = 0; b < B; b++) sh.push_back(random_shape(rng, rng() % 2u, rng() % 2u));
  const sm::Plan P = sm::plan(sh, 8 * (1 + rng() % 64));
  std::vector<std::pair<size_t, size_t>> spans;
  spans.push_back({0, P.table_bytes});
  size_t lds_s = 0, lds_l = 0, ns = 0, nl = 0;
  for (int b = 0; b < B; b++) {
    const sm::Shape &s = sh[(size_t)b];
    const sm::Slot &sl = P.slot[(size_t)b];
    const bool lg = s.form == sm::FORM_LARGE;
    (lg ? nl : ns)++;
    for (int k = 0; k < sm::NPARTS; k++) {
      const sm::Span &p = sl.part[k];
      REQUIRE(p.off + p.bytes <= P.total_bytes);
      if (p.bytes) spans.push_back({p.off, p.bytes});
    }
    const size_t lds = (lg ? (s.rho_auto ? sm::lds_doubles_large_auto(s.n, s.M) : sm::lds_doubles_large(s.n, s.M))
                           : (s.rho_auto ? sm::lds_doubles_auto(s.n, s.M) : sm::lds_doubles(s.n, s.M))) * sizeof(double);
    (lg ? lds_l : lds_s) = std::max(lg ? lds_l : lds_s, lds);
  }
  REQUIRE(P.n_small == ns && P.n_large == nl);
  REQUIRE(lds_s == P.lds_bytes && lds_l == P.lds_bytes_large);  // each launch its own size, the auto models' room in it
  REQUIRE(P.lds_bytes <= sm::LDS_LIMIT && P.lds_bytes_large <= sm::LDS_LIMIT);
  spans.push_back({P.rec_off, P.rec_bytes});
  std::sort(spans.begin(), spans.end());
  size_t at = 0;
  for (const auto &s : spans) {
    REQUIRE(s.first == at);  // each part starts where the one before it ends: no overlap, no hole
    at += s.second;
  }
  REQUIRE(at == P.total_bytes);
}

static sm::Args model(int n, int M, const double *l, const double *u, const void *p) {
  sm::Args a;
  a.n = n; a.M = M;
  a.Pp = a.Pi = a.Px = a.Ap = a.Ai = a.Ax = a.q = a.settings = p;
  a.l = l; a.u = u;
  a.rho = 0.1; a.sigma = 1e-6; a.alpha = 1.6; a.max_iter = 100;
  return a;
}

static void check_args() {
  std::vector<double> l(2100, 0.0), u(2100, 1.0), lx(2100, 0.0);
  lx[7] = 2.0;
  int dummy = 0;
  const void *p = &dummy;
  std::string err;
  const sm::Args small = model(10, 7, l.data(), u.data(), p), big = model(150, 320, l.data(), u.data(), p);
  // `on`: the value of the new flag.  Every refusal of setup_plan_large_fuzz.cpp, with the flag off (the calls of that
  // file leave it out: the same overload) and, where the flag does not bear on it, with the flag on
  auto refused = [&](const sm::Args &bad, int code, bool auto_flag, bool on, const char *word) {
    for (int pos = 0; pos < 3; pos++) {
      std::vector<sm::Args> v{big, small, small};
      v[(size_t)pos] = bad;
      std::string e;
      REQUIRE(sm::check_args(3, v.data(), p, p, e, auto_flag, true, on) == code);
      REQUIRE(e.find("(model " + std::to_string(pos) + ")") != std::string::npos);
      if (word) REQUIRE(e.find(word) != std::string::npos);
    }
  };
  sm::Args b;
  for (int flag = 0; flag < 2; flag++)
    for (int on = 0; on < 2; on++) {
      if (!on) {
        b = big; b.rho_auto = 1; refused(b, sm::ERR_UNSUPPORTED, flag != 0, false, "the large launch builds a fixed rho only");
      }
      b = big; b.coop = 1; refused(b, sm::ERR_UNSUPPORTED, flag != 0, on != 0, "large launch");
      b = big; b.resident = 1; refused(b, sm::ERR_UNSUPPORTED, flag != 0, on != 0, "large launch");
      b = big; b.fold = 0; refused(b, sm::ERR_UNSUPPORTED, flag != 0, on != 0, "large launch");
      b = big; b.pers = 2; refused(b, sm::ERR_UNSUPPORTED, flag != 0, on != 0, "large launch");
      b = big; b.setup_on_device = 1; refused(b, sm::ERR_UNSUPPORTED, flag != 0, on != 0, "large launch");
      b = model(199, 3, l.data(), u.data(), p); refused(b, sm::ERR_UNSUPPORTED, flag != 0, on != 0, "neither launch");
      b = model(100, 1949, l.data(), u.data(), p); refused(b, sm::ERR_UNSUPPORTED, flag != 0, on != 0, "neither launch");
      b = big; b.n = 0; refused(b, sm::ERR_ARG, flag != 0, on != 0, nullptr);
      b = big; b.q = nullptr; refused(b, sm::ERR_ARG, flag != 0, on != 0, nullptr);
      b = big; b.rho = 0.0; refused(b, sm::ERR_ARG, flag != 0, on != 0, nullptr);
      b = model(150, 320, lx.data(), u.data(), p); refused(b, sm::ERR_ARG, flag != 0, on != 0, "lower bound");
      b = big; b.n_int = 5; b.m_orig = 300; b.i_idx = p; refused(b, sm::ERR_ARG, flag != 0, on != 0, nullptr);
      b = big; b.l_root = l.data(); b.u_root = u.data(); refused(b, sm::ERR_ARG, flag != 0, on != 0, nullptr);
      b = small; b.coop = 1; refused(b, sm::ERR_UNSUPPORTED, flag != 0, on != 0, nullptr);
      b = small; b.resident = 0; refused(b, sm::ERR_UNSUPPORTED, flag != 0, on != 0, nullptr);
      // a large rho_auto model with settings of another form stays out with the flag on as well
      b = big; b.rho_auto = 1; b.coop = 1; refused(b, sm::ERR_UNSUPPORTED, flag != 0, on != 0, on ? "large launch" : "rho_auto");
    }
  // the new flag decides for the large models only: a small rho_auto model still needs rho_auto_in_launch
  b = small; b.rho_auto = 1;
  refused(b, sm::ERR_UNSUPPORTED, false, true, nullptr);
  // with the flag on: the four kinds in one list, at every position of the large rho_auto model
  sm::Args big_auto = big, small_auto = small;
  big_auto.rho_auto = 1;
  small_auto.rho_auto = 1;
  for (int pos = 0; pos < 4; pos++) {
    std::vector<sm::Args> v{small, small_auto, big, small};
    v[(size_t)pos] = big_auto;
    if (pos == 1) v[0] = small_auto;
    REQUIRE(sm::check_args(4, v.data(), p, p, err, true, true, true) == 0);
    REQUIRE(sm::check_args(4, v.data(), p, p, err, true, true) == sm::ERR_UNSUPPORTED);  // flag off: refused by name
    REQUIRE(err.find("rho_auto = 1 beyond n + M = 192") != std::string::npos);
    REQUIRE(err.find("(model " + std::to_string(pos) + ")") != std::string::npos);
  }
  REQUIRE(sm::check_args(1, &big_auto, p, p, err, false, true, true) == 0);  // alone, and without rho_auto_in_launch
  // ... and a large rho_auto model beyond the rule is refused with the rule and its position; at a fixed rho it is taken
  for (const auto &g : std::vector<std::pair<int, int>>{{198, 3}, {198, 40}, {168, 1866}}) {
    b = model(g.first, g.second, l.data(), u.data(), p);
    REQUIRE(sm::eligible_shape_large(g.first, g.second));
    REQUIRE(sm::check_args(1, &b, p, p, err, false, true, true) == 0);
    b.rho_auto = 1;
    refused(b, sm::ERR_UNSUPPORTED, false, true, "n <= 197");
    refused(b, sm::ERR_UNSUPPORTED, true, true, "probing iterations");
  }
  b = model(197, 3, l.data(), u.data(), p);
  b.rho_auto = 1;
  REQUIRE(sm::check_args(1, &b, p, p, err, false, true, true) == 0);
  b = model(168, 1865, l.data(), u.data(), p);
  b.rho_auto = 1;
  REQUIRE(sm::check_args(1, &b, p, p, err, false, true, true) == 0);
}

int main() {
  std::mt19937 rng(20250311u);
  for (int t = 0; t < 300; t++) check_layout(rng);
  check_size_rule();
  check_args();
  printf("setup_plan_large_auto ok\n");
  return 0;
}
