// Stand-alone check of miosqp_amd/csrc/setup_plan.hpp with MIXED forms (the host logic of miosqp_qp_setup_models_large that
// needs neither an engine nor a device), built with -fsanitize=address,undefined by tests/test_setup_models_large_cpu.py:
// over random lists of small and large shapes the parts of the arena never overlap and stay inside it, a large slot has
// no bytes for W and Kc, the table holds the small models first, each launch gets its own LDS size; the size rule of the
// large launch on the whole grid -- among it every (n, M) the reduced trees take with 256 leaf places --; and every refusal
// names the caller's position.
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

static sm::Shape random_shape(std::mt19937 &rng, bool large) {
  sm::Shape s;
  if (large) {
    do {
      s.n = 1 + (int)(rng() % 198u);
      s.M = 1 + (int)(rng() % 700u);
    } while (!sm::eligible_shape_large(s.n, s.M));
    s.form = sm::FORM_LARGE;
  } else {
    s.n = 1 + (int)(rng() % 191u);
    s.M = 1 + (int)(rng() % (unsigned)(sm::MAX_NM - s.n));
    REQUIRE(sm::eligible_shape(s.n, s.M));
    s.rho_auto = (int)(rng() % 2u);
  }
  const size_t n = (size_t)s.n, M = (size_t)s.M;
  s.nv = 2 * (rng() % (n * M / 2 + 2));
  s.nc = 2 * (rng() % (n * M / 2 + 2));
  s.npb = 2 * (rng() % (n * n / 2 + 2));
  s.npr = 2 * (rng() % (n * n / 2 + 2));
  return s;
}

static void check_layout(std::mt19937 &rng) {
  const int B = 1 + (int)(rng() % 24u), mode = (int)(rng() % 4u);  // all small, all large, two mixtures
  std::vector<sm::Shape> sh;
  for (int b = 0; b < B; b++) sh.push_back(random_shape(rng, mode == 1 || (mode >= 2 && rng() % 2u)));
  const size_t entry = 8 * (1 + rng() % 64);
  const sm::Plan P = sm::plan(sh, entry);
  REQUIRE(P.slot.size() == (size_t)B);
  std::vector<std::pair<size_t, size_t>> spans;
  spans.push_back({0, P.table_bytes});
  size_t sum = P.table_bytes, lds_s = 0, lds_l = 0, ns = 0, nl = 0;
  std::vector<int> seen((size_t)B, 0);
  size_t next_s = 0, next_l = 0;
  for (int b = 0; b < B; b++) nl += sh[(size_t)b].form == sm::FORM_LARGE;
  ns = (size_t)B - nl;
  REQUIRE(P.n_small == ns && P.n_large == nl);
  next_l = ns;
  for (int b = 0; b < B; b++) {
    const sm::Shape &s = sh[(size_t)b];
    const sm::Slot &sl = P.slot[(size_t)b];
    const bool lg = s.form == sm::FORM_LARGE;
    const size_t n = (size_t)s.n, M = (size_t)s.M, N = n + M;
    // the table: small models first, the large ones behind them, each kind in the caller's order; every entry once
    REQUIRE(sl.entry == (lg ? next_l : next_s));
    (lg ? next_l : next_s)++;
    REQUIRE(sl.entry < (size_t)B && !seen[sl.entry]);
    seen[sl.entry] = 1;
    size_t by[sm::NPARTS];
    sm::part_bytes(s, by);
    for (int k = 0; k < sm::NPARTS; k++) {
      const sm::Span &p = sl.part[k];
      REQUIRE(p.bytes == by[k]);
      REQUIRE(p.off % sm::ALIGN == 0 && p.bytes % sm::ALIGN == 0);
      if (lg && (k == sm::W_ || k == sm::KC)) REQUIRE(p.bytes == 0);
      else REQUIRE(p.bytes > 0);
      REQUIRE(p.off + p.bytes <= P.total_bytes);
      REQUIRE((k < sm::FIRST_PRODUCT) == (p.off + p.bytes <= P.up_bytes));
      if (p.bytes) spans.push_back({p.off, p.bytes});
      sum += p.bytes;
    }
    const size_t ld = (n + 15) & ~(size_t)15, ldf = (N + 15) & ~(size_t)15, ldm = (M + 15) & ~(size_t)15;
    REQUIRE(sl.part[sm::F_ROWS].bytes >= (n * ldf + sm::SLACK) * 8 && sl.part[sm::F_ATD].bytes >= (n * ldm + sm::SLACK) * 8);
    REQUIRE(sl.part[sm::F_AD].bytes >= (M * ld + sm::SLACK) * 8 && sl.part[sm::LINV].bytes >= (n * ld + sm::SLACK) * 8);
    if (!lg) REQUIRE(sl.part[sm::W_].bytes >= (N * ((N + 7) & ~(size_t)7) + sm::SLACK) * 8);
    REQUIRE(sl.part[sm::RESERVE].bytes >= sm::round_up(n * 4, 256) + sm::round_up((n * ldf + 64) * 8, 256) + sm::round_up(n * 8, 256));
    REQUIRE(sl.rec == P.rec_off + (size_t)b * sizeof(sm::Record));  // the records stay in the caller's order
    if (lg) lds_l = std::max(lds_l, sm::lds_doubles_large(s.n, s.M) * sizeof(double));
    else lds_s = std::max(lds_s, (s.rho_auto ? sm::lds_doubles_auto(s.n, s.M) : sm::lds_doubles(s.n, s.M)) * sizeof(double));
    REQUIRE(sl.in_cap >= 2 * M + 2 * n && sl.in_cap >= 3 * M + n + 1 && sl.out_cap >= N + 1);
  }
  REQUIRE(next_s == ns && next_l == (size_t)B);
  spans.push_back({P.rec_off, P.rec_bytes});
  sum += P.rec_bytes;
  REQUIRE(sum == P.total_bytes);
  REQUIRE(lds_s == P.lds_bytes && lds_l == P.lds_bytes_large);
  REQUIRE(P.lds_bytes <= sm::LDS_LIMIT && P.lds_bytes_large <= sm::LDS_LIMIT);
  REQUIRE((ns == 0) == (P.lds_bytes == 0) && (nl == 0) == (P.lds_bytes_large == 0));
  std::sort(spans.begin(), spans.end());
  size_t at = 0;
  for (const auto &s : spans) {
    REQUIRE(s.first == at);  // each part starts where the one before it ends: no overlap, no hole
    at += s.second;
  }
  REQUIRE(at == P.total_bytes);
  REQUIRE(P.up_bytes <= P.pin_rec && P.pin_bytes == P.pin_rec + P.rec_bytes);
}

static void check_size_rule() {
  namespace tr = miosqp::tree_reduced;
  int n_max = 0;
  size_t taken = 0, by_tree = 0;
  for (int n = 1; n <= 230; n++)
    for (int M = 1; M <= 2300; M++) {
      const bool s = sm::eligible_shape(n, M), l = sm::eligible_shape_large(n, M);
      REQUIRE(!(s && l));  // a model belongs to one launch
      if (l) {
        REQUIRE(n + M > sm::MAX_NM && n + M <= sm::MAX_NM_LARGE);
        REQUIRE(sm::lds_doubles_large(n, M) * sizeof(double) <= sm::LDS_LIMIT);
        REQUIRE(sm::lds_doubles_large(n, M) == sm::tri((size_t)n) + 3 * (size_t)n + 8);
        n_max = std::max(n_max, n);
        taken++;
        if (M > 1 && n + M - 1 > sm::MAX_NM) REQUIRE(sm::eligible_shape_large(n, M - 1));
      }
      // between the two launches nothing is left out up to n = 198 and n + M = 2048
      if (n <= 198 && n + M <= sm::MAX_NM_LARGE) REQUIRE(s || l);
      if (n > 198 || n + M > sm::MAX_NM_LARGE) REQUIRE(!l);
      // nothing the large tree launch solves (256 leaf places) is left without a set-up launch
      if (tr::lds_doubles(n, M, 256) * sizeof(double) <= tr::LDS_LIMIT) {
        REQUIRE(s || l);
        by_tree++;
      }
    }
  REQUIRE(n_max == 198 && taken > 0 && by_tree > 0);
  REQUIRE(!sm::eligible_shape_large(0, 300) && !sm::eligible_shape_large(100, 0) && !sm::eligible_shape_large(-3, 400));
  const int grid[][2] = {{50, 210}, {100, 215}, {150, 105}, {150, 320}, {100, 93}, {20, 174}, {198, 3}, {20, 534}};
  for (const auto &g : grid) REQUIRE(sm::eligible_shape_large(g[0], g[1]) && !sm::eligible_shape(g[0], g[1]));
  REQUIRE(!sm::eligible_shape_large(199, 3) && !sm::eligible_shape_large(100, 92) && !sm::eligible_shape_large(100, 1949));
  REQUIRE(sm::eligible_shape_large(100, 1948));
  sm::Args a;
  REQUIRE(sm::eligible_settings_large(a));
  a.coop = 0; a.resident = 0; a.fold = 1; a.pers = 0; a.setup_on_device = 0;
  REQUIRE(sm::eligible_settings_large(a));
  for (int k = 0; k < 6; k++) {
    sm::Args b;
    if (k == 0) b.rho_auto = 1;
    if (k == 1) b.coop = 1;
    if (k == 2) b.resident = 1;
    if (k == 3) b.fold = 0;
    if (k == 4) b.setup_on_device = 1;
    if (k == 5) b.pers = 1;
    REQUIRE(!sm::eligible_settings_large(b));
  }
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
  // a mixed list passes with the flag, and is refused at the large model's position without it
  for (int pos = 0; pos < 4; pos++) {
    std::vector<sm::Args> v(4, small);
    v[(size_t)pos] = big;
    REQUIRE(sm::check_args(4, v.data(), p, p, err, false, true) == 0);
    REQUIRE(sm::check_args(4, v.data(), p, p, err, true, true) == 0);
    REQUIRE(sm::check_args(4, v.data(), p, p, err) == sm::ERR_UNSUPPORTED);
    REQUIRE(err.find("(model " + std::to_string(pos) + ")") != std::string::npos);
    REQUIRE(sm::check_args(4, v.data(), p, p, err, true) == sm::ERR_UNSUPPORTED);
  }
  auto refused = [&](const sm::Args &bad, int code, bool auto_flag, const char *word) {
    for (int pos = 0; pos < 3; pos++) {
      std::vector<sm::Args> v{small, big, small};
      std::rotate(v.begin(), v.begin() + 1, v.end());  // big, small, small
      v[(size_t)pos] = bad;
      std::string e;
      REQUIRE(sm::check_args(3, v.data(), p, p, e, auto_flag, true) == code);
      REQUIRE(e.find("(model " + std::to_string(pos) + ")") != std::string::npos);
      if (word) REQUIRE(e.find(word) != std::string::npos);
    }
  };
  sm::Args b;
  for (int flag = 0; flag < 2; flag++) {
    b = big; b.rho_auto = 1; refused(b, sm::ERR_UNSUPPORTED, flag != 0, "rho_auto");  // large and rho_auto: never
    b = big; b.coop = 1; refused(b, sm::ERR_UNSUPPORTED, flag != 0, "large launch");
    b = big; b.resident = 1; refused(b, sm::ERR_UNSUPPORTED, flag != 0, "large launch");
    b = big; b.fold = 0; refused(b, sm::ERR_UNSUPPORTED, flag != 0, "large launch");
    b = big; b.pers = 2; refused(b, sm::ERR_UNSUPPORTED, flag != 0, "large launch");
    b = big; b.setup_on_device = 1; refused(b, sm::ERR_UNSUPPORTED, flag != 0, "large launch");
    b = model(199, 3, l.data(), u.data(), p); refused(b, sm::ERR_UNSUPPORTED, flag != 0, "neither launch");
    b = model(100, 1949, l.data(), u.data(), p); refused(b, sm::ERR_UNSUPPORTED, flag != 0, "neither launch");
    b = big; b.n = 0; refused(b, sm::ERR_ARG, flag != 0, nullptr);
    b = big; b.q = nullptr; refused(b, sm::ERR_ARG, flag != 0, nullptr);
    b = big; b.rho = 0.0; refused(b, sm::ERR_ARG, flag != 0, nullptr);
    b = model(150, 320, lx.data(), u.data(), p); refused(b, sm::ERR_ARG, flag != 0, "lower bound");
    b = big; b.n_int = 5; b.m_orig = 300; b.i_idx = p; refused(b, sm::ERR_ARG, flag != 0, nullptr);  // 300 + 5 != 320
    b = big; b.l_root = l.data(); b.u_root = u.data(); refused(b, sm::ERR_ARG, flag != 0, nullptr);    // a root without integer rows
    b = small; b.coop = 1; refused(b, sm::ERR_UNSUPPORTED, flag != 0, nullptr);                         // the small rule is the old one
    b = small; b.resident = 0; refused(b, sm::ERR_UNSUPPORTED, flag != 0, nullptr);
  }
  b = small; b.rho_auto = 1; refused(b, sm::ERR_UNSUPPORTED, false, nullptr);
  {  // ... and a small rho_auto model beside a large one passes with both flags
    std::vector<sm::Args> v{big, b, small};
    REQUIRE(sm::check_args(3, v.data(), p, p, err, true, true) == 0);
  }
  // a large model with the settings of the engine it becomes, integer rows and a root
  b = big; b.coop = 0; b.resident = 0; b.fold = 1; b.pers = 0; b.n_int = 20; b.m_orig = 300; b.i_idx = p;
  b.l_root = l.data(); b.u_root = u.data();
  REQUIRE(sm::check_args(1, &b, p, p, err, false, true) == 0);  // B = 1: a large model alone
  REQUIRE(sm::check_args(0, &b, p, p, err, false, true) == sm::ERR_ARG);
  REQUIRE(sm::check_args(1, nullptr, p, p, err, false, true) == sm::ERR_ARG);
}

int main() {
  std::mt19937 rng(20250219u);
  for (int t = 0; t < 300; t++) check_layout(rng);
  check_size_rule();
  check_args();
  printf("setup_plan_large ok\n");
  return 0;
}
