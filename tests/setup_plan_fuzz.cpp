// Stand-alone check of miosqp_amd/csrc/setup_plan.hpp (the host logic of miosqp_qp_setup_models that needs neither an
// engine nor a device), built with -fsanitize=address,undefined by tests/test_setup_models_cpu.py: over random shapes the
// parts of the arena never overlap, are aligned and stay inside it, the totals are the sums of the parts, the pinned
// slab holds the upload image and every engine's staging, eligibility is monotone, and every bad argument is refused
// with the model's position in the text.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "../miosqp_amd/csrc/setup_plan.hpp"

namespace sm = miosqp::setup_models;

#define REQUIRE(c)                                                      \
  do {                                                                  \
    if (!(c)) {                                                         \
      fprintf(stderr, "%s:%d: REQUIRE(%s) failed\n", __FILE__, __LINE__, #c); \
      exit(1);                                                          \
    }                                                                   \
  } while (0)

static void check_layout(std::mt19937 &rng) {
  std::uniform_int_distribution<int> nb(1, 40), nn(1, 191);
  const int B = nb(rng);
  std::vector<sm::Shape> sh;
  for (int b = 0; b < B; b++) {
    const int n = nn(rng);
    const int M = 1 + (int)(rng() % (unsigned)(sm::MAX_NM - n));
    REQUIRE(sm::eligible_shape(n, M));
    sm::Shape s;
    s.n = n; s.M = M;
    s.nv = 2 * (rng() % (unsigned)(n * M / 2 + 2));
    s.nc = 2 * (rng() % (unsigned)(n * M / 2 + 2));
    s.npb = 2 * (rng() % (unsigned)(n * n / 2 + 2));
    s.npr = 2 * (rng() % (unsigned)(n * n / 2 + 2));
    sh.push_back(s);
  }
  const size_t entry = 8 * (1 + rng() % 64);
  const sm::Plan P = sm::plan(sh, entry);
  REQUIRE(P.slot.size() == (size_t)B);
  REQUIRE(P.table_bytes >= (size_t)B * entry && P.table_bytes % sm::ALIGN == 0);
  std::vector<std::pair<size_t, size_t>> spans;  // (offset, bytes) of everything in the arena
  spans.push_back({0, P.table_bytes});
  size_t sum = P.table_bytes, lds = 0;
  for (int b = 0; b < B; b++) {
    size_t by[sm::NPARTS];
    sm::part_bytes(sh[(size_t)b], by);
    for (int k = 0; k < sm::NPARTS; k++) {
      const sm::Span &s = P.slot[(size_t)b].part[k];
      REQUIRE(s.bytes == by[k] && s.bytes > 0);
      REQUIRE(s.off % sm::ALIGN == 0 && s.bytes % sm::ALIGN == 0);
      REQUIRE((k < sm::FIRST_PRODUCT) == (s.off + s.bytes <= P.up_bytes));  // uploaded parts, and only they, lie in the image
      REQUIRE(k < sm::FIRST_PRODUCT || s.off >= P.up_bytes);
      spans.push_back({s.off, s.bytes});
      sum += s.bytes;
    }
    const size_t n = (size_t)sh[(size_t)b].n, M = (size_t)sh[(size_t)b].M;
    // room for the data with the slack behind it
    REQUIRE(P.slot[(size_t)b].part[sm::W_].bytes >= ((n + M) * ((n + M + 7) & ~(size_t)7) + sm::SLACK) * 8);
    REQUIRE(P.slot[(size_t)b].part[sm::RAW].bytes >= (3 * M + n) * 8);
    REQUIRE(P.slot[(size_t)b].part[sm::CTRL].bytes >= sm::CTRL_BYTES);
    // what miosqp_qp_set_integer_rows allocates later fits the reserve: int_pos, f_rows2, a_int (each rounded to 256)
    const size_t ld2 = (n + M + 15) & ~(size_t)15;
    REQUIRE(P.slot[(size_t)b].part[sm::RESERVE].bytes >=
            sm::round_up(n * 4, 256) + sm::round_up((n * ld2 + 64) * 8, 256) + sm::round_up(n * 8, 256));
    REQUIRE(P.slot[(size_t)b].rec == P.rec_off + (size_t)b * sizeof(sm::Record));
    lds = std::max(lds, sm::lds_doubles((int)n, (int)M) * sizeof(double));
  }
  spans.push_back({P.rec_off, P.rec_bytes});
  sum += P.rec_bytes;
  REQUIRE(P.rec_bytes >= (size_t)B * sizeof(sm::Record));
  REQUIRE(sum == P.total_bytes);  // the total is the sum of the parts: no holes, hence (with no overlap) an exact cover
  REQUIRE(lds == P.lds_bytes && P.lds_bytes <= sm::LDS_LIMIT);
  std::sort(spans.begin(), spans.end());
  size_t at = 0;
  for (const auto &s : spans) {
    REQUIRE(s.first == at);  // each part starts where the one before it ends
    at += s.second;
  }
  REQUIRE(at == P.total_bytes);
  // the slab: staging of the engines disjoint, aligned, inside; the records behind the larger of image and staging
  std::vector<std::pair<size_t, size_t>> pins;
  for (int b = 0; b < B; b++) {
    const sm::Slot &s = P.slot[(size_t)b];
    const size_t n = (size_t)sh[(size_t)b].n, M = (size_t)sh[(size_t)b].M;
    REQUIRE(s.in_cap >= 2 * M + 2 * n && s.in_cap >= 3 * M + n + 1);            // set-up's staged path, a node's l | u | x | y
    REQUIRE(s.in_cap - 2 * M >= (2 * n + 1) / 2 + n);                              // set_integer_rows' staged path (n_int <= n)
    REQUIRE(s.out_cap >= n + M + 1);
    pins.push_back({s.pin_in, s.in_cap * 8});
    pins.push_back({s.pin_out, s.out_cap * 8});
    pins.push_back({s.pin_ctrl, sm::CTRL_BYTES});
    pins.push_back({s.pin_ctrl2, 2 * sm::CTRL_BYTES});
  }
  std::sort(pins.begin(), pins.end());
  size_t end = 0;
  for (const auto &s : pins) {
    REQUIRE(s.first % sm::ALIGN == 0 && s.first >= end);
    end = s.first + s.second;
  }
  REQUIRE(end <= P.pin_rec && P.up_bytes <= P.pin_rec && P.pin_rec % sm::ALIGN == 0);
  REQUIRE(P.pin_bytes == P.pin_rec + P.rec_bytes);
}

static void check_eligibility() {
  // monotone: a model that fits still fits with fewer variables or fewer rows; the limit is n + M <= 192
  for (int n = 1; n <= 200; n++)
    for (int M = 1; M <= 200; M++) {
      const bool e = sm::eligible_shape(n, M);
      REQUIRE(e == (n + M <= sm::MAX_NM));  // (the LDS need stays below 160 KB on the whole triangle n + M <= 192)
      if (e && n > 1) REQUIRE(sm::eligible_shape(n - 1, M));
      if (e && M > 1) REQUIRE(sm::eligible_shape(n, M - 1));
      if (e) REQUIRE(sm::lds_doubles(n, M) * sizeof(double) <= sm::LDS_LIMIT);
      if (e) REQUIRE(sm::lds_doubles(n, M) >= sm::tri((size_t)n) + (size_t)M * n + 3 * (size_t)n);
      if (e) REQUIRE(sm::lds_doubles(n, M) >= sm::guard_doubles(n, M));
    }
  REQUIRE(!sm::eligible_shape(0, 5) && !sm::eligible_shape(5, 0) && !sm::eligible_shape(-1, 3));
  // the shapes the tests of the set-up kernels use, n = 129 among them
  const int shapes[][2] = {{3, 3}, {63, 25}, {64, 25}, {65, 25}, {128, 40}, {129, 40}, {10, 7}, {100, 92}};
  for (const auto &s : shapes) REQUIRE(sm::eligible_shape(s[0], s[1]));
  REQUIRE(!sm::eligible_shape(200, 150) && !sm::eligible_shape(100, 93));
  sm::Args a;
  REQUIRE(sm::eligible_settings(a));
  for (int k = 0; k < 5; k++) {
    sm::Args b;
    if (k == 0) b.rho_auto = 1;
    if (k == 1) b.coop = 1;
    if (k == 2) b.resident = 0;
    if (k == 3) b.fold = 0;
    if (k == 4) b.setup_on_device = 1;
    REQUIRE(!sm::eligible_settings(b));
  }
}

static sm::Args good(const double *l, const double *u, const void *p) {
  sm::Args a;
  a.n = 4; a.M = 3;
  a.Pp = a.Pi = a.Px = a.Ap = a.Ai = a.Ax = a.q = a.settings = p;
  a.l = l; a.u = u;
  a.rho = 0.1; a.sigma = 1e-6; a.alpha = 1.6; a.max_iter = 100;
  return a;
}

static void check_args() {
  const double l[3] = {0, 0, 0}, u[3] = {1, 1, 1}, lx[3] = {0, 2, 0};
  int dummy = 0;
  const void *p = &dummy;
  std::string err;
  std::vector<sm::Args> a(3, good(l, u, p));
  REQUIRE(sm::check_args(3, a.data(), p, p, err) == 0);
  REQUIRE(sm::check_args(0, a.data(), p, p, err) == sm::ERR_ARG && err.find("at least 1") != std::string::npos);
  REQUIRE(sm::check_args(-2, a.data(), p, p, err) == sm::ERR_ARG);
  REQUIRE(sm::check_args(3, nullptr, p, p, err) == sm::ERR_ARG);
  REQUIRE(sm::check_args(3, a.data(), nullptr, p, err) == sm::ERR_ARG);
  REQUIRE(sm::check_args(3, a.data(), p, nullptr, err) == sm::ERR_ARG);
  auto refused = [&](const sm::Args &bad, int code) {
    for (int pos = 0; pos < 3; pos++) {
      std::vector<sm::Args> v(3, good(l, u, p));
      v[(size_t)pos] = bad;
      std::string e;
      REQUIRE(sm::check_args(3, v.data(), p, p, e) == code);
      REQUIRE(e.find("model " + std::to_string(pos)) != std::string::npos);
    }
  };
  sm::Args b;
  b = good(l, u, p); b.n = 0; refused(b, sm::ERR_ARG);
  b = good(l, u, p); b.M = 0; refused(b, sm::ERR_ARG);
  b = good(l, u, p); b.Pp = nullptr; refused(b, sm::ERR_ARG);
  b = good(l, u, p); b.Ap = nullptr; refused(b, sm::ERR_ARG);
  b = good(l, u, p); b.q = nullptr; refused(b, sm::ERR_ARG);
  b = good(l, u, p); b.l = nullptr; refused(b, sm::ERR_ARG);
  b = good(l, u, p); b.u = nullptr; refused(b, sm::ERR_ARG);
  b = good(l, u, p); b.settings = nullptr; refused(b, sm::ERR_ARG);
  b = good(l, u, p); b.rho = 0.0; refused(b, sm::ERR_ARG);
  b = good(l, u, p); b.sigma = -1.0; refused(b, sm::ERR_ARG);
  b = good(l, u, p); b.alpha = 2.0; refused(b, sm::ERR_ARG);
  b = good(l, u, p); b.max_iter = 0; refused(b, sm::ERR_ARG);
  b = good(lx, u, p); refused(b, sm::ERR_ARG);                       // l > u
  b = good(l, u, p); b.n_int = 2; b.m_orig = 2; b.i_idx = p; refused(b, sm::ERR_ARG);   // 2 + 2 != 3
  b = good(l, u, p); b.n_int = 1; b.m_orig = 2; b.i_idx = nullptr; refused(b, sm::ERR_ARG);
  b = good(l, u, p); b.n_int = 5; b.m_orig = -2; b.i_idx = p; refused(b, sm::ERR_ARG);
  b = good(l, u, p); b.l_root = l; refused(b, sm::ERR_ARG);           // half a root
  b = good(l, u, p); b.l_root = l; b.u_root = u; refused(b, sm::ERR_ARG);  // a root without integer rows
}

int main() {
  std::mt19937 rng(20240607u);
  for (int t = 0; t < 300; t++) check_layout(rng);
  check_eligibility();
  // a shape or settings the launch does not take
  {
    const int M = 64;
    std::vector<double> l((size_t)M, 0.0), u((size_t)M, 1.0);
    int dummy = 0;
    const void *p = &dummy;
    sm::Args a;
    a.n = 150; a.M = M;
    a.Pp = a.Pi = a.Px = a.Ap = a.Ai = a.Ax = a.q = a.settings = p;
    a.l = l.data(); a.u = u.data();
    a.rho = 0.1; a.sigma = 1e-6; a.alpha = 1.6; a.max_iter = 100;
    std::string err;
    REQUIRE(sm::check_args(1, &a, p, p, err) == sm::ERR_UNSUPPORTED && err.find("model 0") != std::string::npos);  // n + M = 214
    a.n = 100;
    REQUIRE(sm::check_args(1, &a, p, p, err) == 0);
    a.rho_auto = 1;
    REQUIRE(sm::check_args(1, &a, p, p, err) == sm::ERR_UNSUPPORTED);
    a.rho_auto = 0; a.n_int = 4; a.m_orig = 60; a.i_idx = p; a.l_root = l.data(); a.u_root = u.data();
    REQUIRE(sm::check_args(1, &a, p, p, err) == 0);
  }
  {
    const int32_t ptr[4] = {0, 2, 2, 5}, ok[5] = {0, 3, 1, 2, 7}, twice[5] = {0, 3, 1, 1, 7}, unsorted[5] = {3, 0, 1, 2, 7};
    REQUIRE(sm::csc_strictly_ascending(3, ptr, ok));
    REQUIRE(!sm::csc_strictly_ascending(3, ptr, twice) && !sm::csc_strictly_ascending(3, ptr, unsorted));
    REQUIRE(sm::csc_strictly_ascending(0, ptr, ok));
  }
  check_args();
  printf("setup_plan ok\n");
  return 0;
}
