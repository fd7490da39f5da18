// Stand-alone check of the argument check miosqp_qp_setup_models_auto adds to miosqp_amd/csrc/setup_plan.hpp, beside
// setup_plan_fuzz.cpp and built like it with -fsanitize=address,undefined: with the flag a list may mix models with
// rho_auto 0 and 1 in any pattern, every other refusal stands at every position with the model named, and without the
// flag the check is the one miosqp_qp_setup_models always had.  The launch that chooses rho takes exactly the shapes the
// fixed-rho launch takes, and the plan asks for the LDS of the largest model in the form it is built in.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
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

static sm::Args good(const double *l, const double *u, const void *p, int rho_auto) {
  sm::Args a;
  a.n = 4; a.M = 3;
  a.Pp = a.Pi = a.Px = a.Ap = a.Ai = a.Ax = a.q = a.settings = p;
  a.l = l; a.u = u;
  a.rho = 0.1; a.sigma = 1e-6; a.alpha = 1.6; a.max_iter = 100;
  a.rho_auto = rho_auto;
  return a;
}

int main() {
  // the size rule does not shrink: every shape of the fixed-rho launch, with the probe's vectors in LDS as well
  for (int n = -1; n <= 200; n++)
    for (int M = -1; M <= 200; M++) {
      REQUIRE(sm::eligible_shape_auto(n, M) == sm::eligible_shape(n, M));
      if (sm::eligible_shape(n, M)) {
        REQUIRE(sm::lds_doubles_auto(n, M) == sm::lds_doubles(n, M) + sm::probe_doubles(n, M));
        REQUIRE(sm::probe_doubles(n, M) >= (size_t)n + 3 * (size_t)M + 2);
        REQUIRE(sm::lds_doubles_auto(n, M) * sizeof(double) <= sm::LDS_LIMIT);
      }
    }
  static_assert(sizeof(sm::Record) == 32, "the record keeps its size");
  const double l[3] = {0, 0, 0}, u[3] = {1, 1, 1}, lx[3] = {0, 2, 0};
  int dummy = 0;
  const void *p = &dummy;
  std::mt19937 rng(20240611u);
  for (int t = 0; t < 2000; t++) {
    const int B = 1 + (int)(rng() % 9);
    std::vector<sm::Args> a;
    bool any = false;
    for (int b = 0; b < B; b++) {
      const int ra = (int)(rng() & 1);
      any = any || ra;
      a.push_back(good(l, u, p, ra));
    }
    std::string err;
    REQUIRE(sm::check_args(B, a.data(), p, p, err, true) == 0);                 // mixed lists pass with the flag
    const int rc = sm::check_args(B, a.data(), p, p, err);                      // ... and without it as they always did
    REQUIRE(rc == (any ? sm::ERR_UNSUPPORTED : 0));
    if (any) {
      int first = 0;
      while (!a[(size_t)first].rho_auto) first++;
      REQUIRE(err.find("model " + std::to_string(first) + ")") != std::string::npos && err.find("a fixed rho") != std::string::npos);
    }
    // every other refusal stands with the flag, at a random position, whatever the rho_auto pattern around it
    const int pos = (int)(rng() % (unsigned)B);
    sm::Args &m = a[(size_t)pos];
    const sm::Args keep = m;
    int want = sm::ERR_ARG;
    switch (rng() % 14) {
      case 0: m.n = 0; break;
      case 1: m.M = 0; break;
      case 2: m.Pp = nullptr; break;
      case 3: m.q = nullptr; break;
      case 4: m.settings = nullptr; break;
      case 5: m.rho = 0.0; break;
      case 6: m.alpha = 2.0; break;
      case 7: m.max_iter = 0; break;
      case 8: m.l = lx; break;                                             // l > u
      case 9: m.n_int = 2; m.m_orig = 2; m.i_idx = p; break;               // 2 + 2 != 3
      case 10: m.l_root = l; break;                                        // half a root
      case 11: m.coop = 1; want = sm::ERR_UNSUPPORTED; break;
      case 12: m.n = 150; m.M = 64; want = sm::ERR_UNSUPPORTED; break;     // n + M = 214 (l, u are not read: refused first?)
      default: m.rho_auto = 2; want = sm::ERR_UNSUPPORTED; break;          // neither 0 nor 1
    }
    if (m.n == 150) {  // (a model of 64 rows needs bounds of 64 entries)
      static const std::vector<double> l64(64, 0.0), u64(64, 1.0);
      m.l = l64.data();
      m.u = u64.data();
    }
    std::string e2;
    REQUIRE(sm::check_args(B, a.data(), p, p, e2, true) == want);
    REQUIRE(e2.find("model " + std::to_string(pos) + ")") != std::string::npos);
    m = keep;
    REQUIRE(sm::check_args(B, a.data(), p, p, e2, true) == 0);
  }
  {
    std::vector<sm::Args> a(2, good(l, u, p, 1));
    std::string err;
    REQUIRE(sm::check_args(0, a.data(), p, p, err, true) == sm::ERR_ARG);
    REQUIRE(sm::check_args(2, nullptr, p, p, err, true) == sm::ERR_ARG);
    REQUIRE(sm::check_args(2, a.data(), nullptr, p, err, true) == sm::ERR_ARG);
    REQUIRE(sm::check_args(2, a.data(), p, nullptr, err, true) == sm::ERR_ARG);
    sm::Args s;
    REQUIRE(sm::eligible_settings(s) && sm::eligible_settings(s, true));
    s.rho_auto = 1;
    REQUIRE(!sm::eligible_settings(s) && sm::eligible_settings(s, true));
    s.fold = 0;
    REQUIRE(!sm::eligible_settings(s, true));
  }
  {  // the plan's LDS: the largest model in the form it is built in
    std::vector<sm::Shape> sh(3);
    sh[0].n = 100; sh[0].M = 92;
    sh[1].n = 10; sh[1].M = 7; sh[1].rho_auto = 1;
    sh[2].n = 50; sh[2].M = 60;
    REQUIRE(sm::plan(sh, 256).lds_bytes == sm::lds_doubles(100, 92) * sizeof(double));
    sh[0].rho_auto = 1;
    REQUIRE(sm::plan(sh, 256).lds_bytes == sm::lds_doubles_auto(100, 92) * sizeof(double));
    REQUIRE(sm::plan(sh, 256).lds_bytes <= sm::LDS_LIMIT);
  }
  printf("setup_plan auto ok\n");
  return 0;
}
