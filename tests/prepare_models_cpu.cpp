// The arithmetic of k_prepare_models (miosqp_amd/csrc/prepare_models_body.hpp) run on the CPU: the same phases, a loop
// over the thread index in place of the workgroup, a barrier where the loop ends.  Every case is a raw problem made
// here; the body runs into buffers of exactly the planned lengths, filled with garbage first (it must write every entry,
// pads included), with exactly the LDS the launch would ask for on the heap, and EVERY output -- the four pointer
// arrays, every index, value and pad of the four packed structures, At_val / A_val, D, E, c, their inverses, the scaled
// q -- is compared bit for bit with what scale_problem + pack_factor_rows (factor.cpp) make of the same problem.  Then
// the plan of a call with prepared models: sizes, an exact cover of the arena, the pinned slab holding the download.
// tests/test_prepare_models_cpu.py builds this with -fsanitize=address,undefined and runs it directly.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "../miosqp_amd/csrc/factor.hpp"
#include "../miosqp_amd/csrc/setup_plan.hpp"

namespace sm = miosqp::setup_models;
namespace pm = miosqp::prepare_models;

#define REQUIRE(c)                                                             \
  do {                                                                         \
    if (!(c)) {                                                                \
      fprintf(stderr, "%s:%d: REQUIRE(%s) failed [%s]\n", __FILE__, __LINE__, #c, g_case.c_str()); \
      exit(1);                                                                 \
    }                                                                          \
  } while (0)
static std::string g_case;

struct ExecLoop {
  template <class F>
  void par(F f) {
    for (int t = 0; t < pm::THREADS; t++) f(t);
  }
};

struct Raw {
  int n = 0, M = 0;
  std::vector<int32_t> Pp, Pi, Ap, Ai;
  std::vector<double> Px, Ax, q;
};

enum Edge {
  EMPTY_COL_A = 1, EMPTY_ROW_A = 2, ZERO_COL_P = 4, FULL_P = 8, EXPLICIT_ZERO_A = 16, TINY_COL = 32, HUGE_COL = 64, ZERO_Q = 128
};

// n variables, m rows of density 0.7 and p rows with one entry each (the rows of the integer variables): M = m + p
static Raw make(int n, int m, int p, unsigned edges, unsigned seed) {
  std::mt19937 rng(seed);
  std::normal_distribution<double> g(0.0, 1.0);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  Raw r;
  r.n = n; r.M = m + p;
  const int jc = n > 3 ? 2 : 0, ir = m > 3 ? 1 : -1, jz = n > 4 ? 3 : -1, jt = n > 5 ? 4 : -1, jh = n > 6 ? 5 : -1;
  // P = G G^T-like dense symmetric values on a pattern of density ~0.5, diagonal always there
  std::vector<double> Pd((size_t)n * n, 0.0);
  for (int j = 0; j < n; j++)
    for (int i = 0; i <= j; i++)
      if (i == j || (u(rng) < 0.5 && !(i == jt && j == jh)))  // (no entry couples the tiny column with the huge one)
        Pd[(size_t)i * n + j] = Pd[(size_t)j * n + i] = i == j ? 1.0 + u(rng) * n : g(rng);
  auto col_scale = [&](int j) { return j == jt && (edges & TINY_COL) ? 1e-7 : j == jh && (edges & HUGE_COL) ? 1e7 : 1.0; };
  r.Pp.push_back(0);
  for (int j = 0; j < n; j++) {
    for (int i = 0; i < n; i++) {
      if (Pd[(size_t)i * n + j] == 0.0) continue;
      if (!(edges & FULL_P) && i > j) continue;
      if ((edges & ZERO_COL_P) && (i == jz || j == jz)) continue;  // (row and column: the matrix stays symmetric)
      r.Pi.push_back(i);
      r.Px.push_back(Pd[(size_t)i * n + j] * col_scale(j) * col_scale(i));
    }
    r.Pp.push_back((int32_t)r.Pi.size());
  }
  r.Ap.push_back(0);
  for (int j = 0; j < n; j++) {
    const bool empty = (edges & EMPTY_COL_A) && j == jc;
    for (int i = 0; i < m && !empty; i++) {
      if ((edges & EMPTY_ROW_A) && i == ir) continue;
      if (u(rng) >= 0.7) continue;
      double v = g(rng) * col_scale(j);
      if ((edges & EXPLICIT_ZERO_A) && (i + j) % 7 == 0) v = 0.0;
      r.Ai.push_back(i);
      r.Ax.push_back(v);
    }
    if (j < p && !empty) {
      r.Ai.push_back(m + j);
      r.Ax.push_back(1.0 * col_scale(j));
    }
    r.Ap.push_back((int32_t)r.Ai.size());
  }
  r.q.resize(n);
  for (int j = 0; j < n; j++) r.q[j] = (edges & ZERO_Q) ? 0.0 : g(rng);
  return r;
}

template <class T>
static bool same(const std::vector<T> &a, const T *b, size_t count) {
  return a.size() == count && (count == 0 || memcmp(a.data(), b, count * sizeof(T)) == 0);
}

static void check(const Raw &r, int passes, double rho) {
  const int n = r.n, M = r.M;
  REQUIRE(sm::csc_strictly_ascending(n, r.Pp.data(), r.Pi.data()) && sm::csc_strictly_ascending(n, r.Ap.data(), r.Ai.data()));
  miosqp::Scaled sc;
  miosqp::scale_problem(n, M, r.Pp.data(), r.Pi.data(), r.Px.data(), r.Ap.data(), r.Ai.data(), r.Ax.data(), r.q.data(), passes, sc);
  miosqp::Factor f;
  f.n = n; f.M = M; f.rho = rho; f.sigma = 1e-6; f.ld = (n + 15) & ~15;
  miosqp::pack_factor_rows(sc, r.Pp.data(), r.Pi.data(), r.Px.data(), rho, f);

  std::vector<int32_t> pv_ptr(n + 1, -1), pc_ptr(M + 1, -1), pb_ptr(n + 1, -1);
  int64_t up = 0;
  pm::prepare_pointers(n, M, r.Pp.data(), r.Pi.data(), r.Ap.data(), r.Ai.data(), pv_ptr.data(), pc_ptr.data(), pb_ptr.data(), &up);
  REQUIRE(pv_ptr == f.panel_by_var.ptr && pc_ptr == f.panel_by_con.ptr && pb_ptr == f.Pbar.ptr && pb_ptr == f.Praw.ptr);
  REQUIRE((size_t)up == sc.Pi.size());
  const size_t nv = (size_t)pv_ptr[n], nc = (size_t)pc_ptr[M], np = (size_t)pb_ptr[n];
  const double junk = -777.25;
  std::vector<int> pv_idx(nv, -9), pc_idx(nc, -9), pb_idx(np, -9), pr_idx(np, -9);
  std::vector<double> pv_L(nv, junk), pv_At(nv, junk), pc_L(nc, junk), pc_A(nc, junk), pb_val(np, junk), pr_val(np, junk);
  std::vector<double> D(n, junk), Dinv(n, junk), E(M, junk), Einv(M, junk), q(n, junk);
  std::vector<double> lds(pm::lds_doubles(n, M), junk);  // exactly the LDS of the launch: the sanitizer sees a phase run past it
  pm::Scalars scal{junk, junk};
  pm::IO io{};
  io.n = n; io.M = M; io.passes = passes; io.rho = rho;
  io.Pp = r.Pp.data(); io.Pi = r.Pi.data(); io.Px = r.Px.data(); io.Ap = r.Ap.data(); io.Ai = r.Ai.data(); io.Ax = r.Ax.data();
  io.qraw = r.q.data();
  io.pv_ptr = pv_ptr.data(); io.pc_ptr = pc_ptr.data(); io.pb_ptr = pb_ptr.data(); io.pr_ptr = pb_ptr.data();
  io.pv_idx = pv_idx.data(); io.pc_idx = pc_idx.data(); io.pb_idx = pb_idx.data(); io.pr_idx = pr_idx.data();
  io.pv_L = pv_L.data(); io.pv_At = pv_At.data(); io.pc_L = pc_L.data(); io.pc_A = pc_A.data();
  io.pb_val = pb_val.data(); io.pr_val = pr_val.data();
  io.D = D.data(); io.Dinv = Dinv.data(); io.E = E.data(); io.Einv = Einv.data(); io.q = q.data();
  io.sc = &scal;
  ExecLoop x;
  pm::body(io, lds.data(), x);

  REQUIRE(same(f.panel_by_var.idx, pv_idx.data(), nv));
  REQUIRE(same(f.panel_by_var.val, pv_L.data(), nv));
  REQUIRE(same(f.At_val, pv_At.data(), nv));
  REQUIRE(same(f.panel_by_con.idx, pc_idx.data(), nc));
  REQUIRE(same(f.panel_by_con.val, pc_L.data(), nc));
  REQUIRE(same(f.A_val, pc_A.data(), nc));
  REQUIRE(same(f.Pbar.idx, pb_idx.data(), np));
  REQUIRE(same(f.Pbar.val, pb_val.data(), np));
  REQUIRE(same(f.Praw.idx, pr_idx.data(), np));
  REQUIRE(same(f.Praw.val, pr_val.data(), np));
  REQUIRE(same(sc.D, D.data(), (size_t)n) && same(sc.Dinv, Dinv.data(), (size_t)n));
  REQUIRE(same(sc.E, E.data(), (size_t)M) && same(sc.Einv, Einv.data(), (size_t)M));
  REQUIRE(same(sc.q, q.data(), (size_t)n));
  REQUIRE(memcmp(&sc.c, &scal.c, 8) == 0 && memcmp(&sc.cinv, &scal.cinv, 8) == 0);
  // what the host's mirror of the scaled CSC is read from: a column of P's upper triangle opens its row of Pbar, a column
  // of A is its row by variable
  for (int j = 0; j < n; j++) {
    const size_t cp = (size_t)(sc.Pp[j + 1] - sc.Pp[j]), ca = (size_t)(sc.Ap[j + 1] - sc.Ap[j]);
    REQUIRE(cp == 0 || memcmp(sc.Px.data() + sc.Pp[j], pb_val.data() + pb_ptr[j], sizeof(double) * cp) == 0);
    REQUIRE(ca == 0 || memcmp(sc.Ax.data() + sc.Ap[j], pv_At.data() + pv_ptr[j], sizeof(double) * ca) == 0);
  }
}

// the edge cases really are in the problem (a generator that forgot one would let the test pass for nothing)
static void check_edges_present(const Raw &r, unsigned edges) {
  const int n = r.n, M = r.M;
  std::vector<int> rowc(M, 0);
  bool empty_col = false, zero = false, lower = false, pcol0 = false, odd = false, even = false;
  for (int j = 0; j < n; j++) {
    const int c = r.Ap[j + 1] - r.Ap[j];
    empty_col |= c == 0;
    odd |= (c & 1) == 1;
    even |= c > 0 && (c & 1) == 0;
    for (int p = r.Ap[j]; p < r.Ap[j + 1]; p++) {
      rowc[r.Ai[p]]++;
      zero |= r.Ax[p] == 0.0;
    }
    pcol0 |= r.Pp[j + 1] == r.Pp[j];
    for (int p = r.Pp[j]; p < r.Pp[j + 1]; p++) lower |= r.Pi[p] > j;
  }
  if (edges & EMPTY_COL_A) REQUIRE(empty_col);
  if (edges & EMPTY_ROW_A) REQUIRE(std::count(rowc.begin(), rowc.end(), 0) > 0);
  if (edges & ZERO_COL_P) REQUIRE(pcol0);
  if (edges & FULL_P) REQUIRE(lower);
  if (edges & EXPLICIT_ZERO_A) REQUIRE(zero);
  if (n > 8) REQUIRE(odd && even);
  auto colnorm = [&](int j) {
    double m = 0;
    for (int p = r.Ap[j]; p < r.Ap[j + 1]; p++) m = std::max(m, std::fabs(r.Ax[p]));
    for (int k = 0; k < n; k++)
      for (int p = r.Pp[k]; p < r.Pp[k + 1]; p++)
        if (r.Pi[p] <= k && (r.Pi[p] == j || k == j)) m = std::max(m, std::fabs(r.Px[p]));
    return m;
  };
  if (edges & TINY_COL) REQUIRE(colnorm(4) < pm::MIN_SCALING && colnorm(4) > 0);
  if (edges & HUGE_COL) REQUIRE(colnorm(5) > pm::MAX_SCALING);
}

static void check_plan() {
  g_case = "plan";
  std::mt19937 rng(7u);
  for (int t = 0; t < 200; t++) {
    const int B = 1 + (int)(rng() % 12);
    std::vector<sm::Shape> sh;
    for (int b = 0; b < B; b++) {
      sm::Shape s;
      const bool lg = rng() % 2;
      s.n = 1 + (int)(rng() % 190);
      s.M = lg ? 193 - std::min(s.n, 192) + (int)(rng() % 400) : 1 + (int)(rng() % (unsigned)(sm::MAX_NM - s.n));
      s.form = sm::eligible_shape(s.n, s.M) ? sm::FORM_SMALL : sm::FORM_LARGE;
      s.nnzA = rng() % (unsigned)(s.n * s.M + 1);
      s.nnzP = rng() % (unsigned)(s.n * s.n + 1);
      s.nv = 2 * ((s.nnzA + s.n) / 2); s.nc = 2 * ((s.nnzA + s.M) / 2);
      s.npb = s.npr = 2 * ((s.nnzP + s.n) / 2);
      s.rho_auto = rng() % 2;
      s.prepare = 1;
      sh.push_back(s);
    }
    const size_t entry = 8 * (1 + rng() % 64);
    const sm::Plan P = sm::plan(sh, entry, sizeof(pm::IO));
    REQUIRE(P.n_prepare == (size_t)B && P.n_small + P.n_large == (size_t)B);
    REQUIRE(P.ptab_off == P.table_bytes && P.ptab_bytes >= (size_t)B * sizeof(pm::IO) && P.ptab_bytes % sm::ALIGN == 0);
    std::vector<std::pair<size_t, size_t>> spans;
    spans.push_back({0, P.table_bytes});
    spans.push_back({P.ptab_off, P.ptab_bytes});
    spans.push_back({P.rec_off, P.rec_bytes});
    size_t lds = 0;
    for (int b = 0; b < B; b++) {
      const sm::Shape &s = sh[(size_t)b];
      const sm::Slot &sl = P.slot[(size_t)b];
      size_t by[sm::NPARTS];
      sm::part_bytes(s, by);
      for (int k = 0; k < sm::NPARTS; k++) {
        const sm::Span &p = sl.part[k];
        REQUIRE(p.bytes == by[k] && p.off % sm::ALIGN == 0);
        if (p.bytes) spans.push_back({p.off, p.bytes});
        const bool up = p.off + p.bytes <= P.up_bytes, prep = p.off >= P.prep_off && p.off + p.bytes <= P.prep_off + P.prep_bytes;
        if (k < sm::FIRST_PRODUCT) REQUIRE(sm::prepared_uploads(k) ? up : prep);  // the rows and scalings come back, the rest goes up
        else REQUIRE(p.bytes == 0 || p.off >= P.rec_off + P.rec_bytes);
      }
      const size_t want[sm::NRAW] = {(size_t)s.n + 1, s.nnzP, s.nnzP, (size_t)s.n + 1, s.nnzA, s.nnzA};
      for (int k = 0; k < sm::NRAW; k++) {
        const size_t el = (k == sm::RAW_PX || k == sm::RAW_AX) ? 8 : 4;
        REQUIRE(sl.raw[k].bytes >= want[k] * el && sl.raw[k].off % sm::ALIGN == 0 && sl.raw[k].off + sl.raw[k].bytes <= P.up_bytes);
        spans.push_back({sl.raw[k].off, sl.raw[k].bytes});
      }
      REQUIRE(sl.scal.bytes >= sizeof(pm::Scalars) && sl.scal.off >= P.prep_off && sl.scal.off + sl.scal.bytes <= P.prep_off + P.prep_bytes);
      spans.push_back({sl.scal.off, sl.scal.bytes});
      REQUIRE(sl.part[sm::PV_IDX].bytes >= s.nv * 4 && sl.part[sm::PC_A].bytes >= s.nc * 8 && sl.part[sm::PR_VAL].bytes >= s.npr * 8);
      REQUIRE(sl.rec == P.rec_off + (size_t)b * sizeof(sm::Record));
      lds = std::max(lds, pm::lds_doubles(s.n, s.M) * sizeof(double));
    }
    REQUIRE(lds == P.lds_bytes_prepare && lds <= 64 * 1024);
    std::sort(spans.begin(), spans.end());
    size_t at = 0;
    for (const auto &s : spans) {  // an exact cover: each part starts where the one before it ends
      REQUIRE(s.first == at);
      at += s.second;
    }
    REQUIRE(at == P.total_bytes);
    // one download: rows and scalings, the records right behind them; the slab holds it behind image and staging
    REQUIRE(P.rec_off == P.prep_off + P.prep_bytes && P.prep_off == P.up_bytes);
    REQUIRE(P.pin_rec == P.pin_prep + P.prep_bytes && P.pin_bytes == P.pin_rec + P.rec_bytes);
    REQUIRE(P.pin_prep >= P.up_bytes && P.pin_prep % sm::ALIGN == 0);
    for (int b = 0; b < B; b++) REQUIRE(P.slot[(size_t)b].pin_ctrl2 + 2 * sm::CTRL_BYTES <= P.pin_prep);
    // the same shapes without the keyword: the plan of before (no table of the new launch, the records at the end)
    for (auto &s : sh) s.prepare = 0;
    const sm::Plan Q = sm::plan(sh, entry);
    REQUIRE(Q.n_prepare == 0 && Q.ptab_bytes == 0 && Q.prep_bytes == 0 && Q.pin_prep == 0 && Q.lds_bytes_prepare == 0);
    REQUIRE(Q.rec_off + Q.rec_bytes == Q.total_bytes && Q.pin_bytes == Q.pin_rec + Q.rec_bytes);
    for (int b = 0; b < B; b++)
      for (int k = 0; k < sm::NRAW; k++) REQUIRE(Q.slot[(size_t)b].raw[k].bytes == 0);
  }
}

int main() {
  const unsigned ALL = EMPTY_COL_A | EMPTY_ROW_A | ZERO_COL_P | FULL_P | EXPLICIT_ZERO_A | TINY_COL | HUGE_COL;
  struct Case {
    int n, m, p;
    unsigned edges;
  };
  const Case cases[] = {
      {10, 5, 2, 0},          {10, 5, 2, ALL},        {10, 5, 2, ZERO_Q | FULL_P},
      {100, 80, 12, ALL},     {100, 81, 12, ALL | ZERO_Q},  // n + M = 192 and 193
      {50, 200, 10, 0},       {50, 200, 10, ALL},
      {20, 530, 4, ALL},      // M > 512
      {198, 1, 1, FULL_P | EXPLICIT_ZERO_A | TINY_COL | HUGE_COL | ZERO_COL_P},  // n = 198, M = 2
      {1, 1, 0, 0},
  };
  int count = 0;
  for (const Case &c : cases) {
    const Raw r = make(c.n, c.m, c.p, c.edges, 1000u + (unsigned)count);
    g_case = "n " + std::to_string(c.n) + " M " + std::to_string(c.m + c.p) + " edges " + std::to_string(c.edges);
    check_edges_present(r, c.edges);
    for (int passes : {0, 1, 10}) {
      g_case += " passes " + std::to_string(passes);
      check(r, passes, count % 2 ? 0.1 : 1.7);
    }
    count++;
  }
  check_plan();
  printf("prepare_models ok (%d problems x 3 scalings)\n", count);
  return 0;
}
