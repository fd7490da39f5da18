// The arithmetic of k_tree_r_m's relaxation (miosqp_amd/csrc/tree_reduced_body.hpp) run on the CPU: the same phases, a
// loop over the thread index in place of the workgroup, a barrier where the loop ends.  Reads one problem (CSC P and A,
// q, l, u, rho, sigma, alpha, scaling passes) from a binary file, equilibrates and factorises it as the per-model host
// set-up does (scale_problem, build_factor, build_folded), lays the LDS of one workgroup out on the heap -- exactly the
// doubles the launch would ask for, so the sanitizer sees a phase that runs past it --, and
//   1. checks the carve-up: inside the block, inside 160 KB when asked to, no two arrays that are live together overlap;
//   2. iterates K0 times from zero on the root's bounds (a solved root: the warm start), tightens two rows, and from that
//      start runs 25 and 100 iterations three ways: the reduced phases on the packed rows of Abar, the same on the dense
//      copies, and a plain loop of res_admm's two product-form sweeps on the rows build_folded makes.
// Everything is written out with the scaled problem itself, so that tests/test_tree_reduced_cpu.py can run the
// long-double restatement from the same start on the same numbers.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "../miosqp_amd/csrc/factor.hpp"
#include "../miosqp_amd/csrc/tree_reduced_body.hpp"

namespace tr = miosqp::tree_reduced;

struct ExecLoop {
  template <class F>
  void par(F f) {
    for (int t = 0; t < tr::THREADS; t++) f(t);
  }
  // lane 0 of a group forms every lane's partial sum and adds them as the device's butterfly does
  template <class F>
  double lane_sum(int TG, int t, F f) {
    if (t != 0) return 0.0;
    double v[64];
    for (int k = 0; k < TG; k++) v[k] = f(k);
    for (int s = 1; s < TG; s *= 2)
      for (int k = 0; k < TG; k += 2 * s) v[k] += v[k + s];
    return v[0];
  }
};

template <class T>
static std::vector<T> rd(FILE *f, size_t count) {
  std::vector<T> v(count);
  if (count && fread(v.data(), sizeof(T), count, f) != count) {
    fprintf(stderr, "short input\n");
    exit(2);
  }
  return v;
}
static void wr(FILE *f, const std::vector<double> &v) { fwrite(v.data(), sizeof(double), v.size(), f); }

static int carve_check(int n, int M, int cap, bool must_fit) {
  const tr::Carve c = tr::carve(n, M, cap);
  const size_t un = (size_t)n, uM = (size_t)M, ucap = (size_t)cap;
  // the arrays that are live while a relaxation runs, with the test's scratch ...
  std::vector<std::pair<size_t, size_t>> a = {
      {c.tri, tr::tri_doubles(n)}, {c.d2, un}, {c.wr, uM + un}, {c.x, un}, {c.q, un}, {c.ut, un}, {c.dx, un}, {c.tx, un},
      {c.z, uM}, {c.y, uM}, {c.l, uM}, {c.u, uM}, {c.dy, uM}, {c.part, (size_t)tr::NQ * tr::WAVES}, {c.res, (size_t)tr::NQ + 8},
      {c.lf_lower, ucap}, {c.order, (3 * ucap + 1) / 2}, {c.sc, 32}, {c.iiL, (un + 1) / 2}};
  std::vector<std::pair<size_t, size_t>> test = a, epi = a;
  test.push_back({c.scr, uM});                    // vp
  test.push_back({c.scr + uM, 8 * uM});           // smc
  test.push_back({c.scr + 9 * uM, 4 * un});       // snc
  // ... and while a node's epilogue runs, with its vectors in the same place
  epi.push_back({c.scr, un});                     // xf
  epi.push_back({c.scr + un, un});                // xi
  epi.push_back({c.scr + 2 * un, 2 * un});        // prow
  epi.push_back({c.scr + 4 * un, uM});            // yf
  epi.push_back({c.scr + 4 * un + uM, uM});       // rowbuf
  for (auto *set : {&test, &epi}) {
    std::sort(set->begin(), set->end());
    for (size_t k = 0; k < set->size(); k++) {
      if ((*set)[k].first + (*set)[k].second > c.end) return 1;
      if (k && (*set)[k - 1].first + (*set)[k - 1].second > (*set)[k].first) return 2;
    }
  }
  if (c.end != tr::lds_doubles(n, M, cap)) return 3;
  if (must_fit && c.end * sizeof(double) > tr::LDS_LIMIT) return 4;
  // the packed triangle: every entry has its own place inside the rectangle
  const int ld = tr::tri_ld(n);
  if (ld % 32 != 32 - tr::TGB || tr::TGB * tr::TGC != 32) return 5;
  std::vector<char> seen(tr::tri_doubles(n), 0);
  for (int i = 0; i < n; i++)
    for (int j = 0; j < i; j++) {
      const size_t at = tr::tri_at(n, ld, i, j);
      if (at >= seen.size() || seen[at]) return 6;
      seen[at] = 1;
      if (j + 1 < i && tr::tri_at(n, ld, i, j + 1) != at + tr::tri_step(n, i)) return 7;
    }
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s problem.bin results.bin\n", argv[0]);
    return 2;
  }
  FILE *in = fopen(argv[1], "rb");
  if (!in) return 2;
  const std::vector<int32_t> h = rd<int32_t>(in, 10);
  const int n = h[0], M = h[1], nnzP = h[2], nnzA = h[3], passes = h[4], K0 = h[5], r0 = h[6], r1 = h[7], cap = h[8],
            must_fit = h[9];
  const auto Pp = rd<int32_t>(in, n + 1), Pi = rd<int32_t>(in, nnzP);
  const auto Px = rd<double>(in, nnzP);
  const auto Ap = rd<int32_t>(in, n + 1), Ai = rd<int32_t>(in, nnzA);
  const auto Ax = rd<double>(in, nnzA);
  const auto q = rd<double>(in, n), l = rd<double>(in, M), u = rd<double>(in, M), rs = rd<double>(in, 3);
  fclose(in);
  const double rho = rs[0], sigma = rs[1], alpha = rs[2];
  if (int rc = carve_check(n, M, cap, must_fit != 0)) {
    fprintf(stderr, "carve-up check %d failed\n", rc);
    return 3;
  }
  for (int cc : {1, 2, 3, 256, 1024})
    for (int nn : {1, 2, 3, 4, 5, 31, 32, 33, 150})
      if (int rc = carve_check(nn, nn + 7, cc, false)) {
        fprintf(stderr, "carve-up check %d failed at n = %d, cap = %d\n", rc, nn, cc);
        return 3;
      }
  miosqp::Scaled sc;
  miosqp::scale_problem(n, M, Pp.data(), Pi.data(), Px.data(), Ap.data(), Ai.data(), Ax.data(), q.data(), passes, sc);
  miosqp::Factor f;
  std::string err;
  if (!miosqp::build_factor(sc, Pp.data(), Pi.data(), Px.data(), rho, sigma, f, err)) {
    fprintf(stderr, "build_factor: %s\n", err.c_str());
    return 4;
  }
  miosqp::Folded fo;
  miosqp::build_folded(f, fo);

  std::vector<double> lds(tr::lds_doubles(n, M, cap), std::numeric_limits<double>::quiet_NaN());
  const tr::State s = tr::state(lds.data(), n, M, cap);
  ExecLoop x;
  tr::load_triangle(x, s, fo.rows.data(), fo.ldf, f.d2inv.data());
  tr::Abar A{f.panel_by_var.ptr.data(), f.panel_by_var.idx.data(), f.At_val.data(), f.panel_by_con.ptr.data(),
             f.panel_by_con.idx.data(), f.A_val.data(), fo.Atd.data(), fo.Ad.data(), fo.ldm, fo.ldn, 0};
  const tr::Par par{rho, 1.0 / rho, sigma, alpha};
  const double rinv = par.rinv;

  std::vector<double> ls(M), us(M);
  for (int j = 0; j < M; j++) {
    ls[j] = sc.E[j] * std::fmax(l[j], -1e30);
    us[j] = sc.E[j] * std::fmin(u[j], 1e30);
  }
  auto set_state = [&](const std::vector<double> &xs, const std::vector<double> &zs, const std::vector<double> &ys) {
    for (int i = 0; i < n; i++) {
      s.x[i] = xs[i];
      s.q[i] = sc.q[i];
      s.dx[i] = 0.0;
      s.wr[M + i] = sigma * xs[i] - sc.q[i];
    }
    for (int j = 0; j < M; j++) {
      s.z[j] = zs[j];
      s.y[j] = ys[j];
      s.l[j] = ls[j];
      s.u[j] = us[j];
      s.dy[j] = 0.0;
      s.wr[j] = zs[j] - rinv * ys[j];
    }
  };
  auto get = [&](std::vector<double> &xs, std::vector<double> &zs, std::vector<double> &ys) {
    xs.assign(s.x, s.x + n);
    zs.assign(s.z, s.z + M);
    ys.assign(s.y, s.y + M);
  };
  // ---- the warm start: a solved root ----
  std::vector<double> x0(n, 0.0), z0(M, 0.0), y0(M, 0.0);
  set_state(x0, z0, y0);
  for (int it = 0; it < K0; it++) tr::iterate(x, s, A, par);
  get(x0, z0, y0);
  // ---- two rows tightened: r0 to its lower bound, r1 to its upper bound ----
  us[r0] = ls[r0];
  ls[r1] = us[r1];

  FILE *out = fopen(argv[2], "wb");
  if (!out) return 2;
  wr(out, {(double)lds.size(), (double)tr::tri_ld(n), (double)fo.ldn, (double)fo.ldm});
  wr(out, fo.Ad);
  wr(out, fo.Pd);
  wr(out, sc.q);
  wr(out, ls);
  wr(out, us);
  wr(out, x0);
  wr(out, z0);
  wr(out, y0);
  std::vector<double> xs, zs, ys;
  for (int dense = 0; dense < 2; dense++) {
    A.dense = dense;
    set_state(x0, z0, y0);
    for (int it = 1; it <= 100; it++) {
      tr::iterate(x, s, A, par);
      if (it == 25 || it == 100) {
        get(xs, zs, ys);
        wr(out, xs);
        wr(out, zs);
        wr(out, ys);
      }
    }
  }
  // ---- res_admm's two sweeps on the product form [ -G | strict_lower(Linv) ] (kernels_resident.inc), one sum per row ----
  {
    const double *R = fo.rows.data();
    const size_t ldr = (size_t)fo.ldf;
    std::vector<double> xv = x0, zv = z0, yv = y0, w(M + n), ut(n);
    for (int j = 0; j < M; j++) w[j] = zv[j] - rinv * yv[j];
    for (int i = 0; i < n; i++) w[M + i] = sigma * xv[i] - sc.q[i];
    for (int it = 1; it <= 100; it++) {
      for (int row = 0; row < n; row++) {
        double acc = 0.0;
        for (int k = 0; k < M + row; k++) acc = std::fma(R[row * ldr + k], w[k], acc);
        ut[row] = f.d2inv[row] * (w[M + row] + acc);
      }
      std::vector<double> wn = w;
      for (int r = 0; r < n; r++) {
        double acc = 0.0;
        for (int i = r + 1; i < n; i++) acc = std::fma(R[i * ldr + M + r], ut[i], acc);
        const double xt = ut[r] + acc, xp = xv[r];
        const double xn = alpha * xt + (1.0 - alpha) * xp;
        xv[r] = xn;
        wn[M + r] = sigma * xn - sc.q[r];
      }
      for (int j = 0; j < M; j++) {
        double acc = 0.0;
        for (int i = 0; i < n; i++) acc = std::fma(R[i * ldr + j], ut[i], acc);
        const double zp = zv[j], yp = yv[j];
        const double nu = -rho * w[j] + acc;
        const double zt = zp + rinv * (nu - yp);
        const double zr = alpha * zt + (1.0 - alpha) * zp;
        const double v = zr + rinv * yp;
        const double zn = std::fmin(std::fmax(v, ls[j]), us[j]);
        const double yn = yp + rho * (zr - zn);
        zv[j] = zn;
        yv[j] = yn;
        wn[j] = zn - rinv * yn;
      }
      w = wn;
      if (it == 25 || it == 100) {
        wr(out, xv);
        wr(out, zv);
        wr(out, yv);
      }
    }
  }
  fclose(out);
  return 0;
}
