// The arithmetic of k_setup_models_large_auto (miosqp_amd/csrc/setup_models_large_body.hpp: body_large_auto) run on the
// CPU, beside setup_models_large_body_cpu.cpp and setup_models_auto_body_cpu.cpp and in their manner: the same phases, a
// loop over the thread index in place of the workgroup.  Reads one problem (CSC P and A, q, l, u, the starting rho, sigma,
// alpha, scaling passes; rho_auto 0 runs the fixed-rho body through the same entry; any_shape 1 lets a shape of the small
// launch through, for the pivot tests), equilibrates it and packs its rows as the entry point does, runs the body into
// zero-filled buffers and writes the record, the number of phases that ran, the probing iterations' x, z, y as they lie
// in the LDS, S as it stands on the packed triangle when the first Schur phases end and when the second ones do (zero
// where they never ran), every product, the panel's values and the plain values they were formed from.
// tests/test_setup_models_large_auto_cpu.py builds this with -fsanitize=address,undefined and compares the output with
// the long-double references.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../miosqp_amd/csrc/factor.hpp"
#include "../miosqp_amd/csrc/setup_plan.hpp"

namespace sm = miosqp::setup_models;

// runs a phase on every thread; after phase number `snap_at[k]` the packed triangle is copied to snap[k]
struct ExecLoop {
  long phases = 0;
  const double *tri_at = nullptr;
  size_t tri_len = 0;
  long snap_at[2] = {0, 0};
  std::vector<double> snap[2];
  template <class F>
  void par(F f) {
    phases++;
    for (int t = 0; t < sm::THREADS; t++) f(t);
    for (int k = 0; k < 2; k++)
      if (phases == snap_at[k]) snap[k].assign(tri_at, tri_at + tri_len);
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

int main(int argc, char **argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s problem.bin products.bin\n", argv[0]);
    return 2;
  }
  FILE *in = fopen(argv[1], "rb");
  if (!in) return 2;
  const std::vector<int32_t> h = rd<int32_t>(in, 7);
  const int n = h[0], M = h[1], nnzP = h[2], nnzA = h[3], passes = h[4], rho_auto = h[5], any_shape = h[6];
  const auto Pp = rd<int32_t>(in, n + 1), Pi = rd<int32_t>(in, nnzP);
  const auto Px = rd<double>(in, nnzP);
  const auto Ap = rd<int32_t>(in, n + 1), Ai = rd<int32_t>(in, nnzA);
  const auto Ax = rd<double>(in, nnzA);
  const auto q = rd<double>(in, n), l = rd<double>(in, M), u = rd<double>(in, M), rs = rd<double>(in, 3);
  fclose(in);
  const double rho = rs[0], sigma = rs[1], alpha = rs[2];
  if (!any_shape && !(rho_auto ? sm::eligible_shape_large_auto(n, M) : sm::eligible_shape_large(n, M))) {
    fprintf(stderr, "shape not eligible for the large launch\n");
    return 3;
  }
  miosqp::Scaled sc;
  miosqp::scale_problem(n, M, Pp.data(), Pi.data(), Px.data(), Ap.data(), Ai.data(), Ax.data(), q.data(), passes, sc);
  miosqp::Factor f;
  f.n = n; f.M = M; f.rho = rho; f.sigma = sigma; f.ld = (n + 15) & ~15;
  miosqp::pack_factor_rows(sc, Pp.data(), Pi.data(), Px.data(), rho, f);

  const int N = n + M, ld = f.ld, ldf = (N + 15) & ~15, ldn = ld, ldm = (M + 15) & ~15;
  std::vector<double> d2inv(n, 0.0), Linv((size_t)n * ld, 0.0), LinvT((size_t)n * ld, 0.0), f_rows((size_t)n * ldf, 0.0),
      f_GmT((size_t)M * ldn, 0.0), f_Ad((size_t)M * ldn, 0.0), f_Atd((size_t)n * ldm, 0.0), f_Pd((size_t)n * ldn, 0.0), ls(M, 0.0),
      us(M, 0.0);
  std::vector<double> pv_L = f.panel_by_var.val, pc_L = f.panel_by_con.val;  // the upload: the values at the starting rho
  // exactly the LDS the launch would ask for, on the heap: the sanitizer sees a phase that runs past it
  std::vector<double> lds(rho_auto ? sm::lds_doubles_large_auto(n, M) : sm::lds_doubles_large(n, M), -7.0);
  sm::Record rec{};
  rec.bad_pivot = -9;  // (the body writes the record on either exit)
  sm::IO io{};
  io.n = n; io.M = M; io.ld = ld; io.ldf = ldf; io.ldn = ldn; io.ldm = ldm; io.ldw = (N + 7) & ~7;
  io.rho = rho; io.sigma = sigma;
  io.pc_ptr = f.panel_by_con.ptr.data(); io.pc_idx = f.panel_by_con.idx.data(); io.pc_A = f.A_val.data();
  io.pb_ptr = f.Pbar.ptr.data(); io.pb_idx = f.Pbar.idx.data(); io.pb_val = f.Pbar.val.data();
  io.E = sc.E.data(); io.raw_l = l.data(); io.raw_u = u.data(); io.l = ls.data(); io.u = us.data();
  io.d2inv = d2inv.data(); io.Linv = Linv.data(); io.LinvT = LinvT.data(); io.f_rows = f_rows.data(); io.f_GmT = f_GmT.data();
  io.f_Ad = f_Ad.data(); io.f_Atd = f_Atd.data(); io.f_Pd = f_Pd.data(); io.W = nullptr; io.Kc = nullptr;  // (never touched)
  io.rec = &rec;
  sm::Auto au{};
  au.on = rho_auto;
  au.nv = (int)pv_L.size(); au.nc = (int)pc_L.size();
  au.alpha = alpha;
  au.q = sc.q.data();
  au.pv_At = f.At_val.data();
  au.pv_L = pv_L.data(); au.pc_L = pc_L.data();
  ExecLoop x;
  x.tri_at = lds.data();
  x.tri_len = sm::tri((size_t)n);
  // the Schur phases are three (copies and clear, Pbar + sigma I, rho Abar^T Abar); the LDL^T with its inverse 3 n
  // (2 n - 1 of the factor, the first row's copy, n - 1 rows, d2inv); the probe 1 + 4 * 50 + 2
  const long ldl = 3L * n, probe = 1 + 4L * sm::RHO_ONCE_ITERS + 2;
  x.snap_at[0] = 3;
  x.snap_at[1] = 3 + ldl + probe + 3;
  sm::body_large_auto(io, au, lds.data(), x);

  FILE *out = fopen(argv[2], "wb");
  if (!out) return 2;
  wr(out, {(double)rec.bad_pivot, (double)rec.pivot, rec.guard, rec.rho_est, rec.rho, (double)lds.size(), (double)x.phases,
           (double)pv_L.size(), (double)pc_L.size(), x.snap[1].empty() ? 0.0 : 1.0});
  if (rho_auto) {  // x | z | y of the last probing iteration: behind the triangle, the two rows and d
    fwrite(lds.data() + sm::lds_doubles_large(n, M), sizeof(double), (size_t)n + 2 * (size_t)M, out);
  } else {
    wr(out, std::vector<double>((size_t)n + 2 * (size_t)M, 0.0));
  }
  for (int k = 0; k < 2; k++) {
    std::vector<double> S((size_t)n * ld, 0.0);
    if (!x.snap[k].empty())
      for (int i = 0; i < n; i++)
        for (int j = 0; j <= i; j++) S[(size_t)i * ld + j] = x.snap[k][sm::tri((size_t)i) + j];
    wr(out, S);
  }
  for (const auto *v : {&d2inv, &Linv, &LinvT, &f_rows, &f_GmT, &f_Ad, &f_Atd, &f_Pd, &ls, &us, &pv_L, &pc_L, &f.At_val, &f.A_val,
                        &sc.q, &sc.E})
    wr(out, *v);
  fclose(out);
  return 0;
}
