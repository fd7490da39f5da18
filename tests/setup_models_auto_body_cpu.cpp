// The arithmetic of k_setup_models_auto (miosqp_amd/csrc/setup_models_body.hpp: body_auto) run on the CPU, beside
// setup_models_body_cpu.cpp and in its manner: the same phases, a loop over the thread index in place of the workgroup.
// Reads one problem (CSC P and A, q, l, u, the starting rho, sigma, alpha, scaling passes, and a rho at which the
// second-factor stage is called once more afterwards -- 0: not), equilibrates it and packs its rows as the entry point
// does, runs the body into zero-filled buffers and writes the record, the number of phases that ran, the probing
// iterations' x, z, y as they lie in the LDS, every product, the panel's values and the plain values they were formed
// from.  tests/test_setup_models_auto_cpu.py builds this with -fsanitize=address,undefined and compares the output with
// the long-double reference of tests/rho_probe_reference.py.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../miosqp_amd/csrc/factor.hpp"
#include "../miosqp_amd/csrc/setup_plan.hpp"

namespace sm = miosqp::setup_models;

struct ExecLoop {
  long phases = 0;
  template <class F>
  void par(F f) {
    phases++;
    for (int t = 0; t < sm::THREADS; t++) f(t);
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
  const std::vector<int32_t> h = rd<int32_t>(in, 6);
  const int n = h[0], M = h[1], nnzP = h[2], nnzA = h[3], passes = h[4], rho_auto = h[5];
  const auto Pp = rd<int32_t>(in, n + 1), Pi = rd<int32_t>(in, nnzP);
  const auto Px = rd<double>(in, nnzP);
  const auto Ap = rd<int32_t>(in, n + 1), Ai = rd<int32_t>(in, nnzA);
  const auto Ax = rd<double>(in, nnzA);
  const auto q = rd<double>(in, n), l = rd<double>(in, M), u = rd<double>(in, M), rs = rd<double>(in, 4);
  fclose(in);
  const double rho = rs[0], sigma = rs[1], alpha = rs[2], rho_again = rs[3];
  if (!sm::eligible_shape_auto(n, M)) {
    fprintf(stderr, "shape not eligible\n");
    return 3;
  }
  miosqp::Scaled sc;
  miosqp::scale_problem(n, M, Pp.data(), Pi.data(), Px.data(), Ap.data(), Ai.data(), Ax.data(), q.data(), passes, sc);
  miosqp::Factor f;
  f.n = n; f.M = M; f.rho = rho; f.sigma = sigma; f.ld = (n + 15) & ~15;
  miosqp::pack_factor_rows(sc, Pp.data(), Pi.data(), Px.data(), rho, f);

  const int N = n + M, ld = f.ld, ldf = (N + 15) & ~15, ldn = ld, ldm = (M + 15) & ~15, ldw = (N + 7) & ~7;
  std::vector<double> d2inv(n, 0.0), Linv((size_t)n * ld, 0.0), LinvT((size_t)n * ld, 0.0), f_rows((size_t)n * ldf, 0.0),
      f_GmT((size_t)M * ldn, 0.0), f_Ad((size_t)M * ldn, 0.0), f_Atd((size_t)n * ldm, 0.0), f_Pd((size_t)n * ldn, 0.0),
      W((size_t)N * ldw, 0.0), Kc((size_t)N * ldw, 0.0), ls(M, 0.0), us(M, 0.0);
  std::vector<double> pv_L = f.panel_by_var.val, pc_L = f.panel_by_con.val;  // the upload: the values at the starting rho
  // exactly the LDS the launch would ask for, on the heap: the sanitizer sees a phase that runs past it
  std::vector<double> lds(rho_auto ? sm::lds_doubles_auto(n, M) : sm::lds_doubles(n, M), -7.0);
  sm::Record rec{};
  sm::IO io{};
  io.n = n; io.M = M; io.ld = ld; io.ldf = ldf; io.ldn = ldn; io.ldm = ldm; io.ldw = ldw;
  io.rho = rho; io.sigma = sigma;
  io.pc_ptr = f.panel_by_con.ptr.data(); io.pc_idx = f.panel_by_con.idx.data(); io.pc_A = f.A_val.data();
  io.pb_ptr = f.Pbar.ptr.data(); io.pb_idx = f.Pbar.idx.data(); io.pb_val = f.Pbar.val.data();
  io.E = sc.E.data(); io.raw_l = l.data(); io.raw_u = u.data(); io.l = ls.data(); io.u = us.data();
  io.d2inv = d2inv.data(); io.Linv = Linv.data(); io.LinvT = LinvT.data(); io.f_rows = f_rows.data(); io.f_GmT = f_GmT.data();
  io.f_Ad = f_Ad.data(); io.f_Atd = f_Atd.data(); io.f_Pd = f_Pd.data(); io.W = W.data(); io.Kc = Kc.data();
  io.rec = &rec;
  sm::Auto au{};
  au.on = rho_auto;
  au.nv = (int)pv_L.size(); au.nc = (int)pc_L.size();
  au.alpha = alpha;
  au.q = sc.q.data();
  au.pv_At = f.At_val.data();
  au.pv_L = pv_L.data(); au.pc_L = pc_L.data();
  ExecLoop x;
  sm::body_auto(io, au, lds.data(), x);
  const long phases = x.phases;

  FILE *out = fopen(argv[2], "wb");
  if (!out) return 2;
  wr(out, {(double)rec.bad_pivot, (double)rec.pivot, rec.guard, rec.rho_est, rec.rho, (double)lds.size(), (double)phases,
           (double)pv_L.size(), (double)pc_L.size()});
  const sm::Lds at = sm::lds_layout(lds.data(), n, M);
  if (rho_auto) {  // x | z | y of the last probing iteration
    fwrite(at.pv, sizeof(double), (size_t)n + 2 * (size_t)M, out);
  } else {
    wr(out, std::vector<double>((size_t)n + 2 * (size_t)M, 0.0));
  }
  for (const auto *v : {&d2inv, &Linv, &LinvT, &f_rows, &f_GmT, &f_Ad, &f_Atd, &f_Pd, &W, &Kc, &ls, &us, &pv_L, &pc_L, &f.At_val,
                        &f.A_val, &sc.q, &sc.E})
    wr(out, *v);
  // the second-factor stage once more, at a rho of the caller's choice (the dense Abar is still in the LDS)
  if (rho_auto && rho_again > 0 && !rec.bad_pivot) {
    sm::Record rec2{};
    io.rec = &rec2;
    const bool ok = sm::refactor(io, au, at.Lp, at.Ad, at.tmp, at.dv, x, rho_again);
    wr(out, {ok ? 1.0 : 0.0, (double)rec2.bad_pivot, (double)rec2.pivot});
    wr(out, d2inv);
  } else {
    wr(out, {-1.0, 0.0, 0.0});
    wr(out, std::vector<double>((size_t)n, 0.0));
  }
  fclose(out);
  return 0;
}
