// The arithmetic of k_setup_models_large (miosqp_amd/csrc/setup_models_large_body.hpp) run on the CPU: the same phases, a
// loop over the thread index in place of the workgroup, a barrier where the loop ends.  Reads one problem (CSC P and A,
// q, l, u, rho, sigma, scaling passes) from a binary file, equilibrates it and packs its rows as the entry point does
// (scale_problem, pack_factor_rows), runs the body into zero-filled buffers -- the arena of the call is zero-filled --
// and writes S as it stands on the packed triangle after phase 2, every product, and what the per-model host set-up
// (build_factor, build_folded) makes of the same problem, its S included (handed out by build_factor to the accelerator
// hook, which declines here, so the host goes on alone).  tests/test_setup_models_large_cpu.py builds this with
// -fsanitize=address,undefined and compares the output with the long-double reference.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../miosqp_amd/csrc/factor.hpp"
#include "../miosqp_amd/csrc/setup_plan.hpp"

namespace sm = miosqp::setup_models;

struct ExecLoop {
  template <class F>
  void par(F f) {
    for (int t = 0; t < sm::THREADS; t++) f(t);
  }
};

struct Capture : miosqp::DenseAccelCtx {
  std::vector<double> S;
};
static int capture_s(int n, int ld, const double *S, double *, double *, double *, void *ctx) {
  Capture *c = static_cast<Capture *>(static_cast<miosqp::DenseAccelCtx *>(ctx));
  c->S.assign(S, S + (size_t)n * ld);
  return -1;  // "device error": build_factor goes on with the host's LDL^T
}

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
  const std::vector<int32_t> h = rd<int32_t>(in, 5);
  const int n = h[0], M = h[1], nnzP = h[2], nnzA = h[3], passes = h[4];
  const auto Pp = rd<int32_t>(in, n + 1), Pi = rd<int32_t>(in, nnzP);
  const auto Px = rd<double>(in, nnzP);
  const auto Ap = rd<int32_t>(in, n + 1), Ai = rd<int32_t>(in, nnzA);
  const auto Ax = rd<double>(in, nnzA);
  const auto q = rd<double>(in, n), l = rd<double>(in, M), u = rd<double>(in, M), rs = rd<double>(in, 2);
  fclose(in);
  const double rho = rs[0], sigma = rs[1];
  if (!sm::eligible_shape_large(n, M)) {
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
      us(M, 0.0), S((size_t)n * ld, 0.0);
  // exactly the LDS the launch would ask for, on the heap: the sanitizer sees a phase that runs past it
  std::vector<double> lds(sm::lds_doubles_large(n, M), -7.0);
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
  ExecLoop x;
  sm::large_schur(io, lds.data(), x);  // body_large is these two calls
  for (int i = 0; i < n; i++)
    for (int j = 0; j <= i; j++) S[(size_t)i * ld + j] = lds[sm::tri((size_t)i) + j];
  sm::large_products(io, lds.data(), x);

  FILE *out = fopen(argv[2], "wb");
  if (!out) return 2;
  wr(out, {(double)rec.bad_pivot, (double)rec.pivot, rec.guard, (double)lds.size()});
  for (const auto *v : {&S, &d2inv, &Linv, &LinvT, &f_rows, &f_GmT, &f_Ad, &f_Atd, &f_Pd, &ls, &us}) wr(out, *v);
  // the per-model host set-up of the same problem
  miosqp::Factor fh;
  std::string err;
  Capture cap;
  const bool ok = miosqp::build_factor(sc, Pp.data(), Pi.data(), Px.data(), rho, sigma, fh, err, capture_s,
                                       static_cast<miosqp::DenseAccelCtx *>(&cap));
  if (cap.S.size() != (size_t)n * ld) return 4;
  wr(out, {ok ? 1.0 : 0.0});
  wr(out, cap.S);
  if (ok) {
    miosqp::Folded fo;
    miosqp::build_folded(fh, fo);
    for (const auto *v : {&fh.d2inv, &fh.Linv, &fo.rows, &fo.GmT, &fo.Ad, &fo.Atd, &fo.Pd, &sc.D, &sc.E}) wr(out, *v);
  }
  fclose(out);
  return 0;
}
