// Stand-alone program over miosqp_amd/csrc/tree_rf_logic.hpp (built with -fsanitize=address,undefined by
// tests/test_solve_trees_rf_cpu.py and run as a subprocess): the decisions of round and fix inside the one-launch trees,
// replayed on the cases the test wrote to a file with what miosqp_amd/bnb.py answers for them -- rf_roundings, the pick
// loop of Workspace.round_and_fix, the firing rule of Workspace.primal_heuristic.  Everything must be equal bit for bit.
//
// File: int32 records, doubles as 8 raw bytes, in the machine's byte order.
//   case 1 (roundings): 1, K, p, x[p], lo[p], hi[p], expected[K][p]
//   case 2 (pick):      2, K, upper, has_x[K] (int32), viol[K], obj[K], expected chosen, expected feasible
//   case 3 (fires):     3, every, N, expected fire[N] (int32)
//   0 ends the file.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../miosqp_amd/csrc/tree_rf_logic.hpp"

namespace rf = miosqp::tree_rf;

static FILE *f;

static int32_t rd_i() {
  int32_t v;
  if (fread(&v, sizeof v, 1, f) != 1) {
    printf("short file\n");
    exit(2);
  }
  return v;
}
static double rd_d() {
  double v;
  if (fread(&v, sizeof v, 1, f) != 1) {
    printf("short file\n");
    exit(2);
  }
  return v;
}
static std::vector<double> rd_dv(int k) {
  std::vector<double> v((size_t)k);
  for (double &e : v) e = rd_d();
  return v;
}
static std::vector<int32_t> rd_iv(int k) {
  std::vector<int32_t> v((size_t)k);
  for (int32_t &e : v) e = rd_i();
  return v;
}

int main(int argc, char **argv) {
  if (argc != 2 || !(f = fopen(argv[1], "rb"))) {
    printf("usage: tree_rf_harness CASES\n");
    return 2;
  }
  long rounded = 0, picks = 0, fires = 0, bad = 0;
  for (;;) {
    const int kind = rd_i();
    if (kind == 0) break;
    if (kind == 1) {
      const int K = rd_i(), p = rd_i();
      if (K < 1 || K > rf::MAX_K || p < 0) return 2;
      const std::vector<double> x = rd_dv(p), lo = rd_dv(p), hi = rd_dv(p), want = rd_dv(K * p);
      for (int k = 0; k < K; k++)
        for (int i = 0; i < p; i++) {
          const double got = rf::fixed_value(x[(size_t)i], rf::theta(k, K), lo[(size_t)i], hi[(size_t)i]);
          if (memcmp(&got, &want[(size_t)k * p + i], sizeof got) != 0) {
            printf("rounding: K %d k %d x %.17g in [%.17g, %.17g]: %.17g, expected %.17g\n", K, k, x[(size_t)i], lo[(size_t)i],
                   hi[(size_t)i], got, want[(size_t)k * p + i]);
            bad++;
          }
          rounded++;
        }
    } else if (kind == 2) {
      const int K = rd_i();
      if (K < 1 || K > rf::MAX_K) return 2;
      const double upper = rd_d();
      const std::vector<int32_t> has_x = rd_iv(K);
      const std::vector<double> viol = rd_dv(K), obj = rd_dv(K);
      const int chosen = rd_i(), feasible = rd_i();
      rf::Pick pick;
      int last_taken = -1;
      for (int k = 0; k < K; k++)
        if (pick.take(k, has_x[(size_t)k] != 0, viol[(size_t)k], obj[(size_t)k], upper)) last_taken = k;
      // (the candidate taken last is the winner: the kernel keeps its rounded point on that signal)
      if (pick.best != chosen || pick.feasible != feasible || last_taken != chosen ||
          (chosen >= 0 && memcmp(&pick.best_obj, &obj[(size_t)chosen], sizeof(double)) != 0)) {
        printf("pick: K %d upper %.17g: chosen %d (taken last %d) feasible %d, expected %d / %d\n", K, upper, pick.best, last_taken,
               pick.feasible, chosen, feasible);
        bad++;
      }
      picks++;
    } else if (kind == 3) {
      const int every = rd_i(), N = rd_i();
      if (every < 1 || N < 0) return 2;
      const std::vector<int32_t> want = rd_iv(N);
      for (int c = 0; c < N; c++) {
        if ((int)rf::fires(c, every) != want[(size_t)c]) {
          printf("fires: node %d every %d: %d, expected %d\n", c, every, (int)rf::fires(c, every), want[(size_t)c]);
          bad++;
        }
        fires++;
      }
    } else {
      printf("unknown record %d\n", kind);
      return 2;
    }
  }
  fclose(f);
  if (bad) {
    printf("tree_rf FAILED: %ld mismatches\n", bad);
    return 1;
  }
  printf("tree_rf ok: %ld fixed values, %ld picks, %ld firing decisions\n", rounded, picks, fires);
  return 0;
}
