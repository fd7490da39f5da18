// Polishes of different models in one launch (miosqp_qp_polish_models): the host logic that needs neither an engine nor
// the device -- the argument checks that refuse a call before anything is queued, and the layout of the call's arena.
// Plain C++ (no HIP): engine.hip includes it, and so does the stand-alone sanitized program under tests/.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "polish_many.hpp"

namespace miosqp {
namespace polish_models {

constexpr int ERR_ARG = -1;          // MIOSQP_EARG
constexpr int ERR_BOUNDS = 1;        // MIOSQP_EBOUNDS
constexpr int ERR_UNSUPPORTED = -5;  // MIOSQP_EUNSUPPORTED
constexpr size_t LDS_LIMIT = 160 * 1024;
constexpr double INFTY = 1e30;  // the engine's infinite bound

// The checks that read only the caller's arrays, in the order the entry point documents.  n[b], M[b]: variables and rows
// of model b, known once engines[b] is known to be non-NULL (0 otherwise).  0, or the error code with `err` naming the model.
inline int check_args(int32_t B, const void *const *engines, const int *n, const int *M, const double *const *q,
                      const double *const *l, const double *const *u, const double *const *x, const double *const *y, double tau,
                      const double *delta, const int32_t *refine_iter, const int32_t *repair_iter, const void *const *x_out,
                      const void *const *y_out, const void *info, const void *stats, std::string &err,
                      const char *entry = "polish_models") {
  const std::string who = std::string(entry) + ": ";  // (miosqp_qp_polish_models_large refuses with the same checks)
  auto model = [](int b) { return "model " + std::to_string(b); };
  if (B < 1) {
    err = who + "B must be at least 1";
    return ERR_ARG;
  }
  if (!engines || !n || !M || !q || !l || !u || !x || !y || !delta || !refine_iter || !repair_iter || !x_out || !y_out || !info ||
      !stats) {
    err = who + "a NULL argument";
    return ERR_ARG;
  }
  for (int b = 0; b < B; b++)
    if (!engines[b] || !l[b] || !u[b] || !x[b] || !x_out[b] || !y_out[b]) {  // (q[b], y[b] may be NULL)
      err = who + "a NULL pointer for " + model(b);
      return ERR_ARG;
    }
  for (int b = 1; b < B; b++)
    for (int a = 0; a < b; a++)
      if (engines[a] == engines[b]) {
        err = who + "the engine of " + model(a) + " is listed again as " + model(b);
        return ERR_ARG;
      }
  for (int b = 0; b < B; b++) {
    if (!(delta[b] > 0.0) || !(delta[b] < INFTY)) {
      err = who + "delta of " + model(b) + " must be positive";
      return ERR_ARG;
    }
    if (refine_iter[b] < 0 || refine_iter[b] > 10) {
      err = who + "refine_iter " + std::to_string(refine_iter[b]) + " of " + model(b) + " is outside 0..10";
      return ERR_ARG;
    }
    if (repair_iter[b] < 0 || repair_iter[b] > 20) {
      err = who + "repair_iter " + std::to_string(repair_iter[b]) + " of " + model(b) + " is outside 0..20";
      return ERR_ARG;
    }
  }
  for (int b = 0; b < B; b++) {
    for (int r = 0; r < M[b]; r++)
      if (l[b][r] != l[b][r] || u[b][r] != u[b][r] || (y[b] && y[b][r] != y[b][r])) {
        err = who + "NaN in l, u or y of " + model(b) + " (a node without a solution cannot be polished)";
        return ERR_ARG;
      }
    for (int i = 0; i < n[b]; i++)
      if (x[b][i] != x[b][i] || (q[b] && q[b][i] != q[b][i])) {
        err = who + "NaN in x or q of " + model(b);
        return ERR_ARG;
      }
  }
  for (int b = 0; b < B; b++)
    if (!y[b] && !(tau > 0.0)) {
      err = who + "no y for " + model(b) + " and tau is not positive (the device guesses y from z only with tau > 0)";
      return ERR_ARG;
    }
  for (int b = 0; b < B; b++)
    for (int r = 0; r < M[b]; r++)
      if (l[b][r] > u[b][r]) {
        err = who + "l > u in " + model(b);
        return ERR_BOUNDS;
      }
  return 0;
}

struct Shape {
  int n, M;
  size_t rows;        // doubles of the unscaled rows of A to stage (the by-constraint pattern's entries); 0: on the device already
  bool has_q, has_y;  // q[b] / y[b] given (otherwise the engine's cost / the device's guess: no room is taken)
};

// the models one workgroup cannot hold: MIOSQP_EUNSUPPORTED naming the first, 0 when all fit
inline int check_fit(const std::vector<Shape> &sh, std::string &err) {
  for (size_t b = 0; b < sh.size(); b++)
    if (polm_lds_bytes(sh[b].n, sh[b].M) > LDS_LIMIT) {
      err = "polish_models: the reduced system and the rows of A of model " + std::to_string(b) +
            " do not fit one workgroup's 160 KB of LDS (n " + std::to_string(sh[b].n) + ", M " + std::to_string(sh[b].M) +
            "): polish that model on its own";
      return ERR_UNSUPPORTED;
    }
  return 0;
}

constexpr size_t NONE = (size_t)-1;

// where model b's arrays lie in the arena (offsets in doubles from its base; NONE: no room taken)
struct Slot {
  size_t A, q, l, u, x, y;  // uploaded
  size_t out;               // downloaded: record | x | y | classes (polm_out_stride)
};

// [ table | rows of A, q, l, u, x, y of every model | output record of every model ]: the first two parts go up in ONE
// copy, the third comes back in ONE copy.  Entry b of the table is model b's, in the caller's order.
struct Plan {
  std::vector<Slot> slot;
  size_t table_doubles = 0;
  size_t up_doubles = 0;                  // what the host stages and uploads: [0, up_doubles)
  size_t down_off = 0, down_doubles = 0;  // what comes back
  size_t total_doubles = 0;
  size_t lds_bytes = 0;  // dynamic LDS of the launch: the largest need among the models
};

inline size_t round_up(size_t v, size_t to) { return (v + to - 1) / to * to; }

inline Plan plan(const std::vector<Shape> &sh) {
  Plan P;
  const size_t B = sh.size();
  P.slot.resize(B);
  P.table_doubles = round_up((B * sizeof(PolManyModel) + 7) / 8, 32);
  size_t at = P.table_doubles;
  for (size_t b = 0; b < B; b++) {
    const size_t n = (size_t)sh[b].n, M = (size_t)sh[b].M;
    Slot &s = P.slot[b];
    auto take = [&at](size_t doubles) { const size_t r = at; at += doubles; return r; };
    s.A = sh[b].rows ? take(sh[b].rows) : NONE;
    s.q = sh[b].has_q ? take(n) : NONE;
    s.l = take(M);
    s.u = take(M);
    s.x = take(n);
    s.y = sh[b].has_y ? take(M) : NONE;
    const size_t lds = polm_lds_bytes(sh[b].n, sh[b].M);
    if (lds != (size_t)-1 && lds > P.lds_bytes) P.lds_bytes = lds;
  }
  P.up_doubles = at;
  at = round_up(at, 2);  // (16-byte alignment of the part that comes back)
  P.down_off = at;
  for (size_t b = 0; b < B; b++) {
    P.slot[b].out = at;
    at += polm_out_stride(sh[b].n, sh[b].M);
  }
  P.down_doubles = at - P.down_off;
  P.total_doubles = at;
  return P;
}

}  // namespace polish_models
}  // namespace miosqp
