// Trees of different models in one launch (miosqp_qp_solve_trees_models): the host logic that needs neither an engine nor
// the device -- the argument checks that refuse a call before anything is queued, and the layout of the call's arena.
// Plain C++ (no HIP): engine.hip includes it, and so does the stand-alone sanitized program under tests/.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "tree_sb_logic.hpp"  // the size of a tree's work area under strong / reliability branching

namespace miosqp {
namespace models {

constexpr int ERR_ARG = -1;     // MIOSQP_EARG
constexpr int ERR_BOUNDS = 1;   // MIOSQP_EBOUNDS
constexpr size_t OUT_DOUBLES = 8;  // room of one outcome record (TreeOut: 48 bytes)

// The checks that read only the caller's arrays, in the order the entry point documents.  M[b]: rows of model b (general
// rows and integer rows), known once engines[b] is known to be non-NULL.  0, or the error code with `err` naming the model.
inline int check_args(int32_t B, const void *const *engines, const int *M, const double *const *q, const double *const *l,
                      const double *const *u, const double *const *x0, const double *const *y0, const double *upper0,
                      const double *const *x_inc0, const int32_t *rule, const int32_t *max_iter_bb, const void *const *x_out,
                      const void *info, const void *stats, std::string &err) {
  const std::string who = "solve_trees_models: ";
  if (B < 1) {
    err = who + "B must be at least 1";
    return ERR_ARG;
  }
  if (!engines || !M || !q || !l || !u || !x0 || !y0 || !upper0 || !x_inc0 || !rule || !max_iter_bb || !x_out || !info || !stats) {
    err = who + "a NULL argument";
    return ERR_ARG;
  }
  for (int b = 0; b < B; b++) {
    if (!engines[b] || !q[b] || !l[b] || !u[b] || !x0[b] || !y0[b] || !x_out[b]) {  // (x_inc0[b] may be NULL: no incumbent)
      err = who + "a NULL pointer for model " + std::to_string(b);
      return ERR_ARG;
    }
  }
  for (int b = 1; b < B; b++)
    for (int a = 0; a < b; a++)
      if (engines[a] == engines[b]) {
        err = who + "the engine of model " + std::to_string(a) + " is listed again as model " + std::to_string(b);
        return ERR_ARG;
      }
  for (int b = 0; b < B; b++) {
    if (rule[b] < 0 || rule[b] > 3) {
      err = who + "tree_explor_rule " + std::to_string(rule[b]) + " of model " + std::to_string(b) + " is outside 0..3";
      return ERR_ARG;
    }
    if (max_iter_bb[b] < 1) {
      err = who + "max_iter_bb of model " + std::to_string(b) + " must be at least 1";
      return ERR_ARG;
    }
  }
  for (int b = 0; b < B; b++)
    for (int i = 0; i < M[b]; i++)
      if (l[b][i] > u[b][i]) {
        err = who + "l > u in the root of model " + std::to_string(b);
        return ERR_BOUNDS;
      }
  return 0;
}

struct Shape {
  int n, M, p;  // variables, rows (general + integer), integer variables
  int form;     // 1: one wavefront, 2: one workgroup, 3: one workgroup in reduced form (miosqp_qp_solve_trees_models_large);
                // with round and fix inside (miosqp_qp_solve_trees_models_rf) 4: one workgroup, 5: the reduced form;
                // with strong / reliability branching inside (miosqp_qp_solve_trees_models_sb) 6: one workgroup, 7: reduced
};

constexpr size_t RF_DOUBLES = 4;  // room of one round-and-fix record (TreeRfOut: 32 bytes)

constexpr size_t SB_DOUBLES = 4;  // room of one strong-branching record (TreeSbOut: 32 bytes)

inline bool reduced_form(int form) { return form == 3 || form == 5 || form == 7; }

// what miosqp_qp_solve_trees_models_sb checks beyond check_args: per model the branching rule (0: the most-fractional
// rule, the model runs as without the entry; 1 strong, 2 reliability branching), and for the models with a rule
// sb_candidates in 1..32, sb_max_iter >= 1, sb_reliability >= 0 and sb_eps > 0.  rule_min: 0 there, 1 for
// miosqp_qp_solve_trees_sb (one model, `who` names the entry).
inline int check_sb(int32_t B, const int32_t *rule, const int32_t *sb_candidates, const int32_t *sb_max_iter,
                    const int32_t *sb_reliability, const double *sb_eps, const void *sb_info, int rule_min, const std::string &who,
                    std::string &err) {
  if (!rule || !sb_candidates || !sb_max_iter || !sb_reliability || !sb_eps || !sb_info) {
    err = who + ": a NULL argument";
    return ERR_ARG;
  }
  for (int b = 0; b < B; b++) {
    const std::string of = " of model " + std::to_string(b);
    if (rule[b] < rule_min || rule[b] > 2) {
      err = who + ": branching_rule " + std::to_string(rule[b]) + of + " is outside " + std::to_string(rule_min) + "..2";
      return ERR_ARG;
    }
    if (rule[b] == 0) continue;
    if (sb_candidates[b] < 1 || sb_candidates[b] > tree_sb::MAX_K) {
      err = who + ": sb_candidates " + std::to_string(sb_candidates[b]) + of + " is outside 1.." + std::to_string(tree_sb::MAX_K);
      return ERR_ARG;
    }
    if (sb_max_iter[b] < 1) {
      err = who + ": sb_max_iter" + of + " must be at least 1";
      return ERR_ARG;
    }
    if (sb_reliability[b] < 0) {
      err = who + ": sb_reliability" + of + " must not be negative";
      return ERR_ARG;
    }
    if (!(sb_eps[b] > 0.0)) {
      err = who + ": sb_eps" + of + " must be positive";
      return ERR_ARG;
    }
  }
  return 0;
}

// what miosqp_qp_solve_trees_models_rf checks beyond check_args: per model the candidates per call (0: the heuristic is
// off for that model), their iteration cap and every how many branching nodes.  K_min: 0 there, 1 for
// miosqp_qp_solve_trees_rf (one model, `who` names the entry).
inline int check_rf(int32_t B, const int32_t *rf_candidates, const int32_t *rf_max_iter, const int32_t *rf_every,
                    const void *rf_info, int K_min, const std::string &who, std::string &err) {
  if (!rf_candidates || !rf_max_iter || !rf_every || !rf_info) {
    err = who + ": a NULL argument";
    return ERR_ARG;
  }
  for (int b = 0; b < B; b++) {
    const std::string of = " of model " + std::to_string(b);
    if (rf_candidates[b] < K_min || rf_candidates[b] > 32) {
      err = who + ": rf_candidates " + std::to_string(rf_candidates[b]) + of + " is outside " + std::to_string(K_min) + "..32";
      return ERR_ARG;
    }
    if (rf_max_iter[b] < 1) {
      err = who + ": rf_max_iter" + of + " must be at least 1";
      return ERR_ARG;
    }
    if (rf_every[b] < 1) {
      err = who + ": rf_every" + of + " must be at least 1";
      return ERR_ARG;
    }
  }
  return 0;
}

// what miosqp_qp_solve_trees_models_large checks beyond check_args: the leaf list of the reduced form needs room for the
// two children of the root's branching
inline int check_leaf_cap(int32_t leaf_cap, std::string &err) {
  if (leaf_cap < 2) {
    err = "solve_trees_models_large: leaf_cap must be at least 2 (got " + std::to_string(leaf_cap) + ")";
    return ERR_ARG;
  }
  return 0;
}

// where model b's arrays lie in the arena (offsets in doubles from its base) and which table entry is its own
struct Slot {
  int entry;
  size_t raw, qraw;  // l | u | x0 | y0 (3 M + n), the raw cost (n): uploaded
  size_t inc, out;   // incumbent (n), outcome (OUT_DOUBLES): uploaded and downloaded
  size_t rf;         // the round-and-fix record (rf_doubles, behind the outcome; 0 without one): uploaded and downloaded
  size_t q;          // the scaled cost (n)
  size_t lf_lo, lf_hi, lf_x, lf_y;  // the leaf store: cap x p, cap x p, cap x n, cap x M
  // strong / reliability branching (0 without): the record (sb_doubles, behind the outcome and the round-and-fix record:
  // uploaded and downloaded); for a model of form 6 or 7 the tree's work area (tree_sb::work_doubles(p)) and Node.pc of
  // every leaf-store place (cap x tree_sb::PC_DOUBLES), behind its leaf store
  size_t sb = 0, sb_work = 0, sb_pc = 0;
};

// [ table | raw, qraw of every model | inc, out of every model | q and leaf store of every model ]: the first three parts
// go up in ONE copy, the third comes back in ONE copy.  The table holds the one-wavefront models first (the launch over
// them reads entries [0, n1)), then the workgroup models (entries [n1, n1 + n2)), then the models of the reduced form
// (entries [n1 + n2, n1 + n2 + n3)), then the two groups with round and fix inside -- workgroup (n4 entries), reduced form
// (n5 entries) --, each group in the caller's order.  The leaf store of a model has `tree_cap` places, that of a
// reduced-form model `leaf_cap_r`.  rf_doubles > 0 (miosqp_qp_solve_trees_models_rf): every model's outcome is followed by
// a round-and-fix record of that many doubles; with 0, and no model of form 4 or 5, the layout is what it was without them.
// The two groups with strong / reliability branching inside follow (n6 workgroup, n7 reduced form); sb_doubles > 0
// (miosqp_qp_solve_trees_models_sb): every model's outcome is followed by a record of that many doubles, and the leaf
// store of a model of form 6 or 7 by its work area and Node.pc; with 0 and no such model the layout is what it was.
struct Plan {
  std::vector<Slot> slot;
  int n1 = 0, n2 = 0, n3 = 0, n4 = 0, n5 = 0;
  size_t table_doubles = 0;
  size_t up_doubles = 0;               // what the host stages and uploads: [0, up_doubles)
  size_t down_off = 0, down_doubles = 0;  // what comes back
  size_t total_doubles = 0;
  int n6 = 0, n7 = 0;
};

inline size_t round_up(size_t v, size_t to) { return (v + to - 1) / to * to; }

inline Plan plan(const std::vector<Shape> &sh, size_t entry_bytes, size_t tree_cap, size_t leaf_cap_r = 0, size_t rf_doubles = 0,
                 size_t sb_doubles = 0) {
  Plan P;
  const size_t B = sh.size();
  P.slot.resize(B);
  for (const Shape &s : sh)
    (s.form == 1 ? P.n1 : s.form == 3 ? P.n3 : s.form == 4 ? P.n4 : s.form == 5 ? P.n5 : s.form == 6 ? P.n6 : s.form == 7 ? P.n7 : P.n2)++;
  int k1 = 0, k2 = P.n1, k3 = P.n1 + P.n2, k4 = k3 + P.n3, k5 = k4 + P.n4, k6 = k5 + P.n5, k7 = k6 + P.n6;
  for (size_t b = 0; b < B; b++) {
    const int f = sh[b].form;
    P.slot[b].entry = f == 1 ? k1++ : f == 3 ? k3++ : f == 4 ? k4++ : f == 5 ? k5++ : f == 6 ? k6++ : f == 7 ? k7++ : k2++;
  }
  P.table_doubles = round_up((B * entry_bytes + 7) / 8, 32);
  size_t at = P.table_doubles;
  for (size_t b = 0; b < B; b++) {
    const size_t n = (size_t)sh[b].n, M = (size_t)sh[b].M;
    P.slot[b].raw = at;
    at += 3 * M + n;
    P.slot[b].qraw = at;
    at += n;
  }
  at = round_up(at, 2);  // (16-byte alignment of the part that comes back)
  P.down_off = at;
  for (size_t b = 0; b < B; b++) {
    P.slot[b].inc = at;
    at += (size_t)sh[b].n;
    P.slot[b].out = at;
    at += OUT_DOUBLES;
    P.slot[b].rf = rf_doubles ? at : 0;
    at += rf_doubles;
    P.slot[b].sb = sb_doubles ? at : 0;
    at += sb_doubles;
  }
  P.down_doubles = at - P.down_off;
  P.up_doubles = at;
  at = round_up(at, 32);
  for (size_t b = 0; b < B; b++) {
    const size_t n = (size_t)sh[b].n, M = (size_t)sh[b].M, p = (size_t)sh[b].p;
    const size_t cap = reduced_form(sh[b].form) ? leaf_cap_r : tree_cap;
    P.slot[b].q = at;
    at += round_up(n, 2);
    P.slot[b].lf_lo = at;
    at += cap * p;
    P.slot[b].lf_hi = at;
    at += cap * p;
    P.slot[b].lf_x = at;
    at += cap * n;
    P.slot[b].lf_y = at;
    at += cap * M;
    if (sh[b].form == 6 || sh[b].form == 7) {
      at = round_up(at, 2);
      P.slot[b].sb_work = at;
      at += tree_sb::work_doubles(sh[b].p);
      P.slot[b].sb_pc = at;
      at += cap * (size_t)tree_sb::PC_DOUBLES;
    }
  }
  P.total_doubles = at;
  return P;
}

// The arena against what the device pool can give (`limit_doubles`): 0, or ERR_ARG with `err` naming the first model
// whose leaf store ends beyond the limit (the staged part in front of the leaf stores counts against model 0).
inline int check_arena(const Plan &P, const std::vector<Shape> &sh, size_t tree_cap, size_t leaf_cap_r, size_t limit_doubles,
                       std::string &err) {
  if (P.total_doubles <= limit_doubles) return 0;
  size_t b = 0;
  for (; b + 1 < sh.size(); b++) {
    const size_t cap = reduced_form(sh[b].form) ? leaf_cap_r : tree_cap;
    const size_t end = P.slot[b].sb_pc ? P.slot[b].sb_pc + cap * (size_t)tree_sb::PC_DOUBLES : P.slot[b].lf_y + cap * (size_t)sh[b].M;
    if (end > limit_doubles) break;
  }
  err = "solve_trees_models_large: the arena of the call (" + std::to_string(P.total_doubles * sizeof(double)) +
        " bytes) is beyond what the device pool can give (" + std::to_string(limit_doubles * sizeof(double)) +
        " bytes): reached at model " + std::to_string(b) + "; fewer models per call, or a smaller leaf_cap";
  return ERR_ARG;
}

}  // namespace models
}  // namespace miosqp
