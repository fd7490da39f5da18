// MI355X (gfx950) relaxation engine: device kernels + host driver + C ABI (include/miosqp_amd.h).
//
// One ADMM iteration of the OSQP algorithm (paper Algorithm 1) = one application of K^-1
// through the block factor of factor.hpp plus the fused vector updates, as FOUR row-parallel
// kernels (each row = one CSR / triangular row handled by a wavefront group: lanes stride the
// row with coalesced loads, partial sums meet in a DPP butterfly and, for multi-wave rows, in
// LDS).  Every reduction has a fixed order, so reruns are bit-identical.
//
//   k_panel_fwd   c  = sigma x - q - L21 wh                    (n rows, pattern of A^T)
//   k_tail_fwd    ut = D22^-1 (c + strict_lower(Linv) c)       (n rows, triangular)
//   k_tail_bwd    xt = ut + strict_upper(Linv^T) ut ;  x, dx   (n rows, triangular)
//   k_panel_bwd   nu = -rho wh - L21^T xt ; z~, z, y, dy, wh   (M rows, pattern of A)
//
// with wh = z - y/rho (the permuted right-hand side of the constraint block).  The termination
// test (every check_termination iterations) is three more kernels and one device-side decision;
// the host only reads a 64-byte control block per chunk.  The per-chunk kernel sequence is
// captured once in a hipGraph.
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <sys/stat.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <queue>
#include <deque>
#include <tuple>
#include <type_traits>
#include <string>
#include <vector>

#include "../../include/miosqp_amd.h"
#include "factor.hpp"
#include "polish_many.hpp"  // polishing of many small instances in one launch (polish_many.hip)
#include "polish_many_large.hpp"  // ... and of larger ones, S in a slab of device scratch per workgroup (polish_many_large.hip)
#include "lockstep_trees.hpp"  // the tree logic of B trees in lock step (plain C++; host_lockstep.inc drives it)
#include "lockstep_ahead.hpp"  // ahead records, shadow leaves and the choice of ahead columns (plain C++; host_lockstep_ahead.inc drives it)
#include "lockstep_sb.hpp"  // strong and reliability branching in the lock-step trees (plain C++; host_lockstep_sb.inc drives it)
#include "setup_plan.hpp"  // set-up of many models in one launch: argument checks, eligibility, arena layout (plain C++; host_setup_models.inc drives it); with guard_probe.hpp and setup_models_body.hpp, the kernel's arithmetic
#include "polish_models_plan.hpp"  // polishes of different models in one launch: argument checks and arena layout (plain C++; host_polish_models.inc drives it)
#include "polish_models_large_plan.hpp"  // ... of different LARGER models: fit rule, workgroups and arena layout with the slabs (plain C++; host_polish_models_large.inc drives it)
#include "tree_reduced_body.hpp"  // the one-launch trees' relaxation in reduced form (k_tree_r_m): LDS rule and the phases of an iteration (plain C++; also run on the CPU under tests/)
#include "tree_rf_logic.hpp"  // round and fix inside the one-launch trees (k_tree_rf*): when it fires, the fixed value, the pick (plain C++; also run on the CPU under tests/)
#include "tree_sb_logic.hpp"  // strong / reliability branching inside the one-launch trees (k_tree_sb*): candidates, scores, pseudo-costs, the pick (plain C++; also run on the CPU under tests/)
#include "models_plan.hpp"  // trees of different models in one launch: argument checks and arena layout (plain C++; host_models.inc drives it)
#include "trees_large_plan.hpp"  // B trees of one model in the reduced form in one launch: the layout of the batch's arena, overflow-checked (plain C++; host_trees_large.inc drives it)
#include "lockstep_refill.hpp"  // which tree goes into which free column when the columns are refilled between chunks (plain C++; host_refill.inc drives it)

#define QP_INFTY 1e30
#define QP_MIN_SCALING 1e-4
#define QP_DIVISION_TOL (1.0 / QP_INFTY)

// dense_setup.hip: dense LDL^T + triangular inverse on the device (miosqp::DenseLdlInv)
int miosqp_device_ldl_inverse(int n, int ld, const double *S, double *d, double *Linv, double *LinvT, void *ctx);
void miosqp_device_ruiz_ops(miosqp::RuizOps *ops, void **storage, void *stream);
void miosqp_device_ruiz_free(void *storage);
// dense_setup.hip: explicit KKT inverse W = F^T D22^-1 F from the product-form rows (device pointers)
int miosqp_device_kkt_inverse(const double *F, int ldf, const double *dinv, int n, int M, double *W, int ldw,
                              hipStream_t stream);
// dense_setup.hip: the same LDL^T + triangular inverse on a matrix that lies in device memory, queued on `stream`
int miosqp_device_ldl_inverse_resident(int n, int ld, double *S, double *X, double *LinvT, double *W, double *d,
                                       int *flag, hipStream_t stream);

namespace {

thread_local std::string g_err;

void set_err(const char *what, hipError_t e, const char *file, int line) {
  char buf[512];
  snprintf(buf, sizeof buf, "%s: %s (%s:%d)", what, hipGetErrorString(e), file, line);
  g_err = buf;
}

#define HIPCHK(call)                                  \
  do {                                                \
    hipError_t e__ = (call);                          \
    if (e__ != hipSuccess) {                          \
      set_err(#call, e__, __FILE__, __LINE__);        \
      return MIOSQP_EHIP;                             \
    }                                                 \
  } while (0)

// The HIP current device is per host thread: every entry point makes the engine's device current
// first, so a handle can be driven from any thread (e.g. the worker thread of a pipelined wave).
#define ENTER(e)                                       \
  do {                                                 \
    if ((e)->device >= 0) HIPCHK(hipSetDevice((e)->device)); \
  } while (0)

struct Ctrl {
  int done, status, iter, pad;
  int B, ndone, pad3[2];  // batched mode: active columns, columns already decided
  double pri_res, dua_res, obj_val, lower;
  double nrm_dy, nrm_dx;  // certificate normalisers
  double pad2[2];
  // node digest (branching epilogue, workspace.py:245-272 on the device)
  int int_inf, nextvar, pad4[2];
  double heur_viol, heur_obj;
};

struct PoolCtl;
struct ReadyEntry;

// everything a kernel needs, passed by value
struct Dev {
  int n, M, ld, n_int, m_orig;
  double rho, rho_inv, sigma, alpha, eps_abs, eps_rel, eps_pinf, eps_dinf, c, cinv;
  // panel by variable (n rows) / by constraint (M rows)
  const int *pv_ptr, *pv_idx;
  const double *pv_L, *pv_At;
  const int *pc_ptr, *pc_idx;
  const double *pc_L, *pc_A;
  // tail
  const double *Linv, *LinvT, *d2inv;
  // symmetric matrices by row
  const int *pb_ptr, *pb_idx;
  const double *pb_val;
  const int *pr_ptr, *pr_idx;
  const double *pr_val;
  const double *D, *Dinv, *E, *Einv;
  const int *i_idx;
  // scaled vectors
  double *q, *l, *u, *x, *z, *y, *wh, *cv, *ut, *xt, *dx, *dy;
  double *qraw;
  // scratch for the termination test: sm = 8 x M, sn = 10 x n
  double *sm, *sn;
  // staging: raw (unscaled) inputs and outputs
  double *raw_l, *raw_u, *raw_x, *raw_y, *out_x, *out_y;
  Ctrl *ctrl;
  // ---- folded (product-form) factor: rows of L^-1, see factor.hpp ----
  const double *f_rows, *f_GmT, *f_Ad, *f_Atd, *f_Pd;
  int ldf, ldn, ldm;
  double *rx;  // sigma x - q, kept right behind wh so that [wh | rx] is one contiguous vector
  // node digest: rounded candidate (unscaled / scaled), root bounds, tolerances
  double *xi, *xis, *root_l, *root_u;
  double eps_int, eps_lin;
  int digest;
  int bm_ablate;  // debug: 1 = no operand loads, 2 = no matrix-core instructions
  unsigned long long *prof;  // debug timeline (per-block start/end, 100 MHz wall clock) or nullptr
  // ---- cooperative register-resident solver (k_coop): explicit KKT inverse, exchange buffers ----
  const double *W;               // N x ldw, N = M + n, ordering [constraints ; variables]
  int ldw;
  unsigned *coop_tag;            // tag of the last exchange round that completed
  unsigned long long *coop_buf;  // the exchange ring: 4 buffers of COOP_RING_WORDS, pair units (kernels_coop.inc)
  unsigned long long *coop_chk;  // 2 x coop_half: the test's operands [y ; x] and [proj(dy) ; dx]
  unsigned long long *coop_q;    // (256 + 16) x COOP_QS: per-workgroup, then per-group norms / sums of the test
  unsigned long long *coop_reg;  // start-up registration counter (grows by the grid size per launch); +64: launches with testers
  unsigned long long *coop_chz;  // coop_half: z, the third operand of the test when it runs on tester workgroups
  unsigned long long *coop_dec;  // the testers' decision {status | tag}
  int coop_nt;                   // tester workgroups behind the exchange grid (0: the test runs inside the grid)
  int coop_lag;                  // iterations between a test and the point where the grid waits for its decision
  int coop_tres;                 // the testers keep their rows of Kc in registers (kernels_coop.inc: coop_tester<.., RES>)
  const double *Kc;              // [ 0 Abar ; Abar^T Pbar ], N x ldw
  int coop_dbg;                  // debug: 1 = no gather (ablation), 64 = workgroup 1 never starts (fault injection)
  int coop_nap;                  // 64-clock naps between publishing and the first poll of a round (calibrated)
  int coop_stride;               // 8-byte words between the blocks of consecutive workgroups (= 2 RW: entries are flat, 2 words each)
  size_t coop_half;              // words per parity
  // the exchange's row layout (kernels_coop.inc "reduced indices"): W' = W without the identity (integer-bound) rows
  const double *coop_W;          // NR x coop_ldw, NR = coop_mg + n  (== W, ldw while nothing is dropped)
  int coop_ldw, coop_mg;         // coop_mg: general rows kept in W' (M while nothing is dropped)
  const int *coop_brow;          // per variable: FULL index of its bound row, -1 without one (nullptr: none anywhere)
  const double *coop_aj;         // per variable: scaled entry of its bound row, 0 without one
  // ---- batched mode: B nodes share the factor; vectors are [len][Bs], batch index fastest ----
  int Bs;  // column stride, multiple of 64
  double *b_l, *b_u, *b_x, *b_z, *b_y, *b_wh, *b_rx, *b_cv, *b_ut, *b_xt, *b_dx, *b_dy;
  double *b_xfs;  // harvest tile: D^-1 (clamped x), next to b_xis = D^-1 (rounded candidate)
  double *b_sm, *b_sn;      // 8 x M x Bs, 4 x n x Bs
  double *b_xfin, *b_yfin;  // unscaled answers, batch-fastest
  double *b_xi, *b_xis;     // rounded candidates (node digest), unscaled / scaled
  double *b_part;           // partial reductions of the batched termination test
  const double *b_zero;     // a page of zeros (matrix-core tiles: operand of a chunk beyond the end)
  // ---- leaf pool + streaming batch (kernels_pool.inc) ----
  int stream;               // 1: columns are refilled from the pool between chunks and count their own iterations
  int max_iter_s, ring;
  int *c_start, *c_child0, *c_child1, *c_harv, *t_has;
  int *fmap, *hmap;         // columns refilled / harvested in the current chunk
  double *lt_x;             // load tile: scaled x of the refilled columns, [n][64]
  const int *int_pos;       // variable -> its position in i_idx, or -1
  // ---- integer-bound rows taken out of the batched products (kernels_batched.inc "identity rows") ----
  int wh_m;                 // rows of the constraint block that go through the matrix products (m, or M when off)
  const double *f_rows2;    // [ -G(general rows) | strict_lower(Linv) ], n x ldf2 (== f_rows, ldf when off)
  int ldf2;
  const double *a_int;      // per variable: rho * (scaled entry of its bound row), 0 for continuous variables
  double *pl_lo, *pl_hi;    // [cap][n_int] integer-row bounds of every node
  int *pl_ws;               // slot whose solution is the node's warm start
  double *sol_x, *sol_y;    // [cap][n], [cap][M] solutions of solved nodes (x clamped as node.py:131-136)
  PoolCtl *pctl;            // device-side counters
  PoolCtl *hctl;            // host memory: [0] host -> device (tail, upper), [1] device -> host (head, fin, active)
  ReadyEntry *ready;        // host memory: ready ring
  miosqp_pool_digest *dg_ring;  // host memory: digests of decided nodes
  int *c_intinf, *c_nextvar;
  int *c_node;   // column position -> node of the wave (columns are swapped when the wave is compacted)
  int *c_pairs;  // swap list of the current compaction
  double *c_hviol, *c_hobj;
  double *b_raw;            // node-major staging in:  l[B][M] | u[B][M] | x0[B][n] | y0[B][M]
  double *b_out;            // node-major staging out: x[B][n] | y[B][M]
  int *c_done, *c_status, *c_iter;
  double *c_pri, *c_dua, *c_obj, *c_lower;
  // ---- one linear cost per column (miosqp_qp_solve_batch_q; allocated on its first call) ----
  double *b_q;     // scaled costs, [n][Bs] batch-fastest: what the <PQ = true> kernels read where the others read q
  double *b_qs;    // the same instance-major [B][n], as k_scale_q_batch leaves them (kb_prepare lays them out)
  double *b_qraw;  // raw costs, instance-major [B][n] (kb_obj_rows, through c_node)
};

struct SearchDigest {  // coherent host memory
  int status, iter, int_inf, nextvar, action, branched, pad;
  int todo;  // 1: the launch only ran the relaxation (or was called off): the host still has to launch the epilogue kernels
  double lower, heur_viol, heur_obj, pri_res, dua_res, obj_val;
  unsigned long long t0, t1;  // device wall clock (100 MHz): the first tester took the node up / wrote this record (0: not stamped)
  unsigned long long seq;  // written last (release, system scope): the record of node `seq` is complete
};
struct SearchArgs {
  const double *lo_s, *hi_s;  // this node's integer-row bounds
  const double *x_w, *y_w;    // its warm start: the parent's solution
  double *x_s, *y_s;          // where its own solution goes
  double *lo0, *hi0, *lo1, *hi1;  // the children's bounds (slots reserved by the host)
  double *inc_x;              // the incumbent
  double upper;               // the incumbent's value as the host knows it
  SearchDigest *dg;
  unsigned long long seq;
};

// node mode of k_coop (hosted search, host_search.inc): prologue and epilogue of a node inside the cooperative launch
struct CoopNode {
  int on;            // 0: plain solve -- iterates in d.*, prologue / epilogue by the host's kernels
  int epi;           // 1: the tester workgroups run the epilogue (unscale, clamp, digest, heuristic, objective, commit)
  int tpr_h, tpr_o;  // threads per row of the sparse rows of Abar / of the unscaled P, as the launches use them
  SearchArgs a;
  unsigned long long *epi_buf;  // exchange buffer of the epilogue: 2 n + (workgroups of the launch) tagged entries
  unsigned long long *stamps;   // debug (MIOSQP_SEARCH_STAMPS=1): 16 wall-clock stamps (100 MHz) of this node, or nullptr
};

// The device code and the host driver live in the .inc files below: ONE translation unit (everything
// sits in the same anonymous namespace and the kernels are templates instantiated by the host code),
// split only for reading.
#include "kernels_iter.inc"  // device helpers; the four kernels of the factor form and the two of the product form
#include "kernels_test.inc"  // termination test of the multi-kernel forms (k_check_*), Norms / decide_status shared by all forms
#include "kernels_coop.inc"  // cooperative register-resident solver (k_coop) and its in-kernel termination test
#include "kernels_guard.inc"  // residual check of the explicit KKT inverse at set-up (falls back to the sweeps when it fails)
#include "kernels_pers.inc"  // persistent streaming solver (k_pers): one launch per solve, the factor read from memory every iteration
#include "kernels_resident.inc"  // LDS-resident single-workgroup solver (k_resident)
#include "kernels_node.inc"  // per-solve prologue / epilogue kernels (scaling, warm start, finish, node digest, objective)
#include "kernels_batched.inc"  // batched mode: sparse row kernels, dense vector-FMA tiles, fp64 matrix-core tiles, batched test
#include "kernels_bpers.inc"  // batched mode: a chunk's lock-step iterations as one persistent launch, the factor in registers and LDS (kbp)
#include "kernels_tree.inc"  // a whole branch-and-bound tree in one launch (LDS-resident problems)
#include "kernels_pool.inc"  // device-resident leaf pool, streaming batch (refill / harvest between chunks)
#include "kernels_bstream.inc"  // the streaming batch as ONE persistent launch: iterations, test, harvest and refill per column group (kbs)
#include "kernels_derived.inc"  // nodes derived from one parent on the device, judged after the batch solve: strong branching, round and fix
#include "kernels_polish.inc"  // polishing of a node's solution: active set, weighted Schur rows, solves and refinement, acceptance
#include "kernels_lockstep.inc"  // B trees in lock step on device-resident leaves: gather / heuristic rows / scatter / incumbent around slice_run; round and fix in those trees
#include "host.inc"  // host side: engine object, allocation, launches, graph capture, solve loops
#include "host_pool.inc"  // host side of the leaf pool (C ABI miosqp_qp_pool_*)
#include "host_search.inc"  // node-at-a-time branch and bound driven from the host in C++ (C ABI miosqp_qp_search_*)
#include "host_stream.inc"  // the host side of the streaming search in C++ (C ABI miosqp_qp_stream_*)
#include "host_lockstep.inc"  // B trees in lock step driven from the host in C++: the store, the pieces every tree driver is built from (ls_*), the wave loop with a driver's step in it; the plain and the round-and-fix step (C ABI miosqp_qp_solve_trees_lockstep, miosqp_qp_solve_trees_lockstep_rf)
#include "host_refill.inc"  // the same trees on columns refilled between chunks: its column arrays and chunk loop between those pieces (C ABI miosqp_qp_solve_trees_refill)
#include "host_lockstep_ahead.inc"  // the lock-step trees with spare columns solving open leaves early: its two kernels and its own wave loop between those pieces (C ABI miosqp_qp_solve_trees_lockstep_ahead)
#include "kernels_lockstep_sb.inc"  // strong and reliability branching in the lock-step trees: x at the integer positions, the children's gather, judge and bounds
#include "host_lockstep_sb.inc"  // ... and its step in host_lockstep.inc's wave loop (C ABI miosqp_qp_solve_trees_lockstep_sb)
#include "kernels_setup_models.inc"  // the dense set-up of many small models in one launch (k_setup_models)
#include "kernels_prepare_models.inc"  // equilibration and packed rows of many models in one launch (k_prepare_models)
#include "host_setup_models.inc"  // ... and its host side: the group, the arena, the engines (C ABI miosqp_qp_setup_models)
#include "host_models.inc"  // what the one-launch tree entries share; trees of different models in one launch (C ABI miosqp_qp_tree_form, miosqp_qp_solve_trees_models)

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
namespace {
// the dynamic-LDS ceiling of a kernel is a property of (process, device, kernel): raised to the chip's 160 KB once instead of
// at every set-up (the call costs ~40 us, a fifth of a small problem's set-up)
hipError_t lds_limit_once(const void *fn, int which) {
  static bool done[28][64] = {};  // (one row per kernel: 0 .. 13 as before, 14: k_setup_models, 15: k_setup_models_auto, 16: k_tree_r_m, 17: k_setup_models_large, 18: k_setup_models_large_auto, 19: k_tree_rf, 20: k_tree_rf_m, 21: k_tree_rf_r_m, 22: k_tree_sb, 23: k_tree_sb_m, 24: k_tree_sb_r_m, 25: k_tree_r, 26: k_tree_rf_r, 27: k_tree_sb_r)
  int dev = 0;
  hipError_t rc = hipGetDevice(&dev);
  if (rc != hipSuccess) return rc;
  if (dev >= 0 && dev < 64 && done[which][dev]) return hipSuccess;
  rc = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (rc == hipSuccess && dev >= 0 && dev < 64) done[which][dev] = true;
  return rc;
}

// ---- polishing (miosqp_qp_polish): scratch of one engine, built on the first call ----
void polish_free(miosqp_qp_engine *e) {
  PolishScratch *s = e->pol;
  if (!s) return;
  for (hipEvent_t ev : s->ev)
    if (ev) hipEventDestroy(ev);
  for (hipEvent_t ev : s->evr)
    if (ev) hipEventDestroy(ev);
  if (s->h) hipHostFree(s->h);
  if (s->din) hipFree(s->din);
  if (s->p.S) hipFree(s->p.S);
  if (s->X) hipFree(s->X);
  if (s->p.LinvT) hipFree(s->p.LinvT);
  delete s;
  e->pol = nullptr;
}

// The values of A as given at set-up in the layout of the scaled rows the device already holds: the same patterns
// (pc_* by constraint, pv_* by variable), pads zero.  Both packings keep a column's / a row's entries in ascending order
// (factor.cpp: pack_rows), which a cursor per row reproduces; every position is checked against the packed index.
// by_con: room for the by-constraint pattern's entries; by_var nullptr: that half is neither built nor checked
// (miosqp_qp_polish_models stages the rows by constraint of every model and needs nothing else).
bool polish_raw_rows(const miosqp_qp_engine *e, double *by_con, std::vector<double> *by_var) {
  const miosqp::PCsr &C = e->fa.panel_by_con, &V = e->fa.panel_by_var;
  const std::vector<int> &Ap = e->sc.Ap, &Ai = e->sc.Ai;
  const int n = e->n, M = e->M;
  if ((int64_t)e->A_raw.size() != (int64_t)Ai.size() || (int)Ap.size() != n + 1) return false;
  std::fill(by_con, by_con + C.idx.size(), 0.0);
  if (by_var) by_var->assign(V.idx.size(), 0.0);
  std::vector<int> cur(M, 0);
  std::vector<std::pair<int, double>> col;
  for (int i = 0; i < n; i++) {
    col.clear();
    for (int p = Ap[i]; p < Ap[i + 1]; p++) col.push_back({Ai[p], e->A_raw[p]});
    if (by_var) {
      std::sort(col.begin(), col.end(), [](const std::pair<int, double> &a, const std::pair<int, double> &b) { return a.first < b.first; });
      if (V.ptr[i] + (int)col.size() > V.ptr[i + 1]) return false;
    }
    for (size_t k = 0; k < col.size(); k++) {
      const int r = col[k].first;
      if (r < 0 || r >= M) return false;
      if (by_var) {
        const int pv = V.ptr[i] + (int)k;
        if (V.idx[pv] != r) return false;
        (*by_var)[pv] = col[k].second;
      }
      const int pc = C.ptr[r] + cur[r]++;
      if (pc >= C.ptr[r + 1] || C.idx[pc] != i) return false;
      by_con[pc] = col[k].second;
    }
  }
  return true;
}

int polish_build(miosqp_qp_engine *e) {
  const size_t n = e->n, M = e->M, ld = e->d.ld;
  if (ld * sizeof(double) > 150 * 1024) {
    g_err = "polish: a row of the reduced system does not fit one workgroup's LDS";
    return MIOSQP_EUNSUPPORTED;
  }
  std::vector<double> by_con(e->fa.panel_by_con.idx.size()), by_var;
  if (!polish_raw_rows(e, by_con.data(), &by_var)) {
    g_err = "polish: the rows of A on the device do not follow the order of the matrix given at set-up";
    return MIOSQP_EUNSUPPORTED;
  }
  PolishScratch *s = new PolishScratch();
  e->pol = s;  // (freed by polish_ensure after a failure below, otherwise with the engine)
  auto al = [](size_t doubles) { return (doubles + 31) & ~(size_t)31; };
  const size_t nA = al(by_con.size() + 64), nAt = al(by_var.size() + 64), nn = al(n + 64), nM = al(M + 64);
  const size_t nin = al(3 * M + n), nout = al(POL_REC_DOUBLES + n + M);
  const size_t ncls = al(M / 8 + 8);  // a class array: one byte per row
  // one block: A | At | in (l u x y) | w b r2 yh prow0 prow1 (M each) | dd xh r1 t v dx dcol0 dcol1 ocol (n each) |
  //            W (n x 64) | counters | record + x + y | the repair loop's: kept x (n), kept y (M), two class arrays,
  //            second record + x + y
  const size_t total = nA + nAt + nin + 6 * nM + 9 * nn + al(n * 64) + 32 + nout + nn + nM + 2 * ncls + nout;
  HIPCHK(hipMalloc((void **)&s->din, total * sizeof(double)));
  HIPCHK(hipMemsetAsync(s->din, 0, total * sizeof(double), e->stream));
  const size_t mat = n * ld + 64;
  HIPCHK(hipMalloc((void **)&s->p.S, mat * sizeof(double)));
  HIPCHK(hipMalloc((void **)&s->X, mat * sizeof(double)));
  HIPCHK(hipMalloc((void **)&s->p.LinvT, mat * sizeof(double)));
  HIPCHK(hipMemsetAsync(s->p.S, 0, mat * sizeof(double), e->stream));
  HIPCHK(hipMemsetAsync(s->X, 0, mat * sizeof(double), e->stream));
  HIPCHK(hipMemsetAsync(s->p.LinvT, 0, mat * sizeof(double), e->stream));
  // pinned: in (l u x y) on the way down, on the way up the final record + x + y and round 0's record; behind both the
  // final classes (they outlive the next call's inputs) and the counters of a round
  const size_t nh = std::max(nin, nout + al(POL_REC_DOUBLES));
  HIPCHK(hipHostMalloc((void **)&s->h, (nh + ncls + 8) * sizeof(double), hipHostMallocDefault));
  s->hcls = (signed char *)(s->h + nh);
  s->hcnt = (int *)(s->h + nh + ncls);
  for (hipEvent_t &ev : s->ev) HIPCHK(hipEventCreate(&ev));
  for (hipEvent_t &ev : s->evr) HIPCHK(hipEventCreate(&ev));
  HIPCHK(hipStreamSynchronize(e->stream));
  Pol &p = s->p;
  const Dev &d = e->d;
  double *c = s->din;
  auto take = [&](size_t doubles) { double *r = c; c += doubles; return r; };
  double *A = take(nA), *At = take(nAt), *in = take(nin);
  if (!by_con.empty()) HIPCHK(hipMemcpy(A, by_con.data(), by_con.size() * sizeof(double), hipMemcpyHostToDevice));
  if (!by_var.empty()) HIPCHK(hipMemcpy(At, by_var.data(), by_var.size() * sizeof(double), hipMemcpyHostToDevice));
  p.n = (int)n; p.M = (int)M; p.ld = (int)ld;
  p.pc_ptr = d.pc_ptr; p.pc_idx = d.pc_idx; p.pv_ptr = d.pv_ptr; p.pv_idx = d.pv_idx; p.pr_ptr = d.pr_ptr; p.pr_idx = d.pr_idx;
  p.A = A; p.At = At; p.pr_val = d.pr_val; p.q = d.qraw;
  p.l = in; p.u = in + M; p.x = in + 2 * M; p.y = in + 2 * M + n;
  p.w = take(nM); p.b = take(nM); p.r2 = take(nM); p.yh = take(nM); p.prow0 = take(nM); p.prow1 = take(nM);
  p.dd = take(nn); p.xh = take(nn); p.r1 = take(nn); p.t = take(nn); p.v = take(nn); p.dx = take(nn);
  p.dcol0 = take(nn); p.dcol1 = take(nn); p.ocol = take(nn);
  s->W = take(al(n * 64));
  p.cnt = (int *)take(32);
  p.rec = (PolRec *)take(nout);
  s->xk = take(nn);
  s->yk = take(nM);
  s->cls_buf[0] = (signed char *)take(ncls);
  s->cls_buf[1] = (signed char *)take(ncls);
  p.cls = s->cls_buf[0];
  p.cls_next = s->cls_buf[1];
  s->rec2 = (PolRec *)take(nout);
  HIPCHK(hipFuncSetAttribute((const void *)k_pol_schur_row, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)(ld * sizeof(double))));
  return 0;
}

int polish_ensure(miosqp_qp_engine *e) {
  if (e->pol) return 0;
  const int rc = polish_build(e);
  if (rc) polish_free(e);  // (a half-built scratch is not kept: the next call starts over)
  return rc;
}

// What both polish entries do first: the argument checks, the scratch, the inputs into the pinned block.  *t0: the wall
// clock once the scratch exists (run_time leaves the one-time allocation out).
int polish_begin(miosqp_qp_engine *e, const double *l, const double *u, const double *x, const double *y, double delta,
                 int32_t refine_iter, int32_t repair_iter, double *t0) {
  ENTER(e);
  if (!(delta > 0.0) || !(delta < QP_INFTY)) {
    g_err = "polish: delta must be positive";
    return MIOSQP_EARG;
  }
  if (refine_iter < 0 || refine_iter > 10) {
    g_err = "polish: refine_iter must be in 0..10";
    return MIOSQP_EARG;
  }
  if (repair_iter < 0 || repair_iter >= POL_MAX_ROUNDS) {
    g_err = "polish: repair_iter must be in 0..20";
    return MIOSQP_EARG;
  }
  const size_t n = e->n, M = e->M;
  for (size_t j = 0; j < M; j++) {
    if (l[j] > u[j]) return MIOSQP_EBOUNDS;
    if (l[j] != l[j] || u[j] != u[j] || y[j] != y[j]) {
      g_err = "polish: NaN in l, u or y (a node without a solution cannot be polished)";
      return MIOSQP_EARG;
    }
  }
  for (size_t i = 0; i < n; i++)
    if (x[i] != x[i]) {
      g_err = "polish: NaN in x (a node without a solution cannot be polished)";
      return MIOSQP_EARG;
    }
  if (int rc = polish_ensure(e)) return rc;
  *t0 = wall();
  PolishScratch *s = e->pol;
  Pol &p = s->p;
  p.delta = delta;
  p.inv_delta = 1.0 / delta;
  p.cls = s->cls_buf[0];
  p.cls_next = s->cls_buf[1];
  double *h = s->h;
  memcpy(h, l, sizeof(double) * M);
  memcpy(h + M, u, sizeof(double) * M);
  memcpy(h + 2 * M, x, sizeof(double) * n);
  memcpy(h + 2 * M + n, y, sizeof(double) * M);
  return 0;
}

// S of the set in p.w, its LDL^T, then (xh, yh) = ksolve(-q, b) and refine_iter corrections by the residuals of the
// unregularised system: with xh = yh = 0 the first pass's residuals are exactly (-q, b).  ev2 / ev3, when given, are
// recorded behind the rows of S and behind the factorisation.
int polish_queue_solve(miosqp_qp_engine *e, const Pol &p, int refine_iter, hipEvent_t ev2, hipEvent_t ev3) {
  PolishScratch *s = e->pol;
  hipStream_t st = e->stream;
  const size_t n = e->n, M = e->M;
  const dim3 gM((unsigned)((M + 3) / 4)), gn((unsigned)((n + 3) / 4)), b256(256);
  hipLaunchKernelGGL(k_pol_schur_row, dim3((unsigned)n), b256, p.ld * sizeof(double), st, p);
  if (ev2) HIPCHK(hipEventRecord(ev2, st));
  if (miosqp_device_ldl_inverse_resident((int)n, p.ld, p.S, s->X, p.LinvT, s->W, p.dd, p.cnt + 2, st)) {
    g_err = "polish: the factorisation of the reduced system could not be queued";
    return MIOSQP_EHIP;
  }
  if (ev3) HIPCHK(hipEventRecord(ev3, st));
  for (int it = 0; it <= refine_iter; it++) {
    if (M) hipLaunchKernelGGL(k_pol_r2, gM, b256, 0, st, p);
    hipLaunchKernelGGL(k_pol_rhs, gn, b256, 0, st, p);
    hipLaunchKernelGGL(k_pol_lower, gn, b256, 0, st, p);
    hipLaunchKernelGGL(k_pol_upper, gn, b256, 0, st, p);
    if (M) hipLaunchKernelGGL(k_pol_dy, gM, b256, 0, st, p);
  }
  return 0;
}

// the residuals of (xh, yh), the acceptance test and the record p.rec with the point behind it
void polish_queue_decide(miosqp_qp_engine *e, const Pol &p) {
  hipStream_t st = e->stream;
  const size_t n = e->n, M = e->M;
  const dim3 gM((unsigned)((M + 3) / 4)), gn((unsigned)((n + 3) / 4)), b256(256);
  if (M) hipLaunchKernelGGL(k_pol_rows_after, gM, b256, 0, st, p);
  hipLaunchKernelGGL(k_pol_cols, gn, b256, 0, st, p);
  hipLaunchKernelGGL(k_pol_decide, dim3(1), b256, 0, st, p);
}

// The polish proper, queued (events 0..4 around its stages): inputs down, the set guessed from (x, y), the solves, the
// decision.  It is all of miosqp_qp_polish up to the copy back, and round 0 of miosqp_qp_polish_repair.
int polish_queue_round0(miosqp_qp_engine *e, int refine_iter) {
  PolishScratch *s = e->pol;
  const Pol &p = s->p;
  hipStream_t st = e->stream;
  const size_t n = e->n, M = e->M;
  HIPCHK(hipEventRecord(s->ev[0], st));
  HIPCHK(hipMemcpyAsync((void *)p.l, s->h, sizeof(double) * (3 * M + n), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(p.cnt, 0, 8 * sizeof(int), st));
  HIPCHK(hipMemsetAsync(p.xh, 0, sizeof(double) * n, st));
  if (M) {
    HIPCHK(hipMemsetAsync(p.yh, 0, sizeof(double) * M, st));
    hipLaunchKernelGGL(k_pol_classify, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, p);
  }
  HIPCHK(hipEventRecord(s->ev[1], st));
  if (int rc = polish_queue_solve(e, p, refine_iter, s->ev[2], s->ev[3])) return rc;
  polish_queue_decide(e, p);
  HIPCHK(hipEventRecord(s->ev[4], st));
  return 0;
}

// ---- polishing of many instances (miosqp_qp_polish_many): the pinned blocks and their device copies, grown with B ----
void polish_many_free(miosqp::PolManyScratch *&s) {
  if (!s) return;
  for (void *ev : s->ev)
    if (ev) hipEventDestroy((hipEvent_t)ev);
  if (s->h_in) hipHostFree(s->h_in);
  if (s->h_out) hipHostFree(s->h_out);
  if (s->d_in) hipFree(s->d_in);
  if (s->d_out) hipFree(s->d_out);
  if (s->slab) hipFree(s->slab);
  delete s;
  s = nullptr;
}

int polish_many_ensure(miosqp_qp_engine *e, miosqp::PolManyScratch *&slot, size_t n_in, size_t n_out, size_t n_slab) {
  if (!slot) {
    slot = new miosqp::PolManyScratch();
    for (void *&ev : slot->ev) HIPCHK(hipEventCreate((hipEvent_t *)&ev));
  }
  miosqp::PolManyScratch *s = slot;
  if (n_slab > s->cap_slab) {  // (the large entry's slabs: one per workgroup of the launch)
    HIPCHK(hipStreamSynchronize(e->stream));
    if (s->slab) hipFree(s->slab);
    s->slab = nullptr;
    s->cap_slab = 0;
    HIPCHK(hipMalloc((void **)&s->slab, n_slab * sizeof(double)));
    s->cap_slab = n_slab;
  }
  if (n_in > s->cap_in) {
    HIPCHK(hipStreamSynchronize(e->stream));
    if (s->h_in) hipHostFree(s->h_in);
    if (s->d_in) hipFree(s->d_in);
    s->h_in = s->d_in = nullptr;
    s->cap_in = 0;
    HIPCHK(hipHostMalloc((void **)&s->h_in, n_in * sizeof(double), hipHostMallocDefault));
    HIPCHK(hipMalloc((void **)&s->d_in, n_in * sizeof(double)));
    s->cap_in = n_in;
  }
  if (n_out > s->cap_out) {
    HIPCHK(hipStreamSynchronize(e->stream));
    if (s->h_out) hipHostFree(s->h_out);
    if (s->d_out) hipFree(s->d_out);
    s->h_out = s->d_out = nullptr;
    s->cap_out = 0;
    s->last_B = 0;
    HIPCHK(hipHostMalloc((void **)&s->h_out, n_out * sizeof(double), hipHostMallocDefault));
    HIPCHK(hipMalloc((void **)&s->d_out, n_out * sizeof(double)));
    s->cap_out = n_out;
  }
  return 0;
}

void polish_fill_info(const PolRec &r, miosqp_polish_info *info) {
  info->accepted = r.accepted;
  info->reason = r.reason;
  info->n_lower = r.n_lower;
  info->n_upper = r.n_upper;
  info->pri_before = r.pri_before;
  info->dua_before = r.dua_before;
  info->pri_after = r.pri_after;
  info->dua_after = r.dua_after;
  info->obj = r.obj;
}
}  // namespace

extern "C" {

const char *miosqp_qp_last_error(void) { return g_err.c_str(); }

int miosqp_qp_default_settings(miosqp_qp_settings *s) {
  if (!s) return MIOSQP_EARG;
  memset(s, 0, sizeof *s);
  s->rho = 0.1;
  s->sigma = 1e-6;
  s->alpha = 1.6;
  s->eps_abs = 1e-3;
  s->eps_rel = 1e-3;
  s->eps_prim_inf = 1e-4;
  s->eps_dual_inf = 1e-4;
  s->max_iter = 4000;
  s->scaling = 10;
  s->check_termination = 25;
  s->warm_start = 1;
  s->device = -1;
  s->max_batch = 1;
  s->fold = -1;
  s->resident = -1;
  s->setup_on_device = -1;
  s->coop = -1;
  s->pers = -1;
  s->batch_pers = -1;
  return 0;
}

int miosqp_qp_constant(const char *name) {
  if (!name) return 0;
  if (!strcmp(name, "OSQP_SOLVED")) return MIOSQP_QP_SOLVED;
  if (!strcmp(name, "OSQP_MAX_ITER_REACHED")) return MIOSQP_QP_MAX_ITER_REACHED;
  if (!strcmp(name, "OSQP_PRIMAL_INFEASIBLE")) return MIOSQP_QP_PRIMAL_INFEASIBLE;
  if (!strcmp(name, "OSQP_DUAL_INFEASIBLE")) return MIOSQP_QP_DUAL_INFEASIBLE;
  if (!strcmp(name, "OSQP_UNSOLVED")) return MIOSQP_QP_UNSOLVED;
  return 0;
}

int miosqp_qp_cleanup(miosqp_qp_engine *e) {
  if (!e) return 0;
  if (e->device >= 0) (void)hipSetDevice(e->device);
  kbs_stop(e);  // (a persistent launch of the stream still queued leaves at its next chunk boundary)
  if (e->stream) hipStreamSynchronize(e->stream);
  if (e->side) {
    hipStreamSynchronize(e->side);
    hipStreamDestroy(e->side);
    e->side = nullptr;
  }
  chip_quit(e);
  if (e->x_full) hipGraphExecDestroy(e->x_full);
  if (e->x_tail) hipGraphExecDestroy(e->x_tail);
  if (e->g_full) hipGraphDestroy(e->g_full);
  if (e->g_tail) hipGraphDestroy(e->g_tail);
  {
    // small pool chunks are parked for the next engine of the process, zero-filled HERE (outside anybody's set-up time):
    // fill on the engine's stream, wait, then offer them
    std::vector<ParkedChunk> park;
    for (void *p : e->allocs) {
      bool keep = false;
      for (const ParkedChunk &c : e->chunks)
        if (c.p == p && c.bytes <= CHUNK_PARK_MAX && park.size() < 8 && !getenv("MIOSQP_NO_CACHE")) {
          keep = hipMemsetAsync(c.p, 0, c.bytes, e->stream) == hipSuccess;
          if (keep) park.push_back(c);
          break;
        }
      if (!keep) hipFree(p);
    }
    if (!park.empty()) {
      const bool filled = hipStreamSynchronize(e->stream) == hipSuccess;
      std::lock_guard<std::mutex> lk(g_rt_mutex);
      for (const ParkedChunk &c : park) {
        if (filled && g_chunk_cache.size() < 8) g_chunk_cache.push_back(c);
        else hipFree(c.p);
      }
    }
  }
  drop_stream_graph(e);
  for (hipEvent_t ev : e->ev_pool)
    if (ev) hipEventDestroy(ev);
  if (e->sdriver) delete static_cast<StreamDriver *>(e->sdriver);
  if (e->search) {
    NodeSearch *S = static_cast<NodeSearch *>(e->search);
    if (S->dg) hipHostFree(S->dg);
    if (S->own_block) hipFree(S->own_block);
    for (hipEvent_t ev : S->ev)
      if (ev) hipEventDestroy(ev);
    for (hipEvent_t ev : S->ev_run)
      if (ev) hipEventDestroy(ev);
    if (S->mail_host) hipHostFree(S->mail_host);
    delete S;
  }
  lockstep_free(e->lockstep);
  if (e->h_ready) hipHostFree(e->h_ready);
  if (e->h_dg) hipHostFree(e->h_dg);
  if (e->h_pctl) hipHostFree(e->h_pctl);
  if (e->hb_in) hipHostFree(e->hb_in);
  if (e->hb_out) hipHostFree(e->hb_out);
  if (e->hb_int) hipHostFree(e->hb_int);
  if (e->hb_dbl) hipHostFree(e->hb_dbl);
  if (e->hb_q) hipHostFree(e->hb_q);
  if (e->h_der) hipHostFree(e->h_der);
  if (e->mm_host) hipHostFree(e->mm_host);
  polish_free(e);
  polish_many_free(e->polm);
  polish_many_free(e->polml);
  drop_chunk_graphs(e);
  if (e->group) group_engine_release(e);  // (miosqp_qp_setup_models: its own events go, one reference to the group is dropped)
  else rt_release(e->rt);  // stream, events and pinned staging go back to the per-process cache
  delete e;
  return 0;
}

static int stage_wait(miosqp_qp_engine *e, int k);
static int stage_mark(miosqp_qp_engine *e, int k);

// rho chosen once per problem (settings.rho_auto): OSQP's update rule on the scaled iterates after RHO_ONCE_ITERS
// iterations from zero, rounded to two significant digits -- loop for loop the arithmetic the CPU restatement under the
// tests uses for the same setting (its rho_estimate), on the host's copy of the scaled matrices (the iterates come from
// the device).
constexpr int RHO_ONCE_ITERS = 50;
static double rho_round2(double r) {
  if (!(r > 0)) return r;
  const double e = floor(log10(r)), p = pow(10.0, e);
  return floor(r / p * 10.0 + 0.5) / 10.0 * p;
}
static double rho_estimate_host(const miosqp::Scaled &sc, double rho, const double *x, const double *z, const double *y) {
  const int n = sc.n, M = sc.M;
  std::vector<double> Ax(M, 0.0), Px(n, 0.0), Aty(n, 0.0);
  for (int j = 0; j < n; j++)
    for (int p = sc.Ap[j]; p < sc.Ap[j + 1]; p++) Ax[sc.Ai[p]] += sc.Ax[p] * x[j];
  for (int j = 0; j < n; j++)
    for (int p = sc.Pp[j]; p < sc.Pp[j + 1]; p++) {
      const int i = sc.Pi[p];
      Px[i] += sc.Px[p] * x[j];
      if (i != j) Px[j] += sc.Px[p] * x[i];
    }
  for (int j = 0; j < n; j++) {
    double t = 0;
    for (int p = sc.Ap[j]; p < sc.Ap[j + 1]; p++) t += sc.Ax[p] * y[sc.Ai[p]];
    Aty[j] = t;
  }
  auto ninf = [](const double *v, int k) { double r = 0; for (int i = 0; i < k; i++) r = fmax(r, fabs(v[i])); return r; };
  double pri = 0, dua = 0;
  for (int i = 0; i < M; i++) pri = fmax(pri, fabs(Ax[i] - z[i]));
  for (int j = 0; j < n; j++) dua = fmax(dua, fabs(Px[j] + sc.q[j] + Aty[j]));
  const double pn = fmax(ninf(z, M), ninf(Ax.data(), M));
  const double dn = fmax(ninf(sc.q.data(), n), fmax(ninf(Aty.data(), n), ninf(Px.data(), n)));
  pri /= (pn + 1e-10);
  dua /= (dn + 1e-10);
  double r = rho * sqrt(pri / (dua + 1e-10));
  r = fmin(fmax(r, 1e-6), 1e6);
  return rho_round2(r);
}

int miosqp_qp_setup(miosqp_qp_engine **out, int32_t n, int32_t M, const int32_t *Pp, const int32_t *Pi,
                    const double *Px, const int32_t *Ap, const int32_t *Ai, const double *Ax,
                    const double *q, const double *l, const double *u, const miosqp_qp_settings *s_in) {
  if (!out || n <= 0 || M < 0 || !Pp || !Ap || !q || !s_in || (M > 0 && (!l || !u))) {
    g_err = "setup: bad argument";
    return MIOSQP_EARG;
  }
  miosqp_qp_settings s_own = *s_in;
  miosqp_qp_settings *s = &s_own;
  // rho chosen at set-up (rho_auto), r05: ONE set-up.  The probing iterations run on THIS engine, in the plain four-kernel
  // factor form, the moment its factor at the starting rho is on the device (before the product form, the explicit
  // inverse, graphs and calibrations exist); then only what depends on rho is built again -- the factor, on the host --
  // and copied over the first one.  Measured at config 2: 153 ms (two set-ups) -> see DESIGN.md; the equilibration, the
  // allocations, the runtime objects, the product form, the inverse, captures and calibrations happen once.
  // Kept on the two-set-up path: problems factorised on the device (n >= 1024: the factor never visits the host) and
  // the small ones whose probe engine is the one-workgroup solver (fifty iterations there cost less than 200 launches).
  bool probe_inline = false;
  if (s->rho_auto && M > 0) {
    int on_dev_pre = s->setup_on_device;
    if (on_dev_pre < 0) on_dev_pre = n >= 1024 ? 1 : 0;
    probe_inline = !on_dev_pre && n + M > 400 && !getenv("MIOSQP_RHO_TWO_SETUPS");
    if (probe_inline) s->rho_auto = 0;
  }
  if (s->rho_auto && M > 0) {
    // a throw-away engine in the plain multi-kernel form for the probing iterations, then the real one at the chosen
    // rho (the equilibration does not depend on rho and is simply repeated: set-up runs once per MIQP)
    miosqp_qp_settings s1 = *s;
    s1.rho_auto = 0;
    miosqp_qp_settings sp = s1;
    sp.coop = 0;
    sp.pers = 0;
    sp.max_batch = 1;
    miosqp_qp_engine *probe = nullptr;
    int rc = miosqp_qp_setup(&probe, n, M, Pp, Pi, Px, Ap, Ai, Ax, q, l, u, &sp);
    if (rc) return rc;
    std::vector<double> xs(n), zs(M), ys(M);
    {
      const int big = n > M ? n : M;
      hipLaunchKernelGGL(k_zero_iterates, dim3((big + 255) / 256), dim3(256), 0, probe->stream, probe->d);
    }
    rc = miosqp_qp_debug_iterate(probe, RHO_ONCE_ITERS, xs.data(), zs.data(), ys.data());
    double rho_new = s1.rho;
    if (!rc) rho_new = rho_estimate_host(probe->sc, s1.rho, xs.data(), zs.data(), ys.data());
    miosqp_qp_cleanup(probe);
    if (rc) return rc;
    if (rho_new > 0) s1.rho = rho_new;
    rc = miosqp_qp_setup(out, n, M, Pp, Pi, Px, Ap, Ai, Ax, q, l, u, &s1);
    if (!rc) (*out)->st.rho_auto = 1;
    return rc;
  }
  if (M == 0) {
    // miOSQP always has rows: data.py:5-33 appends one identity row per integer variable
    g_err = "setup: the engine needs at least one constraint row (M >= 1)";
    return MIOSQP_EARG;
  }
  for (int i = 0; i < M; i++)
    if (l[i] > u[i]) {
      g_err = "setup: lower bound above upper bound";
      return MIOSQP_EARG;
    }
  if (!(s->rho > 0) || !(s->sigma > 0) || !(s->alpha > 0 && s->alpha < 2) || s->max_iter <= 0) {
    g_err = "setup: settings out of range";
    return MIOSQP_EARG;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    g_err = "no HIP device visible: the relaxation engine has no CPU fallback";
    return MIOSQP_ENODEV;
  }
  if (s->device >= 0) HIPCHK(hipSetDevice(s->device));
  miosqp_qp_engine *e = new miosqp_qp_engine();
  HIPCHK(hipGetDevice(&e->device));
  const bool t_on = getenv("MIOSQP_SETUP_TIMING") != nullptr;
  double t_last = wall();
  const double t_begin = t_last;
  auto tick = [&](const char *what) {
    if (!t_on) return;
    const double now = wall();
    fprintf(stderr, "[miosqp setup] %-32s %8.3f ms\n", what, 1e3 * (now - t_last));
    t_last = now;
  };
  e->n = n;
  e->M = M;
  e->st = *s;
  if (e->st.check_termination <= 0 || e->st.check_termination > e->st.max_iter)
    e->st.check_termination = e->st.max_iter;
  std::string err;
  // the array-sized parts of the setup on the device for large problems: the equilibration's
  // maxima and products, the Schur complement, the dense LDL^T and its triangular inverse
  int on_dev = s->setup_on_device;
  if (on_dev < 0) on_dev = n >= 1024 ? 1 : 0;
  e->setup_on_device = on_dev != 0;
  {
    bool done = false;
    if (on_dev && s->scaling > 0 && !getenv("MIOSQP_SETUP_HOST_RUIZ")) {
      miosqp::RuizOps ops;
      void *storage = nullptr;
      miosqp_device_ruiz_ops(&ops, &storage, nullptr);
      done = miosqp::scale_problem(n, M, Pp, Pi, Px, Ap, Ai, Ax, q, s->scaling, e->sc, &ops);
      miosqp_device_ruiz_free(storage);
      if (!done) fprintf(stderr, "miosqp: equilibration on the device failed, redone on the host\n");
    }
    if (!done) miosqp::scale_problem(n, M, Pp, Pi, Px, Ap, Ai, Ax, q, s->scaling, e->sc);
  }
  // Will the product form be built (on the host, from Linv)?  Decided here because the device stage of the setup may
  // then leave Linv / LinvT on the device instead of sending them down and up again.
  int want_fold = s->fold;
  bool coop_pref = false;
  {
    const double dens = M > 0 ? (double)Ap[n] / ((double)n * M) : 0.0;
    const double fold_bytes = 8.0 * ((double)n * (M + n) + (double)M * n);
    const bool res_w_on = !(getenv("MIOSQP_RES_W") && atoi(getenv("MIOSQP_RES_W")) == 0);
    const bool fits_lds = resident_lds_doubles(n, M, res_w_on && M > 0 && n + M <= RES_W_MAX) * sizeof(double) <= 150 * 1024;
    // the cooperative solver only needs the product form to build its explicit inverse from, whatever
    // the sparsity; it is preferred from n + M = 64 on (measured: equal to the LDS-resident workgroup
    // below 100, 1.8x at 160, 2.2x at 240)
    int coop_req = s->coop;
    if (const char *ev = getenv("MIOSQP_COOP")) coop_req = atoi(ev);
    const bool coop_fits = M > 0 && n + M <= 2048;
    // ... and from n + M = 193 on since the LDS-resident workgroup runs its loop on the explicit inverse in registers
    // (res_admm_w: 0.9-1.4 us per iteration at n + M = 85-190 against 2.1-2.2 for the cooperative grid)
    const bool res_w_here = res_w_on && M > 0 && n + M <= RES_W_MAX && s->resident != 0;
    coop_pref = coop_fits && (coop_req == 1 || (coop_req < 0 && n + M >= 64 && !res_w_here)) && s->resident != 1;
    if (want_fold < 0)
      want_fold = (M > 0 && ((dens >= 0.30 && fold_bytes <= 4.0e9) || (fits_lds && s->resident != 0) || coop_pref)) ? 1 : 0;
  }
  miosqp::DenseAccelCtx actx;
  actx.keep_on_device = on_dev && !(want_fold && M > 0) && !getenv("MIOSQP_SETUP_ROUNDTRIP");
  actx.schur_on_device = on_dev && M > 0 && !getenv("MIOSQP_SETUP_HOST_SCHUR");
  if (!miosqp::build_factor(e->sc, Pp, Pi, Px, s->rho, s->sigma, e->fa, err,
                            on_dev ? miosqp_device_ldl_inverse : nullptr, &actx)) {
    g_err = err;
    if (actx.dLinv) hipFree(actx.dLinv);
    if (actx.dLinvT) hipFree(actx.dLinvT);
    delete e;
    return MIOSQP_EFACTOR;
  }
  if (actx.dLinv) e->allocs.push_back(actx.dLinv);    // freed with the engine
  if (actx.dLinvT) e->allocs.push_back(actx.dLinvT);
  tick("host: scaling + factor (total)");
  e->nnzA = Ap[n];
  e->A_raw.assign(Ax, Ax + Ap[n]);  // polishing works on the unscaled A
  e->nnzPtriu = (int64_t)e->sc.Pi.size();
  const miosqp::Factor &f = e->fa;
  Dev &d = e->d;
  d.n = n; d.M = M; d.ld = f.ld; d.n_int = 0; d.m_orig = M; d.wh_m = M;
  d.rho = s->rho; d.rho_inv = 1.0 / s->rho; d.sigma = s->sigma; d.alpha = s->alpha; d.eps_abs = s->eps_abs; d.eps_rel = s->eps_rel;
  d.eps_pinf = s->eps_prim_inf; d.eps_dinf = s->eps_dual_inf; d.c = e->sc.c; d.cinv = e->sc.cinv;
  {
    // one chunk for everything this setup will place on the device
    const size_t np2 = f.panel_by_var.idx.size() + f.panel_by_con.idx.size();
    size_t est = np2 * (4 + 16) + 2 * f.Linv.size() * 8 + (f.Pbar.idx.size() + f.Praw.idx.size()) * 12 +
                 ((size_t)60 * n + (size_t)60 * M) * 8 + ((size_t)n * ((M + n + 8)) + (size_t)M * (n + 8)) * 8 +
                 200 * 512 + ((size_t)1 << 16);
    int rc0 = pool_reserve(e, est);
    if (rc0) { miosqp_qp_cleanup(e); return rc0; }
  }
  tick("device pool: malloc + zero fill");
#define UP(vec, field)                                   \
  do {                                                   \
    int rc__ = dupload(e, vec, &d.field);                \
    if (rc__) { miosqp_qp_cleanup(e); return rc__; }     \
  } while (0)
  upload_begin(e);
  UP(f.panel_by_var.ptr, pv_ptr); UP(f.panel_by_var.idx, pv_idx); UP(f.panel_by_var.val, pv_L); UP(f.At_val, pv_At);
  UP(f.panel_by_con.ptr, pc_ptr); UP(f.panel_by_con.idx, pc_idx); UP(f.panel_by_con.val, pc_L); UP(f.A_val, pc_A);
  if (actx.dLinv) {  // computed on the device and left there
    d.Linv = actx.dLinv;
    d.LinvT = actx.dLinvT;
  } else {
    UP(f.Linv, Linv); UP(f.LinvT, LinvT);
  }
  UP(f.d2inv, d2inv);
  UP(f.Pbar.ptr, pb_ptr); UP(f.Pbar.idx, pb_idx); UP(f.Pbar.val, pb_val);
  UP(f.Praw.ptr, pr_ptr); UP(f.Praw.idx, pr_idx); UP(f.Praw.val, pr_val);
  UP(e->sc.D, D); UP(e->sc.Dinv, Dinv); UP(e->sc.E, E); UP(e->sc.Einv, Einv);
#undef UP
  {
    int rcu = upload_end(e);
    if (rcu) { miosqp_qp_cleanup(e); return rcu; }
  }
#define AL(field, count)                                 \
  do {                                                   \
    int rc__ = dalloc(e, &d.field, (size_t)(count));     \
    if (rc__) { miosqp_qp_cleanup(e); return rc__; }     \
  } while (0)
  AL(q, n); AL(qraw, n); AL(l, M); AL(u, M); AL(x, n); AL(z, M); AL(y, M); AL(wh, (size_t)M + n); AL(cv, n); AL(ut, n);
  AL(xt, n); AL(dx, n); AL(dy, M); AL(sm, 8 * (size_t)M); AL(sn, 10 * (size_t)n);
  d.rx = d.wh + M;
  AL(xi, n); AL(xis, n); AL(root_l, M); AL(root_u, M);
  d.digest = 0;
  AL(ctrl, 1);
  // staging block: raw_l | raw_u | raw_x | raw_y contiguous, out_x | out_y contiguous
  AL(raw_l, 2 * (size_t)M + n + M);
  d.raw_u = d.raw_l + M; d.raw_x = d.raw_u + M; d.raw_y = d.raw_x + n;
  AL(out_x, (size_t)n + M);
  d.out_y = d.out_x + n;
  {
    int *ii = nullptr;
    int rc = dalloc(e, &ii, (size_t)n);
    if (rc) { miosqp_qp_cleanup(e); return rc; }
    d.i_idx = ii;
  }
#undef AL
  tick("uploads (factor, matrices)");
  {
    int rcb = rt_acquire(e->device, 2 * (size_t)M + n + M + 1, (size_t)n + M + 1, e->rt);
    if (rcb) { miosqp_qp_cleanup(e); return rcb; }
    e->stream = e->rt.stream;
    e->ev0 = e->rt.ev0; e->ev1 = e->rt.ev1; e->evc0 = e->rt.evc0; e->evc1 = e->rt.evc1;
    e->ev_chunk[0] = e->rt.ev_chunk[0]; e->ev_chunk[1] = e->rt.ev_chunk[1];
    e->h_in = e->rt.h_in; e->h_out = e->rt.h_out; e->h_ctrl = e->rt.h_ctrl; e->h_ctrl2 = e->rt.h_ctrl2;
  }
  tick("stream, events, pinned buffers");
  // scaled q, raw q, scaled bounds
  if (e->rt.in_cap >= 2 * (size_t)M + 2 * (size_t)n) {
    // through the pinned staging block on the engine's stream (four blocking copies from pageable memory were ~40 us of
    // a small problem's set-up): [ l | u ] in region 0, [ scaled q | q ] in region 1, marked busy until the copies are out
    double *h = e->h_in;
    memcpy(h, l, sizeof(double) * M);
    memcpy(h + M, u, sizeof(double) * M);
    memcpy(h + 2 * (size_t)M, e->sc.q.data(), sizeof(double) * n);
    memcpy(h + 2 * (size_t)M + n, q, sizeof(double) * n);
    if (M > 0) {
      HIPCHK(hipMemcpyAsync(d.raw_l, h, sizeof(double) * M, hipMemcpyHostToDevice, e->stream));
      HIPCHK(hipMemcpyAsync(d.raw_u, h + M, sizeof(double) * M, hipMemcpyHostToDevice, e->stream));
    }
    HIPCHK(hipMemcpyAsync(d.q, h + 2 * (size_t)M, sizeof(double) * n, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(d.qraw, h + 2 * (size_t)M + n, sizeof(double) * n, hipMemcpyHostToDevice, e->stream));
    if (int rcm = stage_mark(e, 0)) { miosqp_qp_cleanup(e); return rcm; }
    if (int rcm = stage_mark(e, 1)) { miosqp_qp_cleanup(e); return rcm; }
  } else {
    HIPCHK(hipMemcpy(d.q, e->sc.q.data(), sizeof(double) * n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d.qraw, q, sizeof(double) * n, hipMemcpyHostToDevice));
    if (M > 0) {
      HIPCHK(hipMemcpy(d.raw_l, l, sizeof(double) * M, hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(d.raw_u, u, sizeof(double) * M, hipMemcpyHostToDevice));
    }
  }
  if (M > 0) hipLaunchKernelGGL(k_scale_bounds, dim3((M + 255) / 256), dim3(256), 0, e->stream, d);
  hipLaunchKernelGGL(k_reset_ctrl, dim3(1), dim3(1), 0, e->stream, d);
  e->tpr_pv = pick_tpr((double)f.nnz_panel / n);
  e->tpr_pc = pick_tpr(M > 0 ? (double)f.nnz_panel / M : 1.0);
  e->tpr_tail = pick_tpr(0.5 * n);
  e->tpr_pb = pick_tpr((double)f.Pbar.nnz / n);
  e->tpr_pr = pick_tpr((double)f.Praw.nnz / n);
  if (probe_inline) {
    // the rule's recipe: RHO_ONCE_ITERS iterations from zero on the set-up's bounds, the rule, a new factor
    std::vector<double> xs(n), zs(M), ys(M);
    {
      const int big = n > M ? n : M;
      hipLaunchKernelGGL(k_zero_iterates, dim3((big + 255) / 256), dim3(256), 0, e->stream, d);
    }
    int rc = miosqp_qp_debug_iterate(e, RHO_ONCE_ITERS, xs.data(), zs.data(), ys.data());
    if (rc) { miosqp_qp_cleanup(e); return rc; }
    double rho_new = rho_estimate_host(e->sc, s->rho, xs.data(), zs.data(), ys.data());
    tick("rho chosen at set-up: probing iterations + the rule");
    if (rho_new > 0 && rho_new != s->rho) {
      std::string err2;
      // (the dense part on the device -- a third of the host's time at config 2 --, the result back on the host for the
      //  product form's rows; MIOSQP_RHO_HOST_REFACTOR=1 keeps it on the host)
      miosqp::DenseAccelCtx actx2;
      actx2.stream = e->stream;
      const bool dev2 = !getenv("MIOSQP_RHO_HOST_REFACTOR");
      if (!miosqp::build_factor(e->sc, Pp, Pi, Px, rho_new, s->sigma, e->fa, err2, dev2 ? miosqp_device_ldl_inverse : nullptr,
                                dev2 ? &actx2 : nullptr, true)) {
        // the factor at the chosen rho failed (a pivot, the device): the factor is rebuilt in place, so the one at the
        // starting rho -- which exists: the probing iterations ran on it -- is built again and the choice is dropped
        fprintf(stderr, "miosqp: rho chosen at set-up (%g): the factor failed (%s); keeping rho = %g\n", rho_new, err2.c_str(), s->rho);
        rho_new = s->rho;
        std::string err3;
        if (!miosqp::build_factor(e->sc, Pp, Pi, Px, rho_new, s->sigma, e->fa, err3, nullptr, nullptr, true)) {
          g_err = err3;
          miosqp_qp_cleanup(e);
          return MIOSQP_EFACTOR;
        }
      }
      const miosqp::Factor &f2 = e->fa;  // same patterns, same sizes: copied over the first factor
      HIPCHK(hipMemcpy(const_cast<double *>(d.pv_L), f2.panel_by_var.val.data(), sizeof(double) * f2.panel_by_var.val.size(), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(const_cast<double *>(d.pc_L), f2.panel_by_con.val.data(), sizeof(double) * f2.panel_by_con.val.size(), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(const_cast<double *>(d.Linv), f2.Linv.data(), sizeof(double) * f2.Linv.size(), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(const_cast<double *>(d.LinvT), f2.LinvT.data(), sizeof(double) * f2.LinvT.size(), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(const_cast<double *>(d.d2inv), f2.d2inv.data(), sizeof(double) * f2.d2inv.size(), hipMemcpyHostToDevice));
      s->rho = rho_new;
      e->st.rho = rho_new;
      d.rho = rho_new;
      d.rho_inv = 1.0 / rho_new;
      tick("rho chosen at set-up: the factor again");
    }
    e->st.rho_auto = 1;
    {
      const int big = n > M ? n : M;
      hipLaunchKernelGGL(k_zero_iterates, dim3((big + 255) / 256), dim3(256), 0, e->stream, d);
    }
    hipLaunchKernelGGL(k_reset_ctrl, dim3(1), dim3(1), 0, e->stream, d);
  }
  {
    // product-form factor: worth it when the panel is dense (bytes no worse, half the launches); decided above
    const int want = want_fold;
    if (want && M > 0) {
      miosqp::build_folded(f, e->fo);
      upload_begin(e);
      int rc = dupload(e, e->fo.rows, &d.f_rows);
      if (!rc) rc = dupload(e, e->fo.GmT, &d.f_GmT);
      if (!rc) rc = dupload(e, e->fo.Ad, &d.f_Ad);
      if (!rc) rc = dupload(e, e->fo.Atd, &d.f_Atd);
      if (!rc) rc = dupload(e, e->fo.Pd, &d.f_Pd);
      if (!rc) rc = upload_end(e);
      else e->up_on = false;
      d.ldm = e->fo.ldm;
      if (rc) { miosqp_qp_cleanup(e); return rc; }
      d.ldf = e->fo.ldf;
      d.ldn = e->fo.ldn;
      d.f_rows2 = d.f_rows;
      d.ldf2 = d.ldf;
      e->fold = true;
      e->tpr_ff = pick_tpr(M + 0.5 * n);
      e->tpr_fx = pick_tpr(0.5 * n);
      e->tpr_fc = pick_tpr((double)n);
      {
        const bool res_w = n + M <= RES_W_MAX && M > 0 && !(getenv("MIOSQP_RES_W") && atoi(getenv("MIOSQP_RES_W")) == 0);
        size_t need = resident_lds_doubles(n, M, res_w) * sizeof(double);
        e->sp_nnzA = f.panel_by_con.idx.size();
        e->sp_nnzP = f.Pbar.idx.size();
        const bool sp_on = res_w && !(getenv("MIOSQP_RES_SP") && atoi(getenv("MIOSQP_RES_SP")) == 0);
        const size_t sp_bytes = res_sp_doubles(e->sp_nnzA, e->sp_nnzP, n, M) * sizeof(double);
        if (sp_on && need + sp_bytes <= 150 * 1024) {  // room for the sparse rows of the termination test in LDS
          e->res_sp_off = (int)(need / sizeof(double));
          need += sp_bytes;
        }
        int wantr = s->resident;
        if (wantr < 0) wantr = (need <= 150 * 1024 && !coop_pref) ? 1 : 0;
        if (wantr && need <= 160 * 1024) {
          e->resident = true;
          e->res_lds = need;
          if (res_w) {
            // the explicit KKT inverse for the register-resident loop (res_admm_w, kernels_resident.inc)
            d.ldw = (n + M + 7) & ~7;
            double *Wd = nullptr;
            rc = dalloc(e, &Wd, (size_t)(n + M) * d.ldw + 64);
            if (!rc) rc = miosqp_device_kkt_inverse(d.f_rows, d.ldf, d.d2inv, n, M, Wd, d.ldw, e->stream);
            double *Kc = nullptr;  // dense [0 Abar ; Abar^T Pbar]: the rows of the termination test in the same form
            if (!rc) rc = dalloc(e, &Kc, (size_t)(n + M) * d.ldw + 64);
            if (rc) { miosqp_qp_cleanup(e); return rc; }
            d.W = Wd;
            d.Kc = Kc;
            hipLaunchKernelGGL(k_build_kc, dim3((n + M + 255) / 256, n + M), dim3(256), 0, e->stream, d, Kc);
            // the explicit inverse is checked before it is used (kernels_guard.inc); when it fails the workgroup keeps
            // the product-form sweeps in LDS, if they fit
            rc = inverse_guard(e);
            if (rc) { miosqp_qp_cleanup(e); return rc; }
            if (e->guard_tripped) {
              d.W = nullptr;
              d.Kc = nullptr;
              e->res_sp_off = -1;
              const size_t need2 = resident_lds_doubles(n, M, false) * sizeof(double);
              if (need2 <= 160 * 1024) e->res_lds = need2;
              else e->resident = false;
            }
          }
          if (e->resident) {
            HIPCHK(lds_limit_once((const void *)k_resident, 0));
            resident_lane_groups(e);
          }
        }
      }
      {
        // cooperative register-resident solver: the explicit KKT inverse spread over the register
        // files of up to one workgroup per CU
        const int N = n + M;
        int wantc = coop_pref ? 1 : 0;
        int dev_now = 0;
        HIPCHK(hipGetDevice(&dev_now));
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, dev_now));
        int rw = coop_pick_rw(N);  // rows of W per workgroup
        if (const char *ev = getenv("MIOSQP_COOP_DBG")) d.coop_dbg = atoi(ev);
        const int T = (N + rw - 1) / rw;
        bool can = !e->resident && N <= 2048 && T <= prop.multiProcessorCount;
        e->coop_cus = prop.multiProcessorCount;
        if (wantc && can) {
          // the grid must fit the device with one workgroup per CU: ask the runtime instead of assuming it
          if (coop_occupancy(rw, coop_pick_cpt(N), N < 1024 ? 2 : 4) < 1) can = false;
        }
        if (wantc && can) {
          e->coop = true;
          e->coop_capable = true;
          e->coop_rw = rw;
          e->coop_cpt = coop_pick_cpt(N);
          e->coop_cptf = N < 1024 ? 2 : 4;
          e->coop_T = T;
          d.coop_mg = M;
          d.ldw = (N + 7) & ~7;
          double *Wd = nullptr;
          rc = dalloc(e, &Wd, (size_t)N * d.ldw + 64);
          if (!rc) rc = dalloc(e, &d.coop_tag, 64);
          d.coop_stride = 2 * rw;
          d.coop_half = 2 * (size_t)((N + 1 + 15) & ~15);  // two words per entry (one more than rows: the testers' decision), room for either row-block size
          if (!rc) rc = dalloc(e, &d.coop_buf, 4 * COOP_RING_WORDS + 64);
          if (!rc) hipLaunchKernelGGL(k_coop_ring_fill, dim3(16), dim3(256), 0, e->stream, d.coop_buf);
          if (!rc) rc = dalloc(e, &d.coop_chk, 2 * d.coop_half + 64);
          if (!rc) rc = dalloc(e, &d.coop_q, (size_t)(256 + 16) * COOP_QS + 64);
          if (!rc) rc = dalloc(e, &d.coop_reg, 128);
          if (!rc) rc = dalloc(e, &d.coop_chz, d.coop_half + 64);
          if (!rc) rc = dalloc(e, &d.coop_dec, 64);
          if (!rc) rc = dalloc(e, &e->coop_epi, 2 * (size_t)COOP_EPI_ENTRIES + 64);
          {
            // the test on workgroups of its own when the exchange grid leaves enough CUs free
            d.coop_nt = coop_decision_slot(N, e->coop_cpt) ? coop_pick_testers(prop.multiProcessorCount - T) : 0;
            coop_pick_lag(e);
          }
          double *Kc = nullptr;
          if (!rc) rc = dalloc(e, &Kc, (size_t)N * d.ldw + 64);
          const bool timing = getenv("MIOSQP_SETUP_TIMING") != nullptr;
          if (timing) HIPCHK(hipStreamSynchronize(e->stream));
          const double tk0 = wall();
          if (!rc) rc = miosqp_device_kkt_inverse(d.f_rows, d.ldf, d.d2inv, n, M, Wd, d.ldw, e->stream);
          if (rc) { miosqp_qp_cleanup(e); return rc; }
          if (timing) {
            HIPCHK(hipStreamSynchronize(e->stream));
            fprintf(stderr, "[miosqp setup] %-32s %8.1f ms\n", "explicit KKT inverse (device)", 1e3 * (wall() - tk0));
          }
          d.W = Wd;
          d.Kc = Kc;
          d.coop_W = Wd;
          d.coop_ldw = d.ldw;
          hipLaunchKernelGGL(k_build_kc, dim3((N + 255) / 256, N), dim3(256), 0, e->stream, d, Kc);
          // the explicit inverse is checked before it is used (kernels_guard.inc); when it fails this engine iterates
          // with the sweeps of the product form (two launches per iteration) instead
          rc = inverse_guard(e);
          if (rc) { miosqp_qp_cleanup(e); return rc; }
          if (e->guard_tripped) {
            e->coop = false;
            e->coop_capable = false;
            d.W = nullptr;
            d.Kc = nullptr;
          }
        }
      }
      tuning_from_env(e);
      std::vector<double>().swap(e->fo.rows);
      std::vector<double>().swap(e->fo.GmT);
      std::vector<double>().swap(e->fo.Ad);
      std::vector<double>().swap(e->fo.Atd);
      std::vector<double>().swap(e->fo.Pd);
    }
  }
  {
    // persistent streaming solver (kernels_pers.inc): for what the cooperative solver cannot hold, or on request
    int want = s->pers;
    if (const char *ev = getenv("MIOSQP_PERS")) want = atoi(ev);
    // (auto, factor form: with the tail as S^-1 -- 42.8 us per iteration at config 5 against 48.7 with the two triangular
    //  sweeps and 50.7 with four launches; pers = 1 keeps the sweeps)
    if (want < 0) want = (!e->resident && !e->coop && n + M > 2048) ? (e->fold ? 1 : 2) : 0;
    if (want && !e->resident && !e->coop && M > 0) {
      e->st.pers = want;  // (2: with the tail as the explicit inverse of the reduced Hessian, see pers_setup)
      int rc = pers_setup(e);
      if (rc) { miosqp_qp_cleanup(e); return rc; }
    }
  }
  tick("product form, resident / cooperative / persistent set-up");
  e->chunk = e->st.check_termination;
  e->tail_iters = e->st.max_iter % e->chunk;
  HIPCHK(hipStreamSynchronize(e->stream));
  if (!e->resident && !e->coop && !e->pers) {  // the single-launch solvers need no captured chunk
    int rc = capture_chunk(e, e->chunk, &e->g_full, &e->x_full);
    if (!rc && e->tail_iters > 0) rc = capture_chunk(e, e->tail_iters, &e->g_tail, &e->x_tail);
    if (rc) { miosqp_qp_cleanup(e); return rc; }
  }
  if (e->coop_capable || e->pers_capable) {  // whole-chip launches of one process take turns (host.inc: ChipTurn)
    int rc = chip_join(e);
    if (rc) { miosqp_qp_cleanup(e); return rc; }
  }
  if (e->coop) {
    int rc = calibrate_coop_nap(e);
    if (rc) { miosqp_qp_cleanup(e); return rc; }
  }
  tick("graph capture / calibration");
  if (t_on) fprintf(stderr, "[miosqp setup] %-32s %8.3f ms\n", "miosqp_qp_setup, all of it", 1e3 * (wall() - t_begin));
  *out = e;
  return 0;
}

// The update / warm-start calls return as soon as their work is queued (the solve that follows is ordered behind it
// on the engine's stream); what must not happen is the NEXT upload overwriting the pinned staging area while the
// previous copy out of it is still under way: one event per staging region, waited for before the region is rewritten.
static int stage_wait(miosqp_qp_engine *e, int k) {
  if (e->stage_busy[k]) {
    HIPCHK(hipEventSynchronize(e->rt.ev_stage[k]));
    e->stage_busy[k] = false;
  }
  return 0;
}
static int stage_mark(miosqp_qp_engine *e, int k) {
  HIPCHK(hipEventRecord(e->rt.ev_stage[k], e->stream));
  e->stage_busy[k] = true;
  return 0;
}

int miosqp_qp_update_bounds(miosqp_qp_engine *e, const double *l, const double *u) {
  if (!e || !l || !u) return MIOSQP_EARG;
  ENTER(e);
  for (int i = 0; i < e->M; i++)
    if (l[i] > u[i]) return MIOSQP_EBOUNDS;
  if (int rc = stage_wait(e, 0)) return rc;
  memcpy(e->h_in, l, sizeof(double) * e->M);
  memcpy(e->h_in + e->M, u, sizeof(double) * e->M);
  HIPCHK(hipMemcpyAsync(e->d.raw_l, e->h_in, sizeof(double) * 2 * e->M, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_scale_bounds, dim3((e->M + 255) / 256), dim3(256), 0, e->stream, e->d);
  return stage_mark(e, 0);
}

int miosqp_qp_update_lin_cost(miosqp_qp_engine *e, const double *q) {
  if (!e || !q) return MIOSQP_EARG;
  ENTER(e);
  if (int rc = stage_wait(e, 1)) return rc;
  double *hx = e->h_in + 2 * (size_t)e->M;
  memcpy(hx, q, sizeof(double) * e->n);
  HIPCHK(hipMemcpyAsync(e->d.raw_x, hx, sizeof(double) * e->n, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_scale_q, dim3((e->n + 255) / 256), dim3(256), 0, e->stream, e->d);
  return stage_mark(e, 1);
}

static int enqueue_warm(miosqp_qp_engine *e) {
  const int big = e->n > e->M ? e->n : e->M;
  hipLaunchKernelGGL(k_scale_warm, dim3((big + 255) / 256), dim3(256), 0, e->stream, e->d);
  DISPATCH_TPR(e->tpr_pc, k_warm_z, e->M, e->stream, e->d);
  return 0;
}

int miosqp_qp_warm_start(miosqp_qp_engine *e, const double *x, const double *y) {
  if (!e || !x || !y) return MIOSQP_EARG;
  ENTER(e);
  if (int rc = stage_wait(e, 1)) return rc;
  double *hx = e->h_in + 2 * (size_t)e->M;
  memcpy(hx, x, sizeof(double) * e->n);
  memcpy(hx + e->n, y, sizeof(double) * e->M);
  HIPCHK(hipMemcpyAsync(e->d.raw_x, hx, sizeof(double) * (e->n + e->M), hipMemcpyHostToDevice, e->stream));
  enqueue_warm(e);
  return stage_mark(e, 1);
}

static int begin_solve(miosqp_qp_engine *e) {
  const int big = e->n > e->M ? e->n : e->M;
  HIPCHK(hipEventRecord(e->ev0, e->stream));
  if (!e->st.warm_start) hipLaunchKernelGGL(k_zero_iterates, dim3((big + 255) / 256), dim3(256), 0, e->stream, e->d);
  hipLaunchKernelGGL(k_reset_ctrl, dim3(1), dim3(1), 0, e->stream, e->d);
  hipLaunchKernelGGL(k_init_wh, dim3(((e->M > e->n ? e->M : e->n) + 255) / 256), dim3(256), 0, e->stream, e->d);
  return 0;
}

int miosqp_qp_solve(miosqp_qp_engine *e, double *x_out, double *y_out, miosqp_qp_info *info) {
  if (!e || !x_out || !y_out || !info) return MIOSQP_EARG;
  ENTER(e);
  const double t0 = wall();
  maybe_rejoin_coop(e);
  for (;;) {
    int rc = begin_solve(e);
    if (!rc) rc = run_loop(e);
    if (!rc) rc = finish_and_fetch(e, 0, x_out, y_out, info, t0);
    if (rc != COOP_RETRY) return rc;
    // called off before any iterate was touched: the same solve again in the two-kernel form
    rc = leave_coop(e);
    if (rc) return rc;
  }
}

int miosqp_qp_set_integer_rows(miosqp_qp_engine *e, int32_t n_int, const int32_t *i_idx, int32_t m_orig) {
  if (!e || n_int < 0 || n_int > e->n || m_orig < 0 || m_orig + n_int != e->M || (n_int && !i_idx)) {
    g_err = "set_integer_rows: need m_orig + n_int == M";
    return MIOSQP_EARG;
  }
  ENTER(e);
  for (int k = 0; k < n_int; k++)
    if (i_idx[k] < 0 || i_idx[k] >= e->n) return MIOSQP_EARG;
  e->h_iidx.assign(i_idx, i_idx + n_int);  // host copy (the streaming driver rounds an incumbent's integer entries)
  // uploads through region 1 of the pinned staging block when they fit (three blocking copies were ~30 us of a small set-up):
  // [ i_idx (n_int ints) | int_pos (n ints) | a_int (n doubles, below) ]
  const size_t stage_doubles = e->rt.in_cap > 2 * (size_t)e->M ? e->rt.in_cap - 2 * (size_t)e->M : 0;
  const size_t ints_doubles = ((size_t)n_int + (size_t)e->n + 1) / 2;
  const bool staged = stage_doubles >= ints_doubles + (size_t)e->n;
  double *const stage = e->h_in + 2 * (size_t)e->M;
  if (staged) {
    if (int rcw = stage_wait(e, 1)) return rcw;
  }
  {
    std::vector<int> pos(e->n, -1);
    for (int k = 0; k < n_int; k++) pos[i_idx[k]] = k;
    if (!e->d.int_pos) {
      int *ip = nullptr;
      int rc = dalloc(e, &ip, (size_t)e->n);
      if (rc) return rc;
      e->d.int_pos = ip;
    }
    if (staged) {
      int *hi = reinterpret_cast<int *>(stage);
      memcpy(hi, i_idx, sizeof(int) * n_int);
      memcpy(hi + n_int, pos.data(), sizeof(int) * e->n);
      if (n_int) HIPCHK(hipMemcpyAsync((void *)e->d.i_idx, hi, sizeof(int) * n_int, hipMemcpyHostToDevice, e->stream));
      HIPCHK(hipMemcpyAsync((void *)e->d.int_pos, hi + n_int, sizeof(int) * e->n, hipMemcpyHostToDevice, e->stream));
    } else {
      if (n_int) HIPCHK(hipMemcpy((void *)e->d.i_idx, i_idx, sizeof(int) * n_int, hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy((void *)e->d.int_pos, pos.data(), sizeof(int) * e->n, hipMemcpyHostToDevice));
    }
  }
  e->d.n_int = n_int;
  e->d.m_orig = m_orig;
  e->have_int = true;
  // Identity rows (kernels_batched.inc): when every bound row has exactly one entry, at its variable's column, and
  // no variable has two, the matrix-core sweeps leave those rows out.  Decided once, before the batched arrays exist.
  if (e->fold && e->bd_cfg == 0 && n_int > 0 && e->Bcap == 0 && !getenv("MIOSQP_NO_IDROWS")) {
    const miosqp::PCsr &C = e->fa.panel_by_con;
    std::vector<double> aint(e->n, 0.0);
    bool ok = true;
    for (int k = 0; k < n_int && ok; k++) {
      const int j = m_orig + k;
      int cnt = 0, col = -1;
      double val = 0.0;
      for (int t = C.ptr[j]; t < C.ptr[j + 1]; t++)
        if (e->fa.A_val[t] != 0.0) { cnt++; col = C.idx[t]; val = e->fa.A_val[t]; }
      ok = cnt == 1 && col == i_idx[k] && aint[col] == 0.0;
      if (ok) aint[col] = e->st.rho * val;
    }
    if (ok) {
      const int n = e->n, m = m_orig;
      const int ld2 = (m + n + 15) & ~15;
      double *f2 = nullptr, *ai = nullptr;
      int rc = dalloc(e, &f2, (size_t)n * ld2 + 64);
      if (!rc) rc = dalloc(e, &ai, (size_t)n);
      if (rc) return rc;
      if (staged) {
        memcpy(stage + ints_doubles, aint.data(), sizeof(double) * n);
        HIPCHK(hipMemcpyAsync(ai, stage + ints_doubles, sizeof(double) * n, hipMemcpyHostToDevice, e->stream));
      } else {
        HIPCHK(hipMemcpy(ai, aint.data(), sizeof(double) * n, hipMemcpyHostToDevice));
      }
      hipLaunchKernelGGL(k_drop_bound_columns, dim3((ld2 + 255) / 256, n), dim3(256), 0, e->stream, e->d.f_rows, e->d.ldf,
                         f2, ld2, m, n_int, n);
      // (no wait: every reader of f2 is a later kernel on this stream)
      e->d.f_rows2 = f2;
      e->d.ldf2 = ld2;
      e->d.a_int = ai;
      e->d.wh_m = m;
    }
  }
  // the captured graphs hold Dev by value but never read n_int / m_orig / i_idx contents
  if (staged) {
    if (int rcm = stage_mark(e, 1)) return rcm;
  }
  return coop_drop_identity_rows(e, n_int, i_idx, m_orig);
}

int miosqp_qp_set_root(miosqp_qp_engine *e, const double *l_root, const double *u_root, double eps_int_feas,
                       double eps_lin) {
  if (!e || !l_root || !u_root || !e->have_int) {
    g_err = "set_root: call miosqp_qp_set_integer_rows first";
    return MIOSQP_EARG;
  }
  ENTER(e);
  if (e->M > 0) {
    // through the pinned staging block, on the engine's stream, no wait: whatever reads the root bounds is queued
    // behind these copies (two blocking copies from pageable memory and two stream synchronisations were 40 us of an
    // MPC step's 90)
    if (int rcw = stage_wait(e, 0)) return rcw;
    memcpy(e->h_in, l_root, sizeof(double) * e->M);
    memcpy(e->h_in + e->M, u_root, sizeof(double) * e->M);
    HIPCHK(hipMemcpyAsync(e->d.root_l, e->h_in, sizeof(double) * e->M, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->d.root_u, e->h_in + e->M, sizeof(double) * e->M, hipMemcpyHostToDevice, e->stream));
    if (int rcm = stage_mark(e, 0)) return rcm;
  }
  if ((e->x_stream || e->x_stream_a) && (e->d.eps_int != eps_int_feas || e->d.eps_lin != eps_lin)) drop_stream_graph(e);  // captured by value
  e->d.eps_int = eps_int_feas;
  e->d.eps_lin = eps_lin;
  e->d.digest = 1;
  e->dh.eps_int = eps_int_feas;  // the pool's harvest tile carries its own copy
  e->dh.eps_lin = eps_lin;
  e->dh.digest = 1;
  return 0;
}

int miosqp_qp_solve_node(miosqp_qp_engine *e, const double *l, const double *u, const double *x0,
                         const double *y0, double *x_out, double *y_out, miosqp_qp_info *info) {
  if (!e || !l || !u || !x0 || !y0 || !x_out || !y_out || !info) return MIOSQP_EARG;
  ENTER(e);
  if (!e->have_int) {
    g_err = "solve_node: call miosqp_qp_set_integer_rows first";
    return MIOSQP_EARG;
  }
  const double t0 = wall();
  const int n = e->n, M = e->M;
  for (int i = 0; i < M; i++)
    if (l[i] > u[i]) return MIOSQP_EBOUNDS;
  if (int rcw = stage_wait(e, 0)) return rcw;
  if (int rcw = stage_wait(e, 1)) return rcw;
  memcpy(e->h_in, l, sizeof(double) * M);
  memcpy(e->h_in + M, u, sizeof(double) * M);
  memcpy(e->h_in + 2 * (size_t)M, x0, sizeof(double) * n);
  memcpy(e->h_in + 2 * (size_t)M + n, y0, sizeof(double) * M);
  maybe_rejoin_coop(e);
  for (;;) {
    HIPCHK(hipEventRecord(e->ev0, e->stream));
    HIPCHK(hipMemcpyAsync(e->d.raw_l, e->h_in, sizeof(double) * (3 * (size_t)M + n), hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_node_pre, dim3(((M > n ? M : n) + 255) / 256), dim3(256), 0, e->stream, e->d);
    DISPATCH_TPR(e->tpr_pc, k_warm_zw, M, e->stream, e->d);
    int rc = run_loop(e);
    if (!rc) rc = finish_and_fetch(e, 1, x_out, y_out, info, t0);
    if (rc != COOP_RETRY) return rc;
    rc = leave_coop(e);
    if (rc) return rc;
  }
}

int miosqp_qp_solve_batch(miosqp_qp_engine *e, int32_t B, const double *l, const double *u, const double *x0,
                          const double *y0, double *x_out, double *y_out, miosqp_qp_info *info) {
  if (!e || B < 0 || (B > 0 && (!l || !u || !x0 || !y0 || !x_out || !y_out || !info))) return MIOSQP_EARG;
  ENTER(e);
  if (!e->have_int) {
    g_err = "solve_batch: call miosqp_qp_set_integer_rows first";
    return MIOSQP_EARG;
  }
  const size_t n = e->n, M = e->M;
  for (size_t k = 0; k < (size_t)B * M; k++)
    if (l[k] > u[k]) return MIOSQP_EBOUNDS;
  if (int rc = ensure_batch(e)) return rc;
  for (int s0 = 0; s0 < B; s0 += e->Bcap) {
    const int nb = B - s0 < e->Bcap ? B - s0 : e->Bcap;
    int rc = solve_slice(e, nb, l + s0 * M, u + s0 * M, x0 + s0 * n, y0 + s0 * M, x_out + s0 * n, y_out + s0 * M,
                         info + s0);
    if (rc) return rc;
  }
  return 0;
}

// One MIQP per column: the lock-step solve of solve_batch with a linear cost of its own in every column (B x n raw costs,
// instance-major).  The engine's own q is neither read nor written.
int miosqp_qp_solve_batch_q(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u,
                            const double *x0, const double *y0, double *x_out, double *y_out, miosqp_qp_info *info) {
  if (!e || B < 0 || (B > 0 && (!q || !l || !u || !x0 || !y0 || !x_out || !y_out || !info))) return MIOSQP_EARG;
  ENTER(e);
  if (!e->have_int) {
    g_err = "solve_batch_q: call miosqp_qp_set_integer_rows first";
    return MIOSQP_EARG;
  }
  const size_t n = e->n, M = e->M;
  for (size_t k = 0; k < (size_t)B * M; k++)
    if (l[k] > u[k]) return MIOSQP_EBOUNDS;
  if (int rc = ensure_batch(e)) return rc;
  if (int rc = ensure_batch_q(e)) return rc;
  PqScope scope(e);  // (host_lockstep.inc)
  for (int s0 = 0; s0 < B; s0 += e->Bcap) {
    const int nb = B - s0 < e->Bcap ? B - s0 : e->Bcap;
    int rc = solve_slice(e, nb, l + s0 * M, u + s0 * M, x0 + s0 * n, y0 + s0 * M, x_out + s0 * n, y_out + s0 * M,
                         info + s0, q + s0 * n);
    if (rc) return rc;
  }
  return 0;
}

int miosqp_qp_strong_branch(miosqp_qp_engine *e, const double *l, const double *u, const double *x, const double *y,
                            double parent_lower, int32_t K, const int32_t *cand, int32_t max_iter, double eps,
                            double *lower_out, int32_t *status_out, int32_t *iter_out, double *score_out,
                            miosqp_sb_info *info) {
  if (!e || !l || !u || !x || !y || !cand || !lower_out || !status_out || !iter_out || !score_out || !info)
    return MIOSQP_EARG;
  ENTER(e);
  if (!e->have_int) {
    g_err = "strong_branch: call miosqp_qp_set_integer_rows first";
    return MIOSQP_EARG;
  }
  if (K < 1 || K > SB_MAX_K) {
    g_err = "strong_branch: K must be in 1..32";
    return MIOSQP_EARG;
  }
  if (max_iter <= 0 || max_iter % e->chunk != 0) {
    g_err = "strong_branch: max_iter must be a positive multiple of check_termination";
    return MIOSQP_EARG;
  }
  const int n_int = (int)e->h_iidx.size();
  for (int k = 0; k < K; k++)
    if (cand[k] < 0 || cand[k] >= n_int || (k > 0 && cand[k] <= cand[k - 1])) {
      g_err = "strong_branch: candidates must be ascending positions in 0..n_int-1";
      return MIOSQP_EARG;
    }
  const size_t n = e->n, M = e->M, m_orig = (size_t)e->d.m_orig;
  // a child whose new bound crosses the other one (Workspace.add_left / add_right refuse it too)
  for (int k = 0; k < K; k++) {
    const double v = x[e->h_iidx[cand[k]]];
    if (std::floor(v) < l[m_orig + cand[k]] || std::ceil(v) > u[m_orig + cand[k]]) return MIOSQP_EBOUNDS;
  }
  const int B = 2 * K;
  double t0;
  if (int rc = derived_begin(e, B, l, u, x, y, cand, sizeof(int32_t) * K, &t0)) return rc;
  const Dev &d = e->d;
  const int big = (int)(n > M ? n : M);
  hipLaunchKernelGGL(k_sb_children, dim3((big + 255) / 256, B), dim3(256), 0, e->stream, d, e->der_in,
                     (const int *)(e->der_in + 3 * M + n), K);
  if (int rc = slice_run(e, B, max_iter)) return rc;
  hipLaunchKernelGGL(k_sb_score, dim3(1), dim3(64), 0, e->stream, d, (SbRec *)e->der_rec, K, parent_lower, eps);
  if (int rc = derived_end(e, (sizeof(SbRec) + 7) / 8, &info->device_time)) return rc;
  const SbRec &r = *(const SbRec *)e->h_der;
  int64_t iters = 0;
  for (int b = 0; b < B; b++) {
    lower_out[b] = r.lower[b];
    status_out[b] = r.status[b];
    iter_out[b] = r.iter[b];
    iters += r.iter[b];
  }
  for (int k = 0; k < K; k++) score_out[k] = r.score[k];
  info->chosen = r.chosen;
  info->children = B;
  info->iters = (int32_t)iters;
  info->run_time = wall() - t0;
  return 0;
}

int miosqp_qp_round_and_fix(miosqp_qp_engine *e, const double *l, const double *u, const double *x, const double *y,
                            double upper, int32_t K, int32_t max_iter, double *x_out, int32_t *status_out,
                            int32_t *iter_out, double *obj_out, double *viol_out, miosqp_rf_info *info) {
  if (!e || !l || !u || !x || !y || !x_out || !status_out || !iter_out || !obj_out || !viol_out || !info)
    return MIOSQP_EARG;
  ENTER(e);
  if (!e->have_int || !e->d.digest) {
    g_err = "round_and_fix: call miosqp_qp_set_integer_rows and miosqp_qp_set_root first";
    return MIOSQP_EARG;
  }
  if (K < 1 || K > RF_MAX_K) {
    g_err = "round_and_fix: K must be in 1..32";
    return MIOSQP_EARG;
  }
  if (max_iter <= 0 || (max_iter % e->chunk != 0 && max_iter != e->st.max_iter)) {
    g_err = "round_and_fix: max_iter must be a positive multiple of check_termination or the engine's max_iter";
    return MIOSQP_EARG;
  }
  const size_t n = e->n, M = e->M;
  const int B = K;
  double t0;
  if (int rc = derived_begin(e, B, l, u, x, y, nullptr, 0, &t0)) return rc;
  const Dev &d = e->d;
  const int big = (int)(n > M ? n : M);
  hipLaunchKernelGGL(k_rf_candidates, dim3((big + 255) / 256, B), dim3(256), 0, e->stream, d, e->der_in, K);
  if (int rc = slice_run(e, B, max_iter)) return rc;
  RfRec *drec = (RfRec *)e->der_rec;
  hipLaunchKernelGGL(k_rf_pick, dim3(1), dim3(64), 0, e->stream, d, drec, K, upper);
  hipLaunchKernelGGL(k_rf_gather, dim3(((int)n + 255) / 256), dim3(256), 0, e->stream, d, drec,
                     e->der_rec + RF_REC_DOUBLES);
  if (int rc = derived_end(e, RF_REC_DOUBLES + n, &info->device_time)) return rc;
  const RfRec &r = *(const RfRec *)e->h_der;
  int64_t iters = 0;
  for (int k = 0; k < K; k++) {
    status_out[k] = r.status[k];
    iter_out[k] = r.iter[k];
    obj_out[k] = r.obj[k];
    viol_out[k] = r.viol[k];
    iters += r.iter[k];
  }
  if (r.chosen >= 0) memcpy(x_out, e->h_der + RF_REC_DOUBLES, sizeof(double) * n);
  info->chosen = r.chosen;
  info->feasible = r.feasible;
  info->candidates = K;
  info->iters = (int32_t)iters;
  info->run_time = wall() - t0;
  return 0;
}

int miosqp_qp_polish(miosqp_qp_engine *e, const double *l, const double *u, const double *x, const double *y,
                     double delta, int32_t refine_iter, double *x_out, double *y_out, miosqp_polish_info *info) {
  if (!e || !l || !u || !x || !y || !x_out || !y_out || !info) return MIOSQP_EARG;
  double t0 = 0.0;
  if (int rc = polish_begin(e, l, u, x, y, delta, refine_iter, 0, &t0)) return rc;
  const size_t n = e->n, M = e->M;
  PolishScratch *s = e->pol;
  double *h = s->h;
  hipStream_t st = e->stream;
  if (int rc = polish_queue_round0(e, refine_iter)) return rc;
  HIPCHK(hipMemcpyAsync(h, s->p.rec, sizeof(double) * (POL_REC_DOUBLES + n + M), hipMemcpyDeviceToHost, st));
  HIPCHK(hipEventRecord(s->ev[5], st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  float ms = 0;
  for (int k = 0; k < 4; k++) {
    HIPCHK(hipEventElapsedTime(&ms, s->ev[k], s->ev[k + 1]));
    s->stage_s[k] = 1e-3 * ms;
  }
  HIPCHK(hipEventElapsedTime(&ms, s->ev[0], s->ev[5]));
  polish_fill_info(*(const PolRec *)h, info);
  memcpy(x_out, h + POL_REC_DOUBLES, sizeof(double) * n);
  memcpy(y_out, h + POL_REC_DOUBLES + n, sizeof(double) * M);
  info->device_time = 1e-3 * ms;
  info->run_time = wall() - t0;
  return 0;
}

int miosqp_qp_polish_repair(miosqp_qp_engine *e, const double *l, const double *u, const double *x, const double *y,
                            double delta, int32_t refine_iter, int32_t repair_iter, double *x_out, double *y_out,
                            miosqp_polish_repair_info *info) {
  if (!e || !l || !u || !x || !y || !x_out || !y_out || !info) return MIOSQP_EARG;
  double t0 = 0.0;
  if (int rc = polish_begin(e, l, u, x, y, delta, refine_iter, repair_iter, &t0)) return rc;
  const size_t n = e->n, M = e->M;
  PolishScratch *s = e->pol;
  Pol p = s->p;
  double *h = s->h;
  hipStream_t st = e->stream;
  const dim3 gM((unsigned)((M + 3) / 4)), b256(256);
  const size_t nrec = POL_REC_DOUBLES + n + M;
  if (int rc = polish_queue_round0(e, refine_iter)) return rc;
  // set k: the set round k solved on (0: guessed from (x, y)); one host decision per round, on the revision's counters
  int nl[POL_MAX_ROUNDS + 1] = {0}, nu[POL_MAX_ROUNDS + 1] = {0};
  int k = 0, judged = 0, stop = 0, added = 0, dropped = 0;
  for (;;) {
    p.cls = s->cls_buf[k & 1];
    p.cls_next = s->cls_buf[(k + 1) & 1];
    HIPCHK(hipMemsetAsync(p.cnt + 4, 0, 4 * sizeof(int), st));
    if (M) hipLaunchKernelGGL(k_pol_revise, gM, b256, 0, st, p);
    HIPCHK(hipMemcpyAsync(s->hcnt, p.cnt, 8 * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(s->evr[k], st));
    const double tw = wall();
    HIPCHK(hipEventSynchronize(s->evr[k]));
    s->wait_s[k] = wall() - tw;
    const int *c = s->hcnt;
    if (k == 0) {
      nl[0] = c[0];
      nu[0] = c[1];
      if (c[2]) break;  // round 0's own factorisation broke: reason 1, nothing to repair
    } else if (c[2]) {
      stop = 2;  // the point and the set of the round before are judged
      break;
    }
    judged = k;
    added += c[4];
    dropped += c[5];
    nl[k + 1] = c[6];
    nu[k + 1] = c[7];
    if (c[4] + c[5] == 0) break;
    if (k == repair_iter) {
      stop = 1;
      break;
    }
    // round k + 1 on the revised set (k_pol_revise left it in w, b): this round's point is kept, then the same solves
    // from xh = yh = 0 (the factorisation clears its own flag)
    HIPCHK(hipMemcpyAsync(s->xk, p.xh, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
    if (M) HIPCHK(hipMemcpyAsync(s->yk, p.yh, sizeof(double) * M, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemsetAsync(p.xh, 0, sizeof(double) * n, st));
    if (M) HIPCHK(hipMemsetAsync(p.yh, 0, sizeof(double) * M, st));
    if (int rc = polish_queue_solve(e, p, refine_iter, nullptr, nullptr)) return rc;
    k++;
  }
  const int rounds = k;
  if (rounds > 0) {
    // the final point gets a record of its own behind round 0's
    if (stop == 2) {
      HIPCHK(hipMemcpyAsync(p.xh, s->xk, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
      if (M) HIPCHK(hipMemcpyAsync(p.yh, s->yk, sizeof(double) * M, hipMemcpyDeviceToDevice, st));
      HIPCHK(hipMemsetAsync(p.cnt + 2, 0, sizeof(int), st));
    }
    p.rec = s->rec2;
    polish_queue_decide(e, p);
    HIPCHK(hipMemcpyAsync(h + nrec, s->p.rec, sizeof(PolRec), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipMemcpyAsync(h, p.rec, sizeof(double) * nrec, hipMemcpyDeviceToHost, st));
  if (M) HIPCHK(hipMemcpyAsync(s->hcls, s->cls_buf[judged & 1], M, hipMemcpyDeviceToHost, st));
  HIPCHK(hipEventRecord(s->ev[5], st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  float ms = 0;
  for (int j = 0; j < 4; j++) {
    HIPCHK(hipEventElapsedTime(&ms, s->ev[j], s->ev[j + 1]));
    s->stage_s[j] = 1e-3 * ms;
  }
  for (int j = 0; j <= rounds; j++) {
    HIPCHK(hipEventElapsedTime(&ms, j ? s->evr[j - 1] : s->ev[0], s->evr[j]));
    s->round_s[j] = 1e-3 * ms;
  }
  s->rounds_run = rounds + 1;
  HIPCHK(hipEventElapsedTime(&ms, s->ev[0], s->ev[5]));
  const PolRec &r = *(const PolRec *)h, &r0 = rounds > 0 ? *(const PolRec *)(h + nrec) : r;
  polish_fill_info(r, &info->polish);
  info->polish.n_lower = nl[judged];
  info->polish.n_upper = nu[judged];
  memcpy(x_out, h + POL_REC_DOUBLES, sizeof(double) * n);
  memcpy(y_out, h + POL_REC_DOUBLES + n, sizeof(double) * M);
  info->polish.device_time = 1e-3 * ms;
  info->rounds = rounds;
  info->stop = stop;
  info->n_added = added;
  info->n_dropped = dropped;
  info->accepted0 = r0.accepted;
  info->reason0 = r0.reason;
  info->polish.run_time = wall() - t0;
  return 0;
}

int miosqp_qp_get_polish_repair_trace(miosqp_qp_engine *e, int8_t *cls, double *round_seconds, double *wait_seconds) {
  if (!e) return MIOSQP_EARG;
  const PolishScratch *s = e->pol;
  const int run = s ? s->rounds_run : 0;
  if (cls)
    for (int j = 0; j < e->M; j++) cls[j] = run ? s->hcls[j] : 0;
  for (int k = 0; k < POL_MAX_ROUNDS; k++) {
    if (round_seconds) round_seconds[k] = k < run ? s->round_s[k] : 0.0;
    if (wait_seconds) wait_seconds[k] = k < run ? s->wait_s[k] : 0.0;
  }
  return 0;
}

#include "host_polish_models.inc"  // polishes of different models in one launch (C ABI miosqp_qp_polish_models)
#include "host_polish_models_large.inc"  // ... beyond one workgroup's LDS (C ABI miosqp_qp_polish_models_large)

// Both batched polish entries: the argument checks, one pinned block down, the one launch -- k_pol_many, or with `large`
// k_pol_many_g on W slabs of device scratch --, one pinned block back, the records.  The answers stay in the entry's
// scratch for its class getter.
static int polish_many_run(miosqp_qp_engine *e, bool large, int32_t B, const double *q, const double *l, const double *u,
                           const double *x, const double *y, double delta, int32_t refine_iter, int32_t repair_iter,
                           double *x_out, double *y_out, miosqp_polish_repair_info *info) {
  if (!e || !l || !u || !x || !y || !x_out || !y_out || !info) return MIOSQP_EARG;
  ENTER(e);
  if (B < 1) {
    g_err = "polish_many: B must be at least 1";
    return MIOSQP_EARG;
  }
  if (!(delta > 0.0) || !(delta < QP_INFTY)) {
    g_err = "polish_many: delta must be positive";
    return MIOSQP_EARG;
  }
  if (refine_iter < 0 || refine_iter > 10) {
    g_err = "polish_many: refine_iter must be in 0..10";
    return MIOSQP_EARG;
  }
  if (repair_iter < 0 || repair_iter >= POL_MAX_ROUNDS) {
    g_err = "polish_many: repair_iter must be in 0..20";
    return MIOSQP_EARG;
  }
  const size_t n = e->n, M = e->M, nB = (size_t)B;
  for (size_t j = 0; j < nB * M; j++) {
    if (l[j] > u[j]) return MIOSQP_EBOUNDS;
    if (l[j] != l[j] || u[j] != u[j] || y[j] != y[j]) {
      g_err = "polish_many: NaN in l, u or y (a node without a solution cannot be polished)";
      return MIOSQP_EARG;
    }
  }
  for (size_t i = 0; i < nB * n; i++)
    if (x[i] != x[i] || (q && q[i] != q[i])) {
      g_err = "polish_many: NaN in x or q";
      return MIOSQP_EARG;
    }
  size_t slab = 0;
  int W = 0;
  if (large) {
    // W = min(B, two workgroups per compute unit, what the slab budget allows); beyond the limits nothing is allocated
    slab = miosqp::polish_many_large_slab_doubles((int)n, (int)M);
    if (slab == (size_t)-1 || slab * sizeof(double) > miosqp::POLG_BUDGET) {
      g_err = "polish_many_large: only for n <= 512 and M <= 65536";
      return MIOSQP_EUNSUPPORTED;
    }
    int cus = 0;
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->device));
    const size_t fit = miosqp::POLG_BUDGET / (slab * sizeof(double));
    W = (int)std::min(std::min(nB, (size_t)2 * (size_t)std::max(cus, 1)), fit);
  } else if (miosqp::polish_many_lds_bytes((int)n, (int)M) > 160 * 1024) {
    g_err = "polish_many: only for problems whose reduced system and rows of A fit one workgroup's 160 KB of LDS";
    return MIOSQP_EUNSUPPORTED;
  }
  if (int rc = polish_ensure(e)) return rc;  // (places the unscaled rows of A on the device; nothing of it is written here)
  const size_t so = miosqp::polm_out_stride((int)n, (int)M);
  const size_t n_in = nB * ((q ? 2 : 1) * n + 3 * M), n_out = nB * so;
  miosqp::PolManyScratch *&slot = large ? e->polml : e->polm;
  if (int rc = polish_many_ensure(e, slot, n_in, n_out, (size_t)W * slab)) return rc;
  const double t0 = wall();
  miosqp::PolManyScratch *s = slot;
  s->last_B = 0;
  // one block down: [q] | l | u | x | y, each instance-major
  double *h = s->h_in;
  const size_t oq = 0, ol = q ? nB * n : 0, ou = ol + nB * M, ox = ou + nB * M, oy = ox + nB * n;
  if (q) memcpy(h + oq, q, sizeof(double) * nB * n);
  memcpy(h + ol, l, sizeof(double) * nB * M);
  memcpy(h + ou, u, sizeof(double) * nB * M);
  memcpy(h + ox, x, sizeof(double) * nB * n);
  memcpy(h + oy, y, sizeof(double) * nB * M);
  const Pol &p = e->pol->p;
  miosqp::PolManyArgs a{};
  a.n = (int)n; a.M = (int)M; a.B = B; a.refine_iter = refine_iter; a.repair_iter = repair_iter;
  a.delta = delta; a.inv_delta = 1.0 / delta;
  a.pc_ptr = p.pc_ptr; a.pc_idx = p.pc_idx; a.pr_ptr = p.pr_ptr; a.pr_idx = p.pr_idx;
  a.A = p.A; a.pr_val = p.pr_val;
  a.q = q ? s->d_in + oq : nullptr;
  a.q_engine = e->d.qraw;
  a.l = s->d_in + ol; a.u = s->d_in + ou; a.x = s->d_in + ox; a.y = s->d_in + oy;
  a.out = s->d_out;
  hipStream_t st = e->stream;
  HIPCHK(hipEventRecord((hipEvent_t)s->ev[0], st));
  HIPCHK(hipMemcpyAsync(s->d_in, h, sizeof(double) * n_in, hipMemcpyHostToDevice, st));
  int lrc;
  if (large) {
    miosqp::PolManyLargeArgs g{};
    g.a = a;
    g.pv_ptr = p.pv_ptr; g.pv_idx = p.pv_idx; g.At = p.At;
    g.slab = s->slab; g.slab_doubles = slab;
    lrc = miosqp::polish_many_large_launch(g, W, (void *)st);
  } else {
    lrc = miosqp::polish_many_launch(a, (void *)st);
  }
  if (lrc) {
    set_err("polish_many: launch", (hipError_t)lrc, __FILE__, __LINE__);
    return MIOSQP_EHIP;
  }
  HIPCHK(hipMemcpyAsync(s->h_out, s->d_out, sizeof(double) * n_out, hipMemcpyDeviceToHost, st));
  HIPCHK(hipEventRecord((hipEvent_t)s->ev[1], st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, (hipEvent_t)s->ev[0], (hipEvent_t)s->ev[1]));
  for (size_t b = 0; b < nB; b++) {
    const double *o = s->h_out + b * so;
    const miosqp::PolManyRec &r = *(const miosqp::PolManyRec *)o;
    miosqp_polish_repair_info &f = info[b];
    f.polish.accepted = r.accepted;
    f.polish.reason = r.reason;
    f.polish.n_lower = r.n_lower;
    f.polish.n_upper = r.n_upper;
    f.polish.pri_before = r.pri_before;
    f.polish.dua_before = r.dua_before;
    f.polish.pri_after = r.pri_after;
    f.polish.dua_after = r.dua_after;
    f.polish.obj = r.obj;
    f.polish.device_time = 1e-3 * ms;
    f.rounds = r.rounds;
    f.stop = r.stop;
    f.n_added = r.n_added;
    f.n_dropped = r.n_dropped;
    f.accepted0 = r.accepted0;
    f.reason0 = r.reason0;
    memcpy(x_out + b * n, o + miosqp::POLM_REC_DOUBLES, sizeof(double) * n);
    memcpy(y_out + b * M, o + miosqp::POLM_REC_DOUBLES + n, sizeof(double) * M);
  }
  s->last_B = B;
  const double rt = wall() - t0;
  for (size_t b = 0; b < nB; b++) info[b].polish.run_time = rt;
  return 0;
}

int miosqp_qp_polish_many(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u,
                          const double *x, const double *y, double delta, int32_t refine_iter, int32_t repair_iter,
                          double *x_out, double *y_out, miosqp_polish_repair_info *info) {
  return polish_many_run(e, false, B, q, l, u, x, y, delta, refine_iter, repair_iter, x_out, y_out, info);
}

int miosqp_qp_polish_many_large(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u,
                                const double *x, const double *y, double delta, int32_t refine_iter, int32_t repair_iter,
                                double *x_out, double *y_out, miosqp_polish_repair_info *info) {
  return polish_many_run(e, true, B, q, l, u, x, y, delta, refine_iter, repair_iter, x_out, y_out, info);
}

static int polish_many_classes(miosqp_qp_engine *e, const miosqp::PolManyScratch *s, int32_t b, int8_t *cls) {
  if (!e || !cls) return MIOSQP_EARG;
  if (!s || b < 0 || b >= s->last_B) {
    g_err = "get_polish_many_classes: no such instance in the last polish_many call";
    return MIOSQP_EARG;
  }
  const size_t n = e->n, M = e->M;
  const double *o = s->h_out + (size_t)b * miosqp::polm_out_stride((int)n, (int)M);
  memcpy(cls, o + miosqp::POLM_REC_DOUBLES + n + M, M);
  return 0;
}

int miosqp_qp_polish_models(int32_t B, miosqp_qp_engine *const *engines, const double *const *q, const double *const *l,
                            const double *const *u, const double *const *x, const double *const *y, double tau,
                            const double *delta, const int32_t *refine_iter, const int32_t *repair_iter, double *const *x_out,
                            double *const *y_out, int8_t *const *cls_out, miosqp_polish_repair_info *info,
                            miosqp_polish_models_stats *stats) {
  return polish_models_run(B, engines, q, l, u, x, y, tau, delta, refine_iter, repair_iter, x_out, y_out, cls_out, info, stats);
}

int miosqp_qp_polish_models_fits(miosqp_qp_engine *e) {
  return e && miosqp::polm_lds_bytes(e->n, e->M) <= miosqp::polish_models::LDS_LIMIT ? 1 : 0;
}

int miosqp_qp_polish_models_large(int32_t B, miosqp_qp_engine *const *engines, const double *const *q, const double *const *l,
                                  const double *const *u, const double *const *x, const double *const *y, double tau,
                                  const double *delta, const int32_t *refine_iter, const int32_t *repair_iter,
                                  double *const *x_out, double *const *y_out, int8_t *const *cls_out,
                                  miosqp_polish_repair_info *info, miosqp_polish_models_large_stats *stats) {
  return polish_models_large_run(B, engines, q, l, u, x, y, tau, delta, refine_iter, repair_iter, x_out, y_out, cls_out, info,
                                 stats);
}

int miosqp_qp_polish_models_large_fits(miosqp_qp_engine *e) {
  return e && miosqp::polish_models_large::fits(e->n, e->M) ? 1 : 0;
}

int miosqp_qp_get_polish_many_classes(miosqp_qp_engine *e, int32_t b, int8_t *cls) {
  return polish_many_classes(e, e ? e->polm : nullptr, b, cls);
}

int miosqp_qp_get_polish_many_large_classes(miosqp_qp_engine *e, int32_t b, int8_t *cls) {
  return polish_many_classes(e, e ? e->polml : nullptr, b, cls);
}

int miosqp_qp_get_polish_stages(miosqp_qp_engine *e, double *seconds) {
  if (!e || !seconds) return MIOSQP_EARG;
  for (int k = 0; k < 4; k++) seconds[k] = e->pol ? e->pol->stage_s[k] : 0.0;
  return 0;
}

int miosqp_qp_solve_tree(miosqp_qp_engine *e, const double *l, const double *u, const double *x0, const double *y0,
                         double upper0, const double *x_inc0, int32_t tree_explor_rule, int32_t max_iter_bb,
                         double *x_out, miosqp_tree_info *info) {
  if (!e || !l || !u || !x0 || !y0 || !x_out || !info || max_iter_bb < 1 || tree_explor_rule < 0 || tree_explor_rule > 3)
    return MIOSQP_EARG;
  ENTER(e);
  if (!e->have_int || !e->d.digest) {
    g_err = "solve_tree: call miosqp_qp_set_integer_rows and miosqp_qp_set_root first";
    return MIOSQP_EARG;
  }
  const int n = e->n, M = e->M, p = e->d.n_int;
  int tree_sp_off = -1;
  const size_t lds = tree_lds_bytes(e, &tree_sp_off);
  if (!e->fold || lds > 160 * 1024 || p < 1) {  // whatever form single nodes use: the product-form rows must exist and fit
    g_err = "solve_tree: only for problems whose product-form factor, iterates and leaf list fit 160 KB of LDS";
    return MIOSQP_EUNSUPPORTED;
  }
  for (int i = 0; i < M; i++)
    if (l[i] > u[i]) return MIOSQP_EBOUNDS;
  const double t0 = wall();
  bool wave = false;  // the one-wavefront kernel (host_models.inc: the lazy build of W / Kc and its guard)
  if (int rcw = tree_wave_prepare(e, &wave)) return rcw;
  if (!e->tree_ready) {
    HIPCHK(lds_limit_once((const void *)k_tree, 1));
    int rc = dalloc(e, &e->ta.lf_lo, (size_t)TREE_CAP * p);
    if (!rc) rc = dalloc(e, &e->ta.lf_hi, (size_t)TREE_CAP * p);
    if (!rc) rc = dalloc(e, &e->ta.lf_x, (size_t)TREE_CAP * n);
    if (!rc) rc = dalloc(e, &e->ta.lf_y, (size_t)TREE_CAP * M);
    if (!rc) rc = dalloc(e, &e->ta.inc_x, (size_t)n);
    if (!rc) rc = dalloc(e, &e->ta.out, 1);
    if (rc) return rc;
    e->tree_ready = true;
  }
  if (int rcw = stage_wait(e, 0)) return rcw;
  if (int rcw = stage_wait(e, 1)) return rcw;
  memcpy(e->h_in, l, sizeof(double) * M);
  memcpy(e->h_in + M, u, sizeof(double) * M);
  memcpy(e->h_in + 2 * (size_t)M, x0, sizeof(double) * n);
  memcpy(e->h_in + 2 * (size_t)M + n, y0, sizeof(double) * M);
  const bool have_inc = x_inc0 != nullptr && upper0 < 1.7e308;
  TreeArgs ta = e->ta;
  ta.rule = tree_explor_rule;
  ta.max_nodes = max_iter_bb;
  ta.max_iter = e->st.max_iter;
  ta.check_every = e->st.check_termination;
  tree_lane_groups(n, M, ta);
  ta.upper0 = have_inc ? upper0 : 1.0 / 0.0;
  ta.done = nullptr;
  ta.sp_off = tree_sp_off;
  const TreeOut *o = nullptr;
  const double *x_found = nullptr;
  float ms = 0;
  if (wave) {
    // The one-wavefront search reads the root straight from the pinned staging block and writes incumbent and
    // outcome into coherent host memory, the completion word last: ONE launch and no copy per MIQP (three copies and
    // two events around a 60-400 us kernel were 25 us).  Device time: the kernel's own 100 MHz stamps.
    if (!e->h_tree) {  // lives in the runtime bundle: a pinned allocation per engine was ~80 us of a 130 us first solve
      if (e->rt.tree_cap < (size_t)n + 16) {
        if (e->rt.h_tree) hipHostFree(e->rt.h_tree);
        e->rt.h_tree = nullptr;
        e->rt.tree_cap = 0;
        const size_t cap = std::max<size_t>(512, (size_t)n + 16);
        HIPCHK(hipHostMalloc((void **)&e->rt.h_tree, sizeof(double) * cap, hipHostMallocCoherent));
        e->rt.tree_cap = cap;
      }
      e->h_tree = e->rt.h_tree;
      memset(e->h_tree, 0, sizeof(double) * ((size_t)n + 16));
    }
    unsigned long long *done = e->h_tree;
    TreeOut *out = reinterpret_cast<TreeOut *>(e->h_tree + 4);
    double *inc = reinterpret_cast<double *>(e->h_tree + 16);
    static_assert(sizeof(TreeOut) <= 12 * sizeof(unsigned long long), "TreeOut fits its place in h_tree");
    __atomic_store_n(&done[0], 0ull, __ATOMIC_RELAXED);
    if (have_inc) memcpy(inc, x_inc0, sizeof(double) * n);
    Dev dp = e->d;
    dp.raw_l = e->h_in;
    dp.raw_u = e->h_in + M;
    dp.raw_x = e->h_in + 2 * (size_t)M;
    dp.raw_y = e->h_in + 2 * (size_t)M + n;
    ta.inc_x = inc;
    ta.out = out;
    ta.done = done;
    static unsigned long long *tree_prof = nullptr;  // debug (MIOSQP_TREE_PROF=1): ticks per phase, summed over launches
    static const bool tree_prof_on = getenv("MIOSQP_TREE_PROF") != nullptr;
    if (tree_prof_on && !tree_prof) {
      HIPCHK(hipMalloc((void **)&tree_prof, 64));
      HIPCHK(hipMemset(tree_prof, 0, 64));
    }
    if (tree_prof_on) dp.prof = tree_prof;
    hipLaunchKernelGGL(k_tree_w, dim3(1), dim3(TW), 0, e->stream, dp, ta);
    if (e->spin_wait) {
      unsigned long long spins = 0;
      while (__atomic_load_n(&done[0], __ATOMIC_ACQUIRE) == 0ull) {
        if ((++spins & 0xfffff) == 0) {
          const hipError_t q = hipStreamQuery(e->stream);
          if (q != hipSuccess && q != hipErrorNotReady) HIPCHK(q);
          if (q == hipSuccess && __atomic_load_n(&done[0], __ATOMIC_ACQUIRE) == 0ull) {
            g_err = "solve_tree: the stream is idle and the outcome never arrived";
            return MIOSQP_EHIP;
          }
        }
      }
    } else {
      HIPCHK(hipStreamSynchronize(e->stream));
    }
    if (tree_prof_on) {
      unsigned long long h[6];
      HIPCHK(hipMemcpy(h, tree_prof, sizeof h, hipMemcpyDeviceToHost));
      fprintf(stderr, "[tree prof] cumulative us: prologue %.1f  iterations %.1f  tests %.1f  epilogue %.1f  branch %.1f\n",
              h[0] / 100.0, h[1] / 100.0, h[2] / 100.0, h[3] / 100.0, h[4] / 100.0);
    }
    o = out;
    x_found = inc;
    ms = (float)(1e-5 * (double)(done[2] - done[1]));  // 100 MHz ticks -> ms
  } else {
    HIPCHK(hipEventRecord(e->ev0, e->stream));
    HIPCHK(hipMemcpyAsync(e->d.raw_l, e->h_in, sizeof(double) * (3 * (size_t)M + n), hipMemcpyHostToDevice, e->stream));
    if (have_inc) {
      memcpy(e->h_out, x_inc0, sizeof(double) * n);
      HIPCHK(hipMemcpyAsync(e->ta.inc_x, e->h_out, sizeof(double) * n, hipMemcpyHostToDevice, e->stream));
    }
    static unsigned long long *ktree_prof = nullptr;  // debug (MIOSQP_TREE_PROF=1), as for the one-wavefront kernel
    static const bool ktree_prof_on = getenv("MIOSQP_TREE_PROF") != nullptr;
    if (ktree_prof_on && !ktree_prof) {
      HIPCHK(hipMalloc((void **)&ktree_prof, 128));
      HIPCHK(hipMemset(ktree_prof, 0, 128));
    }
    Dev dk = e->d;
    if (ktree_prof_on) dk.prof = ktree_prof;
    hipLaunchKernelGGL(k_tree, dim3(1), dim3(RES_THREADS), lds, e->stream, dk, ta);
    if (ktree_prof_on) {
      unsigned long long h[16];
      HIPCHK(hipMemcpyAsync(h, ktree_prof, sizeof h, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipStreamSynchronize(e->stream));
      fprintf(stderr, "[tree prof] k_tree cumulative us: choose+prologue %.1f  relaxation %.1f  epilogue %.1f  branch+children %.1f\n",
              h[8] / 100.0, h[9] / 100.0, h[10] / 100.0, h[11] / 100.0);
    }
    HIPCHK(hipMemcpyAsync(e->h_out, e->ta.inc_x, sizeof(double) * n, hipMemcpyDeviceToHost, e->stream));
    static_assert(sizeof(TreeOut) <= sizeof(Ctrl), "TreeOut travels through the pinned control block");
    HIPCHK(hipMemcpyAsync(e->h_ctrl, e->ta.out, sizeof(TreeOut), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipEventRecord(e->ev1, e->stream));
    if (e->spin_wait) {
      hipError_t q;
      while ((q = hipEventQuery(e->ev1)) == hipErrorNotReady) {}
      if (q != hipSuccess) HIPCHK(q);
    } else {
      HIPCHK(hipStreamSynchronize(e->stream));
    }
    o = reinterpret_cast<const TreeOut *>(e->h_ctrl);
    x_found = e->h_out;
    HIPCHK(hipEventElapsedTime(&ms, e->ev0, e->ev1));
  }
  info->nodes = o->nodes;
  info->osqp_iter = o->osqp_iter;
  info->leaves_left = o->leaves_left;
  info->overflow = o->overflow;
  info->max_leaves = o->max_leaves;
  info->found = o->found;
  info->upper_glob = o->upper;
  info->lower_glob = o->lower_glob;
  info->device_time = 1e-3 * ms;
  info->run_time = wall() - t0;
  if (o->found || have_inc) memcpy(x_out, o->found ? x_found : x_inc0, sizeof(double) * n);
  e->loop_ms += ms;
  e->loop_iters += o->osqp_iter;
  return 0;
}

// the settings of strong / reliability branching for one engine's trees (miosqp_qp_solve_trees_sb), and where the
// counters go
struct TreesSb {
  int32_t rule, K, max_iter, reliability;
  double eps;
  miosqp_tree_sb_info *info;
};

// miosqp_qp_solve_trees, and with rf_info miosqp_qp_solve_trees_rf: the same staging and copies, k_tree_rf in place of
// k_tree / k_tree_w, the counters of round and fix per instance beside the outcomes; with sb miosqp_qp_solve_trees_sb in
// the same way: k_tree_sb, and the work areas of strong / reliability branching per instance
static int trees_run(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u, const double *x0,
                     const double *y0, const double *upper0, const double *x_inc0, int32_t tree_explor_rule,
                     int32_t max_iter_bb, double *x_out, miosqp_tree_info *info, int32_t rf_candidates = 0,
                     int32_t rf_max_iter = 0, int32_t rf_every = 0, miosqp_tree_rf_info *rf_info = nullptr,
                     const TreesSb *sb = nullptr) {
  if (!e || B < 1 || !q || !l || !u || !x0 || !y0 || !upper0 || !x_out || !info || max_iter_bb < 1 || tree_explor_rule < 0 ||
      tree_explor_rule > 3)
    return MIOSQP_EARG;
  ENTER(e);
  if (!e->have_int || !e->d.digest) {
    g_err = "solve_trees: call miosqp_qp_set_integer_rows and miosqp_qp_set_root first";
    return MIOSQP_EARG;
  }
  const int n = e->n, M = e->M, p = e->d.n_int;
  const size_t blk = 3 * (size_t)M + n;
  int tree_sp_off = -1;
  size_t lds = tree_lds_bytes(e, &tree_sp_off);
  if (!e->fold || lds > 160 * 1024 || p < 1) {
    g_err = "solve_trees: only for problems whose product-form factor, iterates and leaf list fit 160 KB of LDS";
    return MIOSQP_EUNSUPPORTED;
  }
  for (size_t k = 0; k < (size_t)B * M; k++)
    if (l[k] > u[k]) return MIOSQP_EBOUNDS;
  const double t0 = wall();
  bool wave = false;  // as miosqp_qp_solve_tree
  if (int rcw = tree_wave_prepare(e, &wave)) return rcw;
  if (rf_info) {  // (k_tree_rf also runs the wave-sized engines: sized for the engine as tree_wave_prepare left it)
    lds = tree_lds_bytes(e, &tree_sp_off);
    HIPCHK(lds_limit_once((const void *)k_tree_rf, 19));
  } else if (sb) {  // (k_tree_sb takes the wave-sized engines in the same way)
    lds = tree_lds_bytes(e, &tree_sp_off);
    HIPCHK(lds_limit_once((const void *)k_tree_sb, 22));
  } else if (!wave) {
    HIPCHK(lds_limit_once((const void *)k_tree, 1));
  }
  if (B > e->tb_cap) {  // (a larger batch takes new arrays; the old ones stay with the pool until cleanup)
    const size_t cap = (size_t)std::max(B, 2 * e->tb_cap);
    int rc = pool_reserve(e, cap * ((size_t)TREE_CAP * (2 * (size_t)p + n + M) + blk + 3 * (size_t)n + 20) * sizeof(double) + 4096);
    if (!rc) rc = dalloc(e, &e->tb_q, cap * n);
    if (!rc) rc = dalloc(e, &e->tb_qraw, cap * n);
    if (!rc) rc = dalloc(e, &e->tb_raw, cap * blk);
    if (!rc) rc = dalloc(e, &e->tb_lo, cap * TREE_CAP * p);
    if (!rc) rc = dalloc(e, &e->tb_hi, cap * TREE_CAP * p);
    if (!rc) rc = dalloc(e, &e->tb_x, cap * TREE_CAP * n);
    if (!rc) rc = dalloc(e, &e->tb_y, cap * TREE_CAP * M);
    if (!rc) rc = dalloc(e, &e->tb_inc, cap * n);
    if (!rc) rc = dalloc(e, &e->tb_upper, cap);
    if (!rc) rc = dalloc(e, &e->tb_out, cap);
    if (!rc) rc = dalloc(e, &e->tb_rf, cap);
    if (rc) return rc;
    e->tb_cap = (int)cap;
  }
  if (sb && (B > e->tb_sb_cap || p != e->tb_sb_p)) {  // (its own capacity: a call without the rule pays nothing for it)
    const size_t cap = (size_t)std::max(B, B > e->tb_sb_cap ? 2 * e->tb_sb_cap : e->tb_sb_cap);
    int rc = dalloc(e, &e->tb_sbw, cap * miosqp::tree_sb::work_doubles(p));
    if (!rc) rc = dalloc(e, &e->tb_sbpc, cap * (size_t)TREE_CAP * miosqp::tree_sb::PC_DOUBLES);
    if (!rc) rc = dalloc(e, &e->tb_sb, cap);
    if (rc) return rc;
    e->tb_sb_cap = (int)cap;
    e->tb_sb_p = p;
  }
  // one staging vector: [raw blocks | q | incumbents | upper] in
  const size_t nin = (size_t)B * (blk + 2 * (size_t)n + 1);
  if (e->tb_host.size() < nin) e->tb_host.resize(nin);
  double *h_raw = e->tb_host.data(), *h_q = h_raw + (size_t)B * blk, *h_inc = h_q + (size_t)B * n, *h_up = h_inc + (size_t)B * n;
  bool any_inc = false;
  for (int b = 0; b < B; b++) {
    double *r = h_raw + (size_t)b * blk;
    memcpy(r, l + (size_t)b * M, sizeof(double) * M);
    memcpy(r + M, u + (size_t)b * M, sizeof(double) * M);
    memcpy(r + 2 * (size_t)M, x0 + (size_t)b * n, sizeof(double) * n);
    memcpy(r + 2 * (size_t)M + n, y0 + (size_t)b * M, sizeof(double) * M);
    const bool have = x_inc0 != nullptr && upper0[b] < 1.7e308;
    h_up[b] = have ? upper0[b] : 1.0 / 0.0;
    if (have) memcpy(h_inc + (size_t)b * n, x_inc0 + (size_t)b * n, sizeof(double) * n);
    else memset(h_inc + (size_t)b * n, 0, sizeof(double) * n);
    any_inc = any_inc || have;
  }
  memcpy(h_q, q, sizeof(double) * (size_t)B * n);
  HIPCHK(hipEventRecord(e->ev0, e->stream));
  HIPCHK(hipMemcpyAsync(e->tb_raw, h_raw, sizeof(double) * (size_t)B * blk, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(e->tb_qraw, h_q, sizeof(double) * (size_t)B * n, hipMemcpyHostToDevice, e->stream));
  if (any_inc) HIPCHK(hipMemcpyAsync(e->tb_inc, h_inc, sizeof(double) * (size_t)B * n, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(e->tb_upper, h_up, sizeof(double) * B, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_scale_q_batch, dim3((unsigned)(((size_t)B * n + 255) / 256)), dim3(256), 0, e->stream, e->d, e->tb_qraw,
                     e->tb_q, B);
  TreeArgs ta{};
  ta.rule = tree_explor_rule;
  ta.max_nodes = max_iter_bb;
  ta.max_iter = e->st.max_iter;
  ta.check_every = e->st.check_termination;
  tree_lane_groups(n, M, ta);
  ta.upper0 = 1.0 / 0.0;
  ta.lf_lo = e->tb_lo; ta.lf_hi = e->tb_hi; ta.lf_x = e->tb_x; ta.lf_y = e->tb_y;
  ta.inc_x = e->tb_inc;
  ta.out = e->tb_out;
  ta.done = nullptr;
  ta.sp_off = tree_sp_off;
  ta.batch = 1;
  ta.upper_b = e->tb_upper;
  if (rf_info) {
    ta.rf_K = rf_candidates;
    ta.rf_max_iter = rf_max_iter;
    ta.rf_every = rf_every;
    ta.rf_out = e->tb_rf;
  }
  if (sb) {
    ta.sb_rule = sb->rule;
    ta.sb_K = sb->K;
    ta.sb_max_iter = sb->max_iter;
    ta.sb_rel = sb->reliability;
    ta.sb_eps = sb->eps;
    ta.sb_work = e->tb_sbw;
    ta.sb_pc = e->tb_sbpc;
    ta.sb_out = e->tb_sb;
  }
  Dev db = e->d;  // instance 0's arrays; workgroup b moves on from there (tree_instance)
  db.q = e->tb_q;
  db.qraw = e->tb_qraw;
  db.raw_l = e->tb_raw;
  db.raw_u = e->tb_raw + M;
  db.raw_x = e->tb_raw + 2 * (size_t)M;
  db.raw_y = e->tb_raw + 2 * (size_t)M + n;
  db.prof = nullptr;
  // (with round and fix the workgroup form also takes the wave-sized models: tree_lds_bytes sized it for the engine as it stands)
  if (rf_info) hipLaunchKernelGGL(k_tree_rf, dim3(B), dim3(RES_THREADS), lds, e->stream, db, ta);
  else if (sb) hipLaunchKernelGGL(k_tree_sb, dim3(B), dim3(RES_THREADS), lds, e->stream, db, ta);
  else if (wave) hipLaunchKernelGGL(k_tree_w, dim3(B), dim3(TW), 0, e->stream, db, ta);
  else hipLaunchKernelGGL(k_tree, dim3(B), dim3(RES_THREADS), lds, e->stream, db, ta);
  if (e->tb_hout.size() < (size_t)B) e->tb_hout.resize(B);
  HIPCHK(hipMemcpyAsync(e->tb_hout.data(), e->tb_out, sizeof(TreeOut) * B, hipMemcpyDeviceToHost, e->stream));
  if (rf_info) {
    if (e->tb_hrf.size() < (size_t)B) e->tb_hrf.resize(B);
    HIPCHK(hipMemcpyAsync(e->tb_hrf.data(), e->tb_rf, sizeof(TreeRfOut) * B, hipMemcpyDeviceToHost, e->stream));
  }
  if (sb) {
    if (e->tb_hsb.size() < (size_t)B) e->tb_hsb.resize(B);
    HIPCHK(hipMemcpyAsync(e->tb_hsb.data(), e->tb_sb, sizeof(TreeSbOut) * B, hipMemcpyDeviceToHost, e->stream));
  }
  HIPCHK(hipMemcpyAsync(h_inc, e->tb_inc, sizeof(double) * (size_t)B * n, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipEventRecord(e->ev1, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, e->ev0, e->ev1));
  const double wall_s = wall() - t0;
  int64_t iters = 0;
  for (int b = 0; b < B; b++) {
    const TreeOut &o = e->tb_hout[b];
    info[b].nodes = o.nodes;
    info[b].osqp_iter = o.osqp_iter;
    info[b].leaves_left = o.leaves_left;
    info[b].overflow = o.overflow;
    info[b].max_leaves = o.max_leaves;
    info[b].found = o.found;
    info[b].upper_glob = o.upper;
    info[b].lower_glob = o.lower_glob;
    info[b].device_time = 1e-3 * ms / B;  // the launch's device time, shared equally
    info[b].run_time = wall_s / B;
    const bool have = x_inc0 != nullptr && upper0[b] < 1.7e308;
    if (o.found) memcpy(x_out + (size_t)b * n, h_inc + (size_t)b * n, sizeof(double) * n);
    else if (have) memcpy(x_out + (size_t)b * n, x_inc0 + (size_t)b * n, sizeof(double) * n);
    iters += o.osqp_iter;
    if (rf_info) {
      const TreeRfOut &r = e->tb_hrf[b];
      rf_info[b] = miosqp_tree_rf_info{r.calls, r.candidates, r.feasible, r.improved, r.osqp_iter, 4, 0, 0};
    }
    if (sb) {
      const TreeSbOut &r = e->tb_hsb[b];
      sb->info[b] = miosqp_tree_sb_info{r.calls, r.children, r.osqp_iter, 6, 0, 0, 0, 0};
    }
  }
  e->loop_ms += ms;
  e->loop_iters += iters;
  return 0;
}

#include "host_trees_large.inc"  // B trees of ONE model beyond one workgroup's product form in one launch, in the reduced form (C ABI miosqp_qp_solve_trees_large, _rf, _sb)

int miosqp_qp_solve_trees(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u,
                          const double *x0, const double *y0, const double *upper0, const double *x_inc0,
                          int32_t tree_explor_rule, int32_t max_iter_bb, double *x_out, miosqp_tree_info *info) {
  return trees_run(e, B, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, x_out, info);
}

int miosqp_qp_solve_trees_rf(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u,
                             const double *x0, const double *y0, const double *upper0, const double *x_inc0,
                             int32_t tree_explor_rule, int32_t max_iter_bb, int32_t rf_candidates, int32_t rf_max_iter,
                             int32_t rf_every, double *x_out, miosqp_tree_info *info, miosqp_tree_rf_info *rf_info) {
  std::string err;
  if (int rc = miosqp::models::check_rf(1, &rf_candidates, &rf_max_iter, &rf_every, rf_info, 1, "solve_trees_rf", err)) {
    g_err = err;
    return rc;
  }
  return trees_run(e, B, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, x_out, info, rf_candidates, rf_max_iter,
                   rf_every, rf_info);
}

int miosqp_qp_solve_trees_sb(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u,
                             const double *x0, const double *y0, const double *upper0, const double *x_inc0,
                             int32_t tree_explor_rule, int32_t max_iter_bb, int32_t branching_rule, int32_t sb_candidates,
                             int32_t sb_max_iter, int32_t sb_reliability, double sb_eps, double *x_out, miosqp_tree_info *info,
                             miosqp_tree_sb_info *sb_info) {
  std::string err;
  if (int rc = miosqp::models::check_sb(1, &branching_rule, &sb_candidates, &sb_max_iter, &sb_reliability, &sb_eps, sb_info, 1,
                                        "solve_trees_sb", err)) {
    g_err = err;
    return rc;
  }
  const TreesSb sb{branching_rule, sb_candidates, sb_max_iter, sb_reliability, sb_eps, sb_info};
  return trees_run(e, B, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, x_out, info, 0, 0, 0, nullptr, &sb);
}

int miosqp_qp_tree_form(miosqp_qp_engine *e) {
  if (!e) return 0;
  if (e->device >= 0 && hipSetDevice(e->device) != hipSuccess) return 0;
  const int form = tree_form_of(e);
  return form < 0 ? 0 : form;
}

int miosqp_qp_solve_trees_models(int32_t B, miosqp_qp_engine *const *engines, const double *const *q, const double *const *l,
                                 const double *const *u, const double *const *x0, const double *const *y0,
                                 const double *upper0, const double *const *x_inc0, const int32_t *tree_explor_rule,
                                 const int32_t *max_iter_bb, double *const *x_out, miosqp_tree_info *info,
                                 miosqp_models_stats *stats) {
  return models_run(B, engines, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, x_out, info, stats);
}

int miosqp_qp_tree_form_large(miosqp_qp_engine *e, int32_t leaf_cap) {
  if (!e) return 0;
  if (e->device >= 0 && hipSetDevice(e->device) != hipSuccess) return 0;
  const int form = tree_form_large_of(e, leaf_cap);
  return form == 3 ? 3 : 0;
}

int miosqp_qp_solve_trees_models_large(int32_t B, miosqp_qp_engine *const *engines, const double *const *q, const double *const *l,
                                       const double *const *u, const double *const *x0, const double *const *y0,
                                       const double *upper0, const double *const *x_inc0, const int32_t *tree_explor_rule,
                                       const int32_t *max_iter_bb, int32_t leaf_cap, double *const *x_out,
                                       miosqp_tree_info *info, miosqp_models_stats *stats) {
  return models_run(B, engines, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, x_out, info, stats, true, leaf_cap);
}

int miosqp_qp_solve_trees_models_rf(int32_t B, miosqp_qp_engine *const *engines, const double *const *q, const double *const *l,
                                    const double *const *u, const double *const *x0, const double *const *y0,
                                    const double *upper0, const double *const *x_inc0, const int32_t *tree_explor_rule,
                                    const int32_t *max_iter_bb, int32_t leaf_cap, const int32_t *rf_candidates,
                                    const int32_t *rf_max_iter, const int32_t *rf_every, double *const *x_out,
                                    miosqp_tree_info *info, miosqp_tree_rf_info *rf_info, miosqp_models_stats *stats) {
  return models_run(B, engines, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, x_out, info, stats, leaf_cap != 0,
                    leaf_cap, true, rf_candidates, rf_max_iter, rf_every, rf_info);
}

int miosqp_qp_solve_trees_models_sb(int32_t B, miosqp_qp_engine *const *engines, const double *const *q, const double *const *l,
                                    const double *const *u, const double *const *x0, const double *const *y0,
                                    const double *upper0, const double *const *x_inc0, const int32_t *tree_explor_rule,
                                    const int32_t *max_iter_bb, int32_t leaf_cap, const int32_t *branching_rule,
                                    const int32_t *sb_candidates, const int32_t *sb_max_iter, const int32_t *sb_reliability,
                                    const double *sb_eps, double *const *x_out, miosqp_tree_info *info,
                                    miosqp_tree_sb_info *sb_info, miosqp_models_stats *stats) {
  const ModelsSb sb{branching_rule, sb_candidates, sb_max_iter, sb_reliability, sb_eps, sb_info};
  return models_run(B, engines, q, l, u, x0, y0, upper0, x_inc0, tree_explor_rule, max_iter_bb, x_out, info, stats, leaf_cap != 0,
                    leaf_cap, false, nullptr, nullptr, nullptr, nullptr, &sb);
}

int miosqp_qp_debug_iterate(miosqp_qp_engine *e, int32_t k, double *x, double *z, double *y) {
  if (!e || k < 0) return MIOSQP_EARG;
  ENTER(e);
  hipLaunchKernelGGL(k_reset_ctrl, dim3(1), dim3(1), 0, e->stream, e->d);
  hipLaunchKernelGGL(k_init_wh, dim3(((e->M > e->n ? e->M : e->n) + 255) / 256), dim3(256), 0, e->stream, e->d);
  if (e->resident) {
    if (k > 0) {
      int rc = launch_resident(e, k, 0, 0);
      if (rc) return rc;
    }
  } else if (e->coop || e->pers) {
    if (k > 0) {
      if (e->coop) launch_coop(e, k, 0, 0);
      else launch_pers(e, k, 0, 0);
      HIPCHK(hipMemcpyAsync(e->h_ctrl, e->d.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipStreamSynchronize(e->stream));
      if (e->h_ctrl->pad == 1) {  // called off, iterates untouched: the same k iterations in the two-kernel form
        reset_registration(e);
        g_err = "cooperative solver: the grid was not co-resident within 100 ms (device shared?), stage 1";
        int rc = leave_coop(e);
        if (rc) return rc;
        hipLaunchKernelGGL(k_reset_ctrl, dim3(1), dim3(1), 0, e->stream, e->d);
        for (int i = 0; i < k; i++) launch_iteration(e);
      } else if (e->h_ctrl->pad) {
        reset_registration(e);
        g_err = "cooperative solver: exchange timed out, stage " + std::to_string(e->h_ctrl->pad);
        return MIOSQP_EHIP;
      }
    }
  } else {
    for (int i = 0; i < k; i++) launch_iteration(e);
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  if (x) HIPCHK(hipMemcpy(x, e->d.x, sizeof(double) * e->n, hipMemcpyDeviceToHost));
  if (z) HIPCHK(hipMemcpy(z, e->d.z, sizeof(double) * e->M, hipMemcpyDeviceToHost));
  if (y) HIPCHK(hipMemcpy(y, e->d.y, sizeof(double) * e->M, hipMemcpyDeviceToHost));
  return 0;
}

int miosqp_qp_setup_models(int32_t B, const miosqp_setup_model *models, miosqp_qp_engine **out, miosqp_setup_models_stats *stats) {
  return setup_models_run(B, models, out, stats, false);
}

int miosqp_qp_setup_models_auto(int32_t B, const miosqp_setup_model *models, miosqp_qp_engine **out, miosqp_setup_models_stats *stats) {
  return setup_models_run(B, models, out, stats, true);
}

int miosqp_qp_setup_models_eligible(int32_t n, int32_t M, const miosqp_qp_settings *s) {
  if (!s) return 0;
  miosqp::setup_models::Args a;
  a.rho_auto = s->rho_auto; a.coop = s->coop; a.resident = s->resident; a.fold = s->fold; a.setup_on_device = s->setup_on_device;
  return miosqp::setup_models::eligible_shape(n, M) && miosqp::setup_models::eligible_settings(a) && setup_models_env_ok() ? 1 : 0;
}

int miosqp_qp_setup_models_large(int32_t B, const miosqp_setup_model *models, miosqp_qp_engine **out, miosqp_setup_models_stats *stats,
                                 int32_t rho_auto_in_launch) {
  return setup_models_run(B, models, out, stats, rho_auto_in_launch != 0, true);
}

int miosqp_qp_setup_models_eligible_large(int32_t n, int32_t M, const miosqp_qp_settings *s) {
  if (!s) return 0;
  miosqp::setup_models::Args a;
  a.rho_auto = s->rho_auto; a.coop = s->coop; a.resident = s->resident; a.fold = s->fold; a.setup_on_device = s->setup_on_device;
  a.pers = s->pers;
  return miosqp::setup_models::eligible_shape_large(n, M) && miosqp::setup_models::eligible_settings_large(a) &&
                 setup_models_large_env_ok()
             ? 1
             : 0;
}

int miosqp_qp_setup_models_large_auto(int32_t B, const miosqp_setup_model *models, miosqp_qp_engine **out,
                                      miosqp_setup_models_stats *stats, int32_t rho_auto_in_launch) {
  return setup_models_run(B, models, out, stats, rho_auto_in_launch != 0, true, true);
}

int miosqp_qp_setup_models_prepared(int32_t B, const miosqp_setup_model *models, miosqp_qp_engine **out,
                                    miosqp_setup_models_stats *stats, int32_t flags) {
  if (flags & ~(MIOSQP_SETUP_MODELS_RHO_AUTO | MIOSQP_SETUP_MODELS_LARGE | MIOSQP_SETUP_MODELS_LARGE_RHO_AUTO)) {
    g_err = "setup_models: unknown flag bits";
    return MIOSQP_EARG;
  }
  const bool lra = (flags & MIOSQP_SETUP_MODELS_LARGE_RHO_AUTO) != 0;
  return setup_models_run(B, models, out, stats, (flags & MIOSQP_SETUP_MODELS_RHO_AUTO) != 0,
                          lra || (flags & MIOSQP_SETUP_MODELS_LARGE) != 0, lra, true);
}

int miosqp_qp_setup_models_eligible_large_auto(int32_t n, int32_t M, const miosqp_qp_settings *s) {
  if (!s) return 0;
  miosqp::setup_models::Args a;
  a.rho_auto = s->rho_auto; a.coop = s->coop; a.resident = s->resident; a.fold = s->fold; a.setup_on_device = s->setup_on_device;
  a.pers = s->pers;
  const bool shape = a.rho_auto ? miosqp::setup_models::eligible_shape_large_auto(n, M) : miosqp::setup_models::eligible_shape_large(n, M);
  return shape && miosqp::setup_models::eligible_settings_large(a, true) && setup_models_large_env_ok() ? 1 : 0;
}

int miosqp_qp_setup_models_shape(int32_t n, int32_t M) {
  if (miosqp::setup_models::eligible_shape(n, M)) return 1;
  return miosqp::setup_models::eligible_shape_large(n, M) ? 2 : 0;
}

int miosqp_qp_setup_groups_live(void) {
  std::lock_guard<std::mutex> lk(g_group_mutex);
  return g_groups_live;
}

int64_t miosqp_qp_setup_group(miosqp_qp_engine *e) { return e && e->group ? e->group->id : 0; }

// debug: the panel's values (L21 = -rho Abar as stored, padding included) from the device or from the host's mirror
int miosqp_qp_debug_panel(miosqp_qp_engine *e, int32_t which, double *out, int64_t capacity, int64_t *count) {
  if (!e || !count || which < 0 || which > 3) {
    g_err = "debug_panel: bad argument";
    return MIOSQP_EARG;
  }
  ENTER(e);
  const std::vector<double> &mirror = (which & 1) ? e->fa.panel_by_con.val : e->fa.panel_by_var.val;
  *count = (int64_t)mirror.size();
  if (!out) return 0;
  if (capacity < *count) {
    g_err = "debug_panel: the output holds fewer than count values";
    return MIOSQP_EARG;
  }
  if (which >= 2) {
    if (*count) memcpy(out, mirror.data(), sizeof(double) * mirror.size());
    return 0;
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  if (*count) HIPCHK(hipMemcpy(out, (which & 1) ? e->d.pc_L : e->d.pv_L, sizeof(double) * mirror.size(), hipMemcpyDeviceToHost));
  return 0;
}

// debug: one array of the product form copied to the host as it lies in device memory (beside miosqp_qp_debug_factor)
int miosqp_qp_debug_product_form(miosqp_qp_engine *e, int32_t which, double *out, int64_t capacity, int32_t *rows, int32_t *ld) {
  if (!e || !rows || !ld || which < 0 || which > 7) {
    g_err = "debug_product_form: bad argument";
    return MIOSQP_EARG;
  }
  ENTER(e);
  const Dev &d = e->d;
  const double *src = nullptr;
  int r = 0, l = 0;
  switch (which) {
    case 0: src = d.f_rows; r = e->n; l = d.ldf; break;
    case 1: src = d.f_GmT; r = e->M; l = d.ldn; break;
    case 2: src = d.f_Ad; r = e->M; l = d.ldn; break;
    case 3: src = d.f_Atd; r = e->n; l = d.ldm; break;
    case 4: src = d.f_Pd; r = e->n; l = d.ldn; break;
    case 5: src = d.q; r = e->n; l = 1; break;  // (vectors: rows of one value)
    case 6: src = d.l; r = e->M; l = 1; break;
    default: src = d.u; r = e->M; l = 1; break;
  }
  if ((which < 5 && !e->fold) || !src || l <= 0) {
    g_err = "debug_product_form: this engine did not build the product form";
    return MIOSQP_EUNSUPPORTED;
  }
  *rows = r;
  *ld = l;
  if (!out) return 0;
  if (capacity < (int64_t)r * l) {
    g_err = "debug_product_form: the output holds fewer than rows * ld values";
    return MIOSQP_EARG;
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(out, src, sizeof(double) * (size_t)r * l, hipMemcpyDeviceToHost));
  return 0;
}

// debug: one device-resident product of the set-up copied to the host as it lies in device memory (row-major, padding
// included).  Reads only: nothing the solvers use is touched.
int miosqp_qp_debug_factor(miosqp_qp_engine *e, int32_t which, double *out, int64_t capacity, int32_t *rows, int32_t *ld) {
  if (!e || !rows || !ld || which < 0 || which > 5) {
    g_err = "debug_factor: bad argument";
    return MIOSQP_EARG;
  }
  ENTER(e);
  const Dev &d = e->d;
  const int n = e->n, N = e->n + e->M;
  const double *src = nullptr;
  int r = 0, l = 0;
  const char *name = "";
  switch (which) {
    case 0: src = d.d2inv; r = n; l = 1; name = "d2inv"; break;  // (a vector: n rows of one value)
    case 1: src = d.Linv; r = n; l = d.ld; name = "Linv"; break;
    case 2: src = d.LinvT; r = n; l = d.ld; name = "LinvT"; break;
    case 3: src = d.W; r = N; l = d.ldw; name = "the explicit KKT inverse W"; break;
    case 4: src = d.Kc; r = N; l = d.ldw; name = "Kc"; break;
    default:
      if (e->pers_capable) src = e->pp.sinv;
      r = n; l = e->pp.sinv_ld; name = "the persistent solver's tail inverse";
      break;
  }
  if (!src || l <= 0) {
    g_err = std::string("debug_factor: this engine did not build ") + name;
    return MIOSQP_EUNSUPPORTED;
  }
  *rows = r;
  *ld = l;
  if (!out) return 0;
  if (capacity < (int64_t)r * l) {
    g_err = "debug_factor: the output holds fewer than rows * ld values";
    return MIOSQP_EARG;
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(out, src, sizeof(double) * (size_t)r * l, hipMemcpyDeviceToHost));
  return 0;
}

int miosqp_qp_get_scaling(miosqp_qp_engine *e, double *D, double *E, double *c) {
  if (!e) return MIOSQP_EARG;
  if (D) memcpy(D, e->sc.D.data(), sizeof(double) * e->n);
  if (E) memcpy(E, e->sc.E.data(), sizeof(double) * e->M);
  if (c) *c = e->sc.c;
  return 0;
}

static void kernel_bytes(const miosqp_qp_engine *e, double b[6]) {
  const double n = e->n, M = e->M, np = (double)e->fa.nnz_panel, nt = (double)e->fa.nnz_tail;
  // 12 B per factor entry (value + index), 4 B row pointers, 8 B vectors
  b[0] = np * 12 + (n + 1) * 4 + (M + 3 * n) * 8;          // panel forward: wh in; x, q in; c out
  b[1] = nt * 12 + (n + 1) * 4 + (3 * n) * 8;              // tail forward: c in, d2inv in, ut out
  b[2] = nt * 12 + (n + 1) * 4 + (5 * n) * 8;              // tail backward: ut in, x in; xt, x, dx out
  b[3] = np * 12 + (M + 1) * 4 + (n + 10 * M) * 8;         // panel backward + z/y update
  const double k = e->st.check_termination;
  const double NK = n + M;
  const double rest = 2 * (NK + 1) * 4 + NK * 8 + NK * 20 + (6 * n + 16 * M) * 8 + (2.0 * e->nnzA + e->nnzPtriu) * 12 / k;
  b[4] = 2 * (np + nt) * 12 + rest;
  // what the kernels of the form in use REQUEST per iteration: the dense tail (and, in the product form, the
  // dense G block) carries no index array, so those entries move 8 bytes, not the 12 of the formula above
  b[5] = (e->fold ? 2 * ((double)n * M + nt) * 8 : 2 * (np * 12 + nt * 8)) + rest;
  if (e->pers && e->pp.sinv && e->pp.res_w) b[5] -= n * (n - e->pp.res_c0) * 8;  // columns of S^-1 that stay in LDS
  if (e->pers && e->pp.sinv && e->pp.sym) {  // the tiles on and above the diagonal instead of the whole of S^-1
    double tiles = 0;
    for (int I = 0; I < e->pp.sym_T; I++)
      for (int J = I; J < e->pp.sym_T; J++)
      {
        const int nr = std::min(e->pp.sym_C, e->n - I * e->pp.sym_C), Rw = (nr + PERS_NW - 1) / PERS_NW;
        int streamed = 0;  // (every wave keeps the first sym_res rows of its share in LDS)
        for (int w = 0; w < PERS_NW; w++) streamed += std::max(0, std::min(Rw, nr - w * Rw) - e->pp.sym_res);
        tiles += (double)streamed * std::min(e->pp.sym_C, e->n - J * e->pp.sym_C);
      }
    b[5] += (tiles - 2 * nt) * 8;
  }
}

int miosqp_qp_get_factor_stats(miosqp_qp_engine *e, int64_t *out) {
  if (!e || !out) return MIOSQP_EARG;
  double b[6];
  kernel_bytes(e, b);
  out[8] = (int64_t)b[5];
  out[9] = e->coop_fallbacks;
  out[0] = e->fa.nnz_panel + e->fa.nnz_tail;
  out[1] = e->fa.nnz_panel;
  out[2] = e->n;
  out[3] = (int64_t)b[4];
  out[4] = e->tpr_pv; out[5] = e->tpr_pc; out[6] = e->tpr_tail; out[7] = (e->fold ? 1 : 0) | (e->resident ? 2 : 0) | (e->setup_on_device ? 4 : 0) | (e->coop ? 8 : 0) |
           (e->pers ? 16 : 0) | ((e->pers && e->pp.sinv) ? 32 : 0) | ((e->pers && e->pp.small) ? 64 : 0) |
           ((e->d.coop_nap & 0xff) << 8) | (e->kbp ? (1 << 16) : 0) | (e->guard_tripped ? (1 << 17) : 0) |
           (e->run_launches > 0 ? (1 << 18) : 0);
  return 0;
}

int miosqp_qp_get_rho(miosqp_qp_engine *e, double *rho) {
  if (!e || !rho) return MIOSQP_EARG;
  *rho = e->d.rho;
  return 0;
}

int miosqp_qp_get_inverse_guard(miosqp_qp_engine *e, double *out) {
  if (!e || !out) return MIOSQP_EARG;
  out[0] = e->guard_resid;
  out[1] = e->guard_tol;
  out[2] = e->guard_tripped ? 1.0 : 0.0;
  return 0;
}

int miosqp_qp_get_loop_stats(miosqp_qp_engine *e, double *ms, int64_t *iters, int32_t reset) {
  if (!e) return MIOSQP_EARG;
  if (ms) *ms = e->loop_ms;
  if (iters) *iters = e->loop_iters;
  if (reset) {
    e->loop_ms = 0.0;
    e->loop_iters = 0;
    e->loop_launches = 0;
    e->run_launches = 0;
    e->node_ms.clear();
    e->node_it.clear();
  }
  return 0;
}

// launches of the hosted search's solver kernel since the last reset of the loop statistics: one per node, or -- the
// cooperative grid kept resident (k_coop_run) -- one per miosqp_qp_search_run
int miosqp_qp_get_loop_launches(miosqp_qp_engine *e, int64_t *launches) {
  if (!e || !launches) return MIOSQP_EARG;
  *launches = e->loop_launches;
  return 0;
}

// per node of the hosted search since the last reset of the loop statistics: microseconds of device time per ADMM
// iteration of a node's launch -- minimum, median, maximum over the nodes -- and the number of nodes they are taken over
int miosqp_qp_get_node_stats(miosqp_qp_engine *e, double *us_per_iter_min_med_max, int32_t *nodes) {
  if (!e || !us_per_iter_min_med_max || !nodes) return MIOSQP_EARG;
  const size_t k = std::min(e->node_ms.size(), e->node_it.size());
  std::vector<double> v;
  for (size_t i = 0; i < k; i++)
    if (e->node_it[i] > 0) v.push_back(1e3 * (double)e->node_ms[i] / (double)e->node_it[i]);
  *nodes = (int32_t)v.size();
  us_per_iter_min_med_max[0] = us_per_iter_min_med_max[1] = us_per_iter_min_med_max[2] = 0.0;
  if (v.empty()) return 0;
  std::sort(v.begin(), v.end());
  us_per_iter_min_med_max[0] = v.front();
  us_per_iter_min_med_max[1] = v[v.size() / 2];
  us_per_iter_min_med_max[2] = v.back();
  return 0;
}

// debug: per-block (start, end) wall-clock stamps (100 MHz) of ONE launch of a product-form kernel
int miosqp_qp_debug_timeline(miosqp_qp_engine *e, int32_t which, uint64_t *out, int32_t max_blocks,
                             int32_t *nblocks) {
  if (which == 6) {
    // the persistent stream's own phase clocks (MIOSQP_KBS_PROF=1), summed over the launches since the last call; per
    // workgroup 8 words: shader clocks of thread 0 in {iterations, test, harvest + refill, -}, chunks, -, -, -; then per
    // workgroup 8 more: the phases inside the iterations {forward sweep, reduce + store, barrier, x sweep, x epilogue,
    // constraint tiles, barrier}, -; then per workgroup 16: the phases inside the boundaries {test jobs, row pieces + fold,
    // barrier, members' fold + decision, harvest rows + claim, barrier, table + harvest jobs + fold, prepare, barrier, commit,
    // z jobs + stores, barrier, counters}
    if (!e || !out || !e->kbs_prof || max_blocks < 16 * KBP_WGS) return MIOSQP_EARG;
    ENTER(e);
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(out, e->kbs_prof, sizeof(unsigned long long) * 32 * KBP_WGS, hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(e->kbs_prof, 0, sizeof(unsigned long long) * 32 * KBP_WGS));
    if (nblocks) *nblocks = 16 * KBP_WGS;
    return 0;
  }
  if (!e || !out || which < 0 || which > 5 || (which < 4 && !e->fold) || (which == 2 && !e->coop) || (which == 3 && e->Bcap == 0) ||
      (which == 4 && !e->pers) || (which == 5 && !e->kbp))
    return MIOSQP_EARG;
  ENTER(e);
  unsigned long long *buf = nullptr;
  HIPCHK(hipMalloc((void **)&buf, sizeof(unsigned long long) * 2 * 8192));
  HIPCHK(hipMemsetAsync(buf, 0, sizeof(unsigned long long) * 2 * 8192, e->stream));
  if (which == 5) {
    // every column live for the measurement (the columns of a finished wave are all decided); the caller solves anew
    HIPCHK(hipMemsetAsync(e->d.c_done, 0, sizeof(int) * e->d.Bs, e->stream));
    launch_kbp(e, e->d, e->Bcap / 64, 5);
  } else if (which == 4) {
    launch_pers(e, 20, 0, 0);
  } else if (which == 3) {
    for (int i = 0; i < 5; i++) launch_iteration_b(e, e->Bcap / 64);
  } else {
    for (int i = 0; i < 20; i++) launch_iteration(e);
  }
  Dev saved = e->d;
  e->d.prof = buf;
  // which == 2: 1000 iterations of the cooperative solver; per workgroup 8 words: shader clocks of
  // thread 0 in {reduce, update+publish, gather}, iterations, {test operands+rows, test norms}, tests, -
  // which == 3: the batched forward sweep (kbm_fwd) at full width; per workgroup 8 words (100 MHz stamps of wave 0):
  // start, first loads issued, first operands arrived, sweep done, reduced, stored
  // which == 4: 1000 iterations of the persistent streaming solver, tests every 25; per workgroup 16 words: shader
  // clocks of thread 0 in {sparse forward, forward wait, forward rows, forward epilogue, backward wait, backward rows,
  // backward epilogue (+ sparse backward), tests}, iterations
  // which == 5: 100 lock-step iterations of kbp at full width; per workgroup 16 words: shader clocks of thread 0 in
  // {forward sweep, forward reduce + store, barrier, x sweep, x reduce + epilogue, constraint tiles, barrier}, iterations
  if (which == 5) launch_kbp(e, e->d, e->Bcap / 64, 100, true);
  else if (which == 4) launch_pers(e, 1000, 25, 0);
  else if (which == 3) launch_bd(e, e->Bcap / 64, 0);
  else if (which == 2) launch_coop(e, 1000, 25, 0);
  else if (which == 0) launch_fold_fwd(e); else launch_fold_bwd(e);
  e->d = saved;
  HIPCHK(hipStreamSynchronize(e->stream));
  const int nb = max_blocks < 8192 ? max_blocks : 8192;
  HIPCHK(hipMemcpy(out, buf, sizeof(unsigned long long) * 2 * nb, hipMemcpyDeviceToHost));
  if (nblocks) *nblocks = nb;
  hipFree(buf);
  return 0;
}

// debug: shader cycles and 100 MHz wall ticks recorded by the last LDS-resident launch
int miosqp_qp_debug_clock(miosqp_qp_engine *e, double *cycles, double *ticks) {
  if (!e) return MIOSQP_EARG;
  ENTER(e);
  HIPCHK(hipStreamSynchronize(e->stream));
  Ctrl c;
  HIPCHK(hipMemcpy(&c, e->d.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost));
  *cycles = c.nrm_dy;
  *ticks = c.nrm_dx;
  return 0;
}

// debug counters: 0 = wave compactions performed by solve_batch so far
int64_t miosqp_qp_debug_counter(miosqp_qp_engine *e, int32_t which) {
  if (!e) return -1;
  if (which == 2) {  // whole-chip launches of this device that were ordered behind another stream's (host.inc: ChipTurn)
    ChipTurn *t = chip_of(e);
    if (!t) return -1;
    std::lock_guard<std::mutex> lk(t->mu);
    return t->waits;
  }
  if (which == 3) {  // the control block's call-off / time-out word, after everything queued on the engine's stream
    if (e->device >= 0 && hipSetDevice(e->device) != hipSuccess) return -1;
    int pad = -1;
    if (hipStreamSynchronize(e->stream) != hipSuccess) return -1;
    if (hipMemcpy(&pad, &e->d.ctrl->pad, sizeof pad, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return pad;
  }
  if (which == 4) {  // engines of this device that take turns
    ChipTurn *t = chip_of(e);
    if (!t) return -1;
    std::lock_guard<std::mutex> lk(t->mu);
    return t->users;
  }
  if (which == 5) return (e->pers_capable && e->pp.sinv && e->pp.res_w) ? e->n - e->pp.res_c0 : 0;
  if (which == 6) return (e->pers_capable && e->pp.sinv && e->pp.sym) ? e->pp.sym_tiles : 0;
  if (which == 7) return e->kbs_launches;
  if (which == 8) return e->kbs_chunks_run;
  if (which == 9) return e->graph_chunks_run;
  if (which == 10) return e->run_nap_in_use;
  if (which == 11) return e->run_cal_nodes;
  if (which == 12) return e->polml ? (int64_t)(e->polml->cap_slab * sizeof(double)) : 0;  // slabs of polish_many_large
  return which == 0 ? e->compactions : which == 1 ? e->kbp_fallbacks : -1;
}

int miosqp_qp_get_batch_stats(miosqp_qp_engine *e, double *ms, int64_t *batch_iters, int64_t *node_iters,
                              int32_t reset) {
  if (!e) return MIOSQP_EARG;
  if (ms) *ms = e->bloop_ms;
  if (batch_iters) *batch_iters = e->bloop_iters;
  if (node_iters) *node_iters = e->bloop_node_iters;
  if (reset) {
    e->bloop_ms = 0.0;
    e->bloop_iters = e->bloop_node_iters = 0;
  }
  return 0;
}

int miosqp_qp_time_kernel(miosqp_qp_engine *e, int32_t which, int32_t reps, double *usec, double *bytes) {
  if (!e || which < 0 || (which > 4 && which < 10) || which > 15 || reps <= 0 || !usec) return MIOSQP_EARG;
  ENTER(e);
  if (which >= 10 && e->Bcap == 0) {
    g_err = "time_kernel: batched kernels need a prior solve_batch";
    return MIOSQP_EARG;
  }
  const Dev &d = e->d;
  const int ntiles = e->Bcap / 64;
  if (which >= 10) hipLaunchKernelGGL(kb_reset, dim3((d.Bs + 255) / 256), dim3(256), 0, e->stream, d, e->Bcap);
  hipLaunchKernelGGL(k_reset_ctrl, dim3(1), dim3(1), 0, e->stream, d);
  auto one = [&]() {
    if (e->fold && which < 4) {
      if (which == 0) launch_fold_fwd(e);
      if (which == 1) launch_fold_bwd(e);
      return;
    }
    if (e->fold && which >= 10 && which < 14) {
      if (which == 10) launch_bd(e, ntiles, 0);
      if (which == 11) launch_bd(e, ntiles, 1);
      return;
    }
    switch (which) {
      case 10: hipLaunchKernelGGL(kb_panel_fwd<false>, dim3((d.n + 3) / 4, ntiles), dim3(256), 0, e->stream, d); break;
      case 11: hipLaunchKernelGGL(kb_tail_fwd, dim3((d.n + 3) / 4, ntiles), dim3(256), 0, e->stream, d); break;
      case 12: hipLaunchKernelGGL(kb_tail_bwd, dim3((d.n + 3) / 4, ntiles), dim3(256), 0, e->stream, d); break;
      case 13: hipLaunchKernelGGL(kb_panel_bwd, dim3((d.M + 3) / 4, ntiles), dim3(256), 0, e->stream, d); break;
      case 14: launch_iteration_b(e, ntiles); break;
      case 0: DISPATCH_TPR(e->tpr_pv, k_panel_fwd, d.n, e->stream, d); break;
      case 1: DISPATCH_TPR(e->tpr_tail, k_tail_fwd, d.n, e->stream, d); break;
      case 2: DISPATCH_TPR(e->tpr_tail, k_tail_bwd, d.n, e->stream, d); break;
      case 3: DISPATCH_TPR(e->tpr_pc, k_panel_bwd, d.M, e->stream, d); break;
      default: launch_iteration(e); break;
    }
  };
  if (which == 15) {  // `reps` lock-step iterations of the batched sweeps in ONE persistent launch (kbp), every column live
    if (!e->kbp) {
      g_err = "time_kernel: the persistent batched sweeps are not in use on this engine";
      return MIOSQP_EARG;
    }
    launch_kbp(e, d, ntiles, 5);
    HIPCHK(hipEventRecord(e->ev0, e->stream));
    launch_kbp(e, d, ntiles, reps < 200 ? reps : 200);
    HIPCHK(hipEventRecord(e->ev1, e->stream));
    reps = reps < 200 ? reps : 200;
  } else if ((e->coop || e->pers) && which == 4) {  // `reps` iterations of the single-launch solver in ONE launch, no tests
    if (e->coop) launch_coop(e, 5, 0, 0); else launch_pers(e, 5, 0, 0);
    HIPCHK(hipEventRecord(e->ev0, e->stream));
    if (e->coop) launch_coop(e, reps, 0, 0); else launch_pers(e, reps, 0, 0);
    HIPCHK(hipEventRecord(e->ev1, e->stream));
  } else {
    for (int i = 0; i < 5; i++) one();
    HIPCHK(hipEventRecord(e->ev0, e->stream));
    for (int i = 0; i < reps; i++) one();
    HIPCHK(hipEventRecord(e->ev1, e->stream));
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, e->ev0, e->ev1));
  *usec = 1e3 * ms / reps;
  if (bytes) {
    double b[6];
    kernel_bytes(e, b);
    if (which < 10) {
      *bytes = b[which];
      if (e->fold && which < 4)  // forward sweep = panel + tail forward, backward likewise
        *bytes = which == 0 ? b[0] + b[1] : which == 1 ? b[2] + b[3] : 0.0;
    } else {
      // batched: matrix terms once per launch, per-node vector terms times the columns
      const double n = e->n, M = e->M, np = (double)e->fa.nnz_panel, nt = (double)e->fa.nnz_tail, B = e->Bcap;
      const double mat[5] = {np * 12 + (n + 1) * 4, nt * 12 + (n + 1) * 4, nt * 12 + (n + 1) * 4,
                             np * 12 + (M + 1) * 4, 2 * (np + nt) * 12 + 2 * (n + M + 1) * 4 + (n + M) * 12};
      const double vec[5] = {(M + 3 * n) * 8, 3 * n * 8, 5 * n * 8, (n + 10 * M) * 8, (6 * n + 16 * M) * 8};
      const int wb = which == 15 ? 14 : which;
      *bytes = mat[wb - 10] + B * vec[wb - 10];
      if (e->fold && which < 14)
        *bytes = which == 10 ? mat[0] + mat[1] + B * (vec[0] + vec[1])
                 : which == 11 ? mat[2] + mat[3] + B * (vec[2] + vec[3]) : 0.0;
    }
  }
  return 0;
}

}  // extern "C"
