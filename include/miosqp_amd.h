/*
 * miosqp_amd.h -- C ABI of the MI355X QP-relaxation engine (libmiosqp_hip.so).
 *
 * Drop-in boundary for ONE path of miOSQP: the relaxation solve that Node.solve() triggers.
 * The reference reaches that path through five Python calls on one shared `osqp.OSQP` object;
 * each entry point below names the reference call it replaces.  Plain pointers and sizes only;
 * every array argument is copied during the call (the reference keeps mutating its numpy
 * arrays afterwards: /root/reference/miosqp/data.py:120,126), outputs are written into
 * caller-owned buffers.  All functions return 0 on success, a negative MIOSQP_E* code on error,
 * or a positive value where documented.  Not re-entrant per handle (the reference is
 * single-threaded: one solver object mutated in place, workspace.py:63).
 *
 * Matrices: CSC, 32-bit indices, fp64 values (scipy's native layout, README.md:31 of the
 * reference).  P may be the full symmetric matrix or its upper triangle; only entries with
 * row <= col are read.  A is the EXTENDED constraint matrix [A; I[i_idx,:]] built by
 * /root/reference/miosqp/data.py:5-33, M = m + n_int rows.
 */
#ifndef MIOSQP_AMD_H
#define MIOSQP_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* solve outcome (info.status_val); values follow OSQP 0.6.x, looked up by name through
 * miosqp_qp_constant() exactly as the reference does with osqp.constant(name)
 * (/root/reference/miosqp/node.py:88,128-129; workspace.py:294-295,403-404,419). */
#define MIOSQP_QP_SOLVED 1
#define MIOSQP_QP_MAX_ITER_REACHED (-2)
#define MIOSQP_QP_PRIMAL_INFEASIBLE (-3)
#define MIOSQP_QP_DUAL_INFEASIBLE (-4)
#define MIOSQP_QP_UNSOLVED (-10)

/* error codes */
#define MIOSQP_EARG (-1)      /* bad argument (NULL, negative size, crossed bounds at setup) */
#define MIOSQP_EHIP (-2)      /* a HIP runtime call failed; see miosqp_qp_last_error() */
#define MIOSQP_EFACTOR (-3)   /* KKT factorisation broke down (non-convex P?) */
#define MIOSQP_ENODEV (-4)    /* no usable gfx950 device */
#define MIOSQP_EUNSUPPORTED (-5) /* the entry point does not cover this problem size / engine form (caller falls back) */
#define MIOSQP_EFULL (-6)     /* the leaf store of miosqp_qp_search_* has no free slot (raise the capacity) */
#define MIOSQP_EBOUNDS 1      /* update_bounds: some l[i] > u[i]; nothing was changed */

/* Solver parameters = the keyword arguments the reference forwards verbatim to
 * osqp.OSQP.setup (/root/reference/miosqp/workspace.py:67-68).  The reference's examples set
 * only eps_abs, eps_rel, eps_prim_inf, verbose (examples/random_miqp/run_example.py:113-116);
 * everything else is this table (DESIGN.md "frozen spec"). rho is ONE scalar for all rows and
 * is never adapted, so the factor is shared by every branch-and-bound node. */
typedef struct miosqp_qp_settings {
  double rho;          /* 0.1  */
  double sigma;        /* 1e-6 */
  double alpha;        /* 1.6  */
  double eps_abs;      /* 1e-3 */
  double eps_rel;      /* 1e-3 */
  double eps_prim_inf; /* 1e-4 */
  double eps_dual_inf; /* 1e-4 */
  int32_t max_iter;          /* 4000 */
  int32_t scaling;           /* 10 Ruiz passes, 0 = off */
  int32_t check_termination; /* 25: residuals are tested every this many iterations */
  int32_t warm_start;        /* 1: solve() continues from the stored iterates */
  int32_t device;            /* HIP device ordinal; -1 = current device */
  int32_t max_batch;         /* capacity of miosqp_qp_solve_batch (>= 1) */
  int32_t fold;              /* -1 auto, 0 factor form L (4 kernels/iteration), 1 product form L^-1
                                (2 kernels/iteration; auto picks it for panels denser than 30 %) */
  int32_t resident;          /* -1 auto, 0 off, 1 on: whole solve in ONE workgroup: iterates in LDS; the factor as the
                                explicit KKT inverse in the workgroup's registers (n+M <= 192, the automatic
                                choice there) or in product form in LDS (when that fits 160 KB) */
  int32_t setup_on_device;   /* -1 auto (n >= 1024), 0 host, 1 device: dense LDL^T of the reduced Hessian and
                                the inverse of its triangular factor computed on the GPU at setup */
  int32_t coop;              /* -1 auto, 0 off, 1 on: cooperative register-resident solver -- the explicit KKT
                                inverse (n+M)^2 spread over the register files of up to one workgroup per
                                CU, ONE exchange per iteration (n+M <= 2048; auto from n+M = 193 on) */
  int32_t pers;              /* -1 auto, 0 off, 1 on: persistent streaming solver -- ONE launch per solve that reads the
                                factor (product or factor form, whichever `fold` selects) from memory in every
                                iteration; the kernel boundaries of the multi-kernel forms become tagged exchanges
                                between co-resident workgroups.  Any size that fits one workgroup's LDS operand
                                buffers (n+M <= ~17 000 in product form, n <= ~9 000 in factor form); auto: problems
                                beyond the cooperative solver's n+M <= 2048.  2 (factor form): the dense tail as the
                                explicit inverse of the reduced Hessian, S^-1 = L22^-T D22^-1 L22^-1 -- the bytes of the
                                two triangles, ONE dense phase per iteration instead of two */
  int32_t batch_pers;        /* -1 auto, 0 off, 1 on: batched mode (solve_batch, the leaf pool's stream) runs the lock-step
                                iterations of a chunk as ONE persistent launch with the product-form factor held in the
                                registers and LDS of 256 co-resident workgroups (n <= 512, rows in the products <= 1024;
                                auto: n >= 256).  Called off -- the chunk goes through two launches per iteration
                                instead -- when the device is shared and the workgroups are not co-resident in time */
  int32_t rho_auto;          /* 0 (default): `rho` as given.  1: rho is chosen ONCE per problem at setup and then frozen
                                (opt-in; Python: rho="auto").  The reference hands only eps_* to osqp.setup
                                (/root/reference/miosqp/workspace.py:67-68, examples/random_miqp/run_example.py:113-116),
                                i.e. OSQP's defaults, which adapt rho while solving; here one factor serves every node of
                                a tree, so OSQP's update rule -- rho <- rho sqrt(normalised primal residual / normalised
                                dual residual), scaled quantities, clamped to [1e-6, 1e6] -- is applied once, to the
                                iterates 50 iterations from zero on the setup's bounds, rounded to two significant
                                digits, and the KKT matrix is factorised for that value.  Config 2: 0.1 -> 0.013,
                                a third of the iterations per node.  miosqp_qp_get_rho reports the value in use */
} miosqp_qp_settings;

/* What the reference reads from `results.info` (/root/reference/miosqp/node.py:111-125) plus
 * residuals and the fused node epilogue. */
typedef struct miosqp_qp_info {
  int32_t status_val; /* node.py:111 */
  int32_t iter;       /* node.py:118 */
  double run_time;    /* node.py:121: host wall seconds of this solve call */
  double obj_val;     /* relaxation objective at the returned x (unused by the reference) */
  double pri_res;
  double dua_res;
  double device_time; /* seconds between HIP events around the device work of this call */
  double lower;       /* solve_node/solve_batch only: objective at the clamped x (node.py:143) */
  /* node digest (after miosqp_qp_set_root; -1 / NaN otherwise): what bound_and_branch needs next */
  int32_t int_inf;    /* number of integer variables off by more than eps_int_feas (workspace.py:245-264) */
  int32_t nextvar;    /* position in i_idx of the most fractional one (workspace.py:205-230) */
  double heur_viol;   /* worst violation of the root bounds by the rounded candidate, eps_abs slack
                         included: <= 0 means satisfies_lin_constraints (workspace.py:232-243, 321-323) */
  double heur_obj;    /* objective of the rounded candidate (workspace.py:324) */
} miosqp_qp_info;

typedef struct miosqp_qp_engine miosqp_qp_engine;

/* fills *s with the defaults tabulated above */
int miosqp_qp_default_settings(miosqp_qp_settings *s);

/* osqp.constant(name) -- /root/reference/miosqp/node.py:88.  Unknown name -> 0. */
int miosqp_qp_constant(const char *name);

/* osqp.OSQP().setup(P, q, A, l, u, **qp_settings) -- /root/reference/miosqp/workspace.py:63-68.
 * Scales the problem, factorises the KKT matrix once and places factor + matrices in HBM. */
int miosqp_qp_setup(miosqp_qp_engine **out, int32_t n, int32_t M,
                    const int32_t *P_colptr, const int32_t *P_rowidx, const double *P_val,
                    const int32_t *A_colptr, const int32_t *A_rowidx, const double *A_val,
                    const double *q, const double *l, const double *u,
                    const miosqp_qp_settings *settings);

/* solver.update(l=l, u=u) -- /root/reference/miosqp/node.py:102.  l, u: M doubles each. */
int miosqp_qp_update_bounds(miosqp_qp_engine *e, const double *l, const double *u);

/* solver.update(q=q) -- /root/reference/miosqp/solver.py:183-185.  q: n doubles. */
int miosqp_qp_update_lin_cost(miosqp_qp_engine *e, const double *q);

/* solver.warm_start(x=x, y=y) -- /root/reference/miosqp/node.py:105.  x: n, y: M doubles. */
int miosqp_qp_warm_start(miosqp_qp_engine *e, const double *x, const double *y);

/* results = solver.solve() -- /root/reference/miosqp/node.py:108-125.
 * x_out: n doubles, y_out: M doubles (fresh copies), info filled. */
int miosqp_qp_solve(miosqp_qp_engine *e, double *x_out, double *y_out, miosqp_qp_info *info);

/* Declares which rows of A are the integer-bound rows so that the node epilogue can run on
 * the device: rows m .. m+n_int-1 of A are I[i_idx,:] (/root/reference/miosqp/data.py:19-29).
 * i_idx: n_int variable indices.  Must be called before solve_node / solve_batch. */
int miosqp_qp_set_integer_rows(miosqp_qp_engine *e, int32_t n_int, const int32_t *i_idx,
                               int32_t m_orig);

/* Enables the node digest: the part of Workspace.bound_and_branch that only needs the node's x
 * (/root/reference/miosqp/workspace.py:245-272, 321-324) is evaluated on the device at the end of
 * solve_node.  l_root/u_root: the ROOT bounds data.l / data.u (M doubles); eps_int_feas from the
 * B&B settings; eps_lin = qp_settings['eps_abs'].  Call again after MIOSQP.update_vectors. */
int miosqp_qp_set_root(miosqp_qp_engine *e, const double *l_root, const double *u_root,
                       double eps_int_feas, double eps_lin);

/* Whole body of Node.solve() in one call -- /root/reference/miosqp/node.py:96-143:
 * update(l,u) -> warm_start(x0,y0) -> solve -> x[i_idx] clamped into [l[-n_int:], u[-n_int:]]
 * (node.py:131-136) -> lower = .5 x'Px + q'x at the clamped x (node.py:143, data.py:99-103).
 * For infeasible outcomes x/y hold the certificate as solve() returns it and lower is NaN. */
int miosqp_qp_solve_node(miosqp_qp_engine *e, const double *l, const double *u,
                         const double *x0, const double *y0, double *x_out, double *y_out,
                         miosqp_qp_info *info);

/* B independent nodes sharing the factor (leaves of Workspace.leaves,
 * /root/reference/miosqp/workspace.py:83), node-major arrays: l,u,y0,y_out [B][M];
 * x0,x_out [B][n]; info [B].  Each node's result equals what solve_node returns for it. */
int miosqp_qp_solve_batch(miosqp_qp_engine *e, int32_t B, const double *l, const double *u,
                          const double *x0, const double *y0, double *x_out, double *y_out,
                          miosqp_qp_info *info);

/* One MIQP per column: solve_batch with a linear cost of its own in every column, q [B][n] raw costs (node-major like the
 * other arrays).  Replaces, per column, solver.update(q=q) of the reference's MIOSQP.update_vectors
 * (miosqp/solver.py:183-185) followed by the update / warm_start / solve of its Node.solve
 * (miosqp/node.py:102-108): column k is what the engine computes after miosqp_qp_update_lin_cost(q_k) and
 * miosqp_qp_solve_node(l_k, u_k, x0_k, y0_k).  The engine's own q is neither read nor written.  Everything else --
 * slices of max_batch columns, compaction, digest, epilogue, the refusal while pool chunks are in flight -- is
 * miosqp_qp_solve_batch's.  The cost arrays are allocated on the first call. */
int miosqp_qp_solve_batch_q(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u,
                            const double *x0, const double *y0, double *x_out, double *y_out,
                            miosqp_qp_info *info);

/* ---- strong branching: the 2K children of one node solved together and scored on the device ----------------
 * For K candidates (ascending positions in i_idx, 1 <= K <= 32) of a solved parent (l, u: its bounds; x, y: its
 * clamped x and its y), child k (down) has u[m + cand[k]] = floor(x[i_idx[cand[k]]]) and child K + k (up) has
 * l[m + cand[k]] = ceil(x[i_idx[cand[k]]]); every child is warm-started from (x, y) and solved like solve_node with
 * max_iter iterations (a positive multiple of check_termination).  The children are built on the device from the one
 * parent uploaded and run as one batch (the solve_batch path); only the record below comes back.
 * lower_out[2K]: the children's lower (NaN where infeasible); status_out / iter_out [2K]; score_out[K]:
 * max(gain_down, eps) * max(gain_up, eps), gain = max(lower - parent_lower, 0), 1e30 for an infeasible child;
 * info->chosen: the argmax (ties to the lowest k), an index into cand.  Needs miosqp_qp_set_integer_rows.
 * MIOSQP_EARG: K, max_iter or a candidate out of range; MIOSQP_EBOUNDS: l > u in the parent or in a child. */
typedef struct miosqp_sb_info {
  int32_t chosen;      /* index into cand */
  int32_t children;    /* 2K */
  int32_t iters;       /* ADMM iterations of all children */
  double device_time;  /* seconds between the events around the call */
  double run_time;     /* wall seconds of the call */
} miosqp_sb_info;

int miosqp_qp_strong_branch(miosqp_qp_engine *e, const double *l, const double *u, const double *x, const double *y,
                            double parent_lower, int32_t K, const int32_t *cand, int32_t max_iter, double eps,
                            double *lower_out, int32_t *status_out, int32_t *iter_out, double *score_out,
                            miosqp_sb_info *info);

/* ---- round and fix: a primal heuristic on K rounded-and-fixed candidates of one node ----------------------------
 * Extends the reference's rounding heuristic (/root/reference/miosqp/workspace.py:266-272 rounds the node's x,
 * workspace.py:321-327 adopts it when it satisfies the root's linear constraints), which with continuous variables
 * almost never passes: here the integers are rounded, FIXED, and the continuous variables re-solved.
 * For a solved parent (l, u: its bounds; x, y: its clamped x and its y) candidate k = 0 .. K-1 (1 <= K <= 32) has, on
 * every integer row, l = u = min(max(floor(x_i + theta_k), l_row), u_row) with theta_k = (k + 1) / (K + 1) (one double
 * division); every other row and the warm start (x, y) are the parent's.  The candidates are built on the device from
 * the one parent uploaded and run as one batch (the solve_batch path) with at most max_iter iterations: a positive
 * multiple of check_termination, or the engine's own max_iter.
 * status_out / iter_out / obj_out / viol_out [K]: per candidate; obj is the objective of its rounded point, viol that
 * point's worst violation of the ROOT bounds with the eps_abs slack included (<= 0: satisfies_lin_constraints), both
 * NaN for an infeasible candidate.  A candidate counts when its status is SOLVED or MAX_ITER_REACHED, viol <= 0 and
 * obj < upper.  info->chosen: the counting candidate of lowest obj (ties to the lowest k), -1 when none counts;
 * x_out (n doubles): its rounded point, integer entries exact -- left untouched when chosen is -1.
 * Needs miosqp_qp_set_integer_rows and miosqp_qp_set_root (MIOSQP_EARG otherwise, as for K or max_iter out of range);
 * MIOSQP_EBOUNDS: l > u in the parent.  Leaves no state behind: solve_node answers the same before and after. */
typedef struct miosqp_rf_info {
  int32_t chosen;      /* the winning candidate, -1: none */
  int32_t feasible;    /* candidates with an x and viol <= 0 (whatever their objective) */
  int32_t candidates;  /* K */
  int32_t iters;       /* ADMM iterations of all candidates */
  double device_time;  /* seconds between the events around the call */
  double run_time;     /* wall seconds of the call */
} miosqp_rf_info;

int miosqp_qp_round_and_fix(miosqp_qp_engine *e, const double *l, const double *u, const double *x, const double *y,
                            double upper, int32_t K, int32_t max_iter, double *x_out, int32_t *status_out,
                            int32_t *iter_out, double *obj_out, double *viol_out, miosqp_rf_info *info);

/* ---- polishing: the exact optimum on the active set a first-order solution points to --------------------------
 * OSQP's solution polishing (osqp_polish / polish.c of OSQP 0.6.x, which the reference's users reach by passing
 * `polish` through qp_settings to osqp.OSQP.setup, /root/reference/miosqp/workspace.py:67-68; OSQP paper sec. 4),
 * as a call of its own on one node: l, u its bounds (M), x, y an approximate solution of it (n, M), all unscaled.
 *   1. z = A x.  Row j is lower-active when l_j == u_j or z_j - l_j < -y_j, otherwise upper-active when
 *      u_j - z_j < y_j (OSQP's rule, plus: an equality row is always active); a bound at or beyond +-1e30 is infinite
 *      and never active.  A_act: the active rows, b: their active bounds.
 *   2. S = P + delta I + A_act^T A_act / delta (dense, factorised on the device by the set-up's blocked LDL^T);
 *      ksolve(r1, r2): dx = S^-1 (r1 + A_act^T r2 / delta), dy = (A_act dx - r2) / delta -- block elimination of the
 *      regularised KKT matrix [[P + delta I, A_act^T], [A_act, -delta I]].
 *   3. (xh, yh) = ksolve(-q, b), then refine_iter times += ksolve(-q - P xh - A_act^T yh, b - A_act xh): the residuals
 *      of the UNregularised system.  yh is zero on inactive rows.
 *   4. pri = max_j max(l_j - (A xh)_j, (A xh)_j - u_j, 0), dua = |P xh + q + A^T yh|_inf over ALL rows, and the same two
 *      numbers for (x, y).  Accepted when no pivot of S was <= 0, pri_after <= max(pri_before, 1e-10) and
 *      dua_after <= max(dua_before, 1e-10) -- decided on the device.
 * The arithmetic is done on the unscaled matrices.  x_out / y_out: the polished point when accepted, otherwise the input
 * bit for bit.  Reads nothing and writes nothing the node solvers use: solve_node answers the same before and after.
 * MIOSQP_EBOUNDS: some l > u; MIOSQP_EARG: delta <= 0, refine_iter outside 0..10, or a NaN in l, u, x or y (a primal
 * infeasible node has no x to polish); MIOSQP_EUNSUPPORTED: n beyond 19 000 (one row of S per workgroup in LDS). */
typedef struct miosqp_polish_info {
  int32_t accepted;     /* 1: x_out / y_out hold the polished point */
  int32_t reason;       /* 0 ok, 1 factorisation (a pivot <= 0), 2 primal residual grew, 3 dual residual grew */
  int32_t n_lower;      /* rows active at their lower bound (equality rows included) */
  int32_t n_upper;
  double pri_before, dua_before;  /* of the input */
  double pri_after, dua_after;    /* of the polished point, accepted or not (NaN after reason 1) */
  double obj;           /* .5 xh' P xh + q' xh of the polished point, accepted or not (NaN after reason 1) */
  double device_time;   /* seconds between the events around the call */
  double run_time;      /* wall seconds of the call (the one-time allocation of the first call excluded) */
} miosqp_polish_info;

int miosqp_qp_polish(miosqp_qp_engine *e, const double *l, const double *u, const double *x, const double *y,
                     double delta, int32_t refine_iter, double *x_out, double *y_out, miosqp_polish_info *info);

/* device seconds of the last miosqp_qp_polish call by stage: classification, rows of S, factorisation and inverse,
 * solves + refinement + acceptance (zeros before the first call).  No counterpart in OSQP, which reports one polish_time. */
int miosqp_qp_get_polish_stages(miosqp_qp_engine *e, double *seconds);

/* ---- polishing with a repair loop around the active set ---------------------------------------------------------
 * OSQP's polish (polish.c of OSQP 0.6.x) guesses the active set once and gives the point up when the guess was wrong.
 * This entry extends it: OSQP has NO such loop.  Round 0 is miosqp_qp_polish unchanged (steps 1-3 above).  After the
 * solves of round k, with (xh, yh) the point just computed, z = A xh and tol = 1e-10 (the floor of the acceptance
 * test), every row is revised:
 *   - an equality row (l == u) stays active;
 *   - a lower-active row with yh > tol becomes inactive; an upper-active row with yh < -tol becomes inactive;
 *   - an inactive row with finite l and l - z > tol becomes lower-active, otherwise an inactive row with finite u and
 *     z - u > tol becomes upper-active; bounds at or beyond +-1e30 are never active;
 *   - a row dropped in a revision is not added again in the same revision.
 * changed = added + dropped.  changed == 0: stop 0, the set is a fixed point and the point is the node's KKT point up
 * to tol.  changed > 0 and k == repair_iter: stop 1.  Otherwise round k + 1 runs on the revised set: S rebuilt from
 * scratch, the LDL^T again, xh = yh = 0, 1 + refine_iter solves -- identical sets give identical bits whatever path led
 * to them.  A pivot <= 0 in a round k + 1 >= 1: stop 2, and the point and the set of round k are the ones judged.
 * Step 4 runs once more on the point the loop ended with: accepted when round 0 had no bad pivot,
 * pri_after <= max(pri_before, 1e-10) and dua_after <= max(dua_before, 1e-10); reasons 0-3 as above.  The host decides
 * once per round, on four counters of the revision.  With repair_iter 0 the answer is miosqp_qp_polish's bit for bit,
 * plus `stop` from one revision.  After reason 1 in round 0 nothing is revised (rounds 0, stop 0).
 * Errors: those of miosqp_qp_polish; MIOSQP_EARG also for repair_iter outside 0..20. */
typedef struct miosqp_polish_repair_info {
  miosqp_polish_info polish;   /* of the point the loop ended with; n_lower / n_upper of the final set */
  int32_t rounds;              /* repair rounds run (0 .. repair_iter), one that stopped on a bad pivot included */
  int32_t stop;                /* 0 fixed point, 1 round limit, 2 bad pivot in a repair round */
  int32_t n_added, n_dropped;  /* summed over the revisions */
  int32_t accepted0, reason0;  /* what round 0 alone would have answered */
} miosqp_polish_repair_info;

int miosqp_qp_polish_repair(miosqp_qp_engine *e, const double *l, const double *u, const double *x, const double *y,
                            double delta, int32_t refine_iter, int32_t repair_iter, double *x_out, double *y_out,
                            miosqp_polish_repair_info *info);

/* of the last miosqp_qp_polish_repair call: cls (M) the class of every row in the final set (-1 lower-active, 1
 * upper-active, 0 inactive); round_seconds (21) the device seconds of round 0, 1, .. up to the revision's counters;
 * wait_seconds (21) the host's wait for them.  Entries of rounds not run are zero; any pointer may be NULL.
 * (miosqp_qp_get_polish_stages reports round 0's stages after such a call.) */
int miosqp_qp_get_polish_repair_trace(miosqp_qp_engine *e, int8_t *cls, double *round_seconds, double *wait_seconds);

/* ---- polishing of many small instances in one launch -----------------------------------------------------------
 * The polish of the MPC re-solve pattern (/root/reference/miosqp/solver.py:174-212 per MIQP,
 * examples/power_converter/power_converter.py:467-476 per sampling step; `polish` reaches OSQP through qp_settings,
 * /root/reference/miosqp/workspace.py:67-68): B instances on this engine's P and A, each with its own linear cost and
 * bounds, polished side by side.  OSQP has NO batched polish (osqp_polish of OSQP 0.6.x works on one workspace), and no
 * repair loop either.
 * All arrays are instance-major: q, x, x_out B x n; l, u, y, y_out B x M; info B records.  q == NULL: the engine's
 * current linear cost for every instance.  Per instance b the answer is what miosqp_qp_polish_repair gives after
 * miosqp_qp_update_lin_cost(q_b): the same classification rule, the same S built in the same order, 1 + refine_iter
 * solves against the unregularised system, the same revision (tol 1e-10), stops 0 / 1 / 2, the kept point after a bad
 * pivot in a repair round, the same acceptance test and reasons 0-3, accepted0 / reason0, and the input bit for bit on
 * rejection.  Only the order of the sums differs (one workgroup owns an instance from start to finish: S is factorised
 * by a textbook LDL^T in LDS and solved by substitution, and the rounds run inside the launch with no host decision):
 * integer fields are equal wherever no comparison sits on a tie.  repair_iter 0 is the plain polish plus one revision.
 * An instance's answer has the same bits whatever B is and wherever it sits in the batch.  device_time / run_time in
 * every record are the call's totals.
 * The engine's q, bounds, iterates and the single polish's scratch are not touched.
 * MIOSQP_EARG: B < 1, delta <= 0, refine_iter outside 0..10, repair_iter outside 0..20, a NaN anywhere in q, l, u, x, y;
 * MIOSQP_EBOUNDS: l > u in any instance (nothing is computed); MIOSQP_EUNSUPPORTED: the reduced system and the rows of
 * A do not fit one workgroup's 160 KB of LDS -- every n + M <= 192 fits, which is everything miosqp_qp_solve_tree(s)
 * takes. */
int miosqp_qp_polish_many(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u,
                          const double *x, const double *y, double delta, int32_t refine_iter, int32_t repair_iter,
                          double *x_out, double *y_out, miosqp_polish_repair_info *info);

/* of the last miosqp_qp_polish_many call: cls (M) the class of every row of instance b in its final set (-1
 * lower-active, 1 upper-active, 0 inactive).  MIOSQP_EARG when that call had no instance b. */
int miosqp_qp_get_polish_many_classes(miosqp_qp_engine *e, int32_t b, int8_t *cls);

/* ---- polishing of many larger instances in one launch ----------------------------------------------------------
 * miosqp_qp_polish_many beyond one workgroup's LDS: the same MPC re-solve pattern
 * (/root/reference/miosqp/solver.py:174-212, examples/power_converter/power_converter.py:467-476; `polish` reaches OSQP
 * through qp_settings, /root/reference/miosqp/workspace.py:67-68) for the problems the lock-step trees of solve_many
 * were written for.  OSQP has NO batched polish and no repair loop.
 * Arguments, validation, error codes, records, the meaning of q == NULL and the guarantee that the engine is not touched
 * are those of miosqp_qp_polish_many, and per instance the contract is the same, step for step: the classification
 * rule, S = P + delta I + A_act^T A_act / delta, an LDL^T that stops at the first pivot with !(d > 0), 1 + refine_iter
 * solves against the unregularised system, the revision at tol 1e-10, stops 0 / 1 / 2 with the kept point of the round
 * before a bad pivot, the acceptance test and reasons 0-3, accepted0 / reason0, the input bit for bit on rejection.
 * One workgroup owns an instance from classification to record; S (n x ld) and the work vectors live in that
 * workgroup's slab of device scratch, A is read from the sparse unscaled rows, the factorisation is blocked (panels of
 * 32 factorised in LDS, the trailing update streams S) and so are the substitutions.  W = min(B, 2 x the compute
 * units, 1 GiB / slab) workgroups are launched; workgroup w takes instances w, w + W, ..  Slabs and pinned blocks are
 * allocated on first use, grown on demand and freed with the engine.  Every sum has a fixed order: an instance's answer
 * has the same bits whatever B is, wherever it sits in the batch and whichever slab it lands in.  It need not have
 * miosqp_qp_polish_many's or miosqp_qp_polish_repair's bits: only the order of the sums differs.
 * There is no lower size limit.  MIOSQP_EUNSUPPORTED: n > 512 or M > 65536 (nothing is allocated). */
int miosqp_qp_polish_many_large(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u,
                                const double *x, const double *y, double delta, int32_t refine_iter, int32_t repair_iter,
                                double *x_out, double *y_out, miosqp_polish_repair_info *info);

/* of the last miosqp_qp_polish_many_large call, as miosqp_qp_get_polish_many_classes */
int miosqp_qp_get_polish_many_large_classes(miosqp_qp_engine *e, int32_t b, int8_t *cls);

/* ---- a whole tree search in one launch (small problems) ------------------------------------------------
 * the MPC re-solve path (/root/reference/miosqp/solver.py:65-172 per MIQP,
 * examples/power_converter/power_converter.py:421-508 per sampling step).  For problems the LDS-resident solver
 * handles, the loop `while can_continue: choose_leaf -> Node.solve -> bound_and_branch` runs inside ONE launch of
 * one workgroup with the host logic's exact decisions (miosqp_amd/csrc/kernels_tree.inc); the host sends the root
 * and gets the incumbent back.  Returns MIOSQP_EUNSUPPORTED when the problem is too large for that form. */
typedef struct miosqp_tree_info {
  int32_t nodes;        /* nodes visited = iter_num - 1 */
  int32_t osqp_iter;    /* ADMM iterations over all of them */
  int32_t leaves_left;  /* open leaves when the loop ended (0: the tree is closed) */
  int32_t overflow;     /* 1: more than 1024 leaves alive -- the result is not usable, redo on the host */
  int32_t max_leaves;
  int32_t found;        /* 1: an incumbent was found in this launch (x_out holds it) */
  double upper_glob, lower_glob;
  double device_time, run_time;
} miosqp_tree_info;

/* l, u, x0, y0: the root node (M, M, n, M doubles); upper0 / x_inc0: incumbent from MIOSQP.set_x0 (x_inc0 NULL or
 * upper0 >= 1.7e308: none); tree_explor_rule, max_iter_bb: the B&B settings; branching_rule 0 is implied.
 * tree_explor_rule: 0 depth first (the first deepest leaf); 1 the reference's default (depth first until an incumbent
 * exists, then the leaf with the LARGEST inherited bound); 2 best bound: the open leaf with the SMALLEST inherited bound
 * (the root's is -inf); 3 depth first until an incumbent exists -- x_inc0 counts from the first node --, then best bound.
 * Ties go to the first leaf in list order under every rule (two siblings share their parent's bound, so under best bound
 * ties are the normal case and this rule decides the tree); the rest of the list keeps its order.  Any other value:
 * MIOSQP_EARG.  Under rule 2 many more leaves are alive at once than under depth first: info->overflow (more than 1024)
 * is to be expected more often, and means what it always meant -- redo on the host. */
int miosqp_qp_solve_tree(miosqp_qp_engine *e, const double *l, const double *u, const double *x0, const double *y0,
                         double upper0, const double *x_inc0, int32_t tree_explor_rule, int32_t max_iter_bb,
                         double *x_out, miosqp_tree_info *info);

/* B independent MIQPs that share P and A -- hence the factor -- and differ in q, l, u, warm start and incumbent (the
 * reference's MPC pattern: MIOSQP.update_vectors + set_x0 + solve per instance, /root/reference/miosqp/solver.py:174-212),
 * every tree in ONE launch: workgroup (or wavefront, n + M <= 64) b runs instance b exactly as miosqp_qp_solve_tree would
 * after miosqp_qp_update_lin_cost(q_b).  All arrays are instance-major: q, x0, x_inc0, x_out B x n; l, u, y0 B x M;
 * upper0 B (>= 1.7e308: no incumbent; x_inc0 may be NULL when none has one); info B.  The engine's own linear cost and
 * bounds are not touched.  MIOSQP_EUNSUPPORTED as for miosqp_qp_solve_tree.  tree_explor_rule 0 .. 3 and the tie rule
 * as for miosqp_qp_solve_tree (rule 3: an instance with upper0 < 1.7e308 takes the best bound from its first node);
 * overflow is per instance. */
int miosqp_qp_solve_trees(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u,
                          const double *x0, const double *y0, const double *upper0, const double *x_inc0,
                          int32_t tree_explor_rule, int32_t max_iter_bb, double *x_out, miosqp_tree_info *info);

/* ---- trees of DIFFERENT models in one launch ----------------------------------------------------------
 * Which of the one-launch tree kernels takes this engine as it stands: 0 none (what miosqp_qp_solve_trees answers with
 * MIOSQP_EUNSUPPORTED or MIOSQP_EARG: no product-form factor, no integer rows or root, no integer variable, more than
 * 160 KB of LDS; also a NULL engine or a failed runtime call), 1 the one-wavefront kernel (n + M <= 64, the explicit
 * inverse passed its guard, MIOSQP_TREE_WAVE not 0), 2 the one-workgroup kernel.  The call performs what the first tree
 * launch of such an engine performs: for n + M <= 64 the explicit inverse and Kc are built if they are missing and the
 * inverse is checked (a tripped guard turns the engine to form 2 for good). */
int miosqp_qp_tree_form(miosqp_qp_engine *e);

typedef struct miosqp_models_stats {
  int32_t launches;         /* tree launches of the call: 0, 1 or 2 -- up to 3 from miosqp_qp_solve_trees_models_large -- (the cost scaling before them is not counted) */
  int32_t models_wave;      /* models run by the one-wavefront kernel (form 1) */
  int32_t models_group;     /* models run by the one-workgroup kernel (form 2) */
  int32_t pad;              /* 0; from miosqp_qp_solve_trees_models_large: models run by the reduced form (form 3) */
  int64_t lds_bytes;        /* dynamic LDS of the workgroup launches: the largest need among their models (0: no such launch) */
  double device_time;       /* seconds between the events around upload, launches and download */
  double run_time;          /* wall seconds of the call */
} miosqp_models_stats;

/* B MIQPs on B DIFFERENT engines -- each with its own P, A, shapes, factor, scalings and settings -- every tree in one
 * launch per kernel form: workgroup (or wavefront) b runs model b exactly as miosqp_qp_solve_trees(engines[b], 1, q[b], ...)
 * would, bit for bit.  It replaces B calls of miosqp_qp_solve_trees with B = 1, i.e. the reference's pattern
 * MIOSQP.update_vectors + set_x0 + solve (/root/reference/miosqp/solver.py:174-212) repeated on B different models, by one
 * upload, at most two tree launches (form 1 models, form 2 models; a form without a model launches nothing), one download
 * and one synchronisation.  One pointer per model, because shapes differ: q[b], x0[b], x_out[b] n_b doubles; l[b], u[b],
 * y0[b] M_b; upper0 B (>= 1.7e308: no incumbent); x_inc0[b] n_b doubles or NULL; tree_explor_rule[b] 0..3 and
 * max_iter_bb[b] >= 1 per model; the ADMM settings are each engine's own.  info[b] as miosqp_qp_solve_trees fills it
 * (device_time: the call's divided by B); x_out[b]: the incumbent found, else the one handed in.  No engine's own linear
 * cost or bounds are touched.
 * Refused before anything is queued, with a last_error text naming the model: B < 1 or a NULL argument, an engine listed
 * twice, a tree_explor_rule outside 0..3, max_iter_bb < 1 (MIOSQP_EARG); l > u in a root (MIOSQP_EBOUNDS); engines on
 * different devices, an engine with streaming chunks in flight (MIOSQP_EARG); an engine whose miosqp_qp_tree_form is 0
 * (MIOSQP_EUNSUPPORTED: the caller runs that model on its own).
 * Memory: the leaf stores, staging blocks and the table of per-workgroup arguments are one arena taken from the device
 * pool of engines[0], with a pinned host mirror of its staged part; both then BELONG TO THAT ENGINE: they are reused by
 * later calls that have this engine first, grow when such a call needs more, and are released by its miosqp_qp_cleanup.
 * Nothing of a call outlives it in any other engine, so the engines may be cleaned up in any order between calls.
 * The launches run on engines[0]'s stream; work queued on the other engines' streams is waited for first. */
int miosqp_qp_solve_trees_models(int32_t B, miosqp_qp_engine *const *engines, const double *const *q, const double *const *l,
                                 const double *const *u, const double *const *x0, const double *const *y0,
                                 const double *upper0, const double *const *x_inc0, const int32_t *tree_explor_rule,
                                 const int32_t *max_iter_bb, double *const *x_out, miosqp_tree_info *info,
                                 miosqp_models_stats *stats);

/* ---- ... also for models beyond one workgroup's product form (opt-in) ----------------------------------
 * The third one-launch form: one workgroup keeps the strict lower triangle of L^-1 packed in LDS (n (n - 1) / 2 doubles)
 * and iterates in REDUCED form, x~ = L^-T D^-1 L^-1 (rx + rho Abar^T wh), nu = rho (Abar x~ - wh), reading Abar from LDS
 * copies of its packed rows where they fit and from L2 otherwise (miosqp_amd/csrc/tree_reduced_body.hpp).  Its leaf list
 * has leaf_cap places (at least 2; 256 is the customary value) instead of the 1024 of the other forms: the leaf store of
 * a model costs leaf_cap x (2 n_int + n + M) doubles of the arena.
 * miosqp_qp_tree_form_large: 3 when this engine has integer rows, the root, the digest, the product-form rows on the
 * device, an integer variable, an LDS need of the reduced form within 160 KB, AND miosqp_qp_tree_form answers 0 -- an
 * engine that fits form 1 or 2 keeps it; else 0.
 * miosqp_qp_solve_trees_models_large: miosqp_qp_solve_trees_models for engines of forms 1, 2 and 3 in one call -- at
 * most three launches (wave, group, reduced), the same arena, ownership by engines[0], one upload, one download, one
 * synchronisation.  A form 1 or 2 model gets bit for bit what miosqp_qp_solve_trees_models gives it.  A form 3 model's
 * decisions are those of the host logic; its sums run in another order than the sequential path's, so its values agree
 * with that path's to rounding, and they do not depend on B, on the model's position or on its neighbours.  stats->pad
 * holds the number of form 3 models (miosqp_qp_solve_trees_models leaves 0 there); launches may be 3.
 * Refused as miosqp_qp_solve_trees_models refuses, and: leaf_cap < 2 (MIOSQP_EARG); an arena beyond what the device can
 * give, naming the model at which it is reached (MIOSQP_EARG) -- nothing is queued, no allocation is tried. */
int miosqp_qp_tree_form_large(miosqp_qp_engine *e, int32_t leaf_cap);
int miosqp_qp_solve_trees_models_large(int32_t B, miosqp_qp_engine *const *engines, const double *const *q, const double *const *l,
                                       const double *const *u, const double *const *x0, const double *const *y0,
                                       const double *upper0, const double *const *x_inc0, const int32_t *tree_explor_rule,
                                       const int32_t *max_iter_bb, int32_t leaf_cap, double *const *x_out,
                                       miosqp_tree_info *info, miosqp_models_stats *stats);

/* ---- ... with round and fix inside the one-launch trees (opt-in) ----------------------------------------
 * The primal heuristic of Workspace.primal_heuristic / Workspace.round_and_fix (miosqp_amd/bnb.py) inside the tree launch:
 * a tree counts the nodes it is about to branch, and on every rf_every-th of them (the first included), after the node's
 * own rounding heuristic has updated the incumbent and pruned, the workgroup solves rf_candidates copies of the node with
 * every integer row fixed to min(max(floor(x_i + theta_k), lo), hi), theta_k = (k + 1) / (rf_candidates + 1), lo / hi the
 * node's bounds, x the node's clamped solution -- warm-started from the node, at most rf_max_iter iterations each, the
 * node's termination test.  A candidate with an x (solved or at its cap) whose rounded point keeps the ROOT's rows within
 * eps_abs is feasible; the feasible candidate of lowest objective below the incumbent's, ties to the lowest k, becomes the
 * incumbent (its value is the device's sum) and the list is pruned; then the node branches as without the heuristic.
 * The semantics are those of miosqp_qp_round_and_fix and miosqp_qp_solve_trees_lockstep_rf; the kernels are k_tree_rf,
 * k_tree_rf_m and k_tree_rf_r_m (miosqp_amd/csrc/kernels_tree.inc), which need no LDS beyond their plain forms: every
 * engine those take is taken.  There is no one-wavefront form with the heuristic: n + M <= 64 runs in the workgroup form.
 * info->osqp_iter counts the nodes' iterations only; the heuristic's are in the record below. */
typedef struct miosqp_tree_rf_info {
  int32_t calls;       /* firings of the heuristic (what rf_stats['calls'] counts) */
  int32_t candidates;  /* candidates solved: calls x rf_candidates */
  int32_t feasible;    /* candidates with an x whose rounded point keeps the root's rows */
  int32_t improved;    /* firings that replaced the incumbent */
  int32_t osqp_iter;   /* ADMM iterations of all candidates */
  int32_t form;        /* the launch that ran the tree: 1 wave, 2 group, 3 reduced, 4 group with round and fix, 5 reduced with it */
  int32_t pad0, pad1;
} miosqp_tree_rf_info;

/* miosqp_qp_solve_trees with the heuristic in every tree (Workspace.primal_heuristic): rf_candidates in 1..32,
 * rf_max_iter >= 1, rf_every >= 1 (MIOSQP_EARG otherwise, before anything is queued); rf_info B records, per instance. */
int miosqp_qp_solve_trees_rf(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u,
                             const double *x0, const double *y0, const double *upper0, const double *x_inc0,
                             int32_t tree_explor_rule, int32_t max_iter_bb, int32_t rf_candidates, int32_t rf_max_iter,
                             int32_t rf_every, double *x_out, miosqp_tree_info *info, miosqp_tree_rf_info *rf_info);

/* miosqp_qp_solve_trees_models_large with the heuristic per model (Workspace.primal_heuristic): rf_candidates[b] in
 * 0..32 -- 0: the heuristic is off for model b, which goes into the launch it goes into without this entry and gets that
 * result bit for bit --, rf_max_iter[b] >= 1, rf_every[b] >= 1 (read for every model; MIOSQP_EARG naming the model
 * otherwise, before anything is queued).  The models with the heuristic form up to two more launches behind the other
 * three: the workgroup form (forms 1 and 2 of miosqp_qp_tree_form) and the reduced form (form 3); such a model gets bit
 * for bit what miosqp_qp_solve_trees_rf(engines[b], 1, ...) gives it where that entry takes it.  leaf_cap: 0 keeps the
 * reduced forms out (an engine of miosqp_qp_tree_form 0 is MIOSQP_EUNSUPPORTED, as in miosqp_qp_solve_trees_models), else
 * at least 2.  rf_info[b]: the counters and the launch that ran model b (zeros and form 1..3 with the heuristic off).
 * stats: models_wave, models_group and pad count the models of the three plain launches; launches may be 5. */
int miosqp_qp_solve_trees_models_rf(int32_t B, miosqp_qp_engine *const *engines, const double *const *q, const double *const *l,
                                    const double *const *u, const double *const *x0, const double *const *y0,
                                    const double *upper0, const double *const *x_inc0, const int32_t *tree_explor_rule,
                                    const int32_t *max_iter_bb, int32_t leaf_cap, const int32_t *rf_candidates,
                                    const int32_t *rf_max_iter, const int32_t *rf_every, double *const *x_out,
                                    miosqp_tree_info *info, miosqp_tree_rf_info *rf_info, miosqp_models_stats *stats);

/* ---- ... with strong or reliability branching inside the one-launch trees (opt-in) ----------------------
 * The branching rules 1 and 2 of Workspace.select_branching (miosqp_amd/bnb.py) inside the tree launch: a node that is
 * about to branch builds its fractional set with eps_int_feas and, as candidates, the sb_candidates positions of largest
 * |x - rint(x)| (ties to the lower position, ascending) -- under rule 2 among the positions with fewer than
 * sb_reliability observations in one direction only.  Its workgroup then solves the 2K children, K down and then K up,
 * one after the other: the node with ONE integer row changed (down: u = floor(x_c), up: l = ceil(x_c)), warm-started
 * from the node, at most sb_max_iter iterations, the node's termination test; a child with an x (solved or at its cap)
 * has the objective of its clamped x as its value.  Scores are max(gain, sb_eps) * max(gain, sb_eps) with a gain of
 * 1e30 for a child without a value, the first maximum wins.  Rule 1 branches on that candidate (one fractional position:
 * nothing is solved).  Rule 2 keeps pseudo-costs PER TREE, starting empty: the children's gains are recorded in
 * candidate order, down then up; a node made by a branching records its own solve's gain when it has an x, before it is
 * judged; the position is the first maximum over ALL fractional positions, scored by strong branching where solved and
 * by pseudo-costs (numpy's pairwise mean for positions without observations) otherwise.  The semantics are those of
 * miosqp_qp_strong_branch and miosqp_qp_solve_trees_lockstep_sb; the kernels are k_tree_sb, k_tree_sb_m and
 * k_tree_sb_r_m (miosqp_amd/csrc/kernels_tree.inc), which need no LDS beyond their plain forms: every engine those take
 * is taken.  There is no one-wavefront form with a rule: n + M <= 64 runs in the workgroup form.  info->osqp_iter counts
 * the nodes' iterations only; the children's are in the record below. */
typedef struct miosqp_tree_sb_info {
  int32_t calls;      /* strong-branching calls (what sb_stats['calls'] counts) */
  int32_t children;   /* children solved: 2 x candidates per call */
  int32_t osqp_iter;  /* ADMM iterations of all children */
  int32_t form;       /* the launch that ran the tree: 1 wave, 2 group, 3 reduced, 6 group with the rule, 7 reduced with it */
  int32_t pad0, pad1, pad2, pad3;
} miosqp_tree_sb_info;

/* miosqp_qp_solve_trees with the rule in every tree (Workspace.select_branching): branching_rule 1 or 2, sb_candidates in
 * 1..32, sb_max_iter >= 1, sb_reliability >= 0, sb_eps > 0 (MIOSQP_EARG otherwise, before anything is queued); sb_info B
 * records, per instance. */
int miosqp_qp_solve_trees_sb(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u,
                             const double *x0, const double *y0, const double *upper0, const double *x_inc0,
                             int32_t tree_explor_rule, int32_t max_iter_bb, int32_t branching_rule, int32_t sb_candidates,
                             int32_t sb_max_iter, int32_t sb_reliability, double sb_eps, double *x_out, miosqp_tree_info *info,
                             miosqp_tree_sb_info *sb_info);

/* miosqp_qp_solve_trees_models_large with the rule per model (Workspace.select_branching): branching_rule[b] in 0..2 --
 * 0: "none", model b branches on the most fractional position, goes into the launch it goes into without this entry
 * and gets that result bit for bit (its other four values are not read) --, else sb_candidates[b] in 1..32,
 * sb_max_iter[b] >= 1, sb_reliability[b] >= 0, sb_eps[b] > 0 (MIOSQP_EARG naming the model otherwise, before anything is
 * queued).  The models with a rule form up to two more launches behind the others: the workgroup form (forms 1 and 2 of
 * miosqp_qp_tree_form) and the reduced form (form 3); such a model gets bit for bit what
 * miosqp_qp_solve_trees_sb(engines[b], 1, ...) gives it where that entry takes it.  leaf_cap: 0 keeps the reduced forms
 * out (an engine of miosqp_qp_tree_form 0 is MIOSQP_EUNSUPPORTED), else at least 2.  sb_info[b]: the counters and the
 * launch that ran model b (zeros and form 1..3 without a rule).  stats: models_wave, models_group and pad count the
 * models of the three plain launches; launches may be 5. */
int miosqp_qp_solve_trees_models_sb(int32_t B, miosqp_qp_engine *const *engines, const double *const *q, const double *const *l,
                                    const double *const *u, const double *const *x0, const double *const *y0,
                                    const double *upper0, const double *const *x_inc0, const int32_t *tree_explor_rule,
                                    const int32_t *max_iter_bb, int32_t leaf_cap, const int32_t *branching_rule,
                                    const int32_t *sb_candidates, const int32_t *sb_max_iter, const int32_t *sb_reliability,
                                    const double *sb_eps, double *const *x_out, miosqp_tree_info *info,
                                    miosqp_tree_sb_info *sb_info, miosqp_models_stats *stats);

/* ---- many MIQPs on ONE model beyond one workgroup's product form (opt-in) -----------------------------
 * miosqp_qp_solve_trees for an engine whose miosqp_qp_tree_form is 0 and whose miosqp_qp_tree_form_large(e, leaf_cap) is
 * 3: B MIQPs that share P, A (the factor) and differ in q, l, u, warm start and incumbent, workgroup b running tree b in
 * the reduced form with a leaf list of leaf_cap places -- arguments and layouts as miosqp_qp_solve_trees.  It replaces,
 * for such a model, what the reference does one MIQP after the other (update_vectors + solve per instance,
 * miosqp/solver.py:174-212) and what this library offered so far: miosqp_qp_solve_trees_lockstep (a batch per wave of
 * nodes), or miosqp_qp_solve_trees_models_large over B separately set-up copies of the model (that entry refuses an engine
 * listed twice).  Everything read per model -- the rows the triangle of L^-1 is loaded from, the packed and dense rows of
 * Abar, Pbar's rows, D, E, c -- is the engine's own and shared by all workgroups; per instance the call keeps
 * leaf_cap x (2 n_int + n + M) doubles of leaf store, the staging block, q, the incumbent and the outcome in an arena of
 * the engine (miosqp_amd/csrc/trees_large_plan.hpp).  Instance b comes out bit for bit as
 * miosqp_qp_solve_trees_models_large(1, &e, ..., leaf_cap, ...) gives it alone, whatever B is.
 * One upload, the cost scaling, one tree launch, one download, one synchronisation.
 * Refused before anything is queued: what miosqp_qp_solve_trees refuses (MIOSQP_EARG); leaf_cap < 2 (MIOSQP_EARG); an
 * engine with miosqp_qp_tree_form_large(e, leaf_cap) != 3 -- one of form 1 or 2 keeps miosqp_qp_solve_trees --
 * (MIOSQP_EUNSUPPORTED); l > u in a root (MIOSQP_EBOUNDS); arrays whose size does not fit an address, or beyond what
 * hipMemGetInfo leaves on the device (MIOSQP_EARG, the text names B and the bytes; no allocation is tried).
 * info[b].overflow: the tree needed more than leaf_cap leaves at once and stopped; the caller redoes that instance. */
int miosqp_qp_solve_trees_large(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u,
                                const double *x0, const double *y0, const double *upper0, const double *x_inc0,
                                int32_t tree_explor_rule, int32_t max_iter_bb, int32_t leaf_cap, double *x_out,
                                miosqp_tree_info *info);

/* miosqp_qp_solve_trees_large with round and fix in every tree: miosqp_qp_solve_trees_rf for such an engine (it replaces
 * miosqp_qp_solve_trees_lockstep_rf there, or miosqp_qp_solve_trees_models_rf over copies of the model).  rf_candidates in
 * 1..32, rf_max_iter >= 1, rf_every >= 1 (MIOSQP_EARG otherwise, before anything is queued); rf_info B records, per
 * instance (form 5), equal to those of miosqp_qp_solve_trees_models_rf for the instance alone. */
int miosqp_qp_solve_trees_large_rf(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u,
                                   const double *x0, const double *y0, const double *upper0, const double *x_inc0,
                                   int32_t tree_explor_rule, int32_t max_iter_bb, int32_t leaf_cap, int32_t rf_candidates,
                                   int32_t rf_max_iter, int32_t rf_every, double *x_out, miosqp_tree_info *info,
                                   miosqp_tree_rf_info *rf_info);

/* miosqp_qp_solve_trees_large with strong (1) or reliability branching (2) in every tree: miosqp_qp_solve_trees_sb for such
 * an engine (it replaces miosqp_qp_solve_trees_lockstep_sb there, or miosqp_qp_solve_trees_models_sb over copies of the
 * model).  branching_rule 1 or 2, sb_candidates in 1..32, sb_max_iter >= 1, sb_reliability >= 0, sb_eps > 0 (MIOSQP_EARG
 * otherwise, before anything is queued); per instance the arena also holds the rule's work area and leaf_cap x 4 doubles
 * of Node.pc; sb_info B records, per instance (form 7), equal to those of miosqp_qp_solve_trees_models_sb for the
 * instance alone. */
int miosqp_qp_solve_trees_large_sb(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u,
                                   const double *x0, const double *y0, const double *upper0, const double *x_inc0,
                                   int32_t tree_explor_rule, int32_t max_iter_bb, int32_t leaf_cap, int32_t branching_rule,
                                   int32_t sb_candidates, int32_t sb_max_iter, int32_t sb_reliability, double sb_eps,
                                   double *x_out, miosqp_tree_info *info, miosqp_tree_sb_info *sb_info);

/* ---- polishes of DIFFERENT models in one launch -------------------------------------------------------
 * The polish of the "own P and A per MIQP" pattern: the reference sets up, solves and polishes one model per MIQP
 * (miosqp/solver.py:174-212 per model; `polish` reaches OSQP through qp_settings, miosqp/workspace.py:67-68), and
 * miosqp_qp_solve_trees_models returns B incumbents of B different engines from one call.  This entry polishes them in
 * one call as well: workgroup b runs model b exactly as miosqp_qp_polish_many(engines[b], 1, q[b], ...) would with the
 * same y -- info[b], x_out[b], y_out[b] and cls_out[b] bit for bit, whatever B is and wherever the model sits in the
 * list (the kernel's sums depend on (n, M) and the data alone); only device_time / run_time differ: in every record
 * they are the call's totals.  OSQP has NO batched polish and no repair loop.
 * One pointer per model, because shapes differ: q[b], x[b], x_out[b] n_b doubles; l[b], u[b], y[b], y_out[b] M_b;
 * cls_out[b] M_b bytes, the class of every row in the final set (-1 lower-active, 1 upper-active, 0 inactive), and
 * cls_out or any cls_out[b] may be NULL; delta, refine_iter, repair_iter one per model.  q[b] NULL: engines[b]'s current
 * linear cost.  y[b] NULL: a tree returns no multipliers, so the workgroup guesses them from the z = A x it computes
 * anyway, before it classifies -- y_r = 0 where l_r == u_r or both bounds are at or beyond +-1e30, otherwise -tau where
 * z_r - l_r < u_r - z_r, otherwise +tau (needs tau > 0) --, and that guess is the y a rejection returns.
 * One upload, ONE launch, one download and one synchronisation, all on engines[0]'s stream; work queued on the other
 * engines' streams is waited for first.  No engine's q, bounds, iterates or polish scratch is touched, and none is
 * built: nothing is allocated per engine.  The table of per-workgroup arguments, the unscaled rows of A by constraint,
 * the vectors and the output records are one arena [table | per model: rows of A, q, l, u, x, y | per model: record]
 * taken from the device pool of engines[0], with a pinned host mirror -- the arena of miosqp_qp_solve_trees_models, with
 * the same ownership: it belongs to that engine, is reused and grown by later calls that have it first, and is released
 * by its miosqp_qp_cleanup.  Nothing of a call outlives it in any other engine, so the engines may be cleaned up in any
 * order between calls.
 * Refused before anything is queued, with a last_error text naming the model: B < 1 or a NULL argument, an engine
 * listed twice, delta <= 0, refine_iter outside 0..10, repair_iter outside 0..20, a NaN in q, l, u, x or y, y[b] NULL
 * with tau not positive, engines on different devices, an engine with streaming chunks in flight (MIOSQP_EARG); l > u
 * (MIOSQP_EBOUNDS); a model whose reduced system and rows of A exceed one workgroup's 160 KB of LDS -- every
 * n + M <= 192 fits, which is everything miosqp_qp_solve_trees_models takes --, or whose rows on the device do not
 * follow the set-up's order (MIOSQP_EUNSUPPORTED: the caller polishes that model on its own). */
typedef struct miosqp_polish_models_stats {
  int32_t launches;         /* 1; 0 after a refusal that came later than the argument checks */
  int32_t models;           /* B */
  int64_t lds_bytes;        /* dynamic LDS of the launch: the largest need among its models */
  int64_t arena_bytes;      /* what this call uses of the arena */
  double device_time;       /* seconds between the events around upload, launch and download */
  double run_time;          /* wall seconds of the call once the arena exists */
  double upload_time, launch_time, download_time; /* device_time by part: the events after the upload and after the launch */
} miosqp_polish_models_stats;

int miosqp_qp_polish_models(int32_t B, miosqp_qp_engine *const *engines, const double *const *q, const double *const *l,
                            const double *const *u, const double *const *x, const double *const *y, double tau,
                            const double *delta, const int32_t *refine_iter, const int32_t *repair_iter, double *const *x_out,
                            double *const *y_out, int8_t *const *cls_out, miosqp_polish_repair_info *info,
                            miosqp_polish_models_stats *stats);

/* 1 when miosqp_qp_polish_models takes this engine's sizes (the reduced system and the rows of A within one workgroup's
 * 160 KB of LDS), 0 otherwise or for a NULL engine: what a caller asks before it puts a model into the list. */
int miosqp_qp_polish_models_fits(miosqp_qp_engine *e);

/* ---- ... also for models beyond one workgroup's LDS (opt-in) -------------------------------------------
 * The third leg of the "own P and A per MIQP" pattern for the models miosqp_qp_polish_models does not take (more than
 * 160 KB of LDS, or M > 256: of the reference benchmark's grid (100,200,15), (150,100,5), (150,300,20); the reference polishes
 * per model through qp_settings, miosqp/workspace.py:67-68, after miosqp/solver.py:174-212).  miosqp_qp_polish_models_large is
 * miosqp_qp_polish_models with the kernel of miosqp_qp_polish_many_large in table-driven form (k_pol_many_gm): W
 * workgroups, W = min(B, two per compute unit, 1 GiB / the largest slab), workgroup w polishes models w, w + W, .. one
 * after the other, each from classification to record in slab w of device scratch, which is sized for the largest model
 * of the call.  Model b is exactly what miosqp_qp_polish_many_large(engines[b], 1, q[b], ...) answers with the same y --
 * info[b], x_out[b], y_out[b], cls_out[b] bit for bit, whatever B and W are and wherever the model sits (the kernel's
 * sums depend on (n, M) and the data alone; no floating-point atomics); device_time / run_time are the call's totals.
 * The arguments are those of miosqp_qp_polish_models: q[b] NULL is engines[b]'s current cost, y[b] NULL the device's
 * guess by the same rule (0 on equality and free rows, otherwise -tau / +tau by the nearer bound; needs tau > 0), which
 * is written to the record's y slot, so a rejection returns it.  It takes every engine form miosqp_qp_polish_many_large
 * takes -- the cooperative grid, the product form of miosqp_qp_setup_models_large, and small models as well.
 * One upload, ONE launch, one download, one synchronisation on engines[0]'s stream; work queued on the other engines'
 * streams is waited for first.  No engine's polish scratch is built or touched: the arena is
 * [table | per model: rows of A by constraint, rows of A^T by variable, q, l, u, x, y | per model: record | W slabs],
 * the arena of miosqp_qp_solve_trees_models with the same ownership (engines[0]'s, released by its miosqp_qp_cleanup);
 * the slabs are device-only and take no room in the pinned mirror.  An engine that already holds the single polish's
 * scratch lends its two copies of A instead.
 * Refused before anything is queued exactly as miosqp_qp_polish_models refuses, in the same order, the text naming the
 * model; MIOSQP_EUNSUPPORTED (the caller polishes that model on its own) for a model beyond the slab limits -- n > 512,
 * M > 65536 or one slab beyond the budget -- or whose rows on the device do not follow the set-up's order.
 * miosqp_qp_polish_models_large_fits: 1 when the entry takes this engine's sizes, 0 otherwise or for a NULL engine. */
typedef struct miosqp_polish_models_large_stats {
  int32_t launches, models, workgroups, pad; /* 1 (0 after a late refusal), B, W, 0 */
  int64_t slab_bytes;   /* one workgroup's slab */
  int64_t arena_bytes;  /* staged parts + records + slabs */
  double device_time, run_time, upload_time, launch_time, download_time; /* as in miosqp_polish_models_stats */
} miosqp_polish_models_large_stats;

int miosqp_qp_polish_models_large(int32_t B, miosqp_qp_engine *const *engines, const double *const *q, const double *const *l,
                                  const double *const *u, const double *const *x, const double *const *y, double tau,
                                  const double *delta, const int32_t *refine_iter, const int32_t *repair_iter,
                                  double *const *x_out, double *const *y_out, int8_t *const *cls_out,
                                  miosqp_polish_repair_info *info, miosqp_polish_models_large_stats *stats);
int miosqp_qp_polish_models_large_fits(miosqp_qp_engine *e);

/* ---- set-up of many small models in ONE launch -----------------------------------------------------------
 * What the reference does once per MIQP with osqp.OSQP().setup() (/root/reference/miosqp/workspace.py:63-68), for B
 * models with their own P and A at once: the equilibration and the row packing stay on the host, per model, exactly as
 * miosqp_qp_setup does them; the whole dense part -- S = Pbar + sigma I + rho Abar^T Abar, its LDL^T, Linv / LinvT /
 * d2inv, the product form (f_rows, f_GmT, f_Ad, f_Atd, f_Pd), the explicit inverse W, Kc, the guard residual, the scaled
 * bounds and the control block -- is ONE launch, one workgroup per model (k_setup_models).  One upload, one launch, one
 * download, one synchronisation per call.
 * The engines of one call form a GROUP: they share one stream, one device arena (zero-filled once on that stream, ahead
 * of the upload) and one pinned slab, carved into each engine's staging buffers; each engine keeps events of its own.
 * miosqp_qp_cleanup of such an engine releases what is its own and drops one reference; the last one frees the group
 * (its stream, arena and slab, when none is above 32 MB, wait for the next call of the process instead of being destroyed:
 * one set at most, in a cache of their own; MIOSQP_NO_CACHE switches that off like the other caches).
 * The engines may be cleaned up in any order and at any time.  What an engine allocates later beyond the room its slice
 * of the arena keeps (the arrays of miosqp_qp_set_integer_rows fit) comes from a chunk of its own, as for every engine.
 * The returned engines are ready for every entry of this header and behave as engines of miosqp_qp_setup in the
 * LDS-resident form with the explicit inverse; the products agree with that set-up to rounding (not bit for bit: the order
 * of the sums in the factorisation differs), the scalings, the scaled cost and bounds, f_Ad, f_Atd, f_Pd and Kc bit for bit.
 * A model whose inverse fails the guard stays on the product form, as in miosqp_qp_setup. */
typedef struct miosqp_setup_model {
  int32_t n, M;                  /* variables, rows */
  const int32_t *Pp, *Pi;        /* P, CSC, upper triangle read; row indices strictly ascending within a column */
  const double *Px;
  const int32_t *Ap, *Ai;        /* A, CSC; row indices strictly ascending within a column (no entry twice) */
  const double *Ax;
  const double *q, *l, *u;       /* n, M, M */
  const miosqp_qp_settings *settings;
  int32_t n_int, m_orig;         /* n_int >= 0: miosqp_qp_set_integer_rows(e, n_int, i_idx, m_orig) is applied; < 0: not */
  const int32_t *i_idx;
  const double *l_root, *u_root; /* non-NULL (with integer rows): miosqp_qp_set_root(e, l_root, u_root, eps_int_feas, eps_lin) */
  double eps_int_feas, eps_lin;
} miosqp_setup_model;

typedef struct miosqp_setup_models_stats {
  int32_t models;           /* B */
  int32_t launches;         /* kernel launches of the dense set-up: 1 */
  int32_t device_mallocs;   /* hipMalloc calls of the call: 1 (the arena), whatever B is; 0 when the objects of a freed */
  int32_t host_mallocs;     /* hipHostMalloc calls: 1 (the slab)      group of this process were large enough and are */
  int32_t streams;          /* streams created: 1                     used again (at most one set waits, <= 32 MB each) */
  int32_t reserved;
  int64_t arena_bytes, pinned_bytes;
  int64_t lds_bytes;        /* dynamic LDS of the launch: the largest model's */
  double device_time;       /* seconds between the events around upload, launch and download */
  double run_time;          /* wall seconds of the call */
} miosqp_setup_models_stats;

/* out: B engine handles, in the order of `models` (all NULL after an error).  Refused before anything is queued, with a
 * last_error text naming the model's position: B < 1, a NULL argument, n or M < 1, settings out of range, integer rows that
 * do not add up, l > u, models that ask for different devices (MIOSQP_EARG); a model the launch does not take
 * (MIOSQP_EUNSUPPORTED: see miosqp_qp_setup_models_eligible; also a P or an A with an entry twice or unsorted row indices in
 * a column -- the launch copies entries where miosqp_qp_setup sums duplicates, so such a model goes to miosqp_qp_setup).  A pivot of the LDL^T that is not positive or not finite:
 * MIOSQP_EFACTOR, the text names the model and the pivot.  After any error everything of the call has been released. */
int miosqp_qp_setup_models(int32_t B, const miosqp_setup_model *models, miosqp_qp_engine **out, miosqp_setup_models_stats *stats);
/* miosqp_qp_setup_models with settings->rho_auto = 1 accepted per model (0 and 1 may be mixed in one call; when no model
 * asks for it the call IS miosqp_qp_setup_models): the rho-once recipe of miosqp_qp_setup (engine.hip: for n + M <= 400 two
 * complete set-ups and RHO_ONCE_ITERS = 50 iterations on a throw-away engine; oracle/qp_oracle.c: rho_once) becomes a stage
 * of the launch (k_setup_models_auto).  The workgroup that builds the model runs the 50 iterations from x = z = y = 0 on the
 * factor at the starting rho it holds in LDS, applies the rule (rho_estimate, rounded to two digits by rho_round2) and,
 * where the rule moves rho, builds the factor again at the chosen value; every product and the panel's values are those of
 * the chosen rho.  Still one upload, one launch, one download, one synchronisation.  The chosen rho agrees with
 * miosqp_qp_setup's wherever the rule's value is not within rounding of a two-digit boundary; the engine reports it through
 * miosqp_qp_get_rho and keeps rho_auto = 1 in its settings.  Every shape miosqp_qp_setup_models takes is taken.  A pivot that
 * is not positive in either factor fails the whole call with MIOSQP_EFACTOR; for the second factor the text names the
 * chosen rho as well. */
int miosqp_qp_setup_models_auto(int32_t B, const miosqp_setup_model *models, miosqp_qp_engine **out,
                                miosqp_setup_models_stats *stats);
/* 1 when the launch takes a model of this shape under these settings and this environment, else 0: n + M <= 192 with the
 * kernel's LDS within 160 KB, and everything under which miosqp_qp_setup would choose the LDS-resident form with the product
 * form and the explicit inverse at a fixed rho -- not rho_auto, coop = 1, resident = 0, fold = 0, setup_on_device = 1,
 * MIOSQP_COOP=1 or MIOSQP_RES_W=0. */
int miosqp_qp_setup_models_eligible(int32_t n, int32_t M, const miosqp_qp_settings *settings);
/* miosqp_qp_setup_models (rho_auto_in_launch = 0) or miosqp_qp_setup_models_auto (not 0) with a SECOND launch for the models
 * that one workgroup of k_setup_models cannot hold (n + M > 192): what the reference does for such a model with
 * osqp.OSQP().setup() (/root/reference/miosqp/workspace.py:63-68), and miosqp_qp_setup one model at a time with the Schur
 * complement, the LDL^T and the inverse on one host core, build_folded, five uploads, and for the cooperative grid the
 * (n + M)^2 inverse, Kc, the guard's read-back and a dozen buffers.  k_setup_models_large builds, one workgroup per model,
 * f_Ad / f_Atd / f_Pd from the packed rows, S on the packed triangle in LDS (Abar read back from memory; entry (i1, i2) one
 * fused sum over the constraint rows ascending: the host's S bit for bit), the LDL^T and the inverse with the code of
 * k_setup_models, d2inv, Linv, LinvT, f_rows, f_GmT, the scaled bounds and the control block -- no W, no Kc, no guard.
 * Such a model comes out as the engine miosqp_qp_setup(..., coop = 0, resident = 0, fold = 1, pers = 0) builds: the product
 * form on the device, the iterations as captured chunks, valid for every entry of this header; miosqp_qp_tree_form_large
 * answers 3 for it wherever it does for that engine, and its settings say coop = 0 (whoever wants the cooperative grid for a
 * long sequential search calls miosqp_qp_setup).  Its products agree with that set-up to rounding, the dense copies and
 * the scalings bit for bit.
 * A model miosqp_qp_setup_models_eligible's size rule takes keeps the existing launch.  All models share one group; one
 * upload, at most two launches (stats->launches: 1 or 2), one download, one synchronisation.  out[b] and every "(model b)" of an error text are the caller's positions.  Refused before anything is
 * queued, beside what miosqp_qp_setup_models refuses: a large model whose shape miosqp_qp_setup_models_eligible_large does
 * not take, with settings->rho_auto = 1 (MIOSQP_EUNSUPPORTED: rho for such a model is not chosen in the launch), or with
 * coop = 1, resident = 1, fold = 0, pers > 0 or setup_on_device = 1; MIOSQP_COOP=1 or MIOSQP_PERS in the environment. */
int miosqp_qp_setup_models_large(int32_t B, const miosqp_setup_model *models, miosqp_qp_engine **out,
                                 miosqp_setup_models_stats *stats, int32_t rho_auto_in_launch);
/* 1 when the large launch takes a model of this shape under these settings and this environment, else 0: not a shape of
 * miosqp_qp_setup_models_eligible, the packed triangle of n variables, two rows and d within 160 KB of LDS (n <= 198),
 * n + M <= 2048, a fixed rho, and none of coop = 1, resident = 1, fold = 0, pers > 0, setup_on_device = 1, MIOSQP_COOP=1,
 * MIOSQP_PERS > 0.  Every (n, M) miosqp_qp_tree_form_large takes with 256 leaf places is among them. */
int miosqp_qp_setup_models_eligible_large(int32_t n, int32_t M, const miosqp_qp_settings *settings);
/* miosqp_qp_setup_models_large with settings->rho_auto = 1 accepted for the LARGE models as well (opt-in; small fixed, small
 * rho_auto with rho_auto_in_launch, large fixed and large rho_auto models may be mixed in one call; when no large model asks
 * for it the call IS miosqp_qp_setup_models_large).  It replaces what the reference does for such a model with
 * osqp.OSQP().setup(rho=..) behind its own choice of rho (miosqp/workspace.py:63-68 of the reference), and what
 * miosqp_qp_setup does with rho_auto = 1: for n + M <= 400 two complete set-ups and RHO_ONCE_ITERS = 50 iterations on a
 * throw-away engine, above that an inline probe and a second host factor.  Here the recipe is a stage of the large launch
 * (k_setup_models_large_auto): the workgroup that builds the model runs the 50 iterations from x = z = y = 0 on the first
 * factor -- L^-1 and 1 / d on the packed triangle in LDS, Abar read from f_Ad / f_Atd out of L2, the iterates in LDS behind
 * d -- applies the rule of miosqp_qp_setup_models_auto (the same code; every sum on one thread in ascending order, so the
 * chosen rho does not depend on the list around the model) and, where the rule moves rho, forms S again at the chosen value
 * with the terms of the first pass in their order, factors it and rewrites the panel's values; every product is that of
 * miosqp_qp_setup_models_large at a fixed rho equal to the chosen one, bit for bit.  Still one upload, at most two
 * launches, one download, one synchronisation.  miosqp_qp_get_rho reports the chosen rho, the settings keep rho_auto = 1.
 * Refused before anything is queued, beside what miosqp_qp_setup_models_large refuses (a large rho_auto model no longer
 * is): such a model beyond miosqp_qp_setup_models_eligible_large_auto's size rule (MIOSQP_EUNSUPPORTED, the rule and
 * "(model b)" in the text).  A pivot that is not positive in either factor fails the whole call with MIOSQP_EFACTOR; for
 * the second factor the text names the chosen rho as well. */
int miosqp_qp_setup_models_large_auto(int32_t B, const miosqp_setup_model *models, miosqp_qp_engine **out,
                                      miosqp_setup_models_stats *stats, int32_t rho_auto_in_launch);
/* miosqp_qp_setup_models_eligible_large for the large launch of miosqp_qp_setup_models_large_auto: rho_auto = 1 is
 * taken where the probing iterations' n + 3 M + 8 doubles fit the 160 KB of LDS beside the triangle, two rows and d
 * (n <= 197; every (n, M) miosqp_qp_tree_form_large takes with 256 leaf places is still among them); with rho_auto = 0 the
 * answer is miosqp_qp_setup_models_eligible_large's. */
int miosqp_qp_setup_models_eligible_large_auto(int32_t n, int32_t M, const miosqp_qp_settings *settings);
/* Any of the four entries above (chosen by `flags`: no bit is miosqp_qp_setup_models) with the host's share of a model's
 * preparation moved into the call (opt-in): the Ruiz equilibration (settings->scaling passes) and the packed rows of the
 * panel and of the two symmetric matrices.  The upload holds the RAW problem (the CSC of P as given and of A, q, l, u)
 * and the four pointer arrays of the packed structures, which the host makes from histograms of the row indices; ONE
 * more launch ahead of the set-up launch(es) on the group's stream, one workgroup of 256 threads per model
 * (k_prepare_models, prepare_models_body.hpp), packs the rows, runs the passes in place and derives D, E, c, their
 * inverses, the scaled q and the panel's values.  Everything it writes is bit for bit what the host writes (maxima,
 * correctly rounded 1 / sqrt, products, and one sum formed by one thread in ascending order), hence so is every product
 * of the set-up launches, and an engine that comes out is indistinguishable from one of the same call without this entry:
 * the host's mirrors of the scaled problem and of the rows are filled from the one download behind the launches.  Checks,
 * refusals and eligibility are those of the entry the flags name; stats->launches counts the additional launch. */
#define MIOSQP_SETUP_MODELS_RHO_AUTO 1       /* miosqp_qp_setup_models_auto / rho_auto_in_launch of the large entries */
#define MIOSQP_SETUP_MODELS_LARGE 2          /* miosqp_qp_setup_models_large */
#define MIOSQP_SETUP_MODELS_LARGE_RHO_AUTO 4 /* miosqp_qp_setup_models_large_auto (implies MIOSQP_SETUP_MODELS_LARGE) */
int miosqp_qp_setup_models_prepared(int32_t B, const miosqp_setup_model *models, miosqp_qp_engine **out,
                                    miosqp_setup_models_stats *stats, int32_t flags);
/* the SIZE rules alone, whatever the settings and the environment say: 1 a shape of miosqp_qp_setup_models (n + M <= 192),
 * 2 a shape of the large launch of miosqp_qp_setup_models_large (n <= 198, n + M <= 2048), 0 neither */
int miosqp_qp_setup_models_shape(int32_t n, int32_t M);
/* groups of miosqp_qp_setup_models that are alive in this process (engines of theirs not yet cleaned up) */
int miosqp_qp_setup_groups_live(void);
/* the group this engine belongs to (a positive number, the same for the engines of one call), 0 for an engine of miosqp_qp_setup */
int64_t miosqp_qp_setup_group(miosqp_qp_engine *e);
/* debug, beside miosqp_qp_debug_factor and with its conventions: one array of the product form as it lies in device
 * memory.  which: 0 f_rows (n x ldf: [ -G | strict lower of Linv ])   1 f_GmT (M x ldn)   2 f_Ad (M x ldn)
 * 3 f_Atd (n x ldm)   4 f_Pd (n x ldn); and the scaled vectors of the problem as the solvers read them: 5 q (n x 1)
 * 6 l (M x 1)   7 u (M x 1).  MIOSQP_EUNSUPPORTED for 0..4 on an engine without the product form. */
int miosqp_qp_debug_product_form(miosqp_qp_engine *e, int32_t which, double *out, int64_t capacity, int32_t *rows, int32_t *ld);

/* debug: the values of the factor's panel L21 = -rho Abar as stored (padding included).  which: 0 by variable and 1 by
 * constraint as they lie in device memory, 2 and 3 the host's mirror of the two.  out == NULL: only *count is set. */
int miosqp_qp_debug_panel(miosqp_qp_engine *e, int32_t which, double *out, int64_t capacity, int64_t *count);

/* ---- B trees in lock step, driven from the host in C++ on device-resident leaves -----------------------
 * miosqp_qp_solve_trees for problems of any size: the B instances of the reference's MPC pattern
 * (MIOSQP.update_vectors + set_x0 + solve per instance, /root/reference/miosqp/solver.py:174-212, each solve the loop of
 * solver.py:65-172) advance together, one node of every unfinished tree per wave, the wave being the lock-step batch with a
 * linear cost per column (what miosqp_qp_solve_batch_q runs, sliced at max_batch columns the same way).  The loop
 * `while can_continue: choose_leaf -> Node.solve -> bound_and_branch` (workspace.py:113-155, 274-334) runs per tree in
 * C++ with the list semantics of the Python mirror; the open leaves of all trees are slots of ONE device store and the
 * children are written on the device (workspace.py:157-203).  Per wave the host uploads five integers per column and
 * reads a 64-byte record per column; no vector crosses PCIe between the roots going up and the incumbents coming down.
 * Every tree makes the decisions of its own sequential solve, node for node (a node is a pure function of q, l, u, x0,
 * y0); the value of an incumbent found by the rounding heuristic is the device's sum, as in miosqp_qp_search_run.
 * The rounded point is tested against the INSTANCE's root rows (l, u of that instance), not the engine's root. */
typedef struct miosqp_lockstep_stats {
  int32_t waves;          /* waves run = the largest node count of a tree */
  int32_t max_width;      /* columns of the widest wave */
  int32_t grown;          /* times the slot store grew */
  int32_t wave_cap;       /* IN: entries the three per-wave arrays below can take (max_iter_bb suffices); later waves are not recorded */
  int64_t nodes;          /* over all trees */
  int64_t iters_slowest;  /* sum over waves of the slowest column's ADMM iterations */
  int64_t iters_all;      /* ... and of all columns' iterations */
  double device_time;     /* seconds between the events around the call (the waits for the host between waves included) */
  double run_time;        /* wall seconds */
  double host_time;       /* of those: the tree logic on the host (choosing, absorbing the records), between the waves */
  int32_t *wave_width;    /* IN, optional (NULL: not wanted): columns per wave */
  int32_t *wave_iter_max; /* IN, optional: largest iteration count per wave */
  double *wave_iter_mean; /* IN, optional: mean iteration count per wave */
  int32_t *finished_at;   /* IN, optional, B entries: the wave after which tree b was done (0: it had nothing to do) */
  double *node_hviol;     /* IN, optional debug, B x node_cap: the rounded point's violation at tree b's k-th node */
  int32_t node_cap;       /* IN: nodes per tree node_hviol can take */
  int32_t reserved;
} miosqp_lockstep_stats;

/* Arguments, layouts and meaning as for miosqp_qp_solve_trees (instance-major; upper0 >= 1.7e308: no incumbent;
 * tree_explor_rule 0 .. 3 with the first-in-list tie rule; branching_rule 0 implied).  capacity: the starting number of
 * node slots (0: max(64, 4 B), or whatever an earlier call left); the store doubles on demand.  info[b] as
 * miosqp_qp_solve_trees fills it; overflow is always 0.  The engine's own q, bounds, root and search state are neither
 * read nor written.  The per-call device data is allocated on first use, grown on demand and freed with the engine.
 * Errors: MIOSQP_EARG as for miosqp_qp_solve_trees (also while pool chunks are in flight, as for miosqp_qp_solve_batch);
 * MIOSQP_EBOUNDS for l > u in a root (nothing has been queued then) or for a branching that produced l > u;
 * MIOSQP_EFULL only when the device has no memory for the slot store. */
int miosqp_qp_solve_trees_lockstep(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u,
                                   const double *x0, const double *y0, const double *upper0, const double *x_inc0,
                                   int32_t tree_explor_rule, int32_t max_iter_bb, int32_t capacity,
                                   double *x_out, miosqp_tree_info *info, miosqp_lockstep_stats *stats);

/* ---- the lock-step trees with round and fix ---------------------------------------------------------------
 * miosqp_qp_solve_trees_lockstep with the primal heuristic of miosqp_qp_round_and_fix inside the trees: per tree the
 * decisions of its sequential solve with primal_heuristic = 1 (miosqp_amd/bnb.py: Workspace.bound_and_branch ->
 * Workspace.primal_heuristic -> Workspace.round_and_fix, between the reference's rounding heuristic, workspace.py:321-328,
 * and its branching, workspace.py:330-331).  On a solved fractional node that is not cut off, after the rounding
 * heuristic of the digest: fire = rf_nodes % rf_every == 0, rf_nodes++ -- a counter per tree, 0 at the start of the call,
 * counting exactly the nodes that get here.  The trees that fire in a wave send rf_candidates copies of their node into
 * ONE more batch (F trees, F * rf_candidates columns, sliced at max_batch like a wave; a tree's candidates may straddle
 * two slices): candidate k has the node's bounds with every integer row fixed to
 * fmin(fmax(floor(x_i + (double)(k + 1) / (double)(K + 1)), lo), hi) (rf_roundings of bnb.py), the tree's cost and the
 * node's OWN x, y as the warm start, and at most rf_max_iter iterations.  A candidate counts when its status is SOLVED
 * or MAX_ITER_REACHED and its rounded point keeps the INSTANCE's root rows; the one of lowest objective wins (ties to the
 * lowest k) and becomes the tree's incumbent when that objective is below upper_glob -- the device's sum, like the
 * rounding heuristic's here --, followed by the reference's pruning traversal (workspace.py:274-280).  Then the node's
 * two children enter the list.  Candidates are built, solved and judged on the device; per firing tree a 32-byte record
 * comes back.  A wave in which no tree fires queues nothing more than miosqp_qp_solve_trees_lockstep does. */
typedef struct miosqp_lockstep_rf_stats {
  int32_t batches;        /* heuristic batches run (waves in which at least one tree fired) */
  int32_t reserved;
  int64_t columns;        /* their columns: rf_candidates per firing tree */
  int64_t iters_slowest;  /* sum over the batches of the slowest candidate's ADMM iterations */
  double device_time;     /* seconds between the events around the batches (part of miosqp_lockstep_stats.device_time) */
  int32_t *calls;         /* IN, optional (NULL: not wanted), B entries each: times tree b fired ... */
  int32_t *candidates;    /* ... its candidates (calls * rf_candidates) ... */
  int32_t *feasible;      /* ... those that counted ... */
  int32_t *improved;      /* ... the calls that gave the tree a new incumbent ... */
  int64_t *iters;         /* ... and the candidates' ADMM iterations (info[b].osqp_iter counts node relaxations only) */
  int32_t *cand_status;   /* IN, optional debug, B x rf_candidates each: the candidates of tree b's FIRST call as the batch */
  int32_t *cand_iter;     /* epilogue left them -- status, iterations, the rounded point's objective and its worst violation */
  double *cand_obj;       /* of the instance's root rows (<= 0: feasible), what miosqp_qp_round_and_fix returns per candidate; */
  double *cand_viol;      /* rows of trees that never fired are not written */
} miosqp_lockstep_rf_stats;

/* Arguments, layouts, info[b], stats, capacity and errors as for miosqp_qp_solve_trees_lockstep.  rf_candidates in 1 .. 32;
 * rf_max_iter a positive multiple of settings.check_termination or settings.max_iter itself (the rule of
 * miosqp_qp_round_and_fix); rf_every >= 1: MIOSQP_EARG with a last_error text otherwise, nothing queued. */
int miosqp_qp_solve_trees_lockstep_rf(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u,
                                      const double *x0, const double *y0, const double *upper0, const double *x_inc0,
                                      int32_t tree_explor_rule, int32_t max_iter_bb, int32_t capacity,
                                      int32_t rf_candidates, int32_t rf_max_iter, int32_t rf_every, double *x_out,
                                      miosqp_tree_info *info, miosqp_lockstep_stats *stats,
                                      miosqp_lockstep_rf_stats *rf_stats);

/* ---- the lock-step trees with strong and reliability branching --------------------------------------------
 * miosqp_qp_solve_trees_lockstep with the branching position chosen as the sequential solve with branching_rule 1 or 2
 * chooses it (miosqp_amd/bnb.py: Workspace.bound_and_branch -> Workspace.select_branching -> Workspace.strong_branch,
 * the bookkeeping of Workspace.record_gain / pseudo_costs and the scores of sb_scores; the reference has rule 0 only,
 * workspace.py:205-230).  On a solved fractional node that is not cut off, after the rounding heuristic of the digest:
 *   rule 1: with one fractional position (|x - round(x)| > eps_int_feas of miosqp_qp_set_root) that position; otherwise
 *     the candidates are the sb_candidates most fractional positions (ties to the lower position), ascending;
 *   rule 2: the candidates are the fractional positions with min(observations down, up) < sb_reliability, cut to the
 *     sb_candidates most fractional; without one, nothing is solved.
 * The nodes that have candidates in a wave send their 2K children (K down: u = floor x on the candidate's integer row,
 * then K up: l = ceil x; the tree's cost, the node's OWN x, y as the warm start, at most sb_max_iter iterations) into
 * ONE more batch, sliced at max_batch like a wave; a node's children may straddle two slices.  A child's gain is
 * max(L_child - L_node, 0), 1e30 without an x (status neither SOLVED nor MAX_ITER_REACHED); a candidate's score
 * max(gain_down, sb_eps) * max(gain_up, sb_eps); rule 1 takes the first maximum.  Rule 2 records the children with an
 * x as observations (gain per unit distance to floor / ceil, candidate order, down then up), scores every fractional
 * position -- by pseudo-costs where it has no strong-branching score: mean gain per unit, for a position without
 * observations in a direction the mean of those means in numpy's summation order, or 1.0 -- and takes the first
 * maximum in ascending position order; each child of the branching is one more observation when its own solve has an
 * x.  The tables are per tree and start at zero.  Per wave the host reads the asking nodes' x at the integer
 * positions (one download) and a 16-byte record per child (one download), and writes the children of the chosen
 * positions with one launch.  A wave in which no node asks queues nothing more than miosqp_qp_solve_trees_lockstep
 * does. */
typedef struct miosqp_lockstep_sb_stats {
  int32_t batches;        /* strong-branching batches run (waves in which at least one node had candidates) */
  int32_t reserved;
  int64_t columns;        /* their columns: 2K per node with K candidates */
  int64_t iters_slowest;  /* sum over the batches of the slowest child's ADMM iterations */
  double device_time;     /* seconds between the events around the branching step of the waves that ran a batch, its two
                             downloads included (part of miosqp_lockstep_stats.device_time) */
  int32_t *calls;         /* IN, optional (NULL: not wanted), B entries each: strong_branch calls of tree b ... */
  int32_t *children;      /* ... their children ... */
  int64_t *iters;         /* ... and the children's ADMM iterations (info[b].osqp_iter counts node relaxations only) */
  int32_t *first_k;       /* IN, optional debug, B entries: candidates K of tree b's FIRST call (0: it never called) */
  int32_t *first_chosen;  /* B entries: the argmax of its scores (index into the candidates) */
  int32_t *first_cand;    /* B x sb_candidates: its candidate positions, ascending (the first K of a row) */
  int32_t *first_status;  /* B x 2 sb_candidates each: its children as the batch epilogue left them, K down then K up */
  int32_t *first_iter;    /* (the first 2K of a row): status, iterations, objective at the clamped x -- what */
  double *first_lower;    /* miosqp_qp_strong_branch returns per child */
} miosqp_lockstep_sb_stats;

/* Arguments, layouts, info[b], stats, capacity and errors as for miosqp_qp_solve_trees_lockstep.  branching_rule 1 or 2;
 * sb_candidates in 1 .. 32; sb_max_iter a positive multiple of settings.check_termination (the rule of
 * miosqp_qp_strong_branch); sb_reliability >= 0; sb_eps > 0: MIOSQP_EARG with a last_error text otherwise, nothing
 * queued.  MIOSQP_EBOUNDS also when a candidate's child would have l > u. */
int miosqp_qp_solve_trees_lockstep_sb(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u,
                                      const double *x0, const double *y0, const double *upper0, const double *x_inc0,
                                      int32_t tree_explor_rule, int32_t max_iter_bb, int32_t capacity,
                                      int32_t branching_rule, int32_t sb_candidates, int32_t sb_max_iter,
                                      int32_t sb_reliability, double sb_eps, double *x_out, miosqp_tree_info *info,
                                      miosqp_lockstep_stats *stats, miosqp_lockstep_sb_stats *sb_stats);

/* ---- the same B trees on columns that are refilled between chunks ---------------------------------------
 * miosqp_qp_solve_trees_lockstep without the wave.  The engine's batch runs in chunks of check_termination iterations
 * with one termination test each; here a column holds one node of one tree, counts its own iterations from the chunk it
 * was loaded in and reaches max_iter on its own.  After every chunk the columns the test has just decided are harvested
 * on the device (unscale, clamp, digest, objective, the rounded point against the INSTANCE's root rows, solution into
 * the node's slot, children into the two slots reserved when the column was filled, one 64-byte record per column),
 * their trees absorb the records on the host (bound_and_branch, workspace.py:282-334) and -- at that same boundary --
 * every free column is loaded with the next leaf (choose_leaf, workspace.py:128-155) of a tree that has no node in
 * flight and can continue, lowest tree index first, lowest free column first.  A tree has at most ONE node in flight:
 * its next leaf is chosen only after its previous node was absorbed, so every tree runs the loop of solver.py:85-123
 * node for node, exactly as its sequential solve and as a tree of miosqp_qp_solve_trees_lockstep does, whatever the
 * other trees do (a node is a pure function of q, l, u, x0, y0): status, node and iteration counts are those of the
 * sequential solve, upper_glob and x those of miosqp_qp_solve_trees_lockstep bit for bit.  A column that cannot be
 * refilled (every tree that can continue has its node in flight) stays decided until a tree is free.
 * Columns: min(B, the engine's batch width = max_batch rounded up to 64, at most 1024).  Per boundary the host reads
 * the list of harvested columns with their records (one download, one synchronisation) and sends six integers per
 * filled column and the incumbent pairs (one upload). */
typedef struct miosqp_refill_stats {
  int32_t chunks;           /* chunks run: with B <= columns, the largest iteration count of a tree / check_termination */
  int32_t columns;          /* columns used */
  int32_t grown;            /* times the slot store grew */
  int32_t chunk_cap;        /* IN: entries chunk_busy can take; later chunks are not recorded */
  int64_t nodes;            /* over all trees */
  int64_t iters_all;        /* ADMM iterations over all nodes */
  int64_t col_chunks_busy;  /* sum over chunks of the columns holding a node in flight ... */
  int64_t col_chunks_total; /* ... and of the columns: busy / total is the occupancy */
  double device_time;       /* seconds between the events around the call (the waits for the host at the boundaries included) */
  double run_time;          /* wall seconds */
  double host_time;         /* of those: the tree logic on the host (absorbing, choosing, filling), between the chunks */
  double chunk_time;        /* device seconds inside the chunks themselves (iterations + test): device_time - chunk_time is the boundaries' */
  int64_t nodes_max_iter;   /* nodes whose column ended MAX_ITER_REACHED, by its own count ... */
  int64_t iters_max_iter;   /* ... and their iterations: nodes_max_iter * max_iter, whatever chunk each was loaded in */
  int32_t *chunk_busy;      /* IN, optional (NULL: not wanted): busy columns per chunk */
  int32_t *finished_at;     /* IN, optional, B entries: the chunk after which tree b was done (0: it had nothing to do) */
} miosqp_refill_stats;

/* Arguments, layouts, info[b], capacity and errors as for miosqp_qp_solve_trees_lockstep.  Also MIOSQP_EARG when
 * settings.max_iter is not a multiple of settings.check_termination (a column counts whole chunks, as
 * miosqp_qp_pool_create demands) and while pool chunks are in flight; the call marks the leaf pool's columns as used
 * (miosqp_qp_pool_reset before the next miosqp_qp_pool_launch), as miosqp_qp_solve_batch does.  The engine's own q,
 * bounds, root and search state are neither read nor written. */
int miosqp_qp_solve_trees_refill(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u,
                                 const double *x0, const double *y0, const double *upper0, const double *x_inc0,
                                 int32_t tree_explor_rule, int32_t max_iter_bb, int32_t capacity,
                                 double *x_out, miosqp_tree_info *info, miosqp_refill_stats *stats);

/* ---- the lock-step trees with spare columns solving open leaves early -----------------------------------
 * miosqp_qp_solve_trees_lockstep launches whole tiles of 64 columns per wave; with L live trees the columns behind the L
 * chosen leaves iterate on padding.  Here a tree may hold up to `ahead` columns of a wave: its chosen leaf (the MANDATORY
 * column) and, in the free columns of the tiles the wave launches anyway, other open leaves and children of nodes it has
 * already solved ahead.  The record of a node solved ahead waits with the node -- which stays in the open list with its
 * inherited bound, counted as a leaf -- until the tree's exploration rule chooses it: then it is absorbed without a
 * wave (a HIT), as are further records the rule reaches.  A record whose node is pruned, or that is left when the call
 * ends, is discarded with everything solved below it.  A node is a pure function of (q, l, u, x0, y0): every tree makes
 * the decisions of its sequential solve, node for node, and info[b], x_out are those of miosqp_qp_solve_trees_lockstep
 * bit for bit; only the number of waves changes.  nodes, osqp_iter, incumbents and prunings happen at absorb time only.
 * The wave ends with its mandatory columns: behind every chunk one small launch counts the mandatory columns the test
 * has not decided, the count comes down with the chunk's control block, and an ahead column that is undecided when the
 * loop ends is called off -- nothing of it is kept and its node is solved again when it is next chosen.
 * Free columns: the mandatory columns are sliced at max_batch as miosqp_qp_solve_trees_lockstep slices them; the last
 * slice holds nbl of them and min(64 ceil(nbl / 64), max_batch) - nbl free columns (64 ceil(L / 64) - L when max_batch is
 * a multiple of 64).  They are dealt round-robin over the live trees in tree order, one candidate per tree per round,
 * until a tree holds `ahead` columns, its candidates run out or the free columns run out; a tree's candidates are taken
 * in the order its own rule would choose them (csrc/lockstep_ahead.hpp states it in full).  The order influences speed
 * only.  No tile is launched that miosqp_qp_solve_trees_lockstep would not launch for the same L; ahead = 1 runs its
 * launches exactly. */
typedef struct miosqp_lockstep_ahead_stats {
  int32_t waves;             /* waves run (miosqp_lockstep_stats.waves) */
  int32_t wave_cap;          /* IN: entries the three per-wave arrays below can take; later waves are not recorded */
  int64_t columns;           /* columns solved: mandatory and ahead */
  int64_t sent;              /* ahead columns sent = hits + discarded + called_off */
  int64_t hits;              /* ... whose record was absorbed when the tree's rule reached the node */
  int64_t discarded;         /* ... whose record was dropped (pruned, below a node that did not branch, left at the end) */
  int64_t called_off;        /* ... the wave did not wait for */
  int64_t hit_iters;         /* ADMM iterations of the hits (they are part of info[b].osqp_iter) ... */
  int64_t discarded_iters;   /* ... of the discarded records and ... */
  int64_t called_off_iters;  /* ... of the columns called off: these two appear here only */
  int32_t free_slots;        /* node slots free when the call ended ... */
  int32_t slot_cap;          /* ... of this many: the difference is the open leaves and the parents their warm starts need */
  int32_t *wave_width;           /* IN, optional (NULL: not wanted): columns per wave, ahead columns included */
  int32_t *wave_iter_mandatory;  /* IN, optional: the mandatory columns' largest iteration count per wave */
  int32_t *wave_chunks;          /* IN, optional: chunks the wave's slowest slice ran (a tail at max_iter counts as one) */
} miosqp_lockstep_ahead_stats;

/* Arguments, layouts, info[b], stats, capacity and errors as for miosqp_qp_solve_trees_lockstep (stats: max_width and
 * wave_width count all columns, the iteration figures the mandatory columns per wave and iters_all the absorbed nodes;
 * node_hviol is not written).  ahead >= 1: MIOSQP_EARG with a last_error text otherwise, nothing queued. */
int miosqp_qp_solve_trees_lockstep_ahead(miosqp_qp_engine *e, int32_t B, const double *q, const double *l, const double *u,
                                         const double *x0, const double *y0, const double *upper0, const double *x_inc0,
                                         int32_t tree_explor_rule, int32_t max_iter_bb, int32_t capacity, int32_t ahead,
                                         double *x_out, miosqp_tree_info *info, miosqp_lockstep_stats *stats,
                                         miosqp_lockstep_ahead_stats *ahead_stats);

/* ---- node-at-a-time branch and bound, driven from the host in C++ -------------------------------------
 * The loop of /root/reference/miosqp/solver.py:65-172 (choose_leaf -> Node.solve -> bound_and_branch, workspace.py:
 * 113-155, 274-334) for problems of any size, one relaxation at a time in whatever form the engine uses for single
 * nodes.  The open leaves are device slots (integer-row bounds + solution = the children's warm start), the children
 * are written on the device (workspace.py:157-203), a node's outcome reaches the host as a 96-byte record: no vector
 * crosses PCIe per node and no interpreter runs between two nodes.  Same list semantics as the Python mirror
 * (creation order, first maximum, the prune traversal of workspace.py:278-280); the heuristic incumbent's value is
 * the device's.  Needs set_integer_rows + set_root. */
typedef struct miosqp_search_info {
  int64_t nodes;        /* nodes solved in this call */
  int64_t osqp_iter;    /* ADMM iterations over them */
  int32_t open_leaves;  /* leaves still open (0: the tree is closed) */
  int32_t free_slots;
  int32_t improved;     /* the incumbent improved in this call: 1 = last by an integer-feasible node, 2 = last by the
                           rounding heuristic (its value is the device's sum: recompute on the host and hand it back
                           through miosqp_qp_search_set_incumbent(e, value, NULL) for workspace.py:321-327's number) */
  int32_t reserved;
  double upper_glob, lower_glob;
  double device_time;   /* seconds inside the ADMM loops of these nodes (device events) */
  double run_time;
} miosqp_search_info;

int miosqp_qp_search_create(miosqp_qp_engine *e, int32_t capacity);
/* new MIQP on the same factor: no leaves, no incumbent */
int miosqp_qp_search_reset(miosqp_qp_engine *e);
/* appends a leaf given with explicit vectors (the root, or one from another rank): l_int, u_int (n_int), x0 (n), y0 (M).
 * Here and in take_leaf / miosqp_qp_stream_add_leaf / _take_leaf / miosqp_qp_pool_write_node / _read_node the four vectors
 * may live in HOST or in DEVICE memory (unified addressing; the copies are hipMemcpyDefault): between ranks a leaf
 * travels as one device buffer -- slot store -> RCCL broadcast -> slot store -- and never visits the host
 * (miosqp_amd/dist.py: ShardedStream; the l <= u check is the host's and is skipped for device memory). */
int miosqp_qp_search_add_leaf(miosqp_qp_engine *e, const double *l_int, const double *u_int, const double *x0,
                              const double *y0, int32_t depth, double lower);
/* removes the shallowest open leaf and returns it with explicit vectors; 1 when there is none */
int miosqp_qp_search_take_leaf(miosqp_qp_engine *e, double *l_int, double *u_int, double *x0, double *y0,
                               int32_t *depth, double *lower);
/* adopts an incumbent from outside when it is better (MIOSQP.set_x0, another rank) and prunes against it;
 * x == NULL: only the VALUE of the incumbent the search already holds is replaced (no comparison, no pruning) */
int miosqp_qp_search_set_incumbent(miosqp_qp_engine *e, double upper, const double *x);
/* *upper >= 1.7e308: none yet (x untouched) */
int miosqp_qp_search_get_incumbent(miosqp_qp_engine *e, double *upper, double *x);
/* solves nodes until the list is empty, max_nodes are done or budget_s seconds have passed (<= 0: no time limit).
 * The slot store grows by itself (the capacity of search_create is a starting size); MIOSQP_EFULL only when the
 * device has no memory left for it -- *info is filled with what was done up to then in that case too.
 * tree_explor_rule 0 .. 3 as for miosqp_qp_solve_tree, with the same tie rule (the first leaf in list order); the leaf
 * is chosen on the host between a record and the next mail, and an incumbent from miosqp_qp_search_set_incumbent counts
 * for rules 1 and 3.  Any other value: MIOSQP_EARG. */
int miosqp_qp_search_run(miosqp_qp_engine *e, int32_t tree_explor_rule, int64_t max_nodes, double budget_s,
                         miosqp_search_info *info);

/* ---- device-resident leaf pool + streaming batch -------------------------------------------------------
 * Workspace.leaves and child generation (/root/reference/miosqp/workspace.py:83,
 * 157-203) kept on the device.  A node = its integer-row bounds (rows m .. M-1; workspace.py:227) + a warm
 * start = the solution of its parent's slot (workspace.py:174-176, 198-200).  The host owns slot numbers and
 * the search logic (choose_leaf / prune / incumbent: workspace.py:128-155, 274-334) on 64-byte digests; the
 * only vectors that cross PCIe are an incumbent's x when one is found.  The batch's columns are refilled
 * from a ready ring between chunks (check_termination iterations + one test), so a finished node's column
 * does not wait for the slowest node of a wave; every node still gets exactly the iterations and tests
 * miosqp_qp_solve_node would give it.  Needs set_integer_rows + set_root, and max_iter % check_termination == 0. */
typedef struct miosqp_pool_digest {
  int32_t slot;        /* pool slot of the node */
  int32_t status_val;  /* as miosqp_qp_info.status_val; -100 = dropped at refill: its bound exceeded the incumbent */
  int32_t iter;
  int32_t int_inf;     /* -1 when the relaxation was infeasible */
  int32_t nextvar;     /* branching variable (position in i_idx); the children were written when int_inf > 0 */
  int32_t reserved;
  double lower;        /* objective at the clamped x (node.py:143); NaN when infeasible */
  double heur_viol;    /* <= 0: the rounded candidate satisfies the root constraints */
  double heur_obj;
  double pri_res, dua_res;
} miosqp_pool_digest;

/* capacity: node slots; columns: width of the streaming batch (<= 1024, rounded up to 64) */
int miosqp_qp_pool_create(miosqp_qp_engine *e, int32_t capacity, int32_t columns);
/* empties columns, ready ring and digests (new MIQP on the same factor: after update_vectors / set_root) */
int miosqp_qp_pool_reset(miosqp_qp_engine *e);
/* a node given by the host (root, or a leaf received from another rank): integer-row bounds (n_int each) and an
 * explicit warm start x0 (n), y0 (M) */
int miosqp_qp_pool_write_node(miosqp_qp_engine *e, int32_t slot, const double *l_int, const double *u_int,
                              const double *x0, const double *y0);
/* integer-row bounds and, for a solved node, its solution (any pointer may be NULL) */
int miosqp_qp_pool_read_node(miosqp_qp_engine *e, int32_t slot, double *l_int, double *u_int, double *x, double *y);
/* appends nodes to the ready ring in the order they should be solved: slot, the two slots its children are to be
 * written into (-1: none), and the bound it inherited (dropped unsolved once that exceeds the incumbent) */
int miosqp_qp_pool_push(miosqp_qp_engine *e, int32_t count, const int32_t *slot, const int32_t *child0,
                        const int32_t *child1, const double *lower);
/* incumbent value for the refill-time bound test */
int miosqp_qp_pool_set_upper(miosqp_qp_engine *e, double upper);
/* enqueues `chunks` x (refill, check_termination iterations, test, harvest) and returns at once */
int miosqp_qp_pool_launch(miosqp_qp_engine *e, int32_t chunks);
/* waits until at most `keep_in_flight` launches are still running (oldest first: with 1 the device works on the
 * newest launch while the host handles the results of the one before); digests of the nodes decided (or dropped)
 * since the last call, at most max_out; *active = columns holding a node after the last refill seen,
 * *ready_left = ready-ring entries not yet taken */
int miosqp_qp_pool_collect(miosqp_qp_engine *e, int32_t keep_in_flight, miosqp_pool_digest *out, int32_t max_out,
                           int32_t *n_out, int32_t *active, int64_t *ready_left);

/* frees device and host memory */
int miosqp_qp_cleanup(miosqp_qp_engine *e);

/* ---- introspection used by bench.py and the parity tests (not part of the reference API) -- */

/* human-readable text of the last failure on this thread */
const char *miosqp_qp_last_error(void);

/* scaled iterates after running exactly k ADMM iterations from the current state with the
 * termination test disabled (iterate-level parity against the oracle). x: n, z,y: M. */
int miosqp_qp_debug_iterate(miosqp_qp_engine *e, int32_t k, double *x, double *z, double *y);

/* debug: one device-resident product of the set-up copied to the host exactly as it lies in device memory, row-major,
 * padding included (the tests of the set-up kernels compare it with a high-precision reference).  which:
 *   0 d2inv (n x 1)        1 Linv (n x ld, strict lower)      2 LinvT (n x ld)
 *   3 W, the explicit KKT inverse (N x ldw, N = M + n, constraints first)      4 Kc = [0 Abar; Abar^T Pbar] (N x ldw)
 *   5 the persistent solver's tail inverse S^-1 (n x its own leading dimension)
 * *rows and *ld are always reported; with out == NULL nothing else happens, otherwise capacity (in doubles) must be at
 * least rows * ld.  A product this engine did not build is an error (MIOSQP_EUNSUPPORTED with a last_error text), never zeros.
 * Waits for the engine's stream first; changes no state. */
int miosqp_qp_debug_factor(miosqp_qp_engine *e, int32_t which, double *out, int64_t capacity, int32_t *rows, int32_t *ld);

/* D (n), E (M), c of the Ruiz equilibration */
int miosqp_qp_get_scaling(miosqp_qp_engine *e, double *D, double *E, double *c);

/* sizes of the factor: out[0]=nnz(L) strict (panel + tail), out[1]=nnz panel, out[2]=tail order,
 * out[3]=algorithmic bytes per ADMM iteration (SURVEY.md sec. 8d formula), out[4..6] threads per
 * row of the panel/tail kernels, out[7] bit 0 = product-form factor in use, bit 1 = LDS-resident solver in use,
 * bit 2 = dense setup stages ran on the device, bit 3 = cooperative solver in use, bits 8..15 = its calibrated
 * poll delay (64-clock units); out[8] = bytes per iteration the kernels of the form in use actually request (dense
 * blocks carry no index array: 8 B per entry instead of the formula's 12); out[9] = times the engine fell back from
 * the cooperative form; out[7] bit 17 = the explicit KKT inverse failed its residual check at set-up and the engine
 * iterates with the factor's sweeps instead (see miosqp_qp_get_inverse_guard); bit 18 = launches of the hosted search counted
 * by miosqp_qp_get_loop_launches since the last reset were launches of the resident grid (one per miosqp_qp_search_run).
 * out must hold 10 values. */
int miosqp_qp_get_factor_stats(miosqp_qp_engine *e, int64_t *out);

/* rho in use (differs from settings.rho when settings.rho_auto chose it) */
int miosqp_qp_get_rho(miosqp_qp_engine *e, double *rho);

/* The register-resident solvers iterate on the explicit inverse of the scaled KKT matrix (sigma = 1e-6), which -- unlike
 * the sweeps with the LDL^T factor the reference's linear solver performs at /root/reference/miosqp/workspace.py:63-68
 * (osqp.setup) and node.py:108 (solve) -- is not backward stable.  At set-up the device measures
 * max |K W r - r| / max |r| over three probe vectors; above the threshold (1e-9; MIOSQP_GUARD_TOL overrides, negative
 * switches the check off) the engine does not use the inverse.  out[0] = measured residual (-1: no inverse was built),
 * out[1] = threshold, out[2] = 1 when the engine fell back.  out must hold 3 values. */
int miosqp_qp_get_inverse_guard(miosqp_qp_engine *e, double *out);

/* Times `reps` back-to-back launches of one hot-path kernel with HIP events on the engine's
 * own stream and returns the mean duration in microseconds in *usec and the kernel's
 * algorithmic bytes per launch in *bytes.  which: 0 panel-forward, 1 tail-forward,
 * 2 tail-backward, 3 panel-backward+update, 4 one whole ADMM iteration (all four); with the
 * product-form factor 0 = forward sweep, 1 = backward sweep + update, 2 and 3 are empty;
 * 10..14 the same for the batched kernels at full batch capacity (after a solve_batch). */
int miosqp_qp_time_kernel(miosqp_qp_engine *e, int32_t which, int32_t reps, double *usec,
                          double *bytes);

/* Device time spent in the ADMM loop since the last reset, measured with HIP events recorded on
 * the engine's stream around every chunk (check_termination iterations + one termination test)
 * of every solve: *ms = total milliseconds, *iters = ADMM iterations executed in them. */
int miosqp_qp_get_loop_stats(miosqp_qp_engine *e, double *ms, int64_t *iters, int32_t reset);

/* Per node of the node-at-a-time search in the host library (miosqp_qp_search_run) since the last reset of the loop
 * statistics: microseconds of device time per ADMM iteration of a node -- out[0] minimum, out[1] median, out[2] maximum
 * over the nodes -- and *nodes, how many nodes they are taken over (bench.py prints them next to the mean: a single slow
 * node cannot move the headline unnoticed).  No reference counterpart: the reference only sums OSQP's run_time
 * (/root/reference/miosqp/node.py:118). */
int miosqp_qp_get_node_stats(miosqp_qp_engine *e, double *us_per_iter_min_med_max, int32_t *nodes);

/* Launches of the hosted search's solver kernel since the last reset of the loop statistics.  A node of
 * miosqp_qp_search_run is one cooperative launch (k_coop) -- or, where the cooperative grid can stay resident, the whole
 * call is ONE launch (k_coop_run) that takes its nodes from a mailbox the host writes: the loop
 * `while can_continue: choose_leaf -> solve -> bound_and_branch` of /root/reference/miosqp/solver.py:85-123 with the
 * `solve` of /root/reference/miosqp/node.py:96-143 resident on the device between nodes.  bench.py divides the loop's
 * device time by this count for the kernel's average launch. */
int miosqp_qp_get_loop_launches(miosqp_qp_engine *e, int64_t *launches);

/* Same for solve_batch: *ms device milliseconds in batched chunks, *batch_iters lock-step
 * iterations executed, *node_iters = sum over those iterations of the columns still iterating. */
int miosqp_qp_get_batch_stats(miosqp_qp_engine *e, double *ms, int64_t *batch_iters,
                              int64_t *node_iters, int32_t reset);

/* debug counters: which = 0 -> wave compactions solve_batch has performed; 1 -> times a chunk's persistent launch was
 * called off; 2 -> whole-chip launches on this engine's device that were ordered behind another engine's (engines of
 * one process take turns with k_coop / k_pers / kbp); 3 -> the control block's call-off word once the engine's stream
 * is idle (blocks); 4 -> engines of this device that take turns; 5 -> columns of every row of the tail's inverse that
 * the persistent streaming solver keeps in LDS for a whole launch (0: none); 6 -> tiles of the tail's inverse the
 * persistent streaming solver reads per iteration when it takes it as a symmetric matrix (0: it reads whole rows);
 * 7 -> launches of the stream's persistent kernel (kbs) the leaf pool has queued, 8 -> chunks queued that way, 9 -> chunks
 * queued as the chunk graph / kernel by kernel instead (a launch of kbs that is called off leaves its chunks undone: 1);
 * 10 -> the poll delay the resident search grid ran with last (-1: it has not run), 11 -> synthetic nodes the calibration of
 * that delay has run on this engine (0: looked up); 12 -> bytes of device scratch the slabs of
 * miosqp_qp_polish_many_large hold (0 before its first call; a call that declines allocates none) */
int64_t miosqp_qp_debug_counter(miosqp_qp_engine *e, int32_t which);

/* debug: per-workgroup (start, end) stamps (100 MHz wall clock) of ONE launch of a product-form
 * kernel (which: 0 forward, 1 backward); out holds 2 * max_blocks values */
int miosqp_qp_debug_timeline(miosqp_qp_engine *e, int32_t which, uint64_t *out, int32_t max_blocks,
                             int32_t *nblocks);

/* debug: shader cycles and 100 MHz ticks recorded by the last LDS-resident launch */
int miosqp_qp_debug_clock(miosqp_qp_engine *e, double *cycles, double *ticks);

/* ---- the host side of the streaming search, compiled ------------------------------------------------------
 * What miosqp_amd/stream.py: StreamSearch does per round -- push the next leaves in the exploration rule's order
 * (workspace.py:128-149), launch, collect the launch before, bound_and_branch on every digest (workspace.py:282-334),
 * prune -- as one call per `rounds` rounds on top of miosqp_qp_pool_*: the same exploration order and node counts,
 * no interpreter between two chunks (several pools on several host threads stay bound by the device).  The value of
 * an incumbent found by the rounding heuristic is the device's.  Needs set_integer_rows + set_root. */
typedef struct miosqp_stream_info {
  int64_t alive;        /* leaves open on the host, waiting in the ring or being solved (0: the tree is closed) */
  int64_t open_leaves, in_flight, free_slots;
  int64_t nodes, osqp_iter, chunks, dropped;   /* totals since the driver was created */
  int32_t improved;     /* 1: the incumbent improved during this call */
  int32_t active;       /* columns holding a node after the last refill seen */
  double upper_glob;
} miosqp_stream_info;

/* creates the pool if there is none; ring_margin 0 = max(32, columns / 2) */
int miosqp_qp_stream_create(miosqp_qp_engine *e, int32_t capacity, int32_t columns, int32_t ring_margin);
int miosqp_qp_stream_begin(miosqp_qp_engine *e);
int miosqp_qp_stream_add_leaf(miosqp_qp_engine *e, const double *l_int, const double *u_int, const double *x0,
                              const double *y0, int32_t depth, double lower);
int miosqp_qp_stream_take_leaf(miosqp_qp_engine *e, double *l_int, double *u_int, double *x0, double *y0, int32_t *depth,
                               double *lower);
int miosqp_qp_stream_set_incumbent(miosqp_qp_engine *e, double upper, const double *x);
int miosqp_qp_stream_get_incumbent(miosqp_qp_engine *e, double *upper, double *x);
/* tree_explor_rule 0 / 1 only (the best-bound rules 2 and 3 of miosqp_qp_solve_tree are not offered here: MIOSQP_EARG) */
int miosqp_qp_stream_step(miosqp_qp_engine *e, int32_t tree_explor_rule, int32_t chunks, int32_t rounds,
                          int64_t max_nodes, miosqp_stream_info *info);

#ifdef __cplusplus
}
#endif
#endif /* MIOSQP_AMD_H */
