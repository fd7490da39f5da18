// part of engine.hip (included there, not compiled alone): a whole branch-and-bound tree in ONE launch (small problems)
// ------------------------------------------------------------------------------------------
// SURVEY sec. 8f rank 2: the MPC re-solve path (BASELINE configs[3]: power converter, n = 18, 45 rows, ~12 nodes
// of ~50 iterations per MIQP, thousands of MIQPs in sequence).  With the LDS-resident solver a node costs ~0.1 ms
// on the device and as much again in host round trips (ctypes call, six launches, two copies, the wait).  Here the
// whole tree search of /root/reference/miosqp/solver.py:85-123 runs inside one launch of one workgroup: the factor
// and the iterates live in LDS as in k_resident, the leaf list lives in LDS / global memory, and thread 0 takes
// the decisions of Workspace.choose_leaf / bound_and_branch / prune (workspace.py:128-155, 274-334) exactly as
// miosqp_amd/bnb.py takes them on the host -- same order, same strict comparisons, same list semantics
// (argmax = first maximum; pop keeps the order of the rest; prune skips the element behind a removed one).
// The host sends the root and receives (incumbent x, upper bound, node and iteration counts).
// ------------------------------------------------------------------------------------------
constexpr int TREE_CAP = 1024;  // leaves alive at once (the list is checked for overflow; the host falls back)

struct TreeOut {
  int nodes, osqp_iter, leaves_left, overflow;
  int max_leaves, found, pad0, pad1;
  double upper, lower_glob;
};

// what rf_stats counts, for one tree with round and fix inside (Workspace.primal_heuristic)
struct TreeRfOut {
  int calls, candidates, feasible, improved;
  int osqp_iter, pad0, pad1, pad2;
};

// what sb_stats counts, for one tree with strong / reliability branching inside (Workspace.strong_branch)
struct TreeSbOut {
  int calls, children, osqp_iter, pad0;
  int pad1, pad2, pad3, pad4;
};

struct TreeArgs {
  int rule, max_nodes, max_iter, check_every, TG1, TG2;
  double upper0;
  double *lf_lo, *lf_hi;  // [TREE_CAP][n_int] integer-row bounds (unscaled)
  double *lf_x, *lf_y;    // [TREE_CAP][n], [TREE_CAP][M] warm starts (unscaled)
  double *inc_x;          // [n] incumbent: in (when upper0 is finite), out
  TreeOut *out;
  // k_tree_w with its inputs and outputs in host memory (no copies around the launch): done[0] = 1 (release, system
  // scope) after everything else has been written, done[1], done[2] = 100 MHz ticks at kernel start / end; or nullptr
  unsigned long long *done;
  int sp_off;  // k_tree: offset (doubles) of the LDS copy of the sparse Abar / Pbar rows inside the dynamic block, or -1
  // miosqp_qp_solve_trees: workgroup b runs MIQP b of a batch that shares P, A (the factor) and differs in q, l, u, warm
  // start and incumbent -- every per-instance array holds `batch` instances back to back; upper_b[b]: its incumbent value
  int batch;
  const double *upper_b;
  // k_tree_r_m (the reduced form, tree_reduced_body.hpp): the leaf list's capacity (the leaf store holds as many places);
  // offset (doubles) of the LDS copy of Abar^T's packed rows, or -1 -- it is there exactly when sp_off is; and which rows of
  // Abar the iteration reads where no LDS copy is: 1 the dense copies (f_Atd, f_Ad), 0 the packed panels (pv_At, pc_A)
  int leaf_cap, pv_off, r_dense;
  // k_tree_rf, k_tree_rf_m, k_tree_rf_r_m (round and fix inside the tree, kernels_tree_rf_block.inc): candidates per call
  // (0: never fires), their iteration cap, every how many branching nodes; the tree's counters (per instance in a batch)
  int rf_K, rf_max_iter, rf_every;
  TreeRfOut *rf_out;
  // k_tree_sb, k_tree_sb_m, k_tree_sb_r_m (strong / reliability branching inside the tree, kernels_tree_sb_block.inc):
  // branching_rule 1 or 2, sb_candidates, the children's iteration cap, sb_reliability, sb_eps; the tree's work area
  // (tree_sb::work_doubles(n_int) doubles: pseudo-costs, the asking node's candidates and children), Node.pc of every
  // leaf-store place (tree_sb::PC_DOUBLES each), the tree's counters -- all three per instance in a batch
  int sb_rule, sb_K, sb_max_iter, sb_rel;
  double sb_eps;
  double *sb_work, *sb_pc;
  TreeSbOut *sb_out;
};

// workgroup b of a batched launch: the per-instance pointers of Dev and TreeArgs moved to instance b (the staging block
// raw_l | raw_u | raw_x | raw_y holds 3 M + n doubles per instance; the root bounds of an instance are its l, u).
// cap: places of one instance's leaf store -- TREE_CAP, or ta.leaf_cap for the reduced form (k_tree_r); every product is
// formed in size_t
__device__ __forceinline__ void tree_instance(Dev &d, TreeArgs &ta, size_t cap = TREE_CAP) {
  if (!ta.batch) return;
  const size_t b = blockIdx.x, n = d.n, M = d.M, p = d.n_int, blk = 3 * M + n;
  d.q += b * n;
  d.qraw += b * n;
  d.raw_l += b * blk;
  d.raw_u += b * blk;
  d.raw_x += b * blk;
  d.raw_y += b * blk;
  d.root_l = d.raw_l;
  d.root_u = d.raw_u;
  ta.lf_lo += b * cap * p;
  ta.lf_hi += b * cap * p;
  ta.lf_x += b * cap * n;
  ta.lf_y += b * cap * M;
  ta.inc_x += b * n;
  ta.out += b;
  ta.upper0 = ta.upper_b[b];
}

// ... and the instance's round-and-fix counters (k_tree_rf)
__device__ __forceinline__ void tree_instance_rf(Dev &d, TreeArgs &ta, size_t cap = TREE_CAP) {
  if (ta.batch) ta.rf_out += blockIdx.x;
  tree_instance(d, ta, cap);
}

// ... and the instance's work area, Node.pc and counters of strong / reliability branching (k_tree_sb)
__device__ __forceinline__ void tree_instance_sb(Dev &d, TreeArgs &ta, size_t cap = TREE_CAP) {
  if (ta.batch) {
    const size_t b = blockIdx.x;
    ta.sb_work += b * miosqp::tree_sb::work_doubles(d.n_int);
    ta.sb_pc += b * cap * (size_t)miosqp::tree_sb::PC_DOUBLES;
    ta.sb_out += b;
  }
  tree_instance(d, ta, cap);
}

__host__ __device__ inline size_t tree_lds_doubles(int n, int M, bool wform) {
  // resident arrays + epilogue vectors (xf, xi: n; yf, rowbuf: M; prow: 2 n) + list (lower: CAP doubles; order, depth,
  // freelist: 3 CAP ints = 1.5 CAP doubles) + a few scalars
  // (+ 16: the per-wavefront (value, position) pairs of the best-bound choice, first_min_wave)
  return resident_lds_doubles(n, M, wform) + 4 * (size_t)n + 2 * (size_t)M + (size_t)TREE_CAP * 5 / 2 + 16 + 16 + ((size_t)n + 1) / 2 + 1;
}

// ------------------------------------------------------------------------------------------
// The best-bound choice (tree_explor_rule 2, and 3 once an incumbent exists): the open leaf with the SMALLEST inherited
// bound, the FIRST one in list order on ties (np.argmin; two siblings share their parent's bound, so ties are the
// normal case and the tie rule decides the tree).  Under best bound the list is several times as long as under depth
// first (up to TREE_CAP), and one thread walking it sits between every two nodes.  Every thread takes the positions
// k = tid, tid + T, ... and keeps the pair (lf_lower[order[k]], k); pairs are reduced with "smaller value wins; on equal
// values the smaller k wins", a total order, so the result is the same whatever the order of the reduction.
// ------------------------------------------------------------------------------------------
constexpr int TREE_NO_POS = 0x7fffffff;

__device__ __forceinline__ void first_min_take(double &v, int &k, double ov, int ok) {
  if (ov < v || (ov == v && ok < k)) { v = ov; k = ok; }
}

// this thread's pair over its positions of the list (ascending k: the strict comparison keeps the first)
template <int T>
__device__ __forceinline__ void first_min_scan(const double *lf_lower, const int *order, int count, int tid, double &v, int &k) {
  v = 1.0 / 0.0;
  k = TREE_NO_POS;
  for (int q = tid; q < count; q += T) {
    const double lv = lf_lower[order[q]];
    if (lv < v || k == TREE_NO_POS) { v = lv; k = q; }
  }
}

// across the wavefront: a butterfly, every lane ends with the winning pair
__device__ __forceinline__ void first_min_wave(double &v, int &k) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double ov = __shfl_xor(v, off, 64);
    const int ok = __shfl_xor(k, off, 64);
    first_min_take(v, k, ov, ok);
  }
}

// order[best] leaves the list and the tail moves down by one, T positions at a time: every thread reads its element,
// a barrier, every thread writes it one position lower (a round reads [base + 1, base + T] and writes [base, base + T):
// nothing a later round reads).  Called by all T threads of the workgroup with the same best and count.
template <int T>
__device__ __forceinline__ void order_remove(int *order, int best, int count, int tid) {
  for (int base = best; base + 1 < count; base += T) {
    const int src = base + 1 + tid;
    const int moved = src < count ? order[src] : 0;
    __syncthreads();
    if (src < count) order[src - 1] = moved;
  }
}

#define TREE_LIST_CAP TREE_CAP
__global__ __launch_bounds__(RES_THREADS) void k_tree(Dev d, TreeArgs ta) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  tree_instance(d, ta);
#include "kernels_tree_body.inc"  // the body, shared with k_tree_m and k_tree_r_m
}

// ------------------------------------------------------------------------------------------
// Trees of DIFFERENT models in one launch (miosqp_qp_solve_trees_models, host_models.inc): workgroup b runs entry b of a
// table in device memory.  The host has written final pointers into every entry (the model's own factor and scalings,
// its staging block, cost, leaf store, incumbent and outcome in the call's arena), so nothing is offset here; shapes, the
// LDS carve-up, sp_off, lane groupings, search settings and tolerances are the entry's own.  The entry's address depends
// on blockIdx.x alone and nothing in the launch writes the table: its fields arrive by scalar loads where they are used.
// ------------------------------------------------------------------------------------------
struct TreeModel {
  Dev d;
  TreeArgs ta;
};

__global__ __launch_bounds__(RES_THREADS) void k_tree_m(const TreeModel *__restrict__ tab) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const Dev &d = tab[blockIdx.x].d;
  const TreeArgs &ta = tab[blockIdx.x].ta;
#include "kernels_tree_body.inc"  // the body of k_tree
}

// ------------------------------------------------------------------------------------------
// The same trees with ROUND AND FIX inside (primal_heuristic 1; miosqp_qp_solve_trees_rf, miosqp_qp_solve_trees_models_rf):
// the body under TREE_RF -- on every rf_every-th node that is about to branch the workgroup solves rf_K rounded-and-fixed
// copies of the node, capped at rf_max_iter iterations, and adopts the best one that beats the incumbent
// (kernels_tree_rf_block.inc, tree_rf_logic.hpp).  No LDS beyond k_tree's: the node's xf, yf wait in its place of the
// leaf store.  Sizes n + M <= 64 run here as well (the workgroup form takes them; there is no wavefront form).
// ------------------------------------------------------------------------------------------
#define TREE_RF 1
__global__ __launch_bounds__(RES_THREADS) void k_tree_rf(Dev d, TreeArgs ta) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  tree_instance_rf(d, ta);
#include "kernels_tree_body.inc"  // the body of k_tree, with round and fix
}

__global__ __launch_bounds__(RES_THREADS) void k_tree_rf_m(const TreeModel *__restrict__ tab) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const Dev &d = tab[blockIdx.x].d;
  const TreeArgs &ta = tab[blockIdx.x].ta;
#include "kernels_tree_body.inc"  // the body of k_tree, with round and fix
}
#undef TREE_RF

// ------------------------------------------------------------------------------------------
// The same trees with STRONG or RELIABILITY BRANCHING inside (branching_rule 1 / 2; miosqp_qp_solve_trees_sb,
// miosqp_qp_solve_trees_models_sb): the body under TREE_SB -- a node that is about to branch chooses its position as
// Workspace.select_branching does: the workgroup solves the 2K children of its candidates, capped at sb_max_iter
// iterations, and thread 0 scores them; rule 2 keeps pseudo-costs per tree and solves the unreliable candidates only
// (kernels_tree_sb_block.inc, tree_sb_logic.hpp).  No LDS beyond k_tree's: the node's xf, yf wait in its place of the
// leaf store, pseudo-costs, candidates and children's outcomes live in device memory.  Sizes n + M <= 64 run here as
// well (the workgroup form takes them; there is no wavefront form).
// ------------------------------------------------------------------------------------------
#define TREE_SB 1
__global__ __launch_bounds__(RES_THREADS) void k_tree_sb(Dev d, TreeArgs ta) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  tree_instance_sb(d, ta);
#include "kernels_tree_body.inc"  // the body of k_tree, with strong / reliability branching
}

__global__ __launch_bounds__(RES_THREADS) void k_tree_sb_m(const TreeModel *__restrict__ tab) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const Dev &d = tab[blockIdx.x].d;
  const TreeArgs &ta = tab[blockIdx.x].ta;
#include "kernels_tree_body.inc"  // the body of k_tree, with strong / reliability branching
}
#undef TREE_SB
#undef TREE_LIST_CAP

// ------------------------------------------------------------------------------------------
// The same tree for a model BEYOND one workgroup's product form (n + M > RES_W_MAX and n x (M + n) doubles above the
// LDS): the relaxation in REDUCED form (tree_reduced_body.hpp) -- the packed strict lower triangle of L^-1 in LDS, Abar
// read by variable and by constraint from LDS copies of its packed rows where they fit behind everything else, else
// from L2.  Entry b of the same table; the tree logic is the same text (kernels_tree_body.inc under TREE_REDUCED).
// Decisions, list semantics and results are those of k_tree; the summation order inside an iteration differs, and the
// leaf list has ta.leaf_cap places.  miosqp_qp_solve_trees_models_large (host_models.inc) launches it.
// ------------------------------------------------------------------------------------------
static_assert(miosqp::tree_reduced::THREADS == RES_THREADS && miosqp::tree_reduced::WAVES == RES_WAVES &&
                  miosqp::tree_reduced::NQ == NQ,
              "tree_reduced_body.hpp restates the workgroup's size and the test's scratch");

__host__ __device__ inline size_t tree_r_lds_doubles(int n, int M, int leaf_cap) {
  return miosqp::tree_reduced::lds_doubles(n, M, leaf_cap);
}

// the executor of the phases on the device: every thread runs the phase, a barrier behind it; a row's partial sums meet
// through the lane exchanges of group_reduce (a butterfly, small strides first)
struct TreeRExec {
  template <class F>
  __device__ __forceinline__ void par(F f) {
    f((int)threadIdx.x);
    __syncthreads();
  }
  template <class F>
  __device__ __forceinline__ double lane_sum(int TG, int t, F f) {
    double v[1] = {f(t)};
    group_reduce<1>(v, TG);
    return v[0];
  }
};

// the LDS arrays the termination test, the prologue and the epilogue read, at their places in the reduced carve-up
__device__ __forceinline__ ResCtx res_carve_r(double *sm, const miosqp::tree_reduced::State &s, const miosqp::tree_reduced::Carve &cv) {
  ResCtx c;
  c.n = s.n; c.M = s.M; c.ldr = s.ld;
  c.Rm = s.tri; c.wr = s.wr; c.wr2 = nullptr; c.tv = nullptr;
  c.x = s.x; c.q = s.q; c.d2 = s.d2; c.ut = s.ut; c.dx = s.dx;
  c.z = s.z; c.y = s.y; c.l = s.l; c.u = s.u; c.dy = s.dy;
  c.vp = sm + cv.scr;
  c.smc = c.vp + s.M;
  c.snc = c.smc + 8 * (size_t)s.M;
  c.part = sm + cv.part;
  c.res = sm + cv.res;
  return c;
}

// Abar for the iteration: by constraint the rows the test walks (sp: LDS or L2), by variable pv_* -- copied into LDS at
// ta.pv_off (the caller synchronises afterwards) --, or the dense copies
__device__ __forceinline__ miosqp::tree_reduced::Abar tree_r_abar(const Dev &d, const TreeArgs &ta, const ResSp &sp, double *sm) {
  miosqp::tree_reduced::Abar a{d.pv_ptr, d.pv_idx, d.pv_At, sp.Ap, sp.Ai, sp.A, d.f_Atd, d.f_Ad, d.ldm, d.ldn, ta.r_dense};
  if (ta.pv_off < 0) return a;
  const int tid = threadIdx.x, n = d.n, nV = d.pv_ptr[n];
  double *V = sm + ta.pv_off;
  int *Vi = reinterpret_cast<int *>(V + nV), *Vp = Vi + nV;
  for (int k = tid; k < nV; k += RES_THREADS) { V[k] = d.pv_At[k]; Vi[k] = d.pv_idx[k]; }
  for (int k = tid; k <= n; k += RES_THREADS) Vp[k] = d.pv_ptr[k];
  a.pv_At = V; a.pv_idx = Vi; a.pv_ptr = Vp;
  a.dense = 0;
  return a;
}

// the ADMM loop of res_admm on the reduced form: the same state, the same test at the same iterations
__device__ __forceinline__ int res_admm_r(const Dev &d, const ResCtx &c, const miosqp::tree_reduced::State &s,
                                          const miosqp::tree_reduced::Abar &A, int max_iter, int check_every, int final_check,
                                          int TG1, int *iters, const ResSp &sp) {
  TreeRExec x;
  const miosqp::tree_reduced::Par p{d.rho, d.rho_inv, d.sigma, d.alpha};
  int status = 0, it = 0;
  bool checked = false;
  for (it = 1; it <= max_iter; it++) {
    miosqp::tree_reduced::iterate(x, s, A, p);
    checked = false;
    if (check_every > 0 && it % check_every == 0) {
      checked = true;
      status = res_check(d, c, it, TG1, sp);
      if (status) break;
    }
  }
  if (it > max_iter) it = max_iter;
  if (!status && !checked && final_check) status = res_check(d, c, it, TG1, sp);
  *iters = it;
  return status;
}

#define TREE_LIST_CAP ta.leaf_cap
#define TREE_REDUCED 1
__global__ __launch_bounds__(RES_THREADS) void k_tree_r_m(const TreeModel *__restrict__ tab) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const Dev &d = tab[blockIdx.x].d;
  const TreeArgs &ta = tab[blockIdx.x].ta;
#include "kernels_tree_body.inc"  // the body of k_tree, with the three pieces of the reduced form
}

// ... with round and fix inside (see k_tree_rf)
#define TREE_RF 1
__global__ __launch_bounds__(RES_THREADS) void k_tree_rf_r_m(const TreeModel *__restrict__ tab) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const Dev &d = tab[blockIdx.x].d;
  const TreeArgs &ta = tab[blockIdx.x].ta;
#include "kernels_tree_body.inc"  // the body of k_tree_r_m, with round and fix
}
#undef TREE_RF

// ... with strong / reliability branching inside (see k_tree_sb)
#define TREE_SB 1
__global__ __launch_bounds__(RES_THREADS) void k_tree_sb_r_m(const TreeModel *__restrict__ tab) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const Dev &d = tab[blockIdx.x].d;
  const TreeArgs &ta = tab[blockIdx.x].ta;
#include "kernels_tree_body.inc"  // the body of k_tree_r_m, with strong / reliability branching
}
#undef TREE_SB

// ------------------------------------------------------------------------------------------
// The batch forms of the three kernels above: B MIQPs on ONE such model (miosqp_qp_solve_trees_large, _rf, _sb), workgroup
// b runs instance b as in k_tree -- arguments by value, the per-instance pointers moved on by tree_instance with a leaf
// store of ta.leaf_cap places per instance.  Everything read per model (the triangle's source rows, the packed and dense
// rows of Abar, Pbar's rows, D, E, c) is the engine's own and shared by all workgroups; only q, the staging block, the
// leaf store, the incumbent, the outcome and the rf / sb areas are per instance.  The body, its LDS and its sums are those
// of the _m kernels: an instance comes out bit for bit as k_tree_r_m gives it alone.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RES_THREADS) void k_tree_r(Dev d, TreeArgs ta) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  tree_instance(d, ta, (size_t)ta.leaf_cap);
#include "kernels_tree_body.inc"  // the body of k_tree_r_m
}

#define TREE_RF 1
__global__ __launch_bounds__(RES_THREADS) void k_tree_rf_r(Dev d, TreeArgs ta) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  tree_instance_rf(d, ta, (size_t)ta.leaf_cap);
#include "kernels_tree_body.inc"  // the body of k_tree_rf_r_m
}
#undef TREE_RF

#define TREE_SB 1
__global__ __launch_bounds__(RES_THREADS) void k_tree_sb_r(Dev d, TreeArgs ta) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  tree_instance_sb(d, ta, (size_t)ta.leaf_cap);
#include "kernels_tree_body.inc"  // the body of k_tree_sb_r_m
}
#undef TREE_SB
#undef TREE_REDUCED
#undef TREE_LIST_CAP

// every model's cost vector in one launch: qbar = c D q, the expression (and operation order) of k_scale_q_batch and
// k_scale_q; block b takes entry b (d.qraw -> d.q, both in the arena)
__global__ void k_scale_q_models(const TreeModel *__restrict__ tab) {
  const Dev &d = tab[blockIdx.x].d;
  for (int i = threadIdx.x; i < d.n; i += blockDim.x) d.q[i] = d.c * d.D[i] * d.qraw[i];
}

// ------------------------------------------------------------------------------------------
// The same tree search for n + M <= 64 in ONE WAVEFRONT (BASELINE configs[3]: n + M = 63).  k_tree's iteration costs
// ~5000 cycles at this size: eight waves, two barriers and two LDS round trips for two 63-wide sweeps.  Here lane r
// owns row r of the explicit KKT inverse W (the matrix k_coop spreads over the chip: [nu + rho wh ; x~] = W [wh ; rx],
// dense_setup.hip) in 64 register pairs and the iterates of that row; an iteration is ONE matrix-vector product whose
// right-hand side is read from LDS as broadcasts (every lane reads the same address), then purely lane-local
// updates and one LDS store per lane -- no barrier anywhere (a single wavefront runs in lock step and its LDS
// operations complete in order).  The termination test applies lane r's row of Kc = [0 Abar ; Abar^T Pbar] (kept
// in LDS, 32 KB) to [y ; x] and [proj(dy) ; dx] and reduces the 17 norms / sums with a butterfly.
// Decisions, list semantics and results are those of k_tree; only the summation order inside a node differs.
// ------------------------------------------------------------------------------------------
constexpr int TW = 64;

__device__ __forceinline__ double wave_max64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ double wave_sum64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// y[q] of lane l = x of lane 16 q + l % 16: the four rows of 16 lanes copied to every row, without the LDS crossbar
// (permlane16_swap exchanges the odd rows of its first operand with the even rows of its second, permlane32_swap the
// upper half of the first with the lower half of the second; with both operands equal that duplicates rows / halves)
__device__ __forceinline__ void row_replicate(double x, double (&y)[4]) {
  const unsigned lo = (unsigned)__double2loint(x), hi = (unsigned)__double2hiint(x);
  const auto l16 = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);  // [0] = rows 0 0 2 2, [1] = rows 1 1 3 3
  const auto h16 = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  const auto le = __builtin_amdgcn_permlane32_swap(l16[0], l16[0], false, false);  // [0] = row 0 everywhere, [1] = row 2
  const auto he = __builtin_amdgcn_permlane32_swap(h16[0], h16[0], false, false);
  const auto lod = __builtin_amdgcn_permlane32_swap(l16[1], l16[1], false, false);  // [0] = row 1 everywhere, [1] = row 3
  const auto hod = __builtin_amdgcn_permlane32_swap(h16[1], h16[1], false, false);
  y[0] = __hiloint2double((int)he[0], (int)le[0]);
  y[1] = __hiloint2double((int)hod[0], (int)lod[0]);
  y[2] = __hiloint2double((int)he[1], (int)le[1]);
  y[3] = __hiloint2double((int)hod[1], (int)lod[1]);
}

// acc[v] += sum_c mat[c][r] * x_v[c], c = 0..63 in order, where lane c holds x_v[c] in own[v]: lane r's column of a
// 64 x 64 matrix in LDS against NV vectors that live one entry per lane.  The vectors are copied across the four rows
// of 16 lanes once (xr[v][q] of lane l = own[v] of lane 16 q + l % 16), the matrix entries come 16 at a time from LDS
// (one read per lane, conflict-free), and product c = 16 q + j takes its vector operand from lane j of the row through
// the DPP row broadcast of the FMA.  (A plain loop over LDS paid a round trip per column: 4 us per termination test.)
template <int NV>
__device__ __forceinline__ void lds_col_dot(const double *mat, int r, const double (&own)[NV], double (&acc)[NV]) {
  double xr[NV][4];
#pragma unroll
  for (int v = 0; v < NV; v++) row_replicate(own[v], xr[v]);
  asm volatile("s_nop 1");
#define CD_F(Q, J)                                                                                                   \
  _Pragma("unroll") for (int v = 0; v < NV; v++)                                                                     \
      asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:" #J " row_mask:0xf bank_mask:0xf" : "+v"(acc[v]) : "v"(xr[v][Q]), "v"(a[J]));
#define CD_ROW(Q)                                                                      \
  {                                                                                    \
    double a[16];                                                                      \
    _Pragma("unroll") for (int j = 0; j < 16; j++) a[j] = mat[(16 * (Q) + j) * TW + r]; \
    __builtin_amdgcn_sched_barrier(0);                                                 \
    CD_F(Q, 0) CD_F(Q, 1) CD_F(Q, 2) CD_F(Q, 3) CD_F(Q, 4) CD_F(Q, 5) CD_F(Q, 6) CD_F(Q, 7) CD_F(Q, 8) CD_F(Q, 9)       \
    CD_F(Q, 10) CD_F(Q, 11) CD_F(Q, 12) CD_F(Q, 13) CD_F(Q, 14) CD_F(Q, 15)             \
    __builtin_amdgcn_sched_barrier(0);                                                 \
  }
  CD_ROW(0) CD_ROW(1) CD_ROW(2) CD_ROW(3)
#undef CD_ROW
#undef CD_F
}

__global__ __launch_bounds__(64) void k_tree_w(Dev d, TreeArgs ta) {
  tree_instance(d, ta);
#include "kernels_tree_w_body.inc"  // the body, shared with k_tree_w_m
}

// wavefront b runs entry b of the table (see k_tree_m)
__global__ __launch_bounds__(64) void k_tree_w_m(const TreeModel *__restrict__ tab) {
  const Dev &d = tab[blockIdx.x].d;
  const TreeArgs &ta = tab[blockIdx.x].ta;
#include "kernels_tree_w_body.inc"  // the body of k_tree_w
}
