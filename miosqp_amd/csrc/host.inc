// part of engine.hip (included there, not compiled alone): host side: engine object, allocation, launches, graph capture, solve loops
// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
constexpr int POOL_EVENTS = 8;      // streaming launches that may be in flight at once
constexpr int COOP_RETRY = -1000;  // internal: the cooperative launch was called off, redo in the two-kernel form

inline int pick_tpr(double avg_row) {
  if (avg_row <= 48) return 16;
  if (avg_row <= 192) return 32;
  if (avg_row <= 640) return 64;
  if (avg_row <= 1536) return 128;
  return 256;
}

#define DISPATCH_TPR(tpr, KERNEL, rows, stream, ...)                                              \
  do {                                                                                            \
    switch (tpr) {                                                                                \
      case 16: hipLaunchKernelGGL(KERNEL<16>, dim3(((rows) + 15) / 16), dim3(256), 0, stream, __VA_ARGS__); break;   \
      case 32: hipLaunchKernelGGL(KERNEL<32>, dim3(((rows) + 7) / 8), dim3(256), 0, stream, __VA_ARGS__); break;     \
      case 64: hipLaunchKernelGGL(KERNEL<64>, dim3(((rows) + 3) / 4), dim3(256), 0, stream, __VA_ARGS__); break;     \
      case 128: hipLaunchKernelGGL(KERNEL<128>, dim3(((rows) + 1) / 2), dim3(256), 0, stream, __VA_ARGS__); break;   \
      default: hipLaunchKernelGGL(KERNEL<256>, dim3(rows), dim3(256), 0, stream, __VA_ARGS__); break;                \
    }                                                                                             \
  } while (0)

// stream, events and pinned staging buffers of one engine (cached per process, see rt_acquire below)
// one stream capture at a time in the process (several engines on several host threads: stream.MultiPoolSearch)
std::mutex g_capture_mutex;

// one chunk of an engine's device pool (pool_reserve below)
struct ParkedChunk {
  int device;
  void *p;
  size_t bytes;
};

struct SetupGroup;  // host_setup_models.inc: what the engines of one miosqp_qp_setup_models call share

struct RtBundle {
  int device = -1;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, evc0 = nullptr, evc1 = nullptr, ev_chunk[2] = {nullptr, nullptr};
  hipEvent_t ev_stage[2] = {nullptr, nullptr};  // last upload out of h_in[0, 2M) (bounds) / h_in[2M, ..) (x, y or q)
  double *h_in = nullptr, *h_out = nullptr;
  size_t in_cap = 0, out_cap = 0;  // doubles
  Ctrl *h_ctrl = nullptr, *h_ctrl2 = nullptr;
  unsigned long long *h_tree = nullptr;  // coherent block of the one-wavefront tree launch (engine.hip solve_tree), tree_cap words
  size_t tree_cap = 0;
};

}  // namespace

struct miosqp_qp_engine {
  int n = 0, M = 0;
  int device = -1;  // HIP device ordinal this engine lives on (made current by every entry point)
  miosqp_qp_settings st{};
  miosqp::Scaled sc;
  miosqp::Factor fa;
  Dev d{};
  Dev dh{};  // leaf pool: the 64-column harvest tile (same matrices, its own b_* / c_* arrays)
  RtBundle rt;  // stream, events, pinned staging: from / back to the per-process cache
  SetupGroup *group = nullptr;  // set by miosqp_qp_setup_models: rt's stream and pinned buffers and the first pool chunk are the group's
  TreeArgs ta{};  // whole-tree launch: leaf arrays, incumbent, result record
  bool tree_ready = false;
  // miosqp_qp_solve_trees: per-instance arrays of a batch of trees (capacity tb_cap instances)
  int tb_cap = 0;
  double *tb_q = nullptr, *tb_qraw = nullptr, *tb_raw = nullptr, *tb_lo = nullptr, *tb_hi = nullptr, *tb_x = nullptr, *tb_y = nullptr,
         *tb_inc = nullptr, *tb_upper = nullptr;
  TreeOut *tb_out = nullptr;
  TreeRfOut *tb_rf = nullptr;  // miosqp_qp_solve_trees_rf: the counters of round and fix, per instance
  std::vector<double> tb_host;   // staging: [raw block | inc | upper] in, [inc] out
  std::vector<TreeOut> tb_hout;
  std::vector<TreeRfOut> tb_hrf;
  // miosqp_qp_solve_trees_sb: per instance the work area, Node.pc of every leaf-store place and the counters of strong /
  // reliability branching (capacity tb_sb_cap instances of tb_sb_p integer positions)
  int tb_sb_cap = 0, tb_sb_p = 0;
  double *tb_sbw = nullptr, *tb_sbpc = nullptr;
  TreeSbOut *tb_sb = nullptr;
  std::vector<TreeSbOut> tb_hsb;
  // miosqp_qp_solve_trees_large (_rf, _sb): the arena of a batch of trees in the reduced form (trees_large_plan.hpp; from
  // this engine's pool, capacity in doubles, not shared with tb_*: its leaf stores have leaf_cap places) and its staging
  double *tl_dev = nullptr;
  size_t tl_cap = 0;
  std::vector<double> tl_host;
  // miosqp_qp_solve_trees_models with this engine first: the call's arena (from this engine's pool) and the pinned mirror
  // of its staged part, capacities in doubles
  double *mm_dev = nullptr, *mm_host = nullptr;
  size_t mm_cap = 0, mm_host_cap = 0;
  void *search = nullptr;  // NodeSearch (host_search.inc)
  void *sdriver = nullptr;  // StreamDriver (host_stream.inc)
  void *lockstep = nullptr;  // LockstepStore (host_lockstep.inc)
  std::vector<int> h_iidx;  // host copy of the integer variables' indices
  unsigned long long pool_chunk_total = 0, pool_target[POOL_EVENTS] = {};  // chunks launched since the last reset; per launch: the count when it is done
  bool stage_busy[2] = {false, false};  // an upload out of that part of h_in may still be under way (rt.ev_stage)
  std::vector<void *> allocs;  // pool chunks
  char *pool_base = nullptr;
  size_t pool_cap = 0, pool_used = 0;
  std::vector<ParkedChunk> chunks;  // the pool's chunks among `allocs` (small ones are parked at clean-up, not freed)
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, evc0 = nullptr, evc1 = nullptr;
  double loop_ms = 0.0;
  int64_t loop_iters = 0;
  int64_t run_launches = 0;   // of them: launches of the resident grid (k_coop_run)
  int run_nap_in_use = -1;    // the resident grid's poll delay as of the last run (debug counter 10)
  int64_t run_cal_nodes = 0;  // synthetic nodes its calibration has run (debug counter 11)
  int64_t loop_launches = 0;  // launches of the hosted search's solver kernel (one per node, or one per search_run: k_coop_run)
  // per node of the hosted search since the last reset of the loop statistics: device milliseconds of its launch(es) and
  // its ADMM iterations, in node order (a node's time is read one node later: the vectors may differ by one at the end)
  std::vector<float> node_ms;
  std::vector<int> node_it;
  hipGraph_t g_full = nullptr, g_tail = nullptr;
  hipGraphExec_t x_full = nullptr, x_tail = nullptr;
  int chunk = 25, tail_iters = 0;
  int tpr_pv = 64, tpr_pc = 64, tpr_tail = 64, tpr_pb = 64, tpr_pr = 64;
  int bd_cfg = 0;  // batched dense kernels: 0 = fp64 matrix-core tiles, else 10*row_groups + k_slices (vector FMA)
  int bm_var = 0;  // matrix-core tile variant (waves per workgroup x pipeline depth), MIOSQP_BM_VAR
  // a chunk's lock-step iterations as ONE persistent launch (kernels_bpers.inc): on / fits this problem and device /
  // times it was called off (co-residency) and the chunk went through the launches instead
  bool kbp = false, kbp_capable = false;
  int kbp_fallbacks = 0, kbp_min_cols = 6;
  int64_t kbp_retry_gap = 0, kbp_retry_in = 0;  // chunks between attempts to return to the persistent launch (doubling)
  KbpArgs kbpa{};
  // the streaming batch as one persistent launch (kernels_bstream.inc): built for this pool / chunks per launch of the
  // compiled stream driver / a second stream for slot copies while a launch is running
  bool kbs = false;
  KbsArgs kbsa{};
  int kbs_chunks = 8;
  int64_t kbs_fault_at = 0;  // tests (MIOSQP_KBS_FAULT_AT=k): workgroup 1 of the k-th launch of kbs never shows up -- a call-off mid-stream
  int64_t kbs_launches = 0, kbs_chunks_run = 0, graph_chunks_run = 0;  // the stream's chunks by form (debug counters 7, 8, 9)
  hipStream_t side = nullptr;
  unsigned long long *kbs_prof = nullptr;
  KbsBlock *kbs_blk = nullptr;  // the boundary's copy of the kernel arguments (device memory) and what was last sent there
  KbsBlock kbs_blk_host;
  // leaf pool / streaming batch
  int node_cap = 0, pool_pending = 0;     // node slots of the leaf pool; launches not yet collected
  unsigned long long pool_launched = 0, pool_synced = 0;  // launches so far; at the last full stream synchronisation
  hipEvent_t ev_pool[16] = {};            // (start, end) of the last POOL_EVENTS launches
  int pool_chunks[8] = {};
  unsigned long long pool_seen = 0;       // digests handed to the caller so far
  bool pool_dirty = false;                // solve_batch has used the columns since the last pool_reset
  hipGraph_t g_stream = nullptr;
  hipGraphExec_t x_stream = nullptr;
  ReadyEntry *h_ready = nullptr;
  miosqp_pool_digest *h_dg = nullptr;
  PoolCtl *h_pctl = nullptr;
  int tpr_ff = 256, tpr_fx = 64, tpr_fc = 64;  // product-form kernels: forward rows, x rows, constraint rows
  // pinned staging: [l | u | x0 | y0] in, [x | y] out, ctrl
  double *h_in = nullptr, *h_out = nullptr;
  Ctrl *h_ctrl = nullptr;
  double *d_in = nullptr;
  bool have_int = false;
  bool fold = false;
  bool setup_on_device = false;
  bool res_pending = false, loop_pending = false;
  unsigned long long *h_tree = nullptr;  // coherent host memory of the one-wavefront tree launch: done/ticks | outcome | incumbent
  bool up_on = false;  // uploads of a run are staged and sent together (dupload / upload_flush)
  std::vector<char> up_stage;
  char *up_dev = nullptr;
  size_t up_bytes = 0;
  Ctrl *h_ctrl2 = nullptr;  // two pinned slots for the pipelined chunk loop
  hipEvent_t ev_chunk[2] = {nullptr, nullptr};
  bool resident = false;  // whole solve in one LDS-resident workgroup (small problems)
  bool coop = false;      // register-resident cooperative solver (k_coop), one exchange per iteration
  bool pers = false;      // persistent streaming solver (k_pers): one launch per solve, the factor read from memory every iteration
  bool pers_capable = false;
  PersPlan pp{};
  size_t pers_lds = 0;
  bool coop_timed_out = false;  // set by finish_and_fetch when the control block reports an expired wait
  int64_t coop_fallbacks = 0;   // times this engine left the cooperative form because its workgroups were not co-resident
  bool coop_capable = false;    // setup built the cooperative solver (it may be switched off temporarily)
  int64_t coop_retry_gap = 0, coop_retry_in = 0;  // solves between attempts to return to the cooperative form
  bool spin_wait = true;  // finish_and_fetch polls the final event instead of blocking (MIOSQP_SPIN_WAIT=0)
  int coop_rw = 8, coop_cpt = 4, coop_cptf = 4, coop_T = 0, coop_cus = 0;
  unsigned long long *coop_epi = nullptr;  // exchange buffer of the in-launch node epilogue (kernels_coop.inc: coop_epilogue)
  bool coop_reduced = false;  // the exchange runs without the identity rows (kernels_coop.inc "reduced indices")
  std::vector<int> coop_brow_h;  // host copy of the variables' bound rows in that layout
  bool chip_user = false;   // counted among the engines of this device that launch whole-chip kernels (ChipTurn below)
  bool in_capture = false;  // a stream capture of this engine is under way: no event waits / records around its launches
  hipGraph_t g_stream_a = nullptr, g_stream_b = nullptr;  // the streaming chunk before / after its persistent launch (shared chip)
  hipGraphExec_t x_stream_a = nullptr, x_stream_b = nullptr;
  // residual check of the explicit KKT inverse at set-up (kernels_guard.inc): -1 = no inverse was built
  double guard_resid = -1.0, guard_tol = 0.0;
  bool guard_tripped = false;
  int res_tg1 = 64, res_tg2 = 64;
  size_t res_lds = 0;
  int res_sp_off = -1;             // k_resident: where the LDS copy of the sparse rows starts (doubles), or -1
  size_t sp_nnzA = 0, sp_nnzP = 0;  // entries of the row-compressed Abar / Pbar as stored (padding included)
  miosqp::Folded fo;
  int64_t nnzA = 0, nnzPtriu = 0;
  // batched mode
  int Bcap = 0;  // capacity (columns), multiple of 64; 0 = batched mode not allocated
  double *hb_in = nullptr, *hb_out = nullptr;
  int *hb_int = nullptr;       // status | iter
  double *hb_dbl = nullptr;    // pri | dua | obj | lower
  // derived batches (strong branching, round and fix; derived_begin / derived_end): the parent (l | u | x | y, 3M + n
  // doubles) and strong branching's 32 candidate positions (int32, 16 doubles' room) staged in, the feature's record
  // out (round and fix: the winner's x behind it); device in / device record / ONE pinned block for both directions
  double *der_in = nullptr, *der_rec = nullptr, *h_der = nullptr;
  // polishing (miosqp_qp_polish): the values of A as they were given at set-up (the device holds the scaled copy), and
  // the scratch of the reduced system, built on the first call and freed with the engine
  std::vector<double> A_raw;
  PolishScratch *pol = nullptr;
  miosqp::PolManyScratch *polm = nullptr;  // polishing of many instances in one launch (miosqp_qp_polish_many)
  miosqp::PolManyScratch *polml = nullptr;  // ... beyond one workgroup's LDS (miosqp_qp_polish_many_large): with the slabs
  // captured chunks per tile count; set [1] holds the per-column-cost instantiations (solve_batch_q), set [0] the others
  hipGraphExec_t xb_full[2][16] = {}, xb_tail[2][16] = {};
  hipGraph_t gb_full[2][16] = {}, gb_tail[2][16] = {};
  // solve_trees_refill (host_refill.inc): the chunk with the streaming test on that driver's own column arrays, per tile count
  hipGraphExec_t xr_full[16] = {};
  hipGraph_t gr_full[16] = {};
  int pq = 0;                 // 1 while a solve_batch_q slice is queued: launches and chunk graphs take the <PQ = true> kernels
  double *hb_q = nullptr;     // pinned staging of a slice's raw costs (solve_batch_q, allocated on its first call)
  bool compact = true;   // compaction of converged columns in solve_batch (MIOSQP_COMPACT=0 disables)
  int64_t compactions = 0;
  double bloop_ms = 0.0;
  int64_t bloop_iters = 0, bloop_node_iters = 0;
};

namespace {

void drop_stream_graph(miosqp_qp_engine *e);

// The leaf vectors of add_leaf / take_leaf / pool_write_node / pool_read_node may live in host OR device memory (r05: a
// leaf moves between ranks as ONE device tensor, slot store -> RCCL broadcast -> slot store, no host hop): the copies
// are hipMemcpyDefault, and what the host would have to read itself (the l <= u check) is done only where it may read.
// May the HOST read through p?  Only when the runtime positively says so (pinned / registered / unregistered host memory, or
// managed) -- or does not know the pointer at all, which is what plain malloc'ed memory looks like to runtimes that report
// "invalid value" for it.  A pointer the runtime knows as anything else (device memory, an array) is not dereferenced: a
// device tensor of ANOTHER runtime instance in the process (torch bundles its own) must never reach a host loop.
bool host_may_read(const void *p) {
  hipPointerAttribute_t a;
  const hipError_t rc = hipPointerGetAttributes(&a, p);
  if (rc != hipSuccess) {
    (void)hipGetLastError();
    return rc == hipErrorInvalidValue;
  }
  return a.type == hipMemoryTypeHost || a.type == hipMemoryTypeUnregistered || a.type == hipMemoryTypeManaged;
}

// ------------------------------------------------------------------------------------------
// Whole-chip launches of one process take turns.  k_coop, k_pers and kbp1 / kbp need (nearly) every CU for
// themselves: all their workgroups must be resident before any of them can finish.  Two such launches on two
// streams (two pools of one tree, a pool's chunk and a ramp-up node) that reach the device together each get
// part of the CUs and neither completes until one gives up (the 100 ms call-off).  Inside one process that is
// avoidable: while more than one engine of a device uses these kernels, every such launch first makes its
// stream wait for the event recorded behind the previous one -- whatever stream that was on -- and records its
// own.  Host side: one mutex around {wait, launch, record}; device side: a barrier packet, nothing when the
// predecessor has finished.  With a single engine (the bench's headline) nothing is waited for or recorded.  The
// call-off stays for what this cannot see: other processes on the same device.
// ------------------------------------------------------------------------------------------
struct ChipTurn {
  std::mutex mu;
  int users = 0;
  hipEvent_t ring[64] = {};
  unsigned head = 0;
  hipEvent_t last = nullptr;
  hipStream_t last_stream = nullptr;
  int64_t waits = 0;  // launches that were ordered behind another stream's
};
ChipTurn g_chip[64];

ChipTurn *chip_of(const miosqp_qp_engine *e) { return (e->device >= 0 && e->device < 64) ? &g_chip[e->device] : nullptr; }

int chip_join(miosqp_qp_engine *e) {
  ChipTurn *t = chip_of(e);
  if (!t || e->chip_user || getenv("MIOSQP_NO_CHIP_TURNS")) return 0;
  bool second = false;
  {
    std::lock_guard<std::mutex> lk(t->mu);
    second = ++t->users == 2;
  }
  e->chip_user = true;
  // launches of the first engine that went out unordered must be over before this one's first
  if (second) HIPCHK(hipDeviceSynchronize());
  return 0;
}
void chip_quit(miosqp_qp_engine *e) {
  ChipTurn *t = chip_of(e);
  if (!t || !e->chip_user) return;
  std::lock_guard<std::mutex> lk(t->mu);
  t->users--;
  e->chip_user = false;
}
bool chip_shared(const miosqp_qp_engine *e) {
  ChipTurn *t = chip_of(e);
  if (!t || !e->chip_user) return false;
  std::lock_guard<std::mutex> lk(t->mu);
  return t->users > 1;
}
// brackets ONE whole-chip launch (or a captured graph that holds one) on e->stream
struct ChipGuard {
  ChipTurn *t;
  miosqp_qp_engine *e;
  bool on = false;
  explicit ChipGuard(miosqp_qp_engine *eng) : t(chip_of(eng)), e(eng) {
    if (!t || !e->chip_user || e->in_capture) { t = nullptr; return; }
    t->mu.lock();
    on = t->users > 1;
    if (on && t->last && t->last_stream != e->stream) {
      (void)hipStreamWaitEvent(e->stream, t->last, 0);
      t->waits++;
    }
  }
  ~ChipGuard() {
    if (!t) return;
    if (on) {
      hipEvent_t &ev = t->ring[t->head++ % 64];
      if (!ev && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) ev = nullptr;
      if (ev && hipEventRecord(ev, e->stream) == hipSuccess) {
        t->last = ev;
        t->last_stream = e->stream;
      }
    }
    t->mu.unlock();
  }
  ChipGuard(const ChipGuard &) = delete;
  ChipGuard &operator=(const ChipGuard &) = delete;
};

// Per-process cache of what an engine needs from the runtime besides device memory: its stream, its events and
// its pinned staging buffers.  Creating them costs ~1.7 ms and releasing them ~2.4 ms on ROCm 7.2 -- more than a
// whole small MIQP takes (the reference's benchmark grid sets up 80 engines; an MPC loop that re-factorises
// does the same).  A cleaned-up engine parks them here (at most 8 bundles per process), the next setup on the
// same device takes a bundle whose buffers are large enough.
std::vector<RtBundle> g_rt_cache;
std::mutex g_rt_mutex;
// runtime objects this host thread has created so far (miosqp_qp_setup_models reports what one call added)
thread_local int64_t g_made_device_mallocs = 0, g_made_host_mallocs = 0, g_made_streams = 0;

void rt_destroy(RtBundle &b) {
  if (b.h_in) hipHostFree(b.h_in);
  if (b.h_out) hipHostFree(b.h_out);
  if (b.h_ctrl) hipHostFree(b.h_ctrl);
  if (b.h_ctrl2) hipHostFree(b.h_ctrl2);
  if (b.h_tree) hipHostFree(b.h_tree);
  for (hipEvent_t ev : {b.ev0, b.ev1, b.evc0, b.evc1, b.ev_chunk[0], b.ev_chunk[1], b.ev_stage[0], b.ev_stage[1]})
    if (ev) hipEventDestroy(ev);
  if (b.stream) hipStreamDestroy(b.stream);
  b = RtBundle();
}

// stream, events and pinned buffers for an engine on `device` staging `in_need` / `out_need` doubles
int rt_acquire(int device, size_t in_need, size_t out_need, RtBundle &b) {
  {
    std::lock_guard<std::mutex> lk(g_rt_mutex);
    for (size_t k = 0; k < g_rt_cache.size(); k++)
      if (g_rt_cache[k].device == device && g_rt_cache[k].in_cap >= in_need && g_rt_cache[k].out_cap >= out_need) {
        b = g_rt_cache[k];
        g_rt_cache.erase(g_rt_cache.begin() + k);
        return 0;
      }
  }
  b = RtBundle();
  b.device = device;
  // sizes rounded up (x1.5, at least 4096 doubles) so that a sequence of similar problems reuses one bundle
  b.in_cap = std::max<size_t>(4096, in_need + in_need / 2);
  b.out_cap = std::max<size_t>(4096, out_need + out_need / 2);
  HIPCHK(hipStreamCreateWithFlags(&b.stream, hipStreamNonBlocking));
  g_made_streams++;
  g_made_host_mallocs += 4;
  HIPCHK(hipEventCreate(&b.ev0));
  HIPCHK(hipEventCreate(&b.ev1));
  HIPCHK(hipEventCreate(&b.evc0));
  HIPCHK(hipEventCreate(&b.evc1));
  HIPCHK(hipEventCreateWithFlags(&b.ev_chunk[0], hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&b.ev_chunk[1], hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&b.ev_stage[0], hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&b.ev_stage[1], hipEventDisableTiming));
  HIPCHK(hipHostMalloc((void **)&b.h_in, sizeof(double) * b.in_cap, hipHostMallocDefault));
  HIPCHK(hipHostMalloc((void **)&b.h_out, sizeof(double) * b.out_cap, hipHostMallocDefault));
  HIPCHK(hipHostMalloc((void **)&b.h_ctrl, sizeof(Ctrl), hipHostMallocDefault));
  HIPCHK(hipHostMalloc((void **)&b.h_ctrl2, 2 * sizeof(Ctrl), hipHostMallocDefault));
  return 0;
}

void rt_release(RtBundle &b) {
  if (!b.stream) return;
  {
    std::lock_guard<std::mutex> lk(g_rt_mutex);
    if (g_rt_cache.size() < 8 && !getenv("MIOSQP_NO_CACHE")) {
      g_rt_cache.push_back(b);
      b = RtBundle();
      return;
    }
  }
  rt_destroy(b);
}

// Chunks of cleaned-up engines, kept for the next setup on the same device (hipFree of an 8 MB chunk is ~0.45 ms on
// ROCm 7.2 -- as much as setting a small MIQP up and solving it; at most 8 chunks of at most 32 MB are parked)
std::vector<ParkedChunk> g_chunk_cache;
constexpr size_t CHUNK_PARK_MAX = (size_t)32 << 20;

// Device memory comes from a few large zero-filled chunks (one hipMalloc per chunk instead of one
// per array: setup of a small problem is dominated by allocation calls otherwise).
int pool_reserve(miosqp_qp_engine *e, size_t bytes) {
  void *p = nullptr;
  bytes = (bytes + 4095) & ~(size_t)4095;
  if (bytes <= CHUNK_PARK_MAX) {
    std::lock_guard<std::mutex> lk(g_rt_mutex);
    for (size_t k = 0; k < g_chunk_cache.size(); k++)
      if (g_chunk_cache[k].device == e->device && g_chunk_cache[k].bytes >= bytes) {
        p = g_chunk_cache[k].p;
        bytes = g_chunk_cache[k].bytes;
        g_chunk_cache.erase(g_chunk_cache.begin() + k);
        break;
      }
  }
  const bool parked = p != nullptr;  // a parked chunk was zero-filled (and waited for) when its engine was cleaned up
  if (!p) {
    HIPCHK(hipMalloc(&p, bytes));
    g_made_device_mallocs++;
  }
  // The zero fill must be ORDERED before the first kernel that touches the chunk.  The engine's stream is
  // non-blocking (it does not synchronise with the null stream) and hipMemset on device memory returns
  // before the fill has finished: a null-stream fill of a large chunk (312 MB for 1024 columns at config 2)
  // was still running when the first batched kernels wrote their iterates, and zeroed them again
  // (tests/test_gpu_parity.py::test_config3_full_size_wave_of_256_leaves caught it at 448 columns).
  // Hence: fill, then WAIT -- later users are kernels on the engine's stream and blocking null-stream
  // uploads alike, and only a completed fill is ordered before both.
  if (!parked) {
    HIPCHK(hipMemsetAsync(p, 0, bytes, e->stream));  // stream may still be null during setup: the null stream
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  e->allocs.push_back(p);
  e->chunks.push_back({e->device, p, bytes});
  e->pool_base = (char *)p;
  e->pool_cap = bytes;
  e->pool_used = 0;
  return 0;
}
int pool_alloc(miosqp_qp_engine *e, void **out, size_t bytes) {
  bytes = (bytes + 255) & ~(size_t)255;
  if (e->pool_used + bytes > e->pool_cap) {
    int rc = pool_reserve(e, bytes > ((size_t)8 << 20) ? bytes : ((size_t)8 << 20));
    if (rc) return rc;
  }
  *out = e->pool_base + e->pool_used;
  e->pool_used += bytes;
  return 0;
}
template <typename T>
int dalloc(miosqp_qp_engine *e, T **p, size_t count) {
  return pool_alloc(e, (void **)p, (count ? count : 1) * sizeof(T));
}
// Small uploads that land next to each other in the pool travel as ONE copy (a blocking hipMemcpy is ~10 us however
// small: twenty-odd arrays were half of the set-up time of a small problem).  upload_begin .. upload_flush bracket a
// run of dupload calls; an array above 64 KB, or one that does not continue the run, goes out on its own.
int upload_flush(miosqp_qp_engine *e) {
  if (e->up_bytes) HIPCHK(hipMemcpy(e->up_dev, e->up_stage.data(), e->up_bytes, hipMemcpyHostToDevice));
  e->up_bytes = 0;
  e->up_dev = nullptr;
  return 0;
}
void upload_begin(miosqp_qp_engine *e) { e->up_on = true; }
int upload_end(miosqp_qp_engine *e) {
  e->up_on = false;
  return upload_flush(e);
}
template <typename T>
int dupload(miosqp_qp_engine *e, const std::vector<T> &h, const T **p) {
  T *q = nullptr;
  const size_t want = (h.size() + 64) * sizeof(T);  // slack: tile loads may overshoot a row
  int rc = pool_alloc(e, (void **)&q, want);
  if (rc) return rc;
  *p = q;
  const size_t bytes = h.size() * sizeof(T), span = (want + 255) & ~(size_t)255;  // (what pool_alloc advanced by)
  if (!bytes) return 0;
  if (!e->up_on || bytes > ((size_t)64 << 10)) {
    if (e->up_on) {
      rc = upload_flush(e);
      if (rc) return rc;
    }
    HIPCHK(hipMemcpy(q, h.data(), bytes, hipMemcpyHostToDevice));
    return 0;
  }
  if (e->up_bytes && (char *)q != e->up_dev + e->up_bytes) {
    rc = upload_flush(e);
    if (rc) return rc;
  }
  if (!e->up_bytes) e->up_dev = (char *)q;
  if (e->up_stage.size() < e->up_bytes + span) e->up_stage.resize(e->up_bytes + span);
  memcpy(e->up_stage.data() + e->up_bytes, h.data(), bytes);
  memset(e->up_stage.data() + e->up_bytes + bytes, 0, span - bytes);  // (the pool is zero-filled: so is the slack)
  e->up_bytes += span;
  return 0;
}

void launch_fold_fwd(miosqp_qp_engine *e) {
  const Dev &d = e->d;
  DISPATCH_TPR(e->tpr_ff, k_fold_fwd, d.n, e->stream, d);
}

template <int TX>
void launch_fold_bwd_c(miosqp_qp_engine *e) {
  const Dev &d = e->d;
  const int nbx = (d.n + 256 / TX - 1) / (256 / TX);
#define FB(TC)                                                                                         \
  hipLaunchKernelGGL((k_fold_bwd<TX, TC>), dim3(nbx + (d.M + 256 / TC - 1) / (256 / TC)), dim3(256), 0, \
                     e->stream, d)
  switch (e->tpr_fc) {
    case 32: FB(32); break;
    case 128: FB(128); break;
    case 256: FB(256); break;
    default: FB(64); break;
  }
#undef FB
}

void launch_fold_bwd(miosqp_qp_engine *e) {
  switch (e->tpr_fx) {
    case 16: launch_fold_bwd_c<16>(e); break;
    case 32: launch_fold_bwd_c<32>(e); break;
    case 128: launch_fold_bwd_c<128>(e); break;
    default: launch_fold_bwd_c<64>(e); break;
  }
}

int launch_resident(miosqp_qp_engine *e, int max_iter, int check_every, int final_check) {
  hipLaunchKernelGGL(k_resident, dim3(1), dim3(RES_THREADS), e->res_lds, e->stream, e->d, max_iter, check_every,
                     final_check, e->res_tg1, e->res_tg2, e->res_sp_off);
  return 0;
}

// register layout of the cooperative solver: columns per thread for NR columns (512 threads), rows per workgroup
// (one entry more than NR must fall into some thread's columns: the testers' decision travels as entry NR, kernels_coop.inc)
int coop_pick_cpt(int NR) { return NR < 1024 ? 2 : NR < 1536 ? 3 : 4; }
bool coop_decision_slot(int NR, int cpt) { return NR + 1 <= 512 * cpt; }
int coop_pick_rw(int NR) {
  // 8 rows of W per workgroup.  16 rows -- half the workgroups in the all-to-all, twice the products and a longer
  // butterfly per thread -- measured no faster at any size (r04, tools/probes/coop_layout.py: config 2 reduced layout
  // 1.914 us per iteration with 8 rows, 2.054 with 16; n + M = 900: 1.607 / 1.825): what a round costs is the N entries
  // every workgroup polls, not the number of workgroups.  The kernel stays a template on the row count.
  (void)NR;
  return 8;
}
int coop_pick_testers(int spare) {
  int nt = spare >= 8 ? std::min(COOP_NT_MAX, spare) : 0;
  if (const char *ev = getenv("MIOSQP_COOP_TESTERS")) nt = std::max(0, std::min(std::min(COOP_NT_MAX, spare), atoi(ev)));
  return nt;
}
// Do a tester's rows of Kc fit its registers (kernels_coop.inc: coop_tester<.., RES>)?  And the pick-up lag that goes with
// the answer: iterations between a test and the point where the grid waits for its decision.  From memory the testers
// need ~27 us at config 2 (operands 3, rows 17-21, reduction and decision 5; an iteration takes 1.9): at 12 the grid stood
// still ~5 us at every test (438 k it/s in the hosted search), at 14 / 16 / 18: 458 / 461 / 460 k (r04).  With the rows in
// registers the decision is there ~16 us after the test iteration (operands 3, rows 5.5, the 64 partial results and the
// decision 7.5): lag 6 / 8 / 10 / 16 -> 480 / 513 / 518 / 512 k it/s.
void coop_pick_lag(miosqp_qp_engine *e) {
  Dev &d = e->d;
  const int n = e->n, M = e->M, N = n + M, nt = d.coop_nt;
  bool res = nt > 0 && (N % 2) == 0 && N - (M & ~1) <= 128 * COOP_RC_S && M <= COOP_RC_R * nt * 8 && n <= COOP_RV_R * nt * 8 &&
             N <= 128 * COOP_RV_S;
  if (const char *ev = getenv("MIOSQP_COOP_TRES")) res = res && atoi(ev) != 0;
  d.coop_tres = res ? 1 : 0;
  d.coop_lag = res ? 10 : 16;
  if (const char *ev = getenv("MIOSQP_COOP_LAG")) d.coop_lag = std::max(1, atoi(ev));
}

// every instantiation in use: (rows per workgroup, columns per thread of the exchange, of the test's gathers, testers)
#define COOP_FORMS(X) \
  X(8, 2, 2) X(8, 2, 4) X(8, 3, 4) X(8, 4, 4)
int coop_occupancy(int rw, int cpt, int cptf) {
  int per_cu = 0;
  hipError_t oq = hipErrorInvalidValue;
#define X(RW, CPT, CPTF) \
  if (rw == RW && cpt == CPT && cptf == CPTF) oq = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_coop<512, RW, CPT, CPTF, true>, 512, 0);
  COOP_FORMS(X)
#undef X
  return oq == hipSuccess ? per_cu : 0;
}

void launch_coop(miosqp_qp_engine *e, int max_iter, int check_every, int final_check, const CoopNode *node = nullptr) {
  const Dev &d = e->d;
  CoopNode nd{};
  if (node) nd = *node;
  ChipGuard turn(e);
  // the test on tester workgroups unless tests follow each other more closely than its decision travels
  const bool tst = d.coop_nt > 0 && (check_every <= 0 || check_every > d.coop_lag);
  const int rw = e->coop_rw, cpt = e->coop_cpt, cptf = e->coop_cptf;
#define X(RW, CPT, CPTF)                                                                                              \
  if (rw == RW && cpt == CPT && cptf == CPTF) {                                                                       \
    if (tst)                                                                                                          \
      hipLaunchKernelGGL((k_coop<512, RW, CPT, CPTF, true>), dim3(e->coop_T + d.coop_nt), dim3(512), 0, e->stream, d, \
                         nd, max_iter, check_every, final_check);                                                     \
    else                                                                                                              \
      hipLaunchKernelGGL((k_coop<512, RW, CPT, CPTF, false>), dim3(e->coop_T), dim3(512), 0, e->stream, d, nd,        \
                         max_iter, check_every, final_check);                                                         \
    return;                                                                                                           \
  }
  COOP_FORMS(X)
#undef X
}

void launch_pers(miosqp_qp_engine *e, int max_iter, int check_every, int final_check) {
  ChipGuard turn(e);
  if (e->pp.small)
    hipLaunchKernelGGL(k_pers_small, dim3(e->pp.G), dim3(PERS_B), e->pers_lds, e->stream, e->d, e->pp, max_iter, check_every,
                       final_check);
  else if (e->fold)
    hipLaunchKernelGGL(k_pers<true>, dim3(e->pp.G), dim3(PERS_B), e->pers_lds, e->stream, e->d, e->pp, max_iter, check_every,
                       final_check);
  else if (e->pp.sym)
    hipLaunchKernelGGL((k_pers<false, true>), dim3(e->pp.G), dim3(PERS_B), e->pers_lds, e->stream, e->d, e->pp, max_iter, check_every,
                       final_check);
  else
    hipLaunchKernelGGL(k_pers<false>, dim3(e->pp.G), dim3(PERS_B), e->pers_lds, e->stream, e->d, e->pp, max_iter, check_every,
                       final_check);
}

// The explicit KKT inverse d.W against the scaled matrices d.Kc (kernels_guard.inc): max |K W r - r| / max |r| over
// GUARD_NP probe vectors, one blocking read-back at set-up.  Sets guard_resid / guard_tripped; the caller falls back.
int inverse_guard(miosqp_qp_engine *e) {
  const Dev &d = e->d;
  const int N = e->n + e->M;
  double tol = COOP_GUARD_TOL;
  if (const char *ev = getenv("MIOSQP_GUARD_TOL")) tol = atof(ev);
  e->guard_tol = tol;
  if (tol < 0) {  // switched off
    e->guard_resid = -1.0;
    e->guard_tripped = false;
    return 0;
  }
  double *u = nullptr;
  unsigned long long *out = nullptr;
  int rc = dalloc(e, &u, (size_t)GUARD_NP * N + 8);
  if (!rc) rc = dalloc(e, &out, 8);
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(out, 0, sizeof(unsigned long long), e->stream));
  hipLaunchKernelGGL(kg_apply, dim3((N + 3) / 4), dim3(256), 0, e->stream, d.W, d.ldw, N, e->M, d.rho, u);
  hipLaunchKernelGGL(kg_resid, dim3((N + 3) / 4), dim3(256), 0, e->stream, d.Kc, d.ldw, N, e->M, d.rho_inv, d.sigma, u, out);
  unsigned long long bits = 0;
  HIPCHK(hipMemcpyAsync(&bits, out, sizeof bits, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  double r;
  memcpy(&r, &bits, sizeof r);
  e->guard_resid = r;
  e->guard_tripped = !(r <= tol);
  if (e->guard_tripped)
    fprintf(stderr, "miosqp: explicit KKT inverse residual %.3g above %.3g (ill-conditioned KKT matrix): this engine iterates with "
                    "the factor's sweeps instead\n", r, tol);
  return 0;
}

// lanes per row of the LDS-resident solver's two sweeps: as many as keep every row of a sweep in flight at once
void resident_lane_groups(miosqp_qp_engine *e) {
  auto pow2_floor = [](int v) { int p = 1; while (2 * p <= v) p *= 2; return p; };
  e->res_tg1 = std::min(64, std::max(1, pow2_floor(RES_THREADS / e->n)));
  e->res_tg2 = std::min(64, std::max(1, pow2_floor(RES_THREADS / (e->n + e->M))));
  if (const char *ev = getenv("MIOSQP_RES_TG")) {
    int a1 = 0, b1 = 0;
    if (sscanf(ev, "%d,%d", &a1, &b1) == 2) { e->res_tg1 = a1; e->res_tg2 = b1; }
  }
}

// the tuning hooks of the environment an engine with the product form reads at set-up
void tuning_from_env(miosqp_qp_engine *e) {
  if (const char *ev = getenv("MIOSQP_BD_CFG")) e->bd_cfg = atoi(ev);
  if (const char *ev = getenv("MIOSQP_BM_VAR")) e->bm_var = atoi(ev);
  if (const char *ev = getenv("MIOSQP_SPIN_WAIT")) e->spin_wait = atoi(ev) != 0;
  if (const char *ev = getenv("MIOSQP_COMPACT")) e->compact = atoi(ev) != 0;
  if (const char *ev = getenv("MIOSQP_BM_ABLATE")) e->d.bm_ablate = atoi(ev);
  if (const char *ev = getenv("MIOSQP_FOLD_TPR")) {  // tuning hook: "fwd,x,c"
    int a = 0, b = 0, c = 0;
    if (sscanf(ev, "%d,%d,%d", &a, &b, &c) == 3) {
      e->tpr_ff = a;
      e->tpr_fx = b;
      e->tpr_fc = c;
    }
  }
}

// the registration words of the single-launch solvers start from zero again (after a launch that was called off)
void reset_registration(miosqp_qp_engine *e) {
  if (e->d.coop_reg) (void)hipMemsetAsync(e->d.coop_reg, 0, 128 * sizeof(unsigned long long), e->stream);
  // (and the exchange ring starts afresh: all sentinel is in phase with any round -- a launch that timed out may have
  //  left it half way through one, a changed layout leaves slots behind that its owners no longer reset)
  if (e->d.coop_buf) hipLaunchKernelGGL(k_coop_ring_fill, dim3(16), dim3(256), 0, e->stream, e->d.coop_buf);
  if (e->pp.reg) (void)hipMemsetAsync(e->pp.reg, 0, 128 * sizeof(unsigned long long), e->stream);
}

hipError_t lds_limit_once(const void *fn, int which);

// Row ownership, exchange buffers and launch geometry of the persistent streaming solver (kernels_pers.inc).  Leaves
// e->pers false (no error) when the problem does not fit: more than PERS_RMAX rows of a kind per workgroup, operand
// buffers beyond one workgroup's LDS, or a grid the device cannot hold with one workgroup per CU.
int pers_setup(miosqp_qp_engine *e) {
  const int n = e->n, M = e->M, N = n + M;
  const miosqp::Factor &f = e->fa;
  int dev_now = 0;
  HIPCHK(hipGetDevice(&dev_now));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, dev_now));
  int G = std::min(prop.multiProcessorCount, 256);
  if (const char *ev = getenv("MIOSQP_PERS_GRID")) G = std::max(1, std::min(G, atoi(ev)));
  G = std::min(G, std::max(1, n / 2));  // at least one pair of variable rows per workgroup
  PersPlan &p = e->pp;
  p = PersPlan();
  bool want_si = !e->fold && e->st.pers == 2;
  if (const char *ev = getenv("MIOSQP_PERS_SINV")) want_si = !e->fold && atoi(ev) != 0;
  // S^-1 read as a symmetric matrix (kernels_pers.inc, pers_sym_rows): T x T square tiles of edge C, the T (T + 1) / 2 on and
  // above the diagonal one per workgroup -- half the bytes per iteration, and 2 C operands per workgroup instead of n
  std::vector<int> sym_ij;
  {
    bool sym = want_si && (n & 1) == 0;
    if (const char *ev = getenv("MIOSQP_PERS_SYM")) sym = sym && atoi(ev) != 0;
    if (sym) {
      int T = 1;
      while ((T + 1) * (T + 2) / 2 <= G) T++;
      const int C = 2 * ((n + 2 * T - 1) / (2 * T));  // even: a lane's pair of columns never straddles two tiles
      T = (n + C - 1) / C;
      const int K = (C + 14 + 127) / 128;
      if (T >= 2 && K <= 4) {
        p.sym = 1;
        p.sym_C = C;
        p.sym_T = T;
        p.sym_K = K;
        p.sym_tiles = T * (T + 1) / 2;
        for (int I = 0; I < T; I++)
          for (int J = I; J < T; J++) { sym_ij.push_back(I); sym_ij.push_back(J); }
      }
    }
  }
  p.G = G;
  // variable rows in the order 0, n-1, 1, n-2, ...: consecutive pairs have forward + backward length n - 1
  std::vector<int> vrow(n), vbeg(G + 1), cbeg(G + 1);
  for (int k = 0; k < n; k++) vrow[k] = (k & 1) ? n - 1 - k / 2 : k / 2;
  for (int b = 0; b < G; b++) vbeg[b] = 2 * (int)(((int64_t)b * (n / 2)) / G);
  vbeg[G] = n;
  if (e->fold) {
    for (int b = 0; b <= G; b++) cbeg[b] = (int)(((int64_t)b * M) / G);
  } else {  // sparse rows: equal shares of (entries + a per-row cost: the bound rows have one entry each)
    const std::vector<int> &ptr = f.panel_by_con.ptr;
    const int64_t row_cost = 64, total = ptr[M] + row_cost * M;  // (a sparse phase is paid by the pass of PERS_B / TPR rows more than by the entry)
    int r = 0;
    for (int b = 0; b < G; b++) {
      const int64_t want = (total * b) / G;
      while (r < M && ptr[r] + row_cost * r < want) r++;
      cbeg[b] = r;
    }
    cbeg[G] = M;
  }
  p.vmax = p.cmax = 0;
  for (int b = 0; b < G; b++) {
    p.vmax = std::max(p.vmax, vbeg[b + 1] - vbeg[b]);
    p.cmax = std::max(p.cmax, cbeg[b + 1] - cbeg[b]);
  }
  if (p.cmax > PERS_RMAX && (M + G - 1) / G <= PERS_RMAX) {  // too many short rows in one share: equal row counts instead
    for (int b = 0; b <= G; b++) cbeg[b] = (int)(((int64_t)b * M) / G);
    p.cmax = (M + G - 1) / G;
  }
  if (p.vmax > PERS_RMAX || p.cmax > PERS_RMAX) return 0;
  // segments per dense row: enough (row, segment) tasks for the eight waves, none shorter than 256 columns
  auto segs = [](double rows, double len) {
    int S = 1;
    while (S < 8 && rows * S < 8.0 && len / (2 * S) >= 256.0) S *= 2;
    return S;
  };
  const double nv_avg = (double)n / G, nc_avg = (double)M / G;
  p.s_f = segs(nv_avg, e->fold ? M + 0.5 * n : 0.5 * n);
  p.s_x = segs(nv_avg + (e->fold ? nc_avg : 0.0), 0.5 * n);
  p.s_c = segs(nv_avg + nc_avg, (double)n);
  if (const char *ev = getenv("MIOSQP_PERS_SEGS")) {
    int a = 0, b2 = 0, c = 0;
    if (sscanf(ev, "%d,%d,%d", &a, &b2, &c) == 3 && a >= 1 && b2 >= 1 && c >= 1 && a <= 8 && b2 <= 8 && c <= 8) { p.s_f = a; p.s_x = b2; p.s_c = c; }
  }
  auto tpr64 = [](int t) { return t > 64 ? 64 : t; };
  p.tpr_v = tpr64(pick_tpr((double)f.nnz_panel / n));
  p.tpr_c = tpr64(pick_tpr((double)f.nnz_panel / M));
  p.tpr_p = tpr64(pick_tpr((double)f.Pbar.nnz / n));
  p.len_a = (((e->fold ? N : n) + 1) & ~1) + 4;
  p.len_b = ((n + 1) & ~1) + 4;
  if (p.sym) {  // the symmetric phase's operands and sums lie in the two buffers (one stretch of LDS), see pers_sym_lds
    const int need = pers_sym_lds(p.sym_C, p.sym_K, p.vmax, p.sym_T).res;
    if (p.len_a + p.len_b < need) p.len_b = need - p.len_a;
  }
  const int smax = std::max(p.s_f, std::max(p.s_x, p.s_c));
  const size_t lds_doubles = (size_t)p.len_a + p.len_b + (size_t)(p.vmax + p.cmax) * smax + p.vmax + 4 * (size_t)(p.vmax + p.cmax) +
                             PERS_NW * NQ + 16 * NQ + NQ;
  // ... + 4 ints, the task descriptors of the two dense phases (int4 each) and the owned variable rows
  const size_t lds_ints = 4 + 4 * ((size_t)p.vmax * p.s_f + (size_t)p.vmax * p.s_x + (size_t)p.cmax * p.s_c) + p.vmax;
  const size_t lds_ints_al = 4 + 4 * ((size_t)p.vmax * p.s_f + (size_t)p.vmax * p.s_x + (size_t)p.cmax * p.s_c) + ((p.vmax + 3) & ~3);
  (void)lds_ints;
  e->pers_lds = ((lds_doubles + 1) / 2 * 2 * sizeof(double) + lds_ints_al * sizeof(int) + 15) & ~(size_t)15;
  if (e->pers_lds > 160 * 1024) return 0;
  p.tin_M = M;
  {  // the test's y and projected dy whole in LDS when they fit (rows of a dense A^T: hundreds of indexed fetches per lane otherwise)
    const size_t extra = 2 * (size_t)((M + 1) & ~1) * sizeof(double);
    if (e->pers_lds + extra <= 128 * 1024 && !getenv("MIOSQP_PERS_TEST_SPARSE")) {
      p.test_full = 1;
      e->pers_lds += extra;
    }
  }
  if (p.sym) {  // what is left of the workgroup's LDS, and the two operand buffers behind the symmetric phase's own
    // few KB, hold the first rows of every wave's share of the tile (re-read after a test, whose operands lie there)
    int keep = 1;
    if (const char *ev = getenv("MIOSQP_PERS_RESIDENT")) keep = atoi(ev);
    const int Wc = 128 * p.sym_K, first = pers_sym_lds(p.sym_C, p.sym_K, p.vmax, p.sym_T).res;
    if (keep) {
      const size_t room = e->pers_lds + 512 < 160 * 1024 ? 160 * 1024 - 512 - e->pers_lds : 0;
      const int extra = (int)(room / sizeof(double)) & ~15;
      p.len_b += extra;
      e->pers_lds += sizeof(double) * (size_t)extra;
      const int rows_max = (p.sym_C + PERS_NW - 1) / PERS_NW;
      p.sym_res = std::min(rows_max, std::max(0, (p.len_a + p.len_b - first) / (PERS_NW * Wc)));
    }
  }
  {  // S^-1 form: what is left of the workgroup's LDS holds the last columns of its rows of S^-1 for the whole launch
    bool si = !e->fold && e->st.pers == 2;
    if (const char *ev = getenv("MIOSQP_PERS_SINV")) si = !e->fold && atoi(ev) != 0;
    int keep = 1;
    if (const char *ev = getenv("MIOSQP_PERS_RESIDENT")) keep = atoi(ev);
    p.res_c0 = p.res_w = 0;
    if (si && keep && !p.test_full && p.vmax > 0 && !p.sym) {
      const size_t room = e->pers_lds + 512 < 160 * 1024 ? 160 * 1024 - 512 - e->pers_lds : 0;
      // the streamed part [0, res_c0) in whole wave-instructions per segment (128 columns x s_f): a lane's piece count per
      // task is a ceiling, so only whole pieces taken off every task are bytes taken off the stream
      const int wmax = std::min((int)(room / (sizeof(double) * (size_t)p.vmax)) & ~1, n / 2), unit = 128 * p.s_f;
      const int c0 = (n - wmax + unit - 1) / unit * unit;
      if (wmax >= 128 && c0 + 128 <= n) {
        p.res_c0 = c0;
        p.res_w = (n - c0 + 1) & ~1;
        e->pers_lds += sizeof(double) * (size_t)p.vmax * p.res_w;
      }
    }
  }
  {  // the lean kernel: product form, every wave at most one task per dense phase, a task at most PERS_U pieces per lane
    bool sm = e->fold && N <= 4 * PERS_B && !getenv("MIOSQP_PERS_GENERAL");
    for (int b = 0; b < G && sm; b++) {
      const int nvb = vbeg[b + 1] - vbeg[b], ncb = cbeg[b + 1] - cbeg[b];
      sm = nvb * p.s_f <= PERS_NW && nvb * p.s_x + ncb * p.s_c <= PERS_NW;
    }
    const int per_f = ((M + n + p.s_f - 1) / p.s_f + 127) / 128 + 1, per_b = ((n + std::min(p.s_x, p.s_c) - 1) / std::min(p.s_x, p.s_c) + 127) / 128 + 1;
    if (per_f > PERS_U || per_b > PERS_U) sm = false;
    p.small = sm ? 1 : 0;
  }
  HIPCHK(lds_limit_once(p.small ? (const void *)k_pers_small : e->fold ? (const void *)k_pers<true>
                                  : p.sym ? (const void *)k_pers<false, true> : (const void *)k_pers<false>,
                        p.small ? 4 : e->fold ? 2 : p.sym ? 10 : 3));
  int per_cu = 0;
  const hipError_t oq = p.small ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_pers_small, PERS_B, e->pers_lds)
                        : e->fold ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_pers<true>, PERS_B, e->pers_lds)
                        : p.sym   ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_pers<false, true>, PERS_B, e->pers_lds)
                                  : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_pers<false>, PERS_B, e->pers_lds);
  if (oq != hipSuccess || per_cu < 1 || G > prop.multiProcessorCount) return 0;
  int *dv = nullptr, *dvb = nullptr, *dcb = nullptr;
  int rc = dalloc(e, &dv, (size_t)n);
  if (!rc) rc = dalloc(e, &dvb, (size_t)G + 1);
  if (!rc) rc = dalloc(e, &dcb, (size_t)G + 1);
  if (!rc) rc = dalloc(e, &p.x_w, 2 * (size_t)N + 64);
  if (!rc) rc = dalloc(e, &p.x_u, 2 * (size_t)n + 64);
  if (!rc) rc = dalloc(e, &p.x_t, 2 * (size_t)n + 64);
  if (!rc && p.sym) rc = dalloc(e, &p.x_p, 4 * (size_t)p.sym_tiles * p.sym_C + 64);
  if (!rc && p.sym) {
    int *dij = nullptr;
    rc = dalloc(e, &dij, sym_ij.size());
    if (!rc) HIPCHK(hipMemcpy(dij, sym_ij.data(), sizeof(int) * sym_ij.size(), hipMemcpyHostToDevice));
    p.sym_ij = reinterpret_cast<const int2 *>(dij);
  }
  if (!rc) rc = dalloc(e, &p.k_x, 2 * (size_t)n + 64);
  if (!rc) rc = dalloc(e, &p.k_dx, 2 * (size_t)n + 64);
  if (!rc) rc = dalloc(e, &p.k_y, 2 * (size_t)M + 64);
  if (!rc) rc = dalloc(e, &p.k_v, 2 * (size_t)M + 64);
  if (!rc) rc = dalloc(e, &p.q, (size_t)(256 + 16) * COOP_QS + 64);
  if (!rc) rc = dalloc(e, &p.reg, 128);
  if (!rc) rc = dalloc(e, &p.tag, 64);
  double *zp = nullptr;
  if (!rc) rc = dalloc(e, &zp, 64);  // (the pool is zero-filled)
  if (rc) return rc;
  p.zero = zp;
  p.x_r = p.x_w + 2 * (size_t)M;  // [wh ; rx] is one vector in the product form
  {
    const Dev &d = e->d;
    const PersTestIn ti{d.pc_ptr, d.pc_idx, d.pv_ptr, d.pv_idx, d.pb_ptr, d.pb_idx, d.pc_A, d.pv_At, d.pb_val, d.Einv, d.E, d.Dinv,
                        d.D, d.ctrl, n, M, d.c, d.cinv, d.eps_abs, d.eps_rel, d.eps_pinf, d.eps_dinf};
    PersTestIn *dti = nullptr;
    rc = dalloc(e, &dti, 1);
    if (rc) return rc;
    HIPCHK(hipMemcpy(dti, &ti, sizeof ti, hipMemcpyHostToDevice));
    p.tin = dti;
  }
  HIPCHK(hipMemcpy(dv, vrow.data(), sizeof(int) * n, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dvb, vbeg.data(), sizeof(int) * (G + 1), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dcb, cbeg.data(), sizeof(int) * (G + 1), hipMemcpyHostToDevice));
  p.vrow = dv; p.vbeg = dvb; p.cbeg = dcb;
  // Factor form: the tail as the explicit inverse of the reduced Hessian, S^-1 = L22^-T D22^-1 L22^-1 (dense n x n: exactly
  // the bytes of the two triangles it replaces).  x~ = S^-1 c is ONE row-parallel phase with rows of equal length where
  // the factor needs two (the two triangular sweeps, an all-to-all exchange and the skew of the triangular rows between
  // them) -- the same step k_coop takes for the whole KKT matrix.  Built once on the device from L22^-1 and D22
  // (n^3 / 3 multiply-adds); the factor itself stays: the multi-kernel fallback and the batched path use it.
  // pers = 2 asks for it; MIOSQP_PERS_SINV=0 / 1 overrides.
  {
    bool want = !e->fold && e->st.pers == 2;
    if (const char *ev = getenv("MIOSQP_PERS_SINV")) want = !e->fold && atoi(ev) != 0;
    if (want) {
      double *si = nullptr;
      p.sinv_ld = p.sym ? (n + 15) & ~15 : e->d.ld;  // (symmetric form: every row starts a 128-byte line)
      rc = dalloc(e, &si, (size_t)n * p.sinv_ld + 64);
      if (!rc) rc = miosqp_device_kkt_inverse(e->d.Linv, e->d.ld, e->d.d2inv, n, 0, si, p.sinv_ld, e->stream);
      if (rc) return rc;
      p.sinv = si;
    }
  }
  p.nap = p.small ? 13 : 8;  // (64-clock units; measured on MI355X: config 2 4.85 us per iteration at 12-14, 5.4 at 4)
  if (const char *ev = getenv("MIOSQP_PERS_NAP")) p.nap = std::max(0, atoi(ev));
  if (const char *ev = getenv("MIOSQP_PERS_DBG")) p.dbg = atoi(ev);
  if (const char *ev = getenv("MIOSQP_COOP_DBG")) e->d.coop_dbg = atoi(ev);  // (64: fault injection, see k_pers)
  e->pers = true;
  e->pers_capable = true;
  return 0;
}

// The nap between publishing and the first poll of a round (kernels_coop.inc) has a sharp optimum that
// depends on the number of workgroups in the exchange and on the device: time a hundred iterations from
// zero iterates for a few candidates (coarse grid, then its neighbours) and keep the best.  The result is
// remembered per (device, grid size, register layout) for the life of the process, so a stream of MIQPs of
// one shape calibrates once.  MIOSQP_COOP_NAP=<n> pins it.  Numerics do not depend on it.
struct NapKey {
  int dev, T, cpt;  // cpt: columns per thread + 100 when a workgroup holds 16 rows (the file format's third field)
  bool operator<(const NapKey &o) const { return std::tie(dev, T, cpt) < std::tie(o.dev, o.T, o.cpt); }
};
std::map<NapKey, int> g_nap_cache;
std::mutex g_nap_mutex;

// Persistent side of the cache: "<device name>|<CUs>|<T>|<cpt>|<nap>" lines in
//   $MIOSQP_CACHE_DIR/coop_nap.txt (default ~/.cache/miosqp_amd/), written after every calibration, and
//   coop_nap_table.txt next to libmiosqp_hip.so (read-only, shipped: values measured on MI355X),
// so a fresh process -- and, through the shipped table, a fresh machine -- sets up without the ~9 ms of
// timed launches.  The value only affects speed, never results.
std::string nap_device_key(int dev) {
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return "unknown|0";
  return std::string(prop.name) + "|" + std::to_string(prop.multiProcessorCount);
}
std::string nap_user_file() {
  std::string dir;
  if (const char *ev = getenv("MIOSQP_CACHE_DIR")) dir = ev;
  else if (const char *home = getenv("HOME")) dir = std::string(home) + "/.cache/miosqp_amd";
  else return "";
  return dir + "/coop_nap.txt";
}
std::string nap_shipped_file() {
  Dl_info info;
  if (!dladdr((const void *)&nap_device_key, &info) || !info.dli_fname) return "";
  std::string path(info.dli_fname);
  const size_t slash = path.find_last_of('/');
  return (slash == std::string::npos ? std::string(".") : path.substr(0, slash)) + "/coop_nap_table.txt";
}
// `tol`: how far the grid size of a line may be from T (0 for the user's own cache; the shipped table holds
// a coarse grid of sizes and the optimum moves slowly with T, so the nearest entry within 8 is taken)
bool nap_lookup_file(const std::string &file, const std::string &devkey, int T, int cpt, int tol, int *nap) {
  if (file.empty()) return false;
  FILE *f = fopen(file.c_str(), "r");
  if (!f) return false;
  char line[512];
  int best_dist = tol + 1;
  const std::string want = devkey + "|";
  while (fgets(line, sizeof line, f)) {
    if (strncmp(line, want.c_str(), want.size()) != 0) continue;
    int t = 0, c = 0, v = -1;
    if (sscanf(line + want.size(), "%d|%d|%d", &t, &c, &v) != 3 || c != cpt || v < 0 || v > 255) continue;
    const int dist = t > T ? t - T : T - t;
    if (dist <= best_dist && dist <= tol) {  // the last of equally near lines wins (a re-calibration appends)
      best_dist = dist;
      *nap = v;
    }
  }
  fclose(f);
  return best_dist <= tol;
}
void nap_store_file(const std::string &devkey, int T, int cpt, int nap) {
  const std::string file = nap_user_file();
  if (file.empty() || getenv("MIOSQP_NO_CACHE")) return;
  const size_t slash = file.find_last_of('/');
  std::string dir = file.substr(0, slash);
  for (size_t i = 1; i <= dir.size(); i++)  // mkdir -p
    if (i == dir.size() || dir[i] == '/') (void)mkdir(dir.substr(0, i).c_str(), 0755);
  if (FILE *f = fopen(file.c_str(), "a")) {
    fprintf(f, "%s|%d|%d|%d\n", devkey.c_str(), T, cpt, nap);
    fclose(f);
  }
}

int calibrate_coop_nap(miosqp_qp_engine *e) {
  Dev &d = e->d;
  if (const char *ev = getenv("MIOSQP_COOP_NAP")) {
    d.coop_nap = atoi(ev);
    return 0;
  }
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  const int cpt_key = e->coop_cpt + (e->coop_rw == 16 ? 100 : 0);
  const NapKey key{dev, e->coop_T, cpt_key};
  {
    std::lock_guard<std::mutex> lk(g_nap_mutex);
    auto it = g_nap_cache.find(key);
    if (it != g_nap_cache.end()) {
      d.coop_nap = it->second;
      return 0;
    }
  }
  const std::string devkey = nap_device_key(dev);
  if (!getenv("MIOSQP_NO_CACHE")) {
    int nap = 0;
    if (nap_lookup_file(nap_user_file(), devkey, e->coop_T, cpt_key, 0, &nap) ||
        nap_lookup_file(nap_shipped_file(), devkey, e->coop_T, cpt_key, 8, &nap)) {
      d.coop_nap = nap;
      std::lock_guard<std::mutex> lk(g_nap_mutex);
      g_nap_cache[key] = nap;
      return 0;
    }
  }
  const int big = e->n > e->M ? e->n : e->M, iters = 100;
  auto timed = [&](int nap, float *best) -> int {  // best of two
    for (int rep = 0; rep < 2; rep++) {
      d.coop_nap = nap;
      hipLaunchKernelGGL(k_zero_iterates, dim3((big + 255) / 256), dim3(256), 0, e->stream, d);
      hipLaunchKernelGGL(k_reset_ctrl, dim3(1), dim3(1), 0, e->stream, d);
      hipLaunchKernelGGL(k_init_wh, dim3((big + 255) / 256), dim3(256), 0, e->stream, d);
      HIPCHK(hipEventRecord(e->ev0, e->stream));
      launch_coop(e, iters, 0, 0);
      HIPCHK(hipEventRecord(e->ev1, e->stream));
      HIPCHK(hipStreamSynchronize(e->stream));
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, e->ev0, e->ev1));
      if (rep == 0 || ms < *best) *best = ms;
    }
    return 0;
  };
  float ms = 0;
  int rc = timed(16, &ms);  // warm-up (first launch of the kernel)
  if (rc) return rc;
  int best = 0;
  float best_ms = 1e30f;
  auto consider = [&](int nap) -> int {
    float m = 0;
    int r = timed(nap, &m);
    if (!r && m < best_ms) {
      best_ms = m;
      best = nap;
    }
    return r;
  };
  for (int nap = 0; nap <= 24 && !rc; nap += 4) rc = consider(nap);
  const int centre = best;
  if (!rc && centre >= 2) rc = consider(centre - 2);
  if (!rc) rc = consider(centre + 2);
  if (rc) return rc;
  d.coop_nap = best;
  {
    std::lock_guard<std::mutex> lk(g_nap_mutex);
    g_nap_cache[key] = best;
  }
  nap_store_file(devkey, e->coop_T, cpt_key, best);
  hipLaunchKernelGGL(k_zero_iterates, dim3((big + 255) / 256), dim3(256), 0, e->stream, d);
  hipLaunchKernelGGL(k_reset_ctrl, dim3(1), dim3(1), 0, e->stream, d);
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}

// miosqp_qp_set_integer_rows on an engine with the cooperative solver: when every integer-bound row is an identity row
// (one entry, at its variable's column, no variable with two), the exchange drops them (kernels_coop.inc "reduced
// indices"): W' gathered from W on the device, the grid and its register layout chosen for NR = m_orig + n, the poll
// delay looked up / calibrated for the new grid.  Otherwise (or with MIOSQP_COOP_IDROWS=0) the full layout is (re)instated.
int coop_set_layout(miosqp_qp_engine *e, int NR, int mg, const double *W, int ldw, const int *brow, const double *aj) {
  Dev &d = e->d;
  const int rw = coop_pick_rw(NR), cpt = coop_pick_cpt(NR);
  if (coop_occupancy(rw, cpt, e->coop_cptf) < 1) return 1;
  d.coop_W = W;
  d.coop_ldw = ldw;
  d.coop_mg = mg;
  d.coop_brow = brow;
  d.coop_aj = aj;
  d.coop_stride = 2 * rw;
  const bool grid_changed = e->coop_rw != rw || e->coop_T != (NR + rw - 1) / rw;
  e->coop_rw = rw;
  e->coop_cpt = cpt;
  e->coop_T = (NR + rw - 1) / rw;
  d.coop_nt = coop_decision_slot(NR, cpt) ? coop_pick_testers(e->coop_cus - e->coop_T) : 0;
  coop_pick_lag(e);
  if (grid_changed) reset_registration(e);  // a launch's registration target is a multiple of ITS grid size
  else hipLaunchKernelGGL(k_coop_ring_fill, dim3(16), dim3(256), 0, e->stream, d.coop_buf);  // (slots of the old layout)
  return 0;
}
int coop_drop_identity_rows(miosqp_qp_engine *e, int n_int, const int32_t *i_idx, int m_orig) {
  if (!e->coop_capable) return 0;
  Dev &d = e->d;
  const int n = e->n, M = e->M;
  std::vector<int> brow(n, -1);
  std::vector<double> aj(n, 0.0);
  bool ok = n_int >= 1;
  if (const char *ev = getenv("MIOSQP_COOP_IDROWS"))
    if (atoi(ev) == 0) ok = false;
  const miosqp::PCsr &C = e->fa.panel_by_con;
  for (int k = 0; k < n_int && ok; k++) {
    const int j = m_orig + k;
    int cnt = 0, col = -1;
    double val = 0.0;
    for (int t = C.ptr[j]; t < C.ptr[j + 1]; t++)
      if (e->fa.A_val[t] != 0.0) { cnt++; col = C.idx[t]; val = e->fa.A_val[t]; }
    ok = cnt == 1 && col == i_idx[k] && brow[col] < 0;
    if (ok) { brow[col] = j; aj[col] = val; }
  }
  if (ok && e->coop_reduced && brow == e->coop_brow_h) return 0;  // the same rows as before: nothing to do
  HIPCHK(hipStreamSynchronize(e->stream));  // (no launch of the old layout is in flight when the fields change)
  if (ok) {
    const int NR = m_orig + n, ldr = (NR + 7) & ~7;
    double *Wr = nullptr, *ajd = nullptr;
    int *bd = nullptr;
    int rc = pool_reserve(e, ((size_t)NR * ldr + 2 * (size_t)n + 256) * sizeof(double));
    if (!rc) rc = dalloc(e, &Wr, (size_t)NR * ldr + 64);
    if (!rc) rc = dalloc(e, &ajd, (size_t)n);
    if (!rc) rc = dalloc(e, &bd, (size_t)n);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(ajd, aj.data(), sizeof(double) * n, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(bd, brow.data(), sizeof(int) * n, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));  // (the sources are locals)
    hipLaunchKernelGGL(k_coop_reduce_w, dim3((ldr + 255) / 256, NR), dim3(256), 0, e->stream, d.W, d.ldw, Wr, ldr, m_orig,
                       M - m_orig, NR);
    if (coop_set_layout(e, NR, m_orig, Wr, ldr, bd, ajd) == 0) {
      e->coop_reduced = true;
      e->coop_brow_h = brow;
      return e->coop ? calibrate_coop_nap(e) : 0;
    }
  }
  if (e->coop_reduced) {  // back to the full layout (rows that are no identity rows, or a grid the device cannot hold)
    if (coop_set_layout(e, n + M, M, d.W, d.ldw, nullptr, nullptr)) return MIOSQP_EHIP;
    e->coop_reduced = false;
    e->coop_brow_h.clear();
    return e->coop ? calibrate_coop_nap(e) : 0;
  }
  return 0;
}

void launch_iteration(miosqp_qp_engine *e) {
  const Dev &d = e->d;
  if (e->coop) {
    launch_coop(e, 1, 0, 0);
    return;
  }
  if (e->pers) {
    launch_pers(e, 1, 0, 0);
    return;
  }
  if (e->fold) {
    launch_fold_fwd(e);
    launch_fold_bwd(e);
    return;
  }
  DISPATCH_TPR(e->tpr_pv, k_panel_fwd, d.n, e->stream, d);
  DISPATCH_TPR(e->tpr_tail, k_tail_fwd, d.n, e->stream, d);
  DISPATCH_TPR(e->tpr_tail, k_tail_bwd, d.n, e->stream, d);
  DISPATCH_TPR(e->tpr_pc, k_panel_bwd, d.M, e->stream, d);
}

void launch_check(miosqp_qp_engine *e, int iters_in_chunk) {
  const Dev &d = e->d;
  DISPATCH_TPR(e->tpr_pc, k_check_con, d.M, e->stream, d);
  // P rows and A^T rows in one launch; both use 64 threads per row
  const int nblk = 2 * ((d.n + 3) / 4);
  hipLaunchKernelGGL((k_check_var<64, 64>), dim3(nblk), dim3(256), 0, e->stream, d);
  hipLaunchKernelGGL(k_check_decide, dim3(1), dim3(256), 0, e->stream, d, iters_in_chunk);
}

int capture_chunk(miosqp_qp_engine *e, int iters, hipGraph_t *g, hipGraphExec_t *x) {
  std::lock_guard<std::mutex> capture_lock(g_capture_mutex);
  HIPCHK(hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal));
  e->in_capture = true;
  for (int i = 0; i < iters; i++) launch_iteration(e);
  launch_check(e, iters);
  e->in_capture = false;
  HIPCHK(hipStreamEndCapture(e->stream, g));
  HIPCHK(hipGraphInstantiate(x, *g, nullptr, nullptr, 0));
  return 0;
}

double wall() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// runs the ADMM loop on the device until a status is decided or max_iter is reached
int run_loop(miosqp_qp_engine *e) {
  if (e->resident) {
    HIPCHK(hipEventRecord(e->evc0, e->stream));
    int rc = launch_resident(e, e->st.max_iter, e->st.check_termination, 1);
    if (rc) return rc;
    HIPCHK(hipEventRecord(e->evc1, e->stream));
    e->res_pending = true;
    return 0;
  }
  if (e->coop || e->pers) {  // the single-launch solvers run the whole loop, tests included, in one launch
    HIPCHK(hipEventRecord(e->evc0, e->stream));
    if (e->coop) launch_coop(e, e->st.max_iter, e->st.check_termination, 1);
    else launch_pers(e, e->st.max_iter, e->st.check_termination, 1);
    HIPCHK(hipEventRecord(e->evc1, e->stream));
    e->res_pending = true;
    return 0;
  }
  // One chunk is always queued AHEAD of the one whose verdict the host is waiting for, so the GPU
  // never idles across the host round trip; every kernel of a chunk exits at once when the
  // previous test already decided (ctrl->done).
  const int nfull = e->st.max_iter / e->chunk;
  const int total = nfull + (e->tail_iters > 0 ? 1 : 0);
  HIPCHK(hipEventRecord(e->evc0, e->stream));
  auto enqueue = [&](int k) -> int {
    HIPCHK(hipGraphLaunch(k < nfull ? e->x_full : e->x_tail, e->stream));
    HIPCHK(hipMemcpyAsync(&e->h_ctrl2[k & 1], e->d.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipEventRecord(e->ev_chunk[k & 1], e->stream));
    return 0;
  };
  int rc = enqueue(0);
  if (rc) return rc;
  for (int k = 0; k < total; k++) {
    if (k + 1 < total) {
      rc = enqueue(k + 1);
      if (rc) return rc;
    }
    HIPCHK(hipEventSynchronize(e->ev_chunk[k & 1]));
    if (e->h_ctrl2[k & 1].done) break;
  }
  HIPCHK(hipEventRecord(e->evc1, e->stream));
  e->loop_pending = true;
  return 0;
}

int finish_and_fetch(miosqp_qp_engine *e, int node, double *x_out, double *y_out, miosqp_qp_info *info,
                     double t0) {
  const Dev &d = e->d;
  hipLaunchKernelGGL(k_finish, dim3(1), dim3(1024), 0, e->stream, d, node, e->st.max_iter);
  if (node) {
    if (d.digest) DISPATCH_TPR(e->tpr_pc, k_heur_rows, d.M, e->stream, d);
    DISPATCH_TPR(e->tpr_pr, k_obj_rows, d.n, e->stream, d);
    hipLaunchKernelGGL(k_obj_sum, dim3(1), dim3(1024), 0, e->stream, d);
  }
  HIPCHK(hipMemcpyAsync(e->h_out, d.out_x, sizeof(double) * (e->n + e->M), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(e->h_ctrl, d.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipEventRecord(e->ev1, e->stream));
  if (e->spin_wait) {
    // the answer is ~1 ms away and the caller does nothing meanwhile: polling the event saves the
    // wake-up latency of a blocking wait on every node
    hipError_t q;
    while ((q = hipEventQuery(e->ev1)) == hipErrorNotReady) {}
    if (q != hipSuccess) HIPCHK(q);
  } else {
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  if (e->h_ctrl->pad) {
    reset_registration(e);
    g_err = "cooperative solver: " + std::string(e->h_ctrl->pad == 1 ? "the grid was not co-resident within 100 ms (device shared?)"
                                                                     : "exchange timed out") + ", stage " + std::to_string(e->h_ctrl->pad);
    e->res_pending = e->loop_pending = false;
    if (e->h_ctrl->pad == 1) return COOP_RETRY;  // called off before anything was modified
    return MIOSQP_EHIP;
  }
  memcpy(x_out, e->h_out, sizeof(double) * e->n);
  memcpy(y_out, e->h_out + e->n, sizeof(double) * e->M);
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, e->ev0, e->ev1));
  if (e->res_pending || e->loop_pending) {
    float lms = 0;
    HIPCHK(hipEventElapsedTime(&lms, e->evc0, e->evc1));
    e->loop_ms += lms;
    e->loop_iters += e->h_ctrl->iter;
    e->res_pending = e->loop_pending = false;
  }
  info->status_val = e->h_ctrl->status;
  info->iter = e->h_ctrl->iter;
  info->obj_val = e->h_ctrl->obj_val;
  info->pri_res = e->h_ctrl->pri_res;
  info->dua_res = e->h_ctrl->dua_res;
  info->lower = e->h_ctrl->lower;
  info->int_inf = node ? e->h_ctrl->int_inf : -1;
  info->nextvar = node ? e->h_ctrl->nextvar : -1;
  info->heur_viol = e->h_ctrl->heur_viol;
  info->heur_obj = e->h_ctrl->heur_obj;
  info->device_time = 1e-3 * ms;
  info->run_time = wall() - t0;
  return 0;
}


// The cooperative launch was called off (its workgroups were not co-resident: something else is using the
// device).  This engine continues in the two-kernel product form, which has no such requirement, and tries the
// cooperative form again after `coop_retry_gap` further solves (doubling each time it fails again).  Not silent:
// one line on stderr per fall-back.  Shared by solve(), solve_node() and debug_iterate().
int leave_coop(miosqp_qp_engine *e) {
  fprintf(stderr, "miosqp: %s; this engine continues with the multi-kernel form\n", g_err.c_str());
  e->coop = false;
  e->pers = false;
  e->coop_fallbacks++;
  e->coop_retry_gap = e->coop_retry_gap ? std::min<int64_t>(2 * e->coop_retry_gap, 1 << 16) : 256;
  e->coop_retry_in = e->coop_retry_gap;
  if (!e->x_full) {
    int rc = capture_chunk(e, e->chunk, &e->g_full, &e->x_full);
    if (!rc && e->tail_iters > 0) rc = capture_chunk(e, e->tail_iters, &e->g_tail, &e->x_tail);
    if (rc) return rc;
  }
  return 0;
}
// called at the start of a solve: time to try the cooperative form again?
void maybe_rejoin_coop(miosqp_qp_engine *e) {
  if (e->coop || e->pers || !(e->coop_capable || e->pers_capable) || e->coop_retry_in <= 0) return;
  if (--e->coop_retry_in == 0) {
    if (e->coop_capable) e->coop = true;
    else e->pers = true;
  }
}

// ---- batched mode (host) -------------------------------------------------------------------
// the captured chunks of both sets (they hold the iteration kernels and Dev by value); the stream must be idle
void drop_chunk_graphs(miosqp_qp_engine *e) {
  for (int s = 0; s < 2; s++)
    for (int k = 0; k < 16; k++) {
      if (e->xb_full[s][k]) hipGraphExecDestroy(e->xb_full[s][k]);
      if (e->xb_tail[s][k]) hipGraphExecDestroy(e->xb_tail[s][k]);
      if (e->gb_full[s][k]) hipGraphDestroy(e->gb_full[s][k]);
      if (e->gb_tail[s][k]) hipGraphDestroy(e->gb_tail[s][k]);
      e->xb_full[s][k] = e->xb_tail[s][k] = nullptr;
      e->gb_full[s][k] = e->gb_tail[s][k] = nullptr;
    }
  for (int k = 0; k < 16; k++) {
    if (e->xr_full[k]) hipGraphExecDestroy(e->xr_full[k]);
    if (e->gr_full[k]) hipGraphDestroy(e->gr_full[k]);
    e->xr_full[k] = nullptr;
    e->gr_full[k] = nullptr;
  }
}

// which: 0 forward sweep, 1 backward sweep; workgroup shape from e->bd_cfg (row groups x k slices)
void launch_bd(miosqp_qp_engine *e, int ntiles, int which) {
  const Dev &d = e->d;
  if (e->bd_cfg == 0) {  // fp64 matrix-core tiles: 16 rows x 32 columns per workgroup
    const int nbx = (d.n + 15) / 16, nbc = (d.wh_m + 15) / 16, ncol = ntiles * (64 / BM_COLS);
    // e->bm_var (MIOSQP_BM_VAR = 10 * forward + backward): waves per workgroup x pipeline depth, see the table
#define BMF(KS, DP) hipLaunchKernelGGL((kbm_fwd<KS, DP>), dim3(bm_grid(nbx, ncol)), dim3(KS * 64), 0, e->stream, d, ncol)
#define BMB(KS, DP)                                                                                                             \
  do {                                                                                                                          \
    if (e->pq) hipLaunchKernelGGL((kbm_bwd<KS, DP, true>), dim3(bm_grid(nbx + nbc, ncol)), dim3(KS * 64), 0, e->stream, d, ncol); \
    else hipLaunchKernelGGL((kbm_bwd<KS, DP>), dim3(bm_grid(nbx + nbc, ncol)), dim3(KS * 64), 0, e->stream, d, ncol);            \
  } while (0)
    if (which == 0) {
      switch (e->bm_var / 10) {
        case 1: BMF(8, 6); break;
        case 2: BMF(16, 3); break;
        case 3: BMF(8, 4); break;
        case 4: BMF(16, 2); break;
        case 8: hipLaunchKernelGGL((kbm_fwd<8, 3, 1>), dim3(bm_grid(nbx, ncol)), dim3(512), 0, e->stream, d, ncol); break;  // debug: no loads in the loop
        case 9: hipLaunchKernelGGL((kbm_fwd<8, 3, 2>), dim3(bm_grid(nbx, ncol)), dim3(512), 0, e->stream, d, ncol); break;  // debug: no matrix-core work
        default: BMF(8, 3); break;
      }
    } else {
      switch (e->bm_var % 10) {
        case 1: BMB(8, 3); break;
        case 2: BMB(16, 2); break;
        case 3: BMB(16, 1); break;
        case 4: BMB(8, 4); break;
        default: BMB(8, 2); break;
      }
    }
#undef BMF
#undef BMB
    return;
  }
#define BD(RG, KS)                                                                                         \
  do {                                                                                                     \
    constexpr int R = BdCfg<RG, KS>::ROWS, T = BdCfg<RG, KS>::THREADS;                                      \
    const int nbx = (d.n + R - 1) / R, nbc = (d.M + R - 1) / R;                                            \
    if (which == 0) hipLaunchKernelGGL((kbd_fwd<RG, KS>), dim3(nbx, ntiles), dim3(T), 0, e->stream, d);      \
    else if (e->pq) hipLaunchKernelGGL((kbd_bwd<RG, KS, true>), dim3(nbx + nbc, ntiles), dim3(T), 0, e->stream, d); \
    else hipLaunchKernelGGL((kbd_bwd<RG, KS>), dim3(nbx + nbc, ntiles), dim3(T), 0, e->stream, d);           \
  } while (0)
  switch (e->bd_cfg) {
    case 24: BD(2, 4); break;
    case 44: BD(4, 4); break;
    case 22: BD(2, 2); break;
    case 28: BD(2, 8); break;
    default: BD(4, 2); break;
  }
#undef BD
}

// the persistent form of a chunk's iterations for this many column tiles?  (narrow batches leave column groups idle:
// the launches spread their row blocks over the whole chip instead)
bool kbp_here(const miosqp_qp_engine *e, int ntiles) { return e->kbp && ntiles * (64 / BM_COLS) >= e->kbp_min_cols; }

// tick + `iters` lock-step iterations in one launch (kbp does the tick itself once it knows it will run)
void launch_kbp(miosqp_qp_engine *e, const Dev &d, int ntiles, int iters, bool prof = false) {
  KbpArgs ka = e->kbpa;
  ka.ncol = ntiles * (64 / BM_COLS);
  ka.iters = iters;
  const bool one = ka.ncol <= KBP_G && !getenv("MIOSQP_KBP_GENERAL");  // one tile per group: the iterates stay in registers
  const size_t lds = KBP_LDS_DOUBLES * sizeof(double);
  ChipGuard turn(e);
  if (e->pq && one) hipLaunchKernelGGL((kbp1<false, true>), dim3(KBP_WGS), dim3(512), lds, e->stream, d, ka);  // (no profiled form)
  else if (e->pq) hipLaunchKernelGGL((kbp<false, true>), dim3(KBP_WGS), dim3(512), lds, e->stream, d, ka);
  else if (one && prof) hipLaunchKernelGGL(kbp1<true>, dim3(KBP_WGS), dim3(512), lds, e->stream, d, ka);
  else if (one) hipLaunchKernelGGL(kbp1<false>, dim3(KBP_WGS), dim3(512), lds, e->stream, d, ka);
  else if (prof) hipLaunchKernelGGL(kbp<true>, dim3(KBP_WGS), dim3(512), lds, e->stream, d, ka);
  else hipLaunchKernelGGL(kbp<false>, dim3(KBP_WGS), dim3(512), lds, e->stream, d, ka);
}

// called once the batched arrays exist (wh_m is final): does kbp cover this problem on this device?
int kbp_setup(miosqp_qp_engine *e, int want) {
  const Dev &d = e->d;
  e->kbp = e->kbp_capable = false;
  if (const char *ev = getenv("MIOSQP_KBP")) want = atoi(ev);
  if (const char *ev = getenv("MIOSQP_KBP_MIN_COLS")) e->kbp_min_cols = std::max(1, atoi(ev));
  if (want == 0 || !e->fold || e->bd_cfg != 0) return 0;
  if (d.n > 16 * KBP_MEMBERS || d.wh_m > 2 * 16 * KBP_MEMBERS || d.wh_m + d.n > 16 * KBP_KS * KBP_FC) return 0;
  if (want < 0 && d.n < 256) return 0;  // small factors: a member's 16 rows are mostly padding, the launches do better
  int dev_now = 0;
  HIPCHK(hipGetDevice(&dev_now));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, dev_now));
  if (prop.multiProcessorCount < KBP_WGS) return 0;
  HIPCHK(lds_limit_once((const void *)kbp<false>, 5));
  HIPCHK(lds_limit_once((const void *)kbp<true>, 6));
  HIPCHK(lds_limit_once((const void *)kbp1<false>, 7));
  HIPCHK(lds_limit_once((const void *)kbp1<true>, 8));
  HIPCHK(lds_limit_once((const void *)kbp<false, true>, 11));
  HIPCHK(lds_limit_once((const void *)kbp1<false, true>, 12));
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kbp<false>, 512, KBP_LDS_DOUBLES * sizeof(double)) != hipSuccess || per_cu < 1)
    return 0;
  int rc = dalloc(e, &e->kbpa.reg, 64);
  if (!rc) rc = dalloc(e, &e->kbpa.bar, 16 * KBP_G);
  if (rc) return rc;
  e->kbp_capable = e->kbp = true;
  if (const char *ev = getenv("MIOSQP_COOP_DBG")) e->d.coop_dbg = atoi(ev);  // (64: fault injection)
  return chip_join(e);
}

// kbp was called off (ctrl->pad == 1: the 256 workgroups were not co-resident within 100 ms, nothing was modified):
// from now on this engine's chunks go through the launches.  The captured chunks are dropped (they hold kbp).
void drop_stream_graph(miosqp_qp_engine *e);
int kbp_leave(miosqp_qp_engine *e) {
  fprintf(stderr, "miosqp: batched persistent sweeps: the 256 workgroups were not co-resident within 100 ms (device shared?); "
                  "this engine continues with two launches per iteration and tries again later\n");
  e->kbp = false;
  e->kbp_fallbacks++;
  e->kbp_retry_gap = e->kbp_retry_gap ? std::min<int64_t>(2 * e->kbp_retry_gap, 1 << 14) : 64;
  e->kbp_retry_in = e->kbp_retry_gap;
  HIPCHK(hipStreamSynchronize(e->stream));
  drop_chunk_graphs(e);
  drop_stream_graph(e);
  HIPCHK(hipMemsetAsync(&e->d.ctrl->pad, 0, sizeof(int), e->stream));
  HIPCHK(hipMemsetAsync(e->kbpa.reg + 32, 0, sizeof(unsigned long long), e->stream));
  return 0;
}

// called where no captured chunk of this engine is in flight: time to try the persistent launch again?  (`n` chunks have
// gone through the launches since the last call)
int maybe_rejoin_kbp(miosqp_qp_engine *e, int64_t n) {
  if (e->kbp || !e->kbp_capable || e->kbp_retry_in <= 0) return 0;
  e->kbp_retry_in -= n;
  if (e->kbp_retry_in > 0) return 0;
  e->kbp_retry_in = 0;
  HIPCHK(hipStreamSynchronize(e->stream));
  drop_chunk_graphs(e);  // (the captured chunks hold the launches)
  drop_stream_graph(e);
  e->kbp = true;
  return 0;
}

void launch_iteration_b(miosqp_qp_engine *e, int ntiles) {
  const Dev &d = e->d;
  if (e->fold) {
    launch_bd(e, ntiles, 0);
    launch_bd(e, ntiles, 1);
    return;
  }
  if (e->pq) hipLaunchKernelGGL(kb_panel_fwd<true>, dim3((d.n + 3) / 4, ntiles), dim3(256), 0, e->stream, d);
  else hipLaunchKernelGGL(kb_panel_fwd<false>, dim3((d.n + 3) / 4, ntiles), dim3(256), 0, e->stream, d);
  hipLaunchKernelGGL(kb_tail_fwd, dim3((d.n + 3) / 4, ntiles), dim3(256), 0, e->stream, d);
  hipLaunchKernelGGL(kb_tail_bwd, dim3((d.n + 3) / 4, ntiles), dim3(256), 0, e->stream, d);
  hipLaunchKernelGGL(kb_panel_bwd, dim3((d.M + 3) / 4, ntiles), dim3(256), 0, e->stream, d);
}

int capture_chunk_b(miosqp_qp_engine *e, int iters, int ntiles, hipGraph_t *g, hipGraphExec_t *x) {
  const Dev &d = e->d;
  std::lock_guard<std::mutex> capture_lock(g_capture_mutex);
  HIPCHK(hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal));
  e->in_capture = true;
  if (kbp_here(e, ntiles)) {
    launch_kbp(e, d, ntiles, iters);
  } else {
    hipLaunchKernelGGL(kb_tick, dim3(1), dim3(1), 0, e->stream, d, iters);
    for (int i = 0; i < iters; i++) launch_iteration_b(e, ntiles);
  }
  if (e->fold && e->bd_cfg == 0) {
    const int ncol = ntiles * (64 / BM_COLS);
    hipLaunchKernelGGL(kbm_check_con, dim3(bm_grid((d.M + 15) / 16, ncol)), dim3(BMC_KS * 64), 0, e->stream, d, ncol);
    hipLaunchKernelGGL(kbm_check_var, dim3(bm_grid(2 * ((d.n + 15) / 16), ncol)), dim3(BMC_KS * 64), 0, e->stream, d, ncol);
  } else {
    hipLaunchKernelGGL(kb_check_con, dim3((d.M + 3) / 4, ntiles), dim3(256), 0, e->stream, d);
    hipLaunchKernelGGL(kb_check_var, dim3(2 * ((d.n + 3) / 4), ntiles), dim3(256), 0, e->stream, d);
  }
  if (e->pq) hipLaunchKernelGGL(kb_check_reduce<true>, dim3(ntiles, KR), dim3(256), 0, e->stream, d);
  else hipLaunchKernelGGL(kb_check_reduce<false>, dim3(ntiles, KR), dim3(256), 0, e->stream, d);
  hipLaunchKernelGGL(kb_check_decide, dim3(ntiles), dim3(256), 0, e->stream, d);
  e->in_capture = false;
  HIPCHK(hipStreamEndCapture(e->stream, g));
  HIPCHK(hipGraphInstantiate(x, *g, nullptr, nullptr, 0));
  return 0;
}

int alloc_batch(miosqp_qp_engine *e, int cap) {
  Dev &d = e->d;
  const size_t n = e->n, M = e->M;
  const size_t Bs = ((size_t)cap + 63) & ~(size_t)63;
  d.Bs = (int)Bs;
  {
    int rc0 = pool_reserve(e, Bs * ((size_t)24 * M + (size_t)16 * n + 544 + 7 * 16 + 64) * 8 + ((size_t)1 << 16));
    if (rc0) return rc0;
  }
#define ALB(field, count)                            \
  do {                                               \
    int rc__ = dalloc(e, &d.field, (size_t)(count)); \
    if (rc__) return rc__;                           \
  } while (0)
  // right-hand arrays of the matrix-core tiles carry 16 rows of (zero) slack: whole 16-deep chunks are read
  const size_t S16 = 16 * Bs;
  ALB(b_l, M * Bs); ALB(b_u, M * Bs); ALB(b_x, n * Bs + S16); ALB(b_z, M * Bs); ALB(b_y, M * Bs + S16); ALB(b_wh, (M + n) * Bs + S16);
  ALB(b_cv, n * Bs); ALB(b_ut, n * Bs + S16); ALB(b_xt, n * Bs); ALB(b_dx, n * Bs + S16); ALB(b_dy, M * Bs);
  ALB(b_sm, 8 * M * Bs + S16); ALB(b_sn, 4 * n * Bs); ALB(b_xfin, n * Bs); ALB(b_yfin, M * Bs); ALB(b_xi, n * Bs); ALB(b_xis, n * Bs);
  ALB(c_intinf, Bs); ALB(c_nextvar, Bs); ALB(c_hviol, Bs); ALB(c_hobj, Bs); ALB(c_node, Bs); ALB(c_pairs, 2 * Bs);
  ALB(b_part, (Bs / 64) * 32 * 17 * 64);
  ALB(b_raw, Bs * (3 * M + n)); ALB(b_out, Bs * (n + M));
  ALB(c_done, Bs); ALB(c_status, Bs); ALB(c_iter, Bs); ALB(c_pri, Bs); ALB(c_dua, Bs); ALB(c_obj, Bs);
  ALB(c_lower, Bs);
  {
    double *z = nullptr;
    int rcz = dalloc(e, &z, 64);
    if (rcz) return rcz;
    d.b_zero = z;
  }
#undef ALB
  d.b_rx = d.b_wh + (size_t)d.wh_m * Bs;  // [ wh(rows in the products) | rx | wh(bound rows outside them) ]
  {
    int rck = kbp_setup(e, e->st.batch_pers);
    if (rck) return rck;
  }
  HIPCHK(hipHostMalloc((void **)&e->hb_in, sizeof(double) * Bs * (3 * M + n), hipHostMallocDefault));
  HIPCHK(hipHostMalloc((void **)&e->hb_out, sizeof(double) * Bs * (n + M), hipHostMallocDefault));
  HIPCHK(hipHostMalloc((void **)&e->hb_int, sizeof(int) * 6 * Bs, hipHostMallocDefault));
  HIPCHK(hipHostMalloc((void **)&e->hb_dbl, sizeof(double) * 6 * Bs, hipHostMallocDefault));
  e->Bcap = (int)Bs;
  return 0;
}

// batched mode on first use: settings.max_batch columns, 64 without the setting, 1024 at the most
int ensure_batch(miosqp_qp_engine *e) {
  if (e->Bcap == 0) {
    int cap = e->st.max_batch > 1 ? e->st.max_batch : 64;
    if (cap > 1024) cap = 1024;
    return alloc_batch(e, cap);
  }
  return 0;
}

// Before a slice of B columns is queued: the checks and the chunk graphs of its width (captured on an idle stream)
int slice_begin(miosqp_qp_engine *e, int B) {
  const int ntiles = (B + 63) / 64;
  if (ntiles > 16) { g_err = "solve_batch: more than 1024 columns per slice"; return MIOSQP_EARG; }
  if (e->pool_pending) { g_err = "solve_batch: streaming chunks are still in flight (pool_collect first)"; return MIOSQP_EARG; }
  e->pool_dirty = true;
  if (int rcj = maybe_rejoin_kbp(e, 8)) return rcj;
  if (!e->xb_full[e->pq][ntiles - 1]) {
    int rc = capture_chunk_b(e, e->chunk, ntiles, &e->gb_full[e->pq][ntiles - 1], &e->xb_full[e->pq][ntiles - 1]);
    if (!rc && e->tail_iters > 0)
      rc = capture_chunk_b(e, e->tail_iters, ntiles, &e->gb_tail[e->pq][ntiles - 1], &e->xb_tail[e->pq][ntiles - 1]);
    if (rc) return rc;
  }
  return 0;
}

void launch_ls_heur_rows(miosqp_qp_engine *e, const LsRoots &roots, int ntiles);  // (host_lockstep.inc)

// what slice_run needs to end a wave with its mandatory columns (host_lockstep_ahead.inc): behind every chunk one more
// small launch counts the mandatory columns the test has not decided yet, and the count comes down with the Ctrl copy
struct LsNeed {
  const int *mand;       // device, per node of the slice: the wave waits for this column
  int *d_left, *h_left;  // the count on the device / pinned
  int chunks;            // OUT: chunks run (a tail counts as one)
  bool cut;              // OUT: the loop ended on the count with iterations still to run -- columns with c_done == 0 are unfinished
};
void launch_ls_need(miosqp_qp_engine *e, const LsNeed &need, int B);  // (host_lockstep_ahead.inc)

// The lock-step solve of the B nodes staged in d.b_raw (node-major l | u | x0 | y0), up to `max_iter` iterations:
// full chunks of check_termination iterations, then the tail graph for the rest only when max_iter is the engine's own
// (a strong-branching cap is a multiple of check_termination: no tail).  Ends with the per-column epilogue
// (unscale, clamp, digest, objective) in c_status / c_iter / c_lower / b_xfin / b_yfin, node order through c_node.
// roots: the columns belong to trees with root bounds of their own (kernels_lockstep.inc) -- the rounded points are
// judged against those; nullptr (every other caller): against the engine's root, today's launches.
// need: the chunk loop also ends when no mandatory column is undecided (above); nullptr (every other caller): today's
// launches and today's loop.
int slice_run(miosqp_qp_engine *e, int B, int max_iter, const LsRoots *roots = nullptr, LsNeed *need = nullptr) {
  const Dev &d = e->d;
  const size_t n = e->n, M = e->M;
  const int ntiles = (B + 63) / 64;
  hipLaunchKernelGGL(kb_reset, dim3((d.Bs + 255) / 256), dim3(256), 0, e->stream, d, B);
  const int big = (int)(n > M ? n : M);
  if (e->pq) hipLaunchKernelGGL(kb_prepare<true>, dim3((big + 3) / 4, ntiles), dim3(256), 0, e->stream, d, B);
  else hipLaunchKernelGGL(kb_prepare<false>, dim3((big + 3) / 4, ntiles), dim3(256), 0, e->stream, d, B);
  hipLaunchKernelGGL(kb_warm_z, dim3((d.M + 3) / 4, ntiles), dim3(256), 0, e->stream, d);
  const int nfull = max_iter / e->chunk;
  const bool tail = max_iter == e->st.max_iter && e->tail_iters > 0;
  bool done = false, stop = false;  // (stop: only with `need`)
  int decided = 0;
  int cur = ntiles;  // tiles still launched; shrinks as the wave is compacted
  if (need) {
    need->chunks = 0;
    need->cut = false;
  }
  for (int k = 0; k < nfull && !done && !stop; k++) {
    HIPCHK(hipEventRecord(e->evc0, e->stream));
    {
      ChipGuard turn(e);  // (the captured chunk may hold a whole-chip launch)
      HIPCHK(hipGraphLaunch(e->xb_full[e->pq][cur - 1], e->stream));
    }
    HIPCHK(hipEventRecord(e->evc1, e->stream));
    if (need) launch_ls_need(e, *need, B);
    HIPCHK(hipMemcpyAsync(e->h_ctrl, d.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, e->stream));
    if (need) HIPCHK(hipMemcpyAsync(need->h_left, need->d_left, sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e->evc0, e->evc1));
    e->bloop_ms += ms;
    e->bloop_iters += e->chunk;
    e->bloop_node_iters += (int64_t)e->chunk * (B - decided);  // columns still iterating in this chunk
    if (e->h_ctrl->pad) {
      if (e->h_ctrl->pad != 1) {
        g_err = "batched persistent sweeps: a group barrier timed out, stage " + std::to_string(e->h_ctrl->pad);
        return MIOSQP_EHIP;
      }
      // called off before anything was modified (the test that followed decided nothing): this chunk again, as launches
      e->bloop_iters -= e->chunk;
      e->bloop_node_iters -= (int64_t)e->chunk * (B - decided);
      int rc = kbp_leave(e);
      if (!rc) rc = capture_chunk_b(e, e->chunk, cur, &e->gb_full[e->pq][cur - 1], &e->xb_full[e->pq][cur - 1]);
      if (!rc && e->tail_iters > 0) rc = capture_chunk_b(e, e->tail_iters, cur, &e->gb_tail[e->pq][cur - 1], &e->xb_tail[e->pq][cur - 1]);
      if (rc) return rc;
      k--;
      continue;
    }
    decided = e->h_ctrl->ndone;
    done = e->h_ctrl->done != 0;
    if (need) {
      need->chunks++;
      if (!done && *need->h_left == 0) {
        stop = true;
        need->cut = k + 1 < nfull || tail;
      }
    }
    const int active = B - decided, want = (active + 63) / 64;
    if (!done && !stop && e->compact && want < cur) {
      // move the still-iterating columns into the first `want` tiles
      const int cols = cur * 64;
      int *flags = e->hb_int;  // scratch: the info arrays are only filled at the end
      HIPCHK(hipMemcpyAsync(flags, d.c_done, sizeof(int) * cols, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipStreamSynchronize(e->stream));
      int *pairs = e->hb_int + cols;
      int np = 0, lo = 0, hi = cols - 1;
      for (;;) {
        while (lo < active && !flags[lo]) lo++;      // a decided column inside the front region
        while (hi >= active && flags[hi]) hi--;      // a live column behind it
        if (lo >= active || hi < active) break;
        pairs[2 * np] = lo;
        pairs[2 * np + 1] = hi;
        np++;
        flags[lo] = 0;
        flags[hi] = 1;
      }
      if (np > 0) {
        HIPCHK(hipMemcpyAsync(d.c_pairs, pairs, sizeof(int) * 2 * np, hipMemcpyHostToDevice, e->stream));
        const int rows = (int)(M + n);
        if (e->pq) hipLaunchKernelGGL(kb_swap_cols<true>, dim3((rows + 255) / 256, np), dim3(256), 0, e->stream, d, np);
        else hipLaunchKernelGGL(kb_swap_cols<false>, dim3((rows + 255) / 256, np), dim3(256), 0, e->stream, d, np);
      }
      cur = want;
      if (!e->xb_full[e->pq][cur - 1]) {
        int rc = capture_chunk_b(e, e->chunk, cur, &e->gb_full[e->pq][cur - 1], &e->xb_full[e->pq][cur - 1]);
        if (!rc && e->tail_iters > 0)
          rc = capture_chunk_b(e, e->tail_iters, cur, &e->gb_tail[e->pq][cur - 1], &e->xb_tail[e->pq][cur - 1]);
        if (rc) return rc;
      }
      e->compactions++;
    }
  }
  while (!done && !stop && tail) {
    // the last max_iter % check_termination iterations: the same call-off handling as a full chunk -- a persistent
    // launch that was called off iterated nothing and its test decided nothing, so the tail is redone as launches
    {
      ChipGuard turn(e);
      HIPCHK(hipGraphLaunch(e->xb_tail[e->pq][cur - 1], e->stream));
    }
    HIPCHK(hipMemcpyAsync(e->h_ctrl, d.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (!e->h_ctrl->pad) {
      if (need) need->chunks++;
      break;
    }
    if (e->h_ctrl->pad != 1) {
      g_err = "batched persistent sweeps: a group barrier timed out, stage " + std::to_string(e->h_ctrl->pad);
      return MIOSQP_EHIP;
    }
    int rc = kbp_leave(e);
    if (!rc) rc = capture_chunk_b(e, e->chunk, cur, &e->gb_full[e->pq][cur - 1], &e->xb_full[e->pq][cur - 1]);
    if (!rc) rc = capture_chunk_b(e, e->tail_iters, cur, &e->gb_tail[e->pq][cur - 1], &e->xb_tail[e->pq][cur - 1]);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(kb_finish, dim3(ntiles), dim3(1024), 0, e->stream, d, B);
  if (d.digest && roots) launch_ls_heur_rows(e, *roots, ntiles);
  else if (d.digest) hipLaunchKernelGGL(kb_heur_rows, dim3((d.M + 3) / 4, ntiles), dim3(256), 0, e->stream, d);
  if (e->pq) hipLaunchKernelGGL(kb_obj_rows<true>, dim3((d.n + 3) / 4, ntiles), dim3(256), 0, e->stream, d);
  else hipLaunchKernelGGL(kb_obj_rows<false>, dim3((d.n + 3) / 4, ntiles), dim3(256), 0, e->stream, d);
  hipLaunchKernelGGL(kb_obj_sum, dim3(ntiles), dim3(1024), 0, e->stream, d);
  return 0;
}

// A derived batch (kernels_derived.inc), up to the point where the caller's builder kernel turns the uploaded parent
// into B nodes in d.b_raw: bounds check, batched mode and the staging blocks on first use, slice_begin, then
// l | u | x | y | extra (strong branching's candidate positions) through the pinned block into der_in.  *t0: when the
// call's wall time starts (after the one-time allocations).
int derived_begin(miosqp_qp_engine *e, int B, const double *l, const double *u, const double *x, const double *y,
                  const void *extra, size_t extra_bytes, double *t0) {
  const size_t n = e->n, M = e->M;
  for (size_t j = 0; j < M; j++)
    if (l[j] > u[j]) return MIOSQP_EBOUNDS;
  if (int rc = ensure_batch(e)) return rc;
  if (!e->h_der) {  // (the last of the three to be allocated)
    const size_t nin = 3 * M + n + SB_MAX_K / 2, nrec = std::max((sizeof(SbRec) + 7) / 8, RF_REC_DOUBLES + n);
    int rc = dalloc(e, &e->der_in, nin);
    if (!rc) rc = dalloc(e, &e->der_rec, nrec);
    if (rc) return rc;
    HIPCHK(hipHostMalloc((void **)&e->h_der, sizeof(double) * std::max(nin, nrec), hipHostMallocDefault));
  }
  *t0 = wall();
  if (int rc = slice_begin(e, B)) return rc;
  double *h = e->h_der;
  memcpy(h, l, sizeof(double) * M);
  memcpy(h + M, u, sizeof(double) * M);
  memcpy(h + 2 * M, x, sizeof(double) * n);
  memcpy(h + 2 * M + n, y, sizeof(double) * M);
  if (extra_bytes) memcpy(h + 3 * M + n, extra, extra_bytes);
  HIPCHK(hipEventRecord(e->ev0, e->stream));
  HIPCHK(hipMemcpyAsync(e->der_in, h, sizeof(double) * (3 * M + n) + extra_bytes, hipMemcpyHostToDevice, e->stream));
  return 0;
}

// ... and once the caller's judge kernels are queued: the first rec_doubles of der_rec into the pinned block, the
// stream drained, the device time from the upload to here
int derived_end(miosqp_qp_engine *e, size_t rec_doubles, double *device_seconds) {
  HIPCHK(hipMemcpyAsync(e->h_der, e->der_rec, sizeof(double) * rec_doubles, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipEventRecord(e->ev1, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, e->ev0, e->ev1));
  *device_seconds = 1e-3 * ms;
  return 0;
}

// solve_batch_q on first use: the three cost arrays behind the batched ones, and the pinned block the raw costs travel through
int ensure_batch_q(miosqp_qp_engine *e) {
  if (e->d.b_q) return 0;
  const size_t n = e->n, Bs = (size_t)e->d.Bs;
  double *bq = nullptr, *bqs = nullptr, *bqr = nullptr;
  int rc = dalloc(e, &bq, n * Bs);
  if (!rc) rc = dalloc(e, &bqs, n * Bs);
  if (!rc) rc = dalloc(e, &bqr, n * Bs);
  if (rc) return rc;
  HIPCHK(hipHostMalloc((void **)&e->hb_q, sizeof(double) * Bs * n, hipHostMallocDefault));
  e->d.b_qs = bqs;
  e->d.b_qraw = bqr;
  e->d.b_q = bq;  // (the captured chunks of set [0] hold a Dev without these: they never read them)
  return 0;
}

// one slice of at most Bcap nodes; q: the slice's raw costs, instance-major (e->pq is set), or nullptr
int solve_slice(miosqp_qp_engine *e, int B, const double *l, const double *u, const double *x0, const double *y0,
                double *x_out, double *y_out, miosqp_qp_info *info, const double *q = nullptr) {
  const Dev &d = e->d;
  const size_t n = e->n, M = e->M;
  const double t0 = wall();
  const int ntiles = (B + 63) / 64;
  if (int rcb = slice_begin(e, B)) return rcb;
  double *h = e->hb_in;
  memcpy(h, l, sizeof(double) * B * M);
  memcpy(h + B * M, u, sizeof(double) * B * M);
  memcpy(h + 2 * B * M, x0, sizeof(double) * B * n);
  memcpy(h + 2 * B * M + B * n, y0, sizeof(double) * B * M);
  HIPCHK(hipEventRecord(e->ev0, e->stream));
  HIPCHK(hipMemcpyAsync(d.b_raw, h, sizeof(double) * B * (3 * M + n), hipMemcpyHostToDevice, e->stream));
  if (q) {
    // qbar_k = c D q_k by the kernel that scales solve_trees' costs: the bits update_lin_cost leaves in d.q
    memcpy(e->hb_q, q, sizeof(double) * B * n);
    HIPCHK(hipMemcpyAsync(d.b_qraw, e->hb_q, sizeof(double) * B * n, hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_scale_q_batch, dim3((unsigned)(((size_t)B * n + 255) / 256)), dim3(256), 0, e->stream, d, d.b_qraw, d.b_qs, B);
  }
  if (int rcr = slice_run(e, B, e->st.max_iter)) return rcr;
  const int big = (int)(n > M ? n : M);
  hipLaunchKernelGGL(kb_export, dim3((big + 3) / 4, ntiles), dim3(256), 0, e->stream, d, B);
  HIPCHK(hipMemcpyAsync(e->hb_out, d.b_out, sizeof(double) * B * (n + M), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(e->hb_int, d.c_status, sizeof(int) * B, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(e->hb_int + B, d.c_iter, sizeof(int) * B, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(e->hb_dbl, d.c_pri, sizeof(double) * B, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(e->hb_dbl + B, d.c_dua, sizeof(double) * B, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(e->hb_dbl + 2 * B, d.c_obj, sizeof(double) * B, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(e->hb_dbl + 3 * B, d.c_lower, sizeof(double) * B, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(e->hb_dbl + 4 * B, d.c_hviol, sizeof(double) * B, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(e->hb_dbl + 5 * B, d.c_hobj, sizeof(double) * B, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(e->hb_int + 2 * B, d.c_intinf, sizeof(int) * B, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(e->hb_int + 3 * B, d.c_nextvar, sizeof(int) * B, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(e->hb_int + 4 * B, d.c_node, sizeof(int) * B, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipEventRecord(e->ev1, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  const int *node_of = e->hb_int + 4 * B;  // column position -> node
  for (int c = 0; c < B; c++) {
    memcpy(x_out + (size_t)node_of[c] * n, e->hb_out + (size_t)c * n, sizeof(double) * n);
    memcpy(y_out + (size_t)node_of[c] * M, e->hb_out + B * n + (size_t)c * M, sizeof(double) * M);
  }
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, e->ev0, e->ev1));
  const double wall_s = wall() - t0;
  for (int c = 0; c < B; c++) {
    const int b = node_of[c];
    info[b].status_val = e->hb_int[c];
    info[b].iter = e->hb_int[B + c];
    info[b].pri_res = e->hb_dbl[c];
    info[b].dua_res = e->hb_dbl[B + c];
    info[b].obj_val = e->hb_dbl[2 * B + c];
    info[b].lower = e->hb_dbl[3 * B + c];
    info[b].int_inf = d.digest ? e->hb_int[2 * B + c] : -1;
    info[b].nextvar = d.digest ? e->hb_int[3 * B + c] : -1;
    info[b].heur_viol = e->hb_dbl[4 * B + c];
    info[b].heur_obj = e->hb_dbl[5 * B + c];
    info[b].run_time = wall_s / B;  // the wave's wall time, shared equally
    info[b].device_time = 1e-3 * ms / B;
  }
  return 0;
}

}  // namespace
