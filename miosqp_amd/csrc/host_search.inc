// part of engine.hip (included there, not compiled alone): node-at-a-time branch and bound driven from the host in C++
// (C ABI miosqp_qp_search_*).  The loop `while can_continue: choose_leaf -> Node.solve -> bound_and_branch`
// (/root/reference/miosqp/solver.py:65-172, workspace.py:113-155, 274-334) with the list semantics of the Python
// mirror (miosqp_amd/bnb.py): list order = creation order, choose = first maximum, prune skips the element behind
// a removed one.  What differs from driving solve_node from Python: the open leaves are device slots (no vector
// crosses PCIe per node), the per-node host work is a few hundred nanoseconds, and the heuristic incumbent's value
// is the device's (the Python digest branch recomputes it with numpy; they agree to ~1e-12 relative).
namespace {

struct NodeSearch {
  int cap = 0;
  double *lo = nullptr, *hi = nullptr, *x = nullptr, *y = nullptr, *inc_x = nullptr;  // device
  double *own_block = nullptr;  // the grown store (search_grow), released when it grows again or with the engine
  SearchDigest *dg = nullptr;                                                        // coherent host memory
  unsigned long long seq = 0;
  hipEvent_t ev[4] = {};  // (start, end) of the last two in-launch nodes: a node's device time is read one node later
  int ev_slot = 0;
  bool ev_pending = false;
  unsigned long long *stamps = nullptr;  // debug (MIOSQP_SEARCH_STAMPS=1): ring of 256 x 16 device stamps, see COOP_STAMP
  std::vector<int> stamp_iter;           // iterations of the node in each ring slot
  // ONE launch per search_run (kernels_coop.inc: k_coop_run): the run's constant block (device copy and what was last sent),
  // the mailbox (coherent host memory: CM_HOST_WORDS entries, then at word 32 the run's status) and its device-side copy
  CoopRun *run_blk = nullptr;
  CoopRun run_blk_host;
  bool run_blk_sent = false;
  unsigned long long *mail_host = nullptr, *mail_dev = nullptr;
  unsigned long long mtag = 0;  // mails sent so far (the low 32 bits tag the entries)
  bool run_live = false;
  hipEvent_t ev_run[2] = {};
  int64_t run_off = 0;  // nodes to go through launches of their own before a run is tried again (after a call-off)
  int run_nap = -1;     // poll delay of the resident grid's exchange loop (its own optimum: calibrate_run_nap); -1: not chosen yet
  std::vector<int> open;  // slots of the open leaves, in list order
  std::vector<int> freelist, depth, parent, kids;
  std::vector<char> decided;
  std::vector<double> lower;
  double upper = 1.7e308;
  bool have_inc = false;
  int64_t nodes = 0, iters = 0;
};

NodeSearch *search_of(miosqp_qp_engine *e) { return static_cast<NodeSearch *>(e->search); }
bool getenv_off(const char *name) {
  const char *v = getenv(name);
  return v != nullptr && atoi(v) == 0;
}

// node `s` has been decided or discarded: its slot stays allocated while a child may still read its solution as a
// warm start; the last child to go frees it
void search_done(NodeSearch &S, int s) {
  S.decided[s] = 1;
  if (S.kids[s] == 0) S.freelist.push_back(s);
  const int par = S.parent[s];
  if (par >= 0 && --S.kids[par] == 0 && S.decided[par]) S.freelist.push_back(par);
}

// The reference's leaf list is unbounded (workspace.py:83); the slot store doubles when it runs out.  The first store
// comes from the engine's device pool; a grown one is ONE allocation of its own (lo | hi | x | y), the old contents are
// copied on the engine's stream (every later reader is queued behind the copies) and a grown predecessor is released
// once the copies are done -- device memory stays at the live store (+ the first, small one, which belongs to the pool).
// Returns MIOSQP_EFULL only when the device has no memory left for it.
int search_grow(miosqp_qp_engine *e, NodeSearch &S) {
  const size_t n = e->n, M = e->M, p = e->d.n_int, cap = (size_t)S.cap;
  if (cap > ((size_t)1 << 28)) return MIOSQP_EFULL;
  const size_t ncap = 2 * cap;
  auto al = [](size_t doubles) { return (doubles + 31) & ~(size_t)31; };  // (256-byte boundaries)
  const size_t o_hi = al(ncap * p), o_x = o_hi + al(ncap * p), o_y = o_x + al(ncap * n), total = o_y + al(ncap * M);
  double *blk = nullptr;
  if (hipMalloc((void **)&blk, total * sizeof(double)) != hipSuccess) {
    (void)hipGetLastError();
    g_err = "search: the slot store cannot grow (hipMalloc of " + std::to_string(total * sizeof(double)) + " bytes failed)";
    return MIOSQP_EFULL;
  }
  double *lo = blk, *hi = blk + o_hi, *x = blk + o_x, *y = blk + o_y;
  HIPCHK(hipMemcpyAsync(lo, S.lo, sizeof(double) * cap * p, hipMemcpyDeviceToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(hi, S.hi, sizeof(double) * cap * p, hipMemcpyDeviceToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(x, S.x, sizeof(double) * cap * n, hipMemcpyDeviceToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(y, S.y, sizeof(double) * cap * M, hipMemcpyDeviceToDevice, e->stream));
  if (S.own_block) {  // (growing happens a handful of times per search: the wait does not matter)
    HIPCHK(hipStreamSynchronize(e->stream));
    hipFree(S.own_block);
  }
  S.own_block = blk;
  S.lo = lo; S.hi = hi; S.x = x; S.y = y;
  S.depth.resize(ncap, 0); S.parent.resize(ncap, -1); S.kids.resize(ncap, 0);
  S.decided.resize(ncap, 0); S.lower.resize(ncap, 0.0);
  for (size_t s = ncap; s-- > cap;) S.freelist.push_back((int)s);
  S.cap = (int)ncap;
  return 0;
}

// workspace.py:274-280 with the traversal of the reference: the element following a removed one is not examined
void search_prune(NodeSearch &S) {
  size_t k = 0;
  while (k < S.open.size()) {
    if (S.lower[S.open[k]] > S.upper) {
      const int s = S.open[k];
      S.open.erase(S.open.begin() + (long)k);
      search_done(S, s);
    }
    k++;
  }
}

// workspace.py:128-149: depth first (first deepest) -- always for rule 0, until there is an incumbent for rule 1,
// then the leaf with the LARGEST inherited bound (sic), first one.  Rule 2 is best bound: the leaf with the SMALLEST
// inherited bound, first one (np.argmin; siblings share their parent's bound, so ties are the normal case); rule 3
// dives like rule 0 until there is an incumbent and takes the best bound from then on
size_t search_choose(const NodeSearch &S, int rule) {
  size_t best = 0;
  if (rule == 0 || (rule != 2 && !(S.upper < 1.7e308))) {
    for (size_t k = 1; k < S.open.size(); k++)
      if (S.depth[S.open[k]] > S.depth[S.open[best]]) best = k;
  } else if (rule >= 2) {
    for (size_t k = 1; k < S.open.size(); k++)
      if (S.lower[S.open[k]] < S.lower[S.open[best]]) best = k;
  } else {
    for (size_t k = 1; k < S.open.size(); k++)
      if (S.lower[S.open[k]] > S.lower[S.open[best]]) best = k;
  }
  return best;
}

// k_heur_rows and k_obj_rows as one launch, each with its tuned threads-per-row
void launch_heur_obj_rows(miosqp_qp_engine *e) {
  const Dev &d = e->d;
  auto blocks = [](int rows, int tpr) { return (rows + 256 / tpr - 1) / (256 / tpr); };
  const int th = e->tpr_pc == 16 || e->tpr_pc == 32 || e->tpr_pc == 64 || e->tpr_pc == 128 ? e->tpr_pc : 256;
  const int to = e->tpr_pr == 16 || e->tpr_pr == 32 || e->tpr_pr == 64 || e->tpr_pr == 128 ? e->tpr_pr : 256;
  const int nh = blocks(d.M, th), no = blocks(d.n, to);
#define HO(TH, TO) hipLaunchKernelGGL((ks_heur_obj_rows<TH, TO>), dim3(nh + no), dim3(256), 0, e->stream, d, nh)
#define HO_O(TH)                                   \
  switch (to) {                                    \
    case 16: HO(TH, 16); break;                    \
    case 32: HO(TH, 32); break;                    \
    case 64: HO(TH, 64); break;                    \
    case 128: HO(TH, 128); break;                  \
    default: HO(TH, 256); break;                   \
  }
  switch (th) {
    case 16: HO_O(16); break;
    case 32: HO_O(32); break;
    case 64: HO_O(64); break;
    case 128: HO_O(128); break;
    default: HO_O(256); break;
  }
#undef HO_O
#undef HO
}

// ---- ONE launch per search_run: the cooperative grid stays resident and the host feeds it nodes through a mailbox ----
constexpr int RUN_STATUS_WORD = 32;  // (a cache line of its own behind the CM_HOST_WORDS entries)

// (a chip shared with other engines of this process: the run is one whole-chip launch like any other -- the others' whole-chip
//  launches are ordered behind its end by the turn-taking events, ChipGuard -- it merely holds its turn for the whole call;
//  MIOSQP_COOP_RUN_SHARED=0 keeps a launch per node there)
bool run_possible(const miosqp_qp_engine *e, const NodeSearch &S) {
  const Dev &d = e->d;
  return e->coop && S.run_blk != nullptr && d.coop_nt > 0 && e->st.check_termination > d.coop_lag && e->n <= COOP_EPI_NMAX &&
         e->coop_T + d.coop_nt <= COOP_EPI_GMAX && d.digest && e->coop_epi != nullptr &&
         (!chip_shared(e) || !getenv_off("MIOSQP_COOP_RUN_SHARED")) &&
         !getenv_off("MIOSQP_COOP_RUN") && !getenv_off("MIOSQP_COOP_NODE") && !getenv_off("MIOSQP_COOP_EPI");
}

void launch_coop_run(miosqp_qp_engine *e, const CoopRun *blk, unsigned mtag0) {
  const Dev &d = e->d;
  ChipGuard turn(e);
  const int cpt = e->coop_cpt, cptf = e->coop_cptf;
#define X(RW, CPT, CPTF)                                                                                             \
  if (e->coop_rw == RW && cpt == CPT && cptf == CPTF) {                                                              \
    hipLaunchKernelGGL((k_coop_run<512, RW, CPT, CPTF>), dim3(e->coop_T + d.coop_nt), dim3(512), 0, e->stream, blk, mtag0); \
    return;                                                                                                          \
  }
  COOP_FORMS(X)
#undef X
}

// the grid is launched and waits for its first mail.  cal_iters > 0: a run of the poll-delay calibration -- its nodes take
// exactly cal_iters iterations (no tolerance can be met) and end at the iteration limit
int run_begin(miosqp_qp_engine *e, NodeSearch &S, int cal_iters = 0) {
  CoopRun &now = S.run_blk_host;
  CoopRun was;
  memcpy(&was, &now, sizeof(CoopRun));
  memset(&now, 0, sizeof(CoopRun));
  memcpy(&now.d, &e->d, sizeof(Dev));
  if (S.run_nap >= 0) now.d.coop_nap = S.run_nap;
  e->run_nap_in_use = now.d.coop_nap;
  now.max_iter = e->st.max_iter;
  if (cal_iters > 0) {
    now.max_iter = cal_iters;
    now.d.eps_abs = now.d.eps_rel = now.d.eps_pinf = now.d.eps_dinf = 0.0;
  }
  now.check_every = e->st.check_termination;
  now.final_check = 1;
  now.tpr_h = e->tpr_pc;
  now.tpr_o = e->tpr_pr;
  now.epi_buf = e->coop_epi;
  now.inc_x = S.inc_x;
  now.dg = S.dg;
  now.mail_host = S.mail_host;
  now.mail_dev = S.mail_dev;
  now.status_host = S.mail_host + RUN_STATUS_WORD;
  if (!S.run_blk_sent || memcmp(&was, &now, sizeof(CoopRun)) != 0) {
    HIPCHK(hipMemcpyAsync(S.run_blk, &now, sizeof(CoopRun), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));  // (the source is pageable memory; once per search in practice)
    S.run_blk_sent = true;
  }
  __atomic_store_n(S.mail_host + RUN_STATUS_WORD, (unsigned long long)CR_RUNNING, __ATOMIC_RELEASE);
  HIPCHK(hipEventRecord(S.ev_run[0], e->stream));
  launch_coop_run(e, S.run_blk, (unsigned)(S.mtag + 1));
  HIPCHK(hipEventRecord(S.ev_run[1], e->stream));
  HIPCHK(hipGetLastError());
  S.run_live = true;
  e->loop_launches++;
  e->run_launches++;
  return 0;
}

// one node (or the stop) as tagged entries {lo, tag, hi, tag}; each 8-byte half is one store
void run_send(NodeSearch &S, const SearchArgs &a, unsigned long long flags, unsigned long long *stamps) {
  unsigned long long w[CM_HOST_WORDS] = {};
  w[CM_LO_S] = (unsigned long long)a.lo_s; w[CM_HI_S] = (unsigned long long)a.hi_s;
  w[CM_X_W] = (unsigned long long)a.x_w; w[CM_Y_W] = (unsigned long long)a.y_w;
  w[CM_X_S] = (unsigned long long)a.x_s; w[CM_Y_S] = (unsigned long long)a.y_s;
  w[CM_LO0] = (unsigned long long)a.lo0; w[CM_HI0] = (unsigned long long)a.hi0;
  w[CM_LO1] = (unsigned long long)a.lo1; w[CM_HI1] = (unsigned long long)a.hi1;
  memcpy(&w[CM_UPPER], &a.upper, sizeof(double));
  w[CM_SEQ] = a.seq;
  w[CM_FLAGS] = flags;
  w[CM_STAMPS] = (unsigned long long)stamps;
  const unsigned long long tag = (++S.mtag) & 0xffffffffull;
  for (int k = 0; k < CM_HOST_WORDS; k++) {
    __atomic_store_n(S.mail_host + 2 * k, (w[k] & 0xffffffffull) | (tag << 32), __ATOMIC_RELAXED);
    __atomic_store_n(S.mail_host + 2 * k + 1, (w[k] >> 32) | (tag << 32), __ATOMIC_RELAXED);
  }
  __atomic_thread_fence(__ATOMIC_RELEASE);
}

// the run ends: a stop by mail (unless the kernel is known to be gone), the launch's device time into the statistics.
// Returns the status word the kernel left.
int run_end(miosqp_qp_engine *e, NodeSearch &S, bool send_stop, double *dev_ms, unsigned long long *status) {
  if (!S.run_live) return 0;
  if (send_stop) run_send(S, SearchArgs{}, CM_FLAG_STOP, nullptr);
  S.run_live = false;
  HIPCHK(hipEventSynchronize(S.ev_run[1]));
  float lms = 0;
  HIPCHK(hipEventElapsedTime(&lms, S.ev_run[0], S.ev_run[1]));
  e->loop_ms += lms;
  if (dev_ms) *dev_ms += lms;
  if (status) *status = __atomic_load_n(S.mail_host + RUN_STATUS_WORD, __ATOMIC_ACQUIRE);
  return 0;
}

// The poll delay of the RESIDENT grid.  Its exchange loop is the same source as k_coop's but another function (its own
// registers and schedule), and the optimum of the delay is sharp and moves with the code around the poll: the value
// calibrated on k_coop launches at set-up (calibrate_coop_nap) is 2-4 units off for it (config 2, r06: 18 against 14-16,
// 2.5 % of the search).  So the resident grid gets a value of its own, cached and shipped like the other (same files,
// key: columns per thread + 1000), and measured where there is none: runs of ONE synthetic node each -- the node the search
// is about to solve, with tolerances nothing can meet, 300 iterations, an incumbent value that keeps the epilogue from
// branching or touching the incumbent, its solution written into a free slot -- timed by the first tester's own clock
// (mail taken up -> record), best of two per candidate.  Nothing of it is visible in the search or its statistics.
int calibrate_run_nap(miosqp_qp_engine *e, NodeSearch &S, const SearchArgs &node, double *x_free, double *y_free) {
  const Dev &d = e->d;
  S.run_nap = d.coop_nap;
  if (getenv("MIOSQP_COOP_NAP") || getenv_off("MIOSQP_COOP_RUN_CAL")) return 0;  // (the set-up took the former as it is)
  const bool always = getenv("MIOSQP_COOP_RUN_CAL") && atoi(getenv("MIOSQP_COOP_RUN_CAL")) == 2;  // tests: measure whatever is cached
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  const int cpt_key = e->coop_cpt + (e->coop_rw == 16 ? 100 : 0) + 1000;
  const NapKey key{dev, e->coop_T, cpt_key};
  if (!always) {
    std::lock_guard<std::mutex> lk(g_nap_mutex);
    auto it = g_nap_cache.find(key);
    if (it != g_nap_cache.end()) {
      S.run_nap = it->second;
      return 0;
    }
  }
  const std::string devkey = nap_device_key(dev);
  if (!always && !getenv("MIOSQP_NO_CACHE")) {
    int nap = 0;
    if (nap_lookup_file(nap_user_file(), devkey, e->coop_T, cpt_key, 0, &nap) ||
        nap_lookup_file(nap_shipped_file(), devkey, e->coop_T, cpt_key, 8, &nap)) {
      S.run_nap = nap;
      std::lock_guard<std::mutex> lk(g_nap_mutex);
      g_nap_cache[key] = nap;
      return 0;
    }
  }
  const int64_t launches0 = e->loop_launches, runs0 = e->run_launches;
  const double ms0 = e->loop_ms;
  const int fallback = d.coop_nap;
  bool failed = false;
  auto timed = [&](int nap, double *best) -> int {  // device ticks (10 ns) of one 300-iteration node, best of two
    for (int rep = 0; rep < 2 && !failed; rep++) {
      S.run_nap = nap;
      if (int rc = run_begin(e, S, 300)) return rc;
      SearchArgs a = node;
      a.x_s = x_free;
      a.y_s = y_free;
      a.upper = -1.7e308;
      a.seq = ++S.seq;
      run_send(S, a, 0, nullptr);
      const double t_give_up = wall() + 0.5;
      while (__atomic_load_n(&S.dg->seq, __ATOMIC_ACQUIRE) != a.seq) {
        if (wall() < t_give_up) continue;
        failed = true;  // (called off at its registration, or lost: the search's own path deals with it)
        break;
      }
      const SearchDigest g = *S.dg;
      if (!failed && (g.todo || g.pad || g.t1 <= g.t0)) failed = true;
      if (int rc = run_end(e, S, !failed || hipEventQuery(S.ev_run[1]) == hipErrorNotReady, nullptr, nullptr)) return rc;
      if (failed) {
        S.mtag = (S.mtag + 0xffull) & ~0xffull;
        reset_registration(e);
        break;
      }
      const double ticks = (double)(g.t1 - g.t0);
      e->run_cal_nodes++;
      if (rep == 0 || ticks < *best) *best = ticks;
    }
    return 0;
  };
  int best = fallback;
  double best_t = 1e300;
  auto consider = [&](int nap) -> int {
    if (nap < 0 || failed) return 0;
    double t = 1e300;
    if (int rc = timed(nap, &t)) return rc;
    if (!failed && t < best_t) {
      best_t = t;
      best = nap;
    }
    return 0;
  };
  int rc = 0;
  for (int nap : {fallback, fallback - 2, fallback - 4, fallback + 2})
    if (!rc) rc = consider(nap);
  const int centre = best;
  if (!rc) rc = consider(centre - 1);
  if (!rc) rc = consider(centre + 1);
  e->loop_launches = launches0;
  e->run_launches = runs0;
  e->loop_ms = ms0;
  if (rc) return rc;
  if (failed) {
    S.run_nap = fallback;
    return 0;
  }
  S.run_nap = best;
  {
    std::lock_guard<std::mutex> lk(g_nap_mutex);
    g_nap_cache[key] = best;
  }
  if (!always) nap_store_file(devkey, e->coop_T, cpt_key, best);
  return 0;
}

}  // namespace

extern "C" {

int miosqp_qp_search_create(miosqp_qp_engine *e, int32_t capacity) {
  if (!e || capacity < 4) return MIOSQP_EARG;
  ENTER(e);
  if (!e->have_int || !e->d.digest || e->d.n_int < 1) {
    g_err = "search_create: call miosqp_qp_set_integer_rows and miosqp_qp_set_root first";
    return MIOSQP_EARG;
  }
  if (e->search) {
    g_err = "search_create: the search exists already";
    return MIOSQP_EARG;
  }
  NodeSearch *S = new NodeSearch();
  const size_t n = e->n, M = e->M, p = e->d.n_int, cap = capacity;
  int rc = pool_reserve(e, (cap * (n + M + 2 * p) + n + 4096) * sizeof(double));
  if (!rc) rc = dalloc(e, &S->lo, cap * p);
  if (!rc) rc = dalloc(e, &S->hi, cap * p);
  if (!rc) rc = dalloc(e, &S->x, cap * n);
  if (!rc) rc = dalloc(e, &S->y, cap * M);
  if (!rc) rc = dalloc(e, &S->inc_x, n);
  if (rc) { delete S; return rc; }
  if (hipHostMalloc((void **)&S->dg, sizeof(SearchDigest), hipHostMallocCoherent) != hipSuccess) {
    delete S;
    g_err = "search_create: hipHostMalloc failed";
    return MIOSQP_EHIP;
  }
  memset(S->dg, 0, sizeof(SearchDigest));
  for (hipEvent_t &ev : S->ev) HIPCHK(hipEventCreate(&ev));
  if (e->coop_capable && e->coop_epi) {  // the mailbox and the constant block of k_coop_run
    for (hipEvent_t &ev : S->ev_run) HIPCHK(hipEventCreate(&ev));
    if (hipHostMalloc((void **)&S->mail_host, 64 * sizeof(unsigned long long), hipHostMallocCoherent) != hipSuccess) {
      (void)hipGetLastError();
      S->mail_host = nullptr;
    } else {
      memset(S->mail_host, 0, 64 * sizeof(unsigned long long));
      rc = dalloc(e, &S->mail_dev, 64);
      if (!rc) rc = dalloc(e, (char **)&S->run_blk, sizeof(CoopRun) + 256);
      if (rc) { delete S; return rc; }
    }
  }
  if (getenv("MIOSQP_SEARCH_STAMPS")) {
    rc = dalloc(e, &S->stamps, 256 * 16);
    if (rc) { delete S; return rc; }
    HIPCHK(hipMemset(S->stamps, 0, sizeof(unsigned long long) * 256 * 16));
    S->stamp_iter.assign(256, 0);
  }
  S->cap = capacity;
  S->depth.assign(cap, 0); S->parent.assign(cap, -1); S->kids.assign(cap, 0);
  S->decided.assign(cap, 0); S->lower.assign(cap, 0.0);
  for (int s = capacity - 1; s >= 0; s--) S->freelist.push_back(s);  // pop_back hands out slot 0 first
  e->search = S;
  return 0;
}

// new MIQP on the same factor (after update_vectors / set_root): no leaves, no incumbent
int miosqp_qp_search_reset(miosqp_qp_engine *e) {
  if (!e || !e->search) return MIOSQP_EARG;
  NodeSearch &S = *search_of(e);
  S.open.clear();
  S.freelist.clear();
  for (int s = S.cap - 1; s >= 0; s--) S.freelist.push_back(s);
  std::fill(S.kids.begin(), S.kids.end(), 0);
  std::fill(S.decided.begin(), S.decided.end(), 0);
  S.upper = 1.7e308;
  S.have_inc = false;
  S.nodes = S.iters = 0;
  return 0;
}

// a leaf given with explicit vectors (the root, or one received from another rank): integer-row bounds (n_int each),
// warm start x0 (n), y0 (M), its depth and inherited bound; appended to the list
int miosqp_qp_search_add_leaf(miosqp_qp_engine *e, const double *l_int, const double *u_int, const double *x0,
                              const double *y0, int32_t depth, double lower) {
  if (!e || !e->search || !l_int || !u_int || !x0 || !y0) return MIOSQP_EARG;
  ENTER(e);
  NodeSearch &S = *search_of(e);
  const size_t n = e->n, M = e->M, p = e->d.n_int;
  if (host_may_read(l_int) && host_may_read(u_int))  // (a leaf out of another rank's store was checked when it was made)
    for (size_t k = 0; k < p; k++)
      if (l_int[k] > u_int[k]) return MIOSQP_EBOUNDS;
  if (S.freelist.empty()) {
    const int rcg = search_grow(e, S);
    if (rcg) return rcg;
  }
  const int s = S.freelist.back();
  S.freelist.pop_back();
  HIPCHK(hipMemcpyAsync(S.lo + s * p, l_int, sizeof(double) * p, hipMemcpyDefault, e->stream));
  HIPCHK(hipMemcpyAsync(S.hi + s * p, u_int, sizeof(double) * p, hipMemcpyDefault, e->stream));
  HIPCHK(hipMemcpyAsync(S.x + s * n, x0, sizeof(double) * n, hipMemcpyDefault, e->stream));
  HIPCHK(hipMemcpyAsync(S.y + s * M, y0, sizeof(double) * M, hipMemcpyDefault, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));  // the sources are the caller's
  S.depth[s] = depth;
  S.lower[s] = lower;
  S.parent[s] = -1;
  S.kids[s] = 0;
  S.decided[s] = 0;
  S.open.push_back(s);
  return 0;
}

// takes the shallowest open leaf (first one) out of the list, with explicit vectors: the largest subtree to hand to
// another rank.  Returns 1 when there was none.
int miosqp_qp_search_take_leaf(miosqp_qp_engine *e, double *l_int, double *u_int, double *x0, double *y0,
                               int32_t *depth, double *lower) {
  if (!e || !e->search || !l_int || !u_int || !x0 || !y0 || !depth || !lower) return MIOSQP_EARG;
  ENTER(e);
  NodeSearch &S = *search_of(e);
  if (S.open.empty()) return 1;
  size_t best = 0;
  for (size_t k = 1; k < S.open.size(); k++)
    if (S.depth[S.open[k]] < S.depth[S.open[best]]) best = k;
  const int s = S.open[best];
  S.open.erase(S.open.begin() + (long)best);
  const size_t n = e->n, M = e->M, p = e->d.n_int;
  const int ws = S.parent[s] >= 0 ? S.parent[s] : s;  // its warm start: the parent's solution
  HIPCHK(hipMemcpyAsync(l_int, S.lo + s * p, sizeof(double) * p, hipMemcpyDefault, e->stream));
  HIPCHK(hipMemcpyAsync(u_int, S.hi + s * p, sizeof(double) * p, hipMemcpyDefault, e->stream));
  HIPCHK(hipMemcpyAsync(x0, S.x + ws * n, sizeof(double) * n, hipMemcpyDefault, e->stream));
  HIPCHK(hipMemcpyAsync(y0, S.y + ws * M, sizeof(double) * M, hipMemcpyDefault, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  *depth = S.depth[s];
  *lower = S.lower[s];
  search_done(S, s);
  return 0;
}

// an incumbent from outside (MIOSQP.set_x0, another rank): adopted when better; open leaves are pruned against it.
// x == NULL: the VALUE of the incumbent the search holds is replaced by `upper` (its x stays) -- the caller has
// recomputed the objective of a rounding-heuristic candidate on the host exactly as workspace.py:321-327 does
// (the device sums in another order: ~1e-12 relative apart), see search_info.improved == 2.
int miosqp_qp_search_set_incumbent(miosqp_qp_engine *e, double upper, const double *x) {
  if (!e || !e->search) return MIOSQP_EARG;
  ENTER(e);
  NodeSearch &S = *search_of(e);
  if (!x) {
    if (!S.have_inc) return MIOSQP_EARG;
    S.upper = upper;
    return 0;
  }
  if (!(upper < S.upper)) return 0;
  HIPCHK(hipMemcpyAsync(S.inc_x, x, sizeof(double) * e->n, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  S.upper = upper;
  S.have_inc = true;
  search_prune(S);
  return 0;
}

// *upper >= 1.7e308: none (x untouched)
int miosqp_qp_search_get_incumbent(miosqp_qp_engine *e, double *upper, double *x) {
  if (!e || !e->search || !upper || !x) return MIOSQP_EARG;
  ENTER(e);
  NodeSearch &S = *search_of(e);
  *upper = S.upper;
  if (S.have_inc) {
    HIPCHK(hipMemcpyAsync(x, S.inc_x, sizeof(double) * e->n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  return 0;
}

// Runs nodes until the list is empty, `max_nodes` have been solved in this call, or -- checked between nodes --
// `budget_s` seconds have passed (<= 0: no time limit).
int miosqp_qp_search_run(miosqp_qp_engine *e, int32_t tree_explor_rule, int64_t max_nodes, double budget_s,
                         miosqp_search_info *info) {
  if (!e || !e->search || !info || tree_explor_rule < 0 || tree_explor_rule > 3) return MIOSQP_EARG;
  ENTER(e);
  NodeSearch &S = *search_of(e);
  const double t0 = wall();
  const size_t n = e->n, M = e->M, p = e->d.n_int;
  const Dev &d = e->d;
  int64_t done = 0, it_sum = 0;
  int improved = 0, rc_full = 0;
  double dev_ms = 0.0;
  if (int rc = run_end(e, S, true, nullptr, nullptr)) return rc;  // (a call that left on an error: its grid ends first)
  while (!S.open.empty() && done < max_nodes) {
    if (budget_s > 0 && done > 0 && wall() - t0 >= budget_s) break;
    if (S.freelist.size() < 2) {
      // (the store grows through copies on the engine's stream: a resident run is ended first and started again below)
      if (int rc = run_end(e, S, true, &dev_ms, nullptr)) return rc;
      const int rcg = search_grow(e, S);
      if (rcg) {  // out of device memory: the counters of the nodes done so far still go out
        rc_full = rcg;
        break;
      }
    }
    const size_t idx = search_choose(S, tree_explor_rule);
    const int s = S.open[idx];
    S.open.erase(S.open.begin() + (long)idx);
    const int c0 = S.freelist.back();
    S.freelist.pop_back();
    const int c1 = S.freelist.back();
    S.freelist.pop_back();
    const int ws = S.parent[s] >= 0 ? S.parent[s] : s;
    SearchArgs a;
    a.lo_s = S.lo + s * p; a.hi_s = S.hi + s * p;
    a.x_w = S.x + ws * n; a.y_w = S.y + ws * M;
    a.x_s = S.x + s * n; a.y_s = S.y + s * M;
    a.lo0 = S.lo + c0 * p; a.hi0 = S.hi + c0 * p; a.lo1 = S.lo + c1 * p; a.hi1 = S.hi + c1 * p;
    a.inc_x = S.inc_x;
    a.upper = S.upper;
    a.dg = S.dg;
    if (!S.run_live) maybe_rejoin_coop(e);
    SearchDigest g;
    // the record is ~1 ms away: poll its sequence number (acquire), check the stream for errors now and then
    // (the runtime is asked only when a record is LATE -- 20 ms: a node of 4000 iterations takes 8 -- and by the clock, not
    //  by a count of polls: a stream / event query costs tens of microseconds on some boxes, and one that happens to run
    //  when the record lands is that much turn-around on every node)
    constexpr double LATE_S = 0.02;
    auto await = [&](unsigned long long seq) -> int {
      unsigned long long spins = 0;
      double t_ask = wall() + LATE_S;
      while (__atomic_load_n(&S.dg->seq, __ATOMIC_ACQUIRE) != seq) {
        if ((++spins & 0xfff) == 0 && wall() >= t_ask) {
          t_ask = wall() + LATE_S;
          const hipError_t q = hipStreamQuery(e->stream);
          if (q != hipSuccess && q != hipErrorNotReady) HIPCHK(q);
          if (q == hipSuccess && __atomic_load_n(&S.dg->seq, __ATOMIC_ACQUIRE) != seq) {
            g_err = "search: the stream is idle and the node's record never arrived";
            return MIOSQP_EHIP;
          }
        }
      }
      return 0;
    };
    for (;;) {
      a.seq = ++S.seq;
      // ---- the grid is resident (k_coop_run): the node goes out by mail, its record comes back the same way as below
      if (S.run_off > 0) S.run_off--;
      if (S.run_live || (S.run_off == 0 && run_possible(e, S))) {
        if (!S.run_live) {
          if (S.run_nap < 0) {  // (once per search: looked up, or measured on this very node)
            if (int rc = calibrate_run_nap(e, S, a, S.x + (size_t)c0 * n, S.y + (size_t)c0 * M)) return rc;
            a.seq = ++S.seq;
          }
          if (int rc = run_begin(e, S)) return rc;
        }
        run_send(S, a, 0, S.stamps ? S.stamps + 16 * (a.seq % 256) : nullptr);
        // the record, or the kernel's exit without one (called off at its registration, or it waited a second for this mail)
        bool gone = false;
        double t_ask = wall() + LATE_S;
        for (unsigned long long spins = 0; __atomic_load_n(&S.dg->seq, __ATOMIC_ACQUIRE) != a.seq;) {
          if ((++spins & 0xfff) != 0 || wall() < t_ask) continue;
          t_ask = wall() + LATE_S;
          const hipError_t q = hipEventQuery(S.ev_run[1]);
          if (q == hipErrorNotReady) continue;
          if (q != hipSuccess) HIPCHK(q);
          gone = __atomic_load_n(&S.dg->seq, __ATOMIC_ACQUIRE) != a.seq;
          break;
        }
        if (gone) {
          unsigned long long st = 0;
          if (int rc = run_end(e, S, false, &dev_ms, &st)) return rc;
          S.mtag = (S.mtag + 0xffull) & ~0xffull;  // (mails the grid never took are not to match a later run's tags)
          if (st == CR_MAIL_TIMEOUT) continue;  // this thread was away for a second: the same node again, on a new run
          if (st != CR_CALLED_OFF) {
            g_err = "cooperative run: the resident grid ended without a record (status " + std::to_string(st) + ")";
            return MIOSQP_EHIP;
          }
          // the grid was not co-resident within 100 ms (device shared?): nothing was touched; this node and the next ones
          // go through launches of their own (which call themselves off, and fall back, the same way)
          reset_registration(e);
          e->coop_fallbacks++;
          S.run_off = 64;
          fprintf(stderr, "miosqp: the resident search grid was not co-resident within 100 ms (device shared?); nodes go through "
                          "launches of their own for a while\n");
          continue;
        }
        g = *S.dg;
        if (g.todo || g.pad) {  // an expired wait inside the node: the grid is on its way out
          if (int rc = run_end(e, S, false, &dev_ms, nullptr)) return rc;
          reset_registration(e);
          g_err = "cooperative run: exchange timed out, stage " + std::to_string(g.pad);
          return MIOSQP_EHIP;
        }
        const float nms = g.t1 > g.t0 ? 1e-5f * (float)(g.t1 - g.t0) : 0.0f;
        if (e->node_ms.size() < (size_t)1 << 20) e->node_ms.push_back(nms);
        e->loop_iters += g.iter;
        if (e->node_it.size() < (size_t)1 << 20) e->node_it.push_back(g.iter);
        break;
      }
      // the loop's device time of the node before this one: read now, with this node's work already queued behind it
      const bool stats_due = S.ev_pending;
      const int ev_prev = S.ev_slot;
      bool in_launch = false;
      if (e->coop && !getenv_off("MIOSQP_COOP_NODE")) {
        // ONE launch: prologue by the owners of the rows, iterations, and -- on the tester workgroups, the moment the
        // decision exists -- unscale, clamp, digest, heuristic and objective rows, commit and record
        // (kernels_coop.inc: node mode).  The launch always leaves a record; `todo` asks for the epilogue kernels.
        CoopNode nd{};
        nd.on = 1;
        nd.tpr_h = e->tpr_pc;
        nd.tpr_o = e->tpr_pr;
        nd.epi = d.coop_nt > 0 && e->st.check_termination > d.coop_lag && n <= COOP_EPI_NMAX &&
                 e->coop_T + d.coop_nt <= COOP_EPI_GMAX && d.digest && e->coop_epi != nullptr &&
                 !getenv_off("MIOSQP_COOP_EPI");
        nd.a = a;
        nd.epi_buf = e->coop_epi;
        if (S.stamps) nd.stamps = S.stamps + 16 * (a.seq % 256);
        S.ev_slot ^= 1;
        HIPCHK(hipEventRecord(S.ev[2 * S.ev_slot], e->stream));
        launch_coop(e, e->st.max_iter, e->st.check_termination, 1, &nd);
        e->loop_launches++;
        HIPCHK(hipEventRecord(S.ev[2 * S.ev_slot + 1], e->stream));
        S.ev_pending = true;
        in_launch = true;
      } else {
        // prologue: one launch (bounds, scaled warm start, z = Abar x, wh, rx, control block)
        DISPATCH_TPR(e->tpr_pc, ks_node_begin, (int)M, e->stream, d, a);
        int rc = run_loop(e);
        if (rc) return rc;
      }
      if (stats_due) {
        float lms = 0;
        HIPCHK(hipEventSynchronize(S.ev[2 * ev_prev + 1]));
        HIPCHK(hipEventElapsedTime(&lms, S.ev[2 * ev_prev], S.ev[2 * ev_prev + 1]));
        e->loop_ms += lms;
        dev_ms += lms;
        if (e->node_ms.size() < (size_t)1 << 20) e->node_ms.push_back(lms);
        if (!in_launch) S.ev_pending = false;
      }
      bool need_epilogue = !in_launch;
      if (in_launch) {
        if (int rc = await(a.seq)) return rc;
        g = *S.dg;
        need_epilogue = g.todo != 0 && g.pad == 0;
        if (need_epilogue) a.seq = ++S.seq;
      }
      if (need_epilogue) {
        // epilogue: unscale + clamp + integrality (one workgroup), heuristic and objective rows (one launch), sums + commit
        hipLaunchKernelGGL(k_finish, dim3(1), dim3(1024), 0, e->stream, d, 1, e->st.max_iter);
        launch_heur_obj_rows(e);
        hipLaunchKernelGGL(ks_commit, dim3(1), dim3(1024), 0, e->stream, d, a);
        if (int rc = await(a.seq)) return rc;
        g = *S.dg;
      }
      if (e->res_pending || e->loop_pending) {
        float lms = 0;
        HIPCHK(hipEventSynchronize(e->evc1));
        HIPCHK(hipEventElapsedTime(&lms, e->evc0, e->evc1));
        e->loop_ms += lms;
        dev_ms += lms;
        if (e->node_ms.size() < (size_t)1 << 20) e->node_ms.push_back(lms);
        e->res_pending = e->loop_pending = false;
      }
      e->loop_iters += g.iter;
      if (e->node_it.size() < (size_t)1 << 20) e->node_it.push_back(g.iter);
      if (!g.pad) break;
      reset_registration(e);
      g_err = "cooperative solver: " + std::string(g.pad == 1 ? "the grid was not co-resident within 100 ms (device shared?)"
                                                               : "exchange timed out") + ", stage " + std::to_string(g.pad);
      if (g.pad != 1) return MIOSQP_EHIP;
      if (S.ev_pending) {  // (the launch that was called off is not part of the statistics)
        HIPCHK(hipEventSynchronize(S.ev[2 * S.ev_slot + 1]));
        S.ev_pending = false;
      }
      e->loop_iters -= g.iter;
      if (!e->node_it.empty()) e->node_it.pop_back();
      int rc = leave_coop(e);  // called off before anything was modified: the same node in the two-kernel form
      if (rc) return rc;
    }
    if (S.stamps) S.stamp_iter[a.seq % 256] = g.todo ? -1 : g.iter;
    // ---- bound_and_branch on the record (workspace.py:282-334) ----
    done++;
    S.nodes++;
    S.iters += g.iter;
    it_sum += g.iter;
    bool branch = false;
    const bool ok = g.status == MIOSQP_QP_SOLVED || g.status == MIOSQP_QP_MAX_ITER_REACHED;
    if (ok) {
      S.lower[s] = g.lower;
      if (!(g.lower > S.upper)) {
        if (g.int_inf == 0) {
          S.upper = g.lower;
          S.have_inc = true;
          improved = 1;
          search_prune(S);
        } else {
          if (g.action == 2) {
            S.upper = g.heur_obj;
            S.have_inc = true;
            improved = 2;  // by the rounding heuristic: the value is the device's sum (see set_incumbent, x == NULL)
            search_prune(S);
          }
          branch = g.branched != 0;
        }
      }
    }
    if (branch) {
      for (int c : {c0, c1}) {
        S.depth[c] = S.depth[s] + 1;
        S.lower[c] = S.lower[s];
        S.parent[c] = s;
        S.kids[c] = 0;
        S.decided[c] = 0;
        S.open.push_back(c);
      }
      S.kids[s] = 2;
    } else {
      S.freelist.push_back(c1);
      S.freelist.push_back(c0);
      S.kids[s] = 0;
    }
    search_done(S, s);
  }
  if (int rc = run_end(e, S, true, &dev_ms, nullptr)) return rc;
  if (S.ev_pending) {  // the last node's device time
    float lms = 0;
    HIPCHK(hipEventSynchronize(S.ev[2 * S.ev_slot + 1]));
    HIPCHK(hipEventElapsedTime(&lms, S.ev[2 * S.ev_slot], S.ev[2 * S.ev_slot + 1]));
    e->loop_ms += lms;
    dev_ms += lms;
    if (e->node_ms.size() < (size_t)1 << 20) e->node_ms.push_back(lms);
    S.ev_pending = false;
  }
  if (S.stamps && done > 0) {  // debug: where a node's time goes (means over the in-launch nodes still in the ring)
    HIPCHK(hipStreamSynchronize(e->stream));
    std::vector<unsigned long long> h(256 * 16);
    HIPCHK(hipMemcpy(h.data(), S.stamps, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost));
    double sum[16] = {};
    double its = 0;
    int cnt = 0;
    for (int k = 0; k < 256; k++) {
      const unsigned long long *w = &h[16 * k];
      if (S.stamp_iter[k] <= 0 || !w[0] || !w[10] || w[10] < w[0]) continue;
      for (int q = 1; q <= 15; q++) sum[q] += 0.01 * (double)((long long)w[q] - (long long)w[0]);
      its += S.stamp_iter[k];
      cnt++;
    }
    if (cnt)
      fprintf(stderr, "[search stamps] %d nodes, %.1f it/node; us after kernel entry: go %.1f  round0 %.1f  tester's test rows %.1f  "
                      "tester gathered %.1f  decision %.1f  grid left loop %.1f  grid wrote back %.1f  epilogue rows %.1f  gathered %.1f  "
                      "record %.1f | tester 0's epilogue: entered %.1f  x built %.1f  rows %.1f  sums+digest %.1f  slot written %.1f\n",
              cnt, its / cnt, sum[1] / cnt, sum[2] / cnt, sum[3] / cnt, sum[4] / cnt, sum[5] / cnt,
              sum[6] / cnt, sum[7] / cnt, sum[8] / cnt, sum[9] / cnt, sum[10] / cnt, sum[13] / cnt, sum[11] / cnt, sum[12] / cnt,
              sum[14] / cnt, sum[15] / cnt);
  }
  info->nodes = done;
  info->osqp_iter = it_sum;
  info->open_leaves = (int32_t)S.open.size();
  info->free_slots = (int32_t)S.freelist.size();
  info->improved = improved;
  info->upper_glob = S.upper;
  double lg = 1.0 / 0.0;
  for (int s2 : S.open) lg = S.lower[s2] < lg ? S.lower[s2] : lg;
  info->lower_glob = S.open.empty() ? S.upper : lg;
  info->device_time = 1e-3 * dev_ms;
  info->run_time = wall() - t0;
  return rc_full;
}

}  // extern "C"
