// part of kernels_tree.inc (included there INSIDE k_tree_w and k_tree_w_m, nowhere else): the one body of the two
// one-wavefront kernels.  In scope: `d` (Dev) and `ta` (TreeArgs) with final pointers, as for kernels_tree_body.inc.
  __shared__ __attribute__((aligned(16))) double xfL[TW], xiL[TW], yfL[TW];
  __shared__ double KcL[TW * TW];
  __shared__ double PrL[TW * TW];  // unscaled P, dense, indexed by lanes: element (M + j, M + i) = P_ij
  __shared__ int iiL[TW];          // i_idx
  __shared__ double lf_lower[TREE_CAP];
  __shared__ int order[TREE_CAP], lf_depth[TREE_CAP], freelist[TREE_CAP];
  __shared__ double sc[16];
  const int n = d.n, M = d.M, N = n + M, p = d.n_int, m0 = d.m_orig;
  const int r = threadIdx.x;
  const unsigned long long t_begin = ta.done ? wall_clock64() : 0ull;
  const bool own = r < N, con = r < M;
  const int vi = r - M;  // variable index of a variable lane
  const double rho = d.rho, rinv = d.rho_inv, alpha = d.alpha, sigma = d.sigma;

  // ---- one-time loads: this lane's row of W, Kc into LDS, the row's scalings ----
  // (unconditional loads from clamped rows -- both buffers end with 64 entries of slack -- and a select afterwards: all
  //  64 requests of a row are in flight together; Kc first, while the registers of the row of W are still free)
  const size_t rowoff = (size_t)(own ? r : 0) * d.ldw;
  {
    double kc[TW];
#pragma unroll
    for (int c = 0; c < TW; c++) kc[c] = d.Kc[rowoff + c];
#pragma unroll
    for (int c = 0; c < TW; c++) KcL[c * TW + r] = (own && c < N) ? kc[c] : 0.0;  // symmetric
  }
  double Wr[TW];
#pragma unroll
  for (int k = 0; k < TW; k++) Wr[k] = d.W[rowoff + k];
#pragma unroll
  for (int k = 0; k < TW; k++) Wr[k] = (own && k < N) ? Wr[k] : 0.0;
  for (int c = 0; c < TW; c++) PrL[c * TW + r] = 0.0;
  xfL[r] = xiL[r] = yfL[r] = 0.0;
  iiL[r] = r < d.n_int ? d.i_idx[r] : 0;
  if (own && !con) {  // this lane's row of P (row-compressed in memory), sixteen entries requested at a time
    const int pb = d.pr_ptr[r - d.M], pe = d.pr_ptr[r - d.M + 1];
    for (int k = pb; k < pe; k += 16) {
      double pv[16];
      int pj[16];
#pragma unroll
      for (int j = 0; j < 16; j++) {
        const int kk = k + j < pe ? k + j : pe - 1;
        pv[j] = d.pr_val[kk];
        pj[j] = d.pr_idx[kk];
      }
#pragma unroll
      for (int j = 0; j < 16; j++)
        // (column = the lane that owns variable pj; rows are padded to even length with a zero that REPEATS a column
        //  index: a zero must not overwrite the entry it repeats)
        if (k + j < pe && pv[j] != 0.0) PrL[(M + pj[j]) * TW + r] = pv[j];
    }
  }
  const double sc_dir = own ? (con ? d.E[r] : d.D[vi]) : 0.0, sc_inv = own ? (con ? d.Einv[r] : d.Dinv[vi]) : 0.0;
  const double qbar = (own && !con) ? d.q[vi] : 0.0, qraw = (own && !con) ? d.qraw[vi] : 0.0;
  const double rootl = con ? d.root_l[r] : 0.0, rootu = con ? d.root_u[r] : 0.0;
  const double gl = (con && r < m0) ? d.raw_l[r] : 0.0, gu = (con && r < m0) ? d.raw_u[r] : 0.0;  // general rows: the root's
  const int ipos = (own && !con) ? d.int_pos[vi] : -1;
  for (int k = r; k < TREE_CAP; k += TW) freelist[k] = TREE_CAP - 1 - k;
  // root -> slot 0
  if (r < p) {
    ta.lf_lo[r] = d.raw_l[m0 + r];
    ta.lf_hi[r] = d.raw_u[m0 + r];
  }
  if (r < n) ta.lf_x[r] = d.raw_x[r];
  if (r < M) ta.lf_y[r] = d.raw_y[r];
  int count = 1, nfree = TREE_CAP - 1, nodes = 0, osqp_iter = 0, max_leaves = 1, overflow = 0, found = 0;
  double lower_glob = -1.0 / 0.0;
  if (r == 0) {
    order[0] = 0;
    lf_depth[0] = 0;
    lf_lower[0] = -1.0 / 0.0;
    sc[0] = ta.upper0;
  }
  __syncthreads();

  unsigned long long tp[6] = {0, 0, 0, 0, 0, 0}, tl = d.prof ? wall_clock64() : 0;  // debug: 100 MHz ticks per phase
#define TW_STAMP(k)                                   \
  if (d.prof) {                                       \
    const unsigned long long now__ = wall_clock64(); \
    tp[k] += now__ - tl;                              \
    tl = now__;                                       \
  }
  while (count > 0 && nodes + 1 < ta.max_nodes && !overflow) {
    // ---- choose_leaf (as k_tree; the best-bound choice inside the one wavefront) ----
    const bool best_bound = ta.rule == 2 || (ta.rule == 3 && !isinf(sc[0]));
    if (best_bound) {
      double bv;
      int bk;
      first_min_scan<TW>(lf_lower, order, count, r, bv, bk);
      first_min_wave(bv, bk);
      const int chosen = order[bk];
      order_remove<TW>(order, bk, count, r);
      if (r == 0) sc[2] = (double)chosen;
    } else if (r == 0) {
      const double upper = sc[0];
      const bool by_depth = ta.rule == 0 || isinf(upper);
      int best = 0;
      if (by_depth) {
        int bd = lf_depth[order[0]];
        for (int k = 1; k < count; k++)
          if (lf_depth[order[k]] > bd) { bd = lf_depth[order[k]]; best = k; }
      } else {
        double bl = lf_lower[order[0]];
        for (int k = 1; k < count; k++)
          if (lf_lower[order[k]] > bl) { bl = lf_lower[order[k]]; best = k; }
      }
      const int sl = order[best];
      for (int k = best; k + 1 < count; k++) order[k] = order[k + 1];
      sc[2] = (double)sl;
    }
    count--;
    __syncthreads();
    const int slot = (int)sc[2];
    const double *lo_n = ta.lf_lo + (size_t)slot * p, *hi_n = ta.lf_hi + (size_t)slot * p;
    // ---- prologue: scaled bounds, scaled warm start, z = Abar x ----
    double lo = 0.0, up = 0.0, sa = 0.0, sb = 0.0, sw = 0.0, delta = 0.0;
    double clo = 0.0, chi = 0.0;  // a variable lane: its integer bounds (clamp of node.py:131-136)
    if (con) {
      const double rl = r < m0 ? gl : lo_n[r - m0], ru = r < m0 ? gu : hi_n[r - m0];
      lo = sc_dir * fmax(rl, -QP_INFTY);
      up = sc_dir * fmin(ru, QP_INFTY);
      sb = d.c * sc_inv * ta.lf_y[(size_t)slot * M + r];
    } else if (own) {
      sa = sc_inv * ta.lf_x[(size_t)slot * n + vi];
      sb = qbar;
      if (ipos >= 0) { clo = lo_n[ipos]; chi = hi_n[ipos]; }
    }
    {
      // z = Abar x: the vector is zero outside the variable lanes, so the sum over all 64 columns is the sum over
      // c = M .. N-1
      const double vx[1] = {(own && !con) ? sa : 0.0};  // scaled x, by variable lane
      double zz[1] = {0.0};
      lds_col_dot<1>(KcL, r, vx, zz);
      if (con) {
        sa = zz[0];
        sw = zz[0] - rinv * sb;
      }
    }
    double ucur = own ? (con ? sw : sigma * sa - sb) : 0.0;  // this lane's entry of the right-hand side [wh ; rx]
    TW_STAMP(0)
    // ---- ADMM ----
    int it = 0, st = 0;
    int to_test = ta.check_every > 0 ? ta.check_every : -1;
    for (it = 1; it <= ta.max_iter; it++) {
      // The right-hand side is broadcast inside the registers: ur[q] of lane l holds u of lane 16 q + l % 16 (four
      // cross-row copies of this lane's entry), and product k = 16 q + j takes its operand from lane j of the row
      // through the DPP row broadcast of the FMA itself.  (Through LDS -- 32 broadcast reads of 16 bytes -- an iteration
      // was bound by the LDS read path: 1100 cycles.)  Accumulation order: k ascending, accumulator k % 4, as before.
      double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
      {
        double ur[4];
        row_replicate(ucur, ur);
        asm volatile("s_nop 1");
#define TW_F(ACC, Q, J) \
  asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:" #J " row_mask:0xf bank_mask:0xf" : "+v"(ACC) : "v"(ur[Q]), "v"(Wr[16 * (Q) + (J)]));
#define TW_ROW(Q)                                                                                             \
  TW_F(s0, Q, 0) TW_F(s1, Q, 1) TW_F(s2, Q, 2) TW_F(s3, Q, 3) TW_F(s0, Q, 4) TW_F(s1, Q, 5) TW_F(s2, Q, 6) TW_F(s3, Q, 7) \
  TW_F(s0, Q, 8) TW_F(s1, Q, 9) TW_F(s2, Q, 10) TW_F(s3, Q, 11) TW_F(s0, Q, 12) TW_F(s1, Q, 13) TW_F(s2, Q, 14) TW_F(s3, Q, 15)
        TW_ROW(0) TW_ROW(1) TW_ROW(2) TW_ROW(3)
#undef TW_ROW
#undef TW_F
      }
      const double s = (s0 + s1) + (s2 + s3);
      double pub = 0.0;
      if (con) {
        const double zt = sa + rinv * ((s - rho * sw) - sb);
        const double zr = alpha * zt + (1.0 - alpha) * sa;
        const double vv = zr + rinv * sb;
        const double zn = fmin(fmax(vv, lo), up);
        pub = 2.0 * zn - vv;
        delta = rho * (zr - zn);
        sa = zn;
        sb += delta;
        sw = pub;
      } else if (own) {
        const double xn = alpha * s + (1.0 - alpha) * sa;
        pub = sigma * xn - sb;
        delta = xn - sa;
        sa = xn;
      }
      ucur = pub;
      bool chk = it == ta.max_iter;
      if (--to_test == 0) {
        chk = true;
        to_test = ta.check_every;
      }
      if (!chk) continue;
      TW_STAMP(1)
      // ---- termination test (OSQP paper sec. 3.4), as coop_test ----
      double vproj = 0.0;
      if (con) {
        const bool uinf = up > QP_INFTY * QP_MIN_SCALING, linf = lo < -QP_INFTY * QP_MIN_SCALING;
        vproj = delta;
        if (uinf && linf) vproj = 0.0;
        else if (uinf) vproj = fmin(vproj, 0.0);
        else if (linf) vproj = fmax(vproj, 0.0);
      }
      // [y ; x] and [proj(dy) ; dx], each as a constraint part (zero on the variable lanes) and a variable part: the
      // four sums over all 64 columns are then the sums over c < M and over c >= M of the plain loops, term for term
      double sA1, sA2, sP1, sP2;
      {
        const double vv4[4] = {con ? sb : 0.0, con ? vproj : 0.0, (own && !con) ? sa : 0.0, (own && !con) ? delta : 0.0};
        double acc4[4] = {0.0, 0.0, 0.0, 0.0};
        lds_col_dot<4>(KcL, r, vv4, acc4);
        sA1 = acc4[0];
        sA2 = acc4[1];
        sP1 = acc4[2];
        sP2 = acc4[3];
      }
      double v[NQ];
#pragma unroll
      for (int k = 0; k < NQ; k++) v[k] = (k == 4 || k == 5) ? -1.7e308 : 0.0;
      if (con) {
        const double ei = sc_inv;
        const bool uinf = up > QP_INFTY * QP_MIN_SCALING, linf = lo < -QP_INFTY * QP_MIN_SCALING;
        const double adx = ei * sP2;
        v[0] = fabs(ei * (sP1 - sa));
        v[1] = fabs(ei * sP1);
        v[2] = fabs(ei * sa);
        v[3] = fabs(sc_dir * vproj);
        v[4] = uinf ? -1.7e308 : adx;
        v[5] = -(linf ? 1.7e308 : adx);
        v[13] = up * fmax(vproj, 0.0) + lo * fmin(vproj, 0.0);
      } else if (own) {
        const double di = sc_inv, px = sP1, aty = sA1;
        v[6] = fabs(di * (px + sb + aty));
        v[7] = fabs(di * px);
        v[8] = fabs(di * aty);
        v[9] = fabs(di * sb);
        v[10] = fabs(di * sP2);
        v[11] = fabs(di * sA2);
        v[12] = fabs(sc_dir * delta);
        v[14] = sb * delta;
        v[15] = sa * px;
        v[16] = sb * sa;
      }
      {
        // the thirteen maxima through DPP / permlane swaps (exact in any order); the four sums with the shuffles of
        // wave_sum64, all four in flight per step (one after the other they were 17 x 6 dependent LDS-crossbar round
        // trips: 4 us of a 5 us test)
        double vm[NQ_MAX];
#pragma unroll
        for (int k = 0; k < NQ_MAX; k++) vm[k] = v[k];
        group_max<NQ_MAX>(vm, 64);
#pragma unroll
        for (int k = 0; k < NQ_MAX; k++) v[k] = vm[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          double o4[NQ - NQ_MAX];
#pragma unroll
          for (int k = NQ_MAX; k < NQ; k++) o4[k - NQ_MAX] = __shfl_xor(v[k], off, 64);
#pragma unroll
          for (int k = NQ_MAX; k < NQ; k++) v[k] += o4[k - NQ_MAX];
        }
      }
      Norms nm{v[0], v[1], v[2], v[3], v[4], -v[5], v[6] * d.cinv, v[7], v[8], v[9], v[10], v[11], v[12], v[13], v[14],
               v[15], v[16]};
      double obj;
      st = decide_status(d, nm, obj);
      TW_STAMP(2)
      if (st) break;
    }
    if (it > ta.max_iter) it = ta.max_iter;
    if (st == 0) st = MIOSQP_QP_MAX_ITER_REACHED;
    nodes++;
    osqp_iter += it;
    const bool ok = st == MIOSQP_QP_SOLVED || st == MIOSQP_QP_MAX_ITER_REACHED;
    // ---- epilogue ----
    double lower = 0.0, hobj = 0.0, hviol = -1.7e308;
    int int_inf = 0, nextvar = -1;
    if (ok) {
      double xf = 0.0, xi = 0.0;
      if (own && !con) {
        xf = sc_dir * sa;
        if (ipos >= 0) xf = fmin(fmax(xf, clo), chi);
        xi = ipos >= 0 ? rint(xf) : xf;
        xfL[vi] = xf;
        xiL[vi] = xi;
      }
      if (con) yfL[r] = d.cinv * sc_dir * sb;
      __syncthreads();
      double margin = -1.7e308;
      {
        const double vx[1] = {(own && !con) ? sc_inv * xi : 0.0};  // scaled rounded candidate, by variable lane
        double aa[1] = {0.0};
        lds_col_dot<1>(KcL, r, vx, aa);
        if (con) {
          const double zz = sc_inv * aa[0];
          margin = fmax(rootl - d.eps_lin - zz, zz - rootu - d.eps_lin);
        }
      }
      double t1 = 0.0, t2 = 0.0;
      {
        const double vo[2] = {(own && !con) ? xf : 0.0, (own && !con) ? xi : 0.0};
        double ab[2] = {0.0, 0.0};
        lds_col_dot<2>(PrL, r, vo, ab);  // (entries in column order: the order of the compressed row; the rest is zero)
        if (own && !con) {
          t1 = xf * (0.5 * ab[0] + qraw);
          t2 = xi * (0.5 * ab[1] + qraw);
        }
      }
      {
        double mm[1] = {margin};
        group_max<1>(mm, 64);
        hviol = mm[0];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {  // (wave_sum64's order, both sums in flight)
          const double o1 = __shfl_xor(t1, off, 64), o2 = __shfl_xor(t2, off, 64);
          t1 += o1;
          t2 += o2;
        }
        lower = t1;
        hobj = t2;
      }
      // is_int_feas + pick_nextvar: lane k looks at integer variable k; the first of the largest fractions wins
      {
        double f = -1.0;
        int cnt = 0, kk = 0x7fffffff;
        if (r < p) {
          const double vv = xfL[iiL[r]];
          f = fabs(vv - rint(vv));
          cnt = f > d.eps_int;
          kk = r;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const double of = __shfl_xor(f, off, 64);
          const int ok2 = __shfl_xor(kk, off, 64);
          cnt += __shfl_xor(cnt, off, 64);
          if (of > f || (of == f && ok2 < kk)) { f = of; kk = ok2; }
        }
        int_inf = cnt;
        nextvar = kk == 0x7fffffff ? -1 : kk;
      }
    }
    TW_STAMP(3)
    // ---- bound_and_branch ----
    if (r == 0) {
      double upper = sc[0];
      int action = 0;
      bool prune_now = false;
      if (ok && !(lower > upper)) {
        if (int_inf == 0) {
          action = 1;
          upper = lower;
          prune_now = true;
        } else {
          if (hviol <= 0.0 && hobj < upper) {
            action = 2;
            upper = hobj;
            prune_now = true;
          }
          action |= 4;
        }
      }
      if (prune_now) {
        int k = 0;
        while (k < count) {
          if (lf_lower[order[k]] > upper) {
            freelist[nfree++] = order[k];
            for (int q = k; q + 1 < count; q++) order[q] = order[q + 1];
            count--;
          }
          k++;
        }
        found = 1;
      }
      int c0 = -1, c1 = -1;
      if (action & 4) {
        if (nfree < 2 || count + 2 > TREE_CAP) {
          overflow = 1;
        } else {
          c0 = freelist[--nfree];
          c1 = freelist[--nfree];
          const int dep = lf_depth[slot] + 1;
          lf_depth[c0] = lf_depth[c1] = dep;
          lf_lower[c0] = lf_lower[c1] = lower;
          order[count++] = c0;
          order[count++] = c1;
          double lg = 1.0 / 0.0;
          for (int k = 0; k < count; k++) lg = fmin(lg, lf_lower[order[k]]);
          sc[9] = lg;
        }
      }
      freelist[nfree++] = slot;
      sc[0] = upper;
      sc[1] = (double)action;
      sc[7] = (double)c0;
      sc[8] = (double)c1;
      sc[10] = (double)count;
      sc[11] = (double)nfree;
      sc[12] = (double)overflow;
      sc[13] = (double)found;
    }
    __syncthreads();
    {
      const int action = (int)sc[1], c0 = (int)sc[7], c1 = (int)sc[8];
      count = (int)sc[10];
      nfree = (int)sc[11];
      overflow = (int)sc[12];
      found = (int)sc[13];
      if (count > max_leaves) max_leaves = count;
      if ((action & 3) == 1 && r < n) ta.inc_x[r] = xfL[r];
      if ((action & 3) == 2 && r < n) ta.inc_x[r] = xiL[r];
      if ((action & 4) && c0 >= 0) {
        lower_glob = sc[9];
        const double xv = xfL[iiL[nextvar]];
        if (r < p) {
          const double l0 = lo_n[r], h0 = hi_n[r];
          ta.lf_lo[(size_t)c0 * p + r] = l0;
          ta.lf_hi[(size_t)c0 * p + r] = r == nextvar ? floor(xv) : h0;
          ta.lf_lo[(size_t)c1 * p + r] = r == nextvar ? ceil(xv) : l0;
          ta.lf_hi[(size_t)c1 * p + r] = h0;
        }
        if (r < n) {
          ta.lf_x[(size_t)c0 * n + r] = xfL[r];
          ta.lf_x[(size_t)c1 * n + r] = xfL[r];
        }
        if (r < M) {
          ta.lf_y[(size_t)c0 * M + r] = yfL[r];
          ta.lf_y[(size_t)c1 * M + r] = yfL[r];
        }
      }
    }
    __threadfence_block();
    __syncthreads();
    TW_STAMP(4)
  }
#undef TW_STAMP
  if (d.prof && r == 0) {
    for (int k = 0; k < 6; k++) d.prof[k] += tp[k];
  }
  if (r == 0) {
    TreeOut *o = ta.out;
    o->nodes = nodes;
    o->osqp_iter = osqp_iter;
    o->leaves_left = count;
    o->overflow = overflow;
    o->max_leaves = max_leaves;
    o->found = found;
    o->upper = sc[0];
    o->lower_glob = lower_glob;
  }
  if (ta.done) {
    __threadfence_system();  // this wave's stores (incumbent, outcome) have reached host memory
    if (r == 0) {
      ta.done[1] = t_begin;
      ta.done[2] = wall_clock64();
      __hip_atomic_store(&ta.done[0], 1ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
