// part of kernels_tree_body.inc (included there under TREE_SB, nowhere else): strong and reliability branching on the node
// that is about to branch -- Workspace.select_branching / Workspace.strong_branch (miosqp_amd/bnb.py) with the children
// of miosqp_qp_strong_branch (kernels_derived.inc); the decisions are those of tree_sb_logic.hpp, taken by thread 0 on the
// tree's work area in device memory (ta.sb_work: pseudo-costs, the asking node's fractional set, candidates and children).
// Between thread 0's two halves of bound_and_branch: sc[0] upper, sc[1] action, sc[4] the node's lower, sc[6] the position
// the most-fractional rule would take -- the block replaces it with the rule's.
// The 2K children, K down and then K up, are solved one after the other by the whole workgroup in the node's own LDS
// arrays: a node's prologue with ONE integer row changed, the capped relaxation, a node's epilogue.  xf, xi, prow, yf and
// rowbuf are overwritten (the reduced form's termination test overwrites them as well), so the node's xf and yf are
// parked in the node's own place of the leaf store -- its warm start has been read, and the place is released only when
// the node is done -- and read back before the node branches.  From there they are also the children's warm start.  The
// children's iterations go to the sb counter, not to osqp_iter.
    __syncthreads();
    {
      namespace sbl = miosqp::tree_sb;
      const int action0 = (int)sc[1];
      // the node's own incumbent first: xf / xi are about to be overwritten
      if ((action0 & 3) == 1)
        for (int i = tid; i < n; i += RES_THREADS) ta.inc_x[i] = xf[i];
      if ((action0 & 3) == 2)
        for (int i = tid; i < n; i += RES_THREADS) ta.inc_x[i] = xi[i];
      if (action0 & 4) {  // (sc[1]: the same value in every thread)
        const sbl::View sv = sbl::view(ta.sb_work, p);
        const sbl::Par spar{ta.sb_rule, ta.sb_K, ta.sb_rel, ta.sb_eps, d.eps_int};
        if (tid == 0) {
          for (int k = 0; k < p; k++) sv.x[k] = xf[iiL[k]];
          const int pos = sbl::ask(sv, spar);
          if (pos >= 0) sc[6] = (double)pos;
          sc[15] = pos == -1 ? (double)sv.count[1] : 0.0;  // candidates whose children have to be solved
        }
        __threadfence_block();
        __syncthreads();
        const int K = (int)sc[15];
        if (K > 0) {
          double *park_x = ta.lf_x + (size_t)slot * n, *park_y = ta.lf_y + (size_t)slot * M;
          for (int i = tid; i < n; i += RES_THREADS) park_x[i] = xf[i];
          for (int j = tid; j < M; j += RES_THREADS) park_y[j] = yf[j];
          __threadfence_block();
          __syncthreads();
          for (int b = 0; b < 2 * K; b++) {
            const int up = b >= K, cpos = sv.cand[b - up * K];
            // the child's one changed bound: down u = floor(x_c), up l = ceil(x_c), x the node's clamped entry
            const double xc = park_x[iiL[cpos]], cut = up ? ceil(xc) : floor(xc);
            // ---- the prologue of a node with the child's bounds ----
            for (int j = tid; j < M; j += RES_THREADS) {
              const bool mine = j == tid;
              double lo, hi;
              if (j < m0) {
                lo = mine ? rawl_t : d.raw_l[j];
                hi = mine ? rawu_t : d.raw_u[j];
              } else {
                lo = lo_n[j - m0];
                hi = hi_n[j - m0];
                if (j - m0 == cpos) {
                  if (up) lo = cut;
                  else hi = cut;
                }
              }
              const double Ej = mine ? E_t : d.E[j];
              c.l[j] = Ej * fmax(lo, -QP_INFTY);
              c.u[j] = Ej * fmin(hi, QP_INFTY);
              c.y[j] = d.c * (mine ? Einv_t : d.Einv[j]) * park_y[j];
              c.dy[j] = 0.0;
            }
            for (int i = tid; i < n; i += RES_THREADS) {
              const double xs = (i == tid ? Dinv_t : d.Dinv[i]) * park_x[i];
              c.x[i] = xs;
              c.dx[i] = 0.0;
              c.wr[M + i] = sigma * xs - c.q[i];
            }
            __syncthreads();
            {
              const int TG = ta.TG1, NG = RES_THREADS / TG, g = tid / TG, t = tid % TG;
              for (int j = g; j < M; j += NG) {
                double acc[1] = {0.0};
                for (int e = sp.Ap[j] + t; e < sp.Ap[j + 1]; e += TG) acc[0] = fma(sp.A[e], c.x[sp.Ai[e]], acc[0]);
                group_reduce<1>(acc, TG);
                if (t == 0) {
                  c.z[j] = acc[0];
                  c.wr[j] = acc[0] - rinv * c.y[j];
                }
              }
            }
            if (tid == 0) {
              Ctrl *cb = d.ctrl;
              cb->done = 0;
              cb->status = MIOSQP_QP_UNSOLVED;
              cb->iter = 0;
            }
            __syncthreads();
            // ---- the capped relaxation: the node's test at the node's iterations ----
            int cit = 0;
#ifndef TREE_REDUCED
            int cst = res_admm(d, c, ta.sb_max_iter, ta.check_every, 1, ta.TG1, ta.TG2, &cit, sp);
#else
            int cst = res_admm_r(d, c, rs, ra, ta.sb_max_iter, ta.check_every, 1, ta.TG1, &cit, sp);
#endif
            if (cst == 0) cst = MIOSQP_QP_MAX_ITER_REACHED;
            const bool has_x = cst == MIOSQP_QP_SOLVED || cst == MIOSQP_QP_MAX_ITER_REACHED;
            // ---- the epilogue of a node: unscale, clamp into the child's bounds, the objective rows of the clamped x ----
            if (has_x) {
              for (int i = tid; i < n; i += RES_THREADS) {
                double v = (i == tid ? D_t : d.D[i]) * c.x[i];
                const int pos = i == tid ? pos_t : d.int_pos[i];
                if (pos >= 0) {
                  double lo = lo_n[pos], hi = hi_n[pos];
                  if (pos == cpos) {
                    if (up) lo = cut;
                    else hi = cut;
                  }
                  v = fmin(fmax(v, lo), hi);
                }
                xf[i] = v;
              }
              __syncthreads();
              {
                const int TG = ta.TG1, NG = RES_THREADS / TG, g = tid / TG, t = tid % TG;
                for (int i = g; i < n; i += NG) {
                  double acc[1] = {0.0};
                  const double qi = d.qraw[i];
                  for (int e = d.pr_ptr[i] + t; e < d.pr_ptr[i + 1]; e += TG) acc[0] = fma(d.pr_val[e], xf[d.pr_idx[e]], acc[0]);
                  group_reduce<1>(acc, TG);
                  if (t == 0) prow[i] = xf[i] * (0.5 * acc[0] + qi);
                }
              }
              __syncthreads();
            }
            // the child's objective on the first wavefront, in the order of a node's `lower`
            double w_low = 0.0;
            if (tid < 64 && has_x) {
              double a = 0.0;
              for (int i = tid; i < n; i += 64) a += prow[i];
#pragma unroll
              for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
              w_low = a;
            }
            if (tid == 0) {
              sv.ch_has[b] = has_x ? 1 : 0;
              sv.ch_iter[b] = cit;
              sv.ch_lower[b] = w_low;
            }
            __syncthreads();  // (prow is read before the next child writes it)
          }
          if (tid == 0) {
            int its = 0;
            sc[6] = (double)sbl::decide(sv, spar, sc[4], &its);
            sb_calls++;
            sb_children += 2 * K;
            sb_iter += its;
          }
          // the node's xf and yf again: it branches on them
          for (int i = tid; i < n; i += RES_THREADS) xf[i] = park_x[i];
          for (int j = tid; j < M; j += RES_THREADS) yf[j] = park_y[j];
        }
      }
    }
    __syncthreads();
