// part of kernels_tree_body.inc (included there under TREE_RF, nowhere else): round and fix on the node that is about to
// branch -- Workspace.primal_heuristic / Workspace.round_and_fix (miosqp_amd/bnb.py) with the semantics of k_rf_candidates
// and k_rf_pick (kernels_derived.inc); the decisions are those of tree_rf_logic.hpp.
// Between thread 0's two halves of bound_and_branch: sc[0] upper (after the node's own heuristic and pruning), sc[1] action.
// The K candidates are solved one after the other by the whole workgroup in the node's own LDS arrays: xf, xi, prow, yf
// and rowbuf are overwritten (the reduced form's termination test overwrites them as well), so the node's xf and yf are
// parked in the node's own place of the leaf store -- its warm start has been read, and the place is released only when
// the node is done -- and read back before the node branches.  From there they are also the candidates' warm start,
// through the prologue of a node.  The heuristic's iterations do not enter osqp_iter.
    __syncthreads();
    {
      namespace rf = miosqp::tree_rf;
      const int action0 = (int)sc[1], K = ta.rf_K;
      // the node's own incumbent first: xf / xi are about to be overwritten
      if ((action0 & 3) == 1)
        for (int i = tid; i < n; i += RES_THREADS) ta.inc_x[i] = xf[i];
      if ((action0 & 3) == 2)
        for (int i = tid; i < n; i += RES_THREADS) ta.inc_x[i] = xi[i];
      bool fire = false;
      if ((action0 & 4) && K > 0) {  // (every thread counts: the same value everywhere)
        fire = rf::fires(rf_nodes, ta.rf_every);
        rf_nodes++;
      }
      if (fire) {
        double *park_x = ta.lf_x + (size_t)slot * n, *park_y = ta.lf_y + (size_t)slot * M;
        for (int i = tid; i < n; i += RES_THREADS) park_x[i] = xf[i];
        for (int j = tid; j < M; j += RES_THREADS) park_y[j] = yf[j];
        __threadfence_block();
        __syncthreads();
        rf::Pick pick;  // (thread 0's copy decides)
        for (int k = 0; k < K; k++) {
          const double th = rf::theta(k, K);
          // ---- the prologue of a node, the integer rows fixed to the rounding of the node's x ----
          for (int j = tid; j < M; j += RES_THREADS) {
            const bool mine = j == tid;
            double lo, hi;
            if (j < m0) {
              lo = mine ? rawl_t : d.raw_l[j];
              hi = mine ? rawu_t : d.raw_u[j];
            } else {
              lo = hi = rf::fixed_value(park_x[iiL[j - m0]], th, lo_n[j - m0], hi_n[j - m0]);
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
          int cst = res_admm(d, c, ta.rf_max_iter, ta.check_every, 1, ta.TG1, ta.TG2, &cit, sp);
#else
          int cst = res_admm_r(d, c, rs, ra, ta.rf_max_iter, ta.check_every, 1, ta.TG1, &cit, sp);
#endif
          if (cst == 0) cst = MIOSQP_QP_MAX_ITER_REACHED;
          const bool has_x = cst == MIOSQP_QP_SOLVED || cst == MIOSQP_QP_MAX_ITER_REACHED;
          // ---- the epilogue of a node: unscale, clamp to the fixed bounds, round; margins against the ROOT bounds and the
          //      objective rows of the rounded point ----
          if (has_x) {
            for (int i = tid; i < n; i += RES_THREADS) {
              double v = (i == tid ? D_t : d.D[i]) * c.x[i];
              const int pos = i == tid ? pos_t : d.int_pos[i];
              if (pos >= 0) {
                const double fx = rf::fixed_value(park_x[i], th, lo_n[pos], hi_n[pos]);
                v = fmin(fmax(v, fx), fx);
              }
              xf[i] = v;
              const double r = pos >= 0 ? rint(v) : v;
              xi[i] = r;
              c.ut[i] = (i == tid ? Dinv_t : d.Dinv[i]) * r;
            }
            __syncthreads();
            {
              const int TG = ta.TG1, NG = RES_THREADS / TG, g = tid / TG, t = tid % TG;
              for (int j = g; j < M; j += NG) {
                double acc[1] = {0.0};
                const double ej = d.Einv[j], rl = d.root_l[j], ru = d.root_u[j];
                for (int e = sp.Ap[j] + t; e < sp.Ap[j + 1]; e += TG) acc[0] = fma(sp.A[e], c.ut[sp.Ai[e]], acc[0]);
                group_reduce<1>(acc, TG);
                if (t == 0) {
                  const double zz = ej * acc[0];
                  rowbuf[j] = fmax(rl - d.eps_lin - zz, zz - ru - d.eps_lin);
                }
              }
              for (int i = g; i < n; i += NG) {
                double acc[1] = {0.0};
                const double qi = d.qraw[i];
                for (int e = d.pr_ptr[i] + t; e < d.pr_ptr[i + 1]; e += TG) acc[0] = fma(d.pr_val[e], xi[d.pr_idx[e]], acc[0]);
                group_reduce<1>(acc, TG);
                if (t == 0) prow[n + i] = xi[i] * (0.5 * acc[0] + qi);
              }
            }
            __syncthreads();
          }
          // the rounded point's objective and worst margin on the first wavefront, in the order of a node's sums
          double w_obj = 0.0, w_viol = -1.7e308;
          if (tid < 64 && has_x) {
            double b = 0.0, cmax = -1.7e308;
            for (int i = tid; i < n; i += 64) b += prow[n + i];
            for (int j = tid; j < M; j += 64) cmax = fmax(cmax, rowbuf[j]);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
              const double ob = __shfl_xor(b, off, 64), oc = __shfl_xor(cmax, off, 64);
              b += ob;
              cmax = fmax(cmax, oc);
            }
            w_obj = b;
            w_viol = cmax;
          }
          if (tid == 0) {
            rf_iter += cit;
            sc[15] = pick.take(k, has_x, w_viol, w_obj, sc[0]) ? 1.0 : 0.0;
          }
          __syncthreads();
          if (sc[15] != 0.0)  // the best so far counts, so the call's winner replaces the incumbent whatever follows
            for (int i = tid; i < n; i += RES_THREADS) ta.inc_x[i] = xi[i];
          __syncthreads();  // (sc[15] and xi are read before the next candidate writes them)
        }
        if (tid == 0) {
          rf_calls++;
          rf_cand += K;
          rf_feas += pick.feasible;
          if (pick.best >= 0) {
            const double upper = pick.best_obj;  // the device's sum, as in the lock-step trees
            sc[0] = upper;
            rf_impr++;
            found = 1;
            int k = 0;  // Workspace.prune: the element behind a removed one is skipped
            while (k < count) {
              if (lf_lower[order[k]] > upper) {
                freelist[nfree++] = order[k];
                for (int q = k; q + 1 < count; q++) order[q] = order[q + 1];
                count--;
              }
              k++;
            }
          }
        }
        // the node's xf and yf again: it branches on them
        for (int i = tid; i < n; i += RES_THREADS) xf[i] = park_x[i];
        for (int j = tid; j < M; j += RES_THREADS) yf[j] = park_y[j];
      }
    }
    __syncthreads();
