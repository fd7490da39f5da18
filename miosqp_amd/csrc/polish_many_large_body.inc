// part of polish_many_large.hip (included there, not compiled alone): one instance from classification to record, the
// body of k_pol_many_g and of k_pol_many_gm, as text in both entries (as polish_many_body.inc: a shared __forceinline__
// function moves the register allocation, DESIGN 3l).  The entry defines before it:
//   sh_w, sh_l, sh_t, sh_c, sh_red (the static LDS), g (const PolManyLargeArgs &: the launch's arguments or a table
//   entry with final pointers), slab (this workgroup's slab), inst (the instance's index behind g.a's pointers),
//   POLG_TABLE (constexpr bool: the table entry, whose y may be NULL) and polg_tau (its guess's size)
  const PolManyArgs &a = g.a;
  const int n = a.n, M = a.M, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const PolgSlab o = polg_layout(n, M);
  const int ld = o.ld, ldw = o.ldw;
  double *S = slab + o.S, *Wp = slab + o.Wp, *Lp = slab + o.Lp, *xh = slab + o.xh, *t = slab + o.t, *v = slab + o.v;
  double *xk = slab + o.xk, *dd = slab + o.dd, *ocol = slab + o.ocol, *dcol = slab + o.dcol, *yh = slab + o.yh;
  double *r2 = slab + o.r2, *yk = slab + o.yk, *prow = slab + o.prow, *red = sh_red;
  int *act = (int *)(slab + o.act);
  signed char *clsbuf[2] = {(signed char *)(slab + o.cls), (signed char *)(slab + o.cls) + M};
  const double delta = a.delta, inv_delta = a.inv_delta;

  // sparse dot products by one wavefront (every lane returns them): row r of A, row i of P, column i of A (unrolled so
  // that four index / value / gather loads are in flight; a lane's terms keep their order)
  auto a_row = [&](int r, const double *vec) {
    double acc = 0.0;
#pragma unroll 4
    for (int k = a.pc_ptr[r] + lane; k < a.pc_ptr[r + 1]; k += 64) acc = fma(a.A[k], vec[a.pc_idx[k]], acc);
    return polg_wave_sum(acc);
  };
  auto p_row = [&](int i, const double *vec) {
    double acc = 0.0;
#pragma unroll 4
    for (int k = a.pr_ptr[i] + lane; k < a.pr_ptr[i + 1]; k += 64) acc = fma(a.pr_val[k], vec[a.pr_idx[k]], acc);
    return polg_wave_sum(acc);
  };
  auto a_col = [&](int i, const double *vec) {
    double acc = 0.0;
#pragma unroll 4
    for (int k = g.pv_ptr[i] + lane; k < g.pv_ptr[i + 1]; k += 64) acc = fma(g.At[k], vec[g.pv_idx[k]], acc);
    return polg_wave_sum(acc);
  };

  double *out = a.out + inst * polm_out_stride(n, M);
  const double *qg = a.q ? a.q + inst * n : a.q_engine;
  const double *lg = a.l + inst * M, *ug = a.u + inst * M, *xg = a.x + inst * n, *yg = a.y + inst * M;
  if constexpr (POLG_TABLE) {
    if (!a.y) yg = out + POLM_REC_DOUBLES + n;  // no y: stage 1 writes its guess to the record's y slot and it is read there
  }

  // the residuals and the objective of a point (X, Y), over ALL rows (every thread gets them)
  double j_pri = 0.0, j_dua = 0.0, j_obj = 0.0;
  auto judge_norms = [&](const double *X, const double *Y) {
    for (int r = wv; r < M; r += 4) {
      const double z = a_row(r, X);
      if (lane == 0) prow[r] = polg_max(polg_max(0.0, lg[r] - z), z - ug[r]);
    }
    for (int i = wv; i < n; i += 4) {
      const double px = p_row(i, X), aty = a_col(i, Y);
      if (lane == 0) {
        dcol[i] = fabs((px + qg[i]) + aty);
        ocol[i] = X[i] * fma(0.5, px, qg[i]);
      }
    }
    __syncthreads();
    j_pri = polg_block_max(prow, M, red, tid);
    j_dua = polg_block_max(dcol, n, red, tid);
    j_obj = polg_block_sum(ocol, n, red, tid);
  };

  // ---- 1. the set guessed from (x, y) and the input's residuals
  for (int i = tid; i < n; i += 256) xh[i] = 0.0;
  for (int r = tid; r < M; r += 256) yh[r] = 0.0;
  for (int r = wv; r < M; r += 4) {
    const double z = a_row(r, xg);
    if (lane == 0) {
      const double l = lg[r], u = ug[r];
      double y;
      if constexpr (POLG_TABLE) {
        if (!a.y) {  // a tree returns no y: the side of the nearer bound, tau in size; this is the y a rejection returns
          y = (l == u || (l <= -POLG_INFTY && u >= POLG_INFTY)) ? 0.0 : (z - l < u - z ? -polg_tau : polg_tau);
          (out + POLM_REC_DOUBLES + n)[r] = y;
        } else {
          y = yg[r];
        }
      } else {
        y = yg[r];
      }
      signed char c = 0;
      if (l > -POLG_INFTY && (l == u || z - l < -y)) c = -1;
      else if (u < POLG_INFTY && u - z < y) c = 1;
      clsbuf[0][r] = c;
    }
  }
  if constexpr (POLG_TABLE) {
    if (!a.y) __syncthreads();  // (the guess is read by every wavefront below)
  }
  judge_norms(xg, yg);
  const double pri0 = j_pri, dua0 = j_dua;
  auto judge = [&](const double *X, const double *Y) {
    judge_norms(X, Y);
    return !(j_pri <= fmax(pri0, 1e-10)) ? 2 : !(j_dua <= fmax(dua0, 1e-10)) ? 3 : 0;
  };

  // ---- 2, 3. the rounds
  int k = 0, judged = 0, stop = 0, added = 0, dropped = 0, reason0 = 1;
  bool broke0 = false;
  double pri_r0 = 0.0, dua_r0 = 0.0, obj_r0 = 0.0;
  for (;;) {
    const signed char *cur = clsbuf[k & 1];
    signed char *nxt = clsbuf[(k + 1) & 1];
    // the active rows in ascending order, by the first wavefront (every wavefront counts them)
    int na = 0;
    for (int c0 = 0; c0 < M; c0 += 64) {
      const int r = c0 + lane;
      const bool on = r < M && cur[r] != 0;
      const unsigned long long mask = __ballot(on);
      if (wv == 0 && on) act[na + __popcll(mask & ((1ull << lane) - 1ull))] = r;
      na += __popcll(mask);
    }
    // S = P + delta I on the lower triangle (the entries of a row of P are distinct columns; a pad repeats the last)
    for (int i = wv; i < n; i += 4)
      for (int c = lane; c <= i; c += 64) S[(size_t)i * ld + c] = 0.0;
    __syncthreads();
    for (int i1 = wv; i1 < n; i1 += 4) {
      const int k0 = a.pr_ptr[i1], k1 = a.pr_ptr[i1 + 1];
      for (int kk = k0 + lane; kk < k1; kk += 64) {
        const int i2 = a.pr_idx[kk];
        if (i2 > i1 || (kk > k0 && a.pr_idx[kk - 1] == i2)) continue;
        S[(size_t)i1 * ld + i2] = a.pr_val[kk];
      }
    }
    __syncthreads();
    for (int i = tid; i < n; i += 256) S[(size_t)i * ld + i] += delta;
    // ... plus A_act^T A_act / delta, 32 active rows at a time: their dense image (k-major) in the slab, then one
    // rank-32 update of the whole triangle; the rows a last chunk lacks are zeros
    for (int s0 = 0; s0 < na; s0 += NB) {
      for (int e = tid; e < NB * ldw; e += 256) Lp[e] = 0.0;
      __syncthreads();
      for (int c = wv; c < NB && s0 + c < na; c += 4) {
        const int r = act[s0 + c], k0 = a.pc_ptr[r], k1 = a.pc_ptr[r + 1];
        for (int kk = k0 + lane; kk < k1; kk += 64) {
          const int i = a.pc_idx[kk];
          if (kk > k0 && a.pc_idx[kk - 1] == i) continue;
          Lp[(size_t)c * ldw + i] = a.A[kk];
        }
      }
      __syncthreads();
      polg_rank_update<POLG_TABLE>(S, ld, n, 0, Lp, Lp, ldw, inv_delta, 1.0, sh_w, sh_l, tid);
    }
    __syncthreads();

    // blocked right-looking LDL^T in place: L below the diagonal, the pivots on it and in dd
    bool broke = false;
    for (int j0 = 0; j0 < n; j0 += NB) {
      const int nb = min(NB, n - j0), r0 = j0 + nb;
      for (int e = tid; e < NB * NB; e += 256) {
        const int r = e >> 5, c = e & 31;
        sh_t[r * TD + c] = (r < nb && c <= r) ? S[(size_t)(j0 + r) * ld + j0 + c] : 0.0;
      }
      __syncthreads();
      for (int j = 0; j < nb; j++) {
        const double d = sh_t[j * TD + j];
        if (!(d > 0.0)) {  // (uniform: every thread reads the same pivot)
          broke = true;
          break;
        }
        if (tid > j && tid < nb) sh_c[tid] = sh_t[tid * TD + j] / d;
        __syncthreads();
        for (int e = tid; e < NB * NB; e += 256) {
          const int i = e >> 5, c = e & 31;
          if (c > j && c <= i && i < nb) sh_t[i * TD + c] = fma(-sh_t[i * TD + j], sh_c[c], sh_t[i * TD + c]);
        }
        __syncthreads();
        if (tid > j && tid < nb) sh_t[tid * TD + j] = sh_c[tid];
      }
      if (broke) break;
      __syncthreads();
      for (int e = tid; e < NB * NB; e += 256) {
        const int r = e >> 5, c = e & 31;
        if (r < nb && c <= r) S[(size_t)(j0 + r) * ld + j0 + c] = sh_t[r * TD + c];
      }
      if (tid < nb) dd[j0 + tid] = sh_t[tid * TD + tid];
      if (r0 < n) {
        // the panel below (nb == 32 here), then the trailing update with it
        polg_panel_solve<POLG_TABLE>(S, ld, n, j0, Wp, Lp, ldw, sh_t, tid);
        __syncthreads();
        polg_rank_update<POLG_TABLE>(S, ld, n, r0, Wp, Lp, ldw, 1.0, -1.0, sh_w, sh_l, tid);
      }
      __syncthreads();
    }
    if (broke) {
      if (k == 0) broke0 = true;
      else stop = 2;  // the point and the set of the round before are judged
      break;
    }

    // 1 + refine_iter solves: with xh = yh = 0 the first pass's residuals are exactly (-q, b)
    for (int it = 0; it <= a.refine_iter; it++) {
      for (int r = wv; r < M; r += 4) {
        const signed char c = cur[r];
        double rr = 0.0;
        if (c != 0) rr = (c < 0 ? lg[r] : ug[r]) - (it > 0 ? a_row(r, xh) : 0.0);  // (uniform over the wavefront)
        if (lane == 0) r2[r] = rr;
      }
      __syncthreads();
      // t = (-q - P xh - A^T yh) + A^T r2 / delta; yh and r2 are zero on the inactive rows
      for (int i = wv; i < n; i += 4) {
        const double px = it > 0 ? p_row(i, xh) : 0.0;
        double aty = 0.0, atr = 0.0;
#pragma unroll 4
        for (int kk = g.pv_ptr[i] + lane; kk < g.pv_ptr[i + 1]; kk += 64) {
          const int r = g.pv_idx[kk];
          const double av = g.At[kk];
          aty = fma(av, yh[r], aty);
          atr = fma(av, inv_delta * r2[r], atr);
        }
        aty = polg_wave_sum(aty);
        atr = polg_wave_sum(atr);
        if (lane == 0) t[i] = ((-qg[i] - px) - aty) + atr;
      }
      __syncthreads();
      // forward, L w = t, a block of 32 at a time: each row of the block takes its dot product with the w before
      // the block (one wavefront per row, lanes striding the row of S), then the diagonal block is solved in LDS by
      // the first wavefront; w goes to v
      for (int j0 = 0; j0 < n; j0 += NB) {
        const int nb = min(NB, n - j0);
        for (int e = tid; e < NB * NB; e += 256) {
          const int r = e >> 5, c = e & 31;
          sh_t[r * TD + c] = (r < nb && c < r) ? S[(size_t)(j0 + r) * ld + j0 + c] : 0.0;
        }
        for (int r = wv; r < nb; r += 4) {
          const double *row = S + (size_t)(j0 + r) * ld;
          double acc = 0.0;
#pragma unroll 4
          for (int j = lane; j < j0; j += 64) acc = fma(row[j], v[j], acc);
          acc = polg_wave_sum(acc);
          if (lane == 0) sh_c[r] = t[j0 + r] - acc;
        }
        __syncthreads();
        if (wv == 0) {
          double reg = lane < nb ? sh_c[lane] : 0.0;
          for (int j = 0; j < nb; j++) {
            const double vj = __shfl(reg, j, 64);
            if (lane > j && lane < nb) reg = fma(-sh_t[lane * TD + j], vj, reg);
          }
          if (lane < nb) v[j0 + lane] = reg;
        }
        __syncthreads();
      }
      // the pivots and backward, L^T dx = w / d, from the last block: column c of the block gathers L[i][c] dx[i] over
      // the rows below the block (eight threads per column, each its rows in ascending order, the eight in order),
      // then the diagonal block by the first wavefront; dx replaces w in v
      for (int j0 = ((n - 1) / NB) * NB; j0 >= 0; j0 -= NB) {
        const int nb = min(NB, n - j0), r0 = j0 + nb;
        for (int e = tid; e < NB * NB; e += 256) {
          const int r = e >> 5, c = e & 31;
          sh_t[r * TD + c] = (r < nb && c < r) ? S[(size_t)(j0 + r) * ld + j0 + c] : 0.0;
        }
        {
          const int c = tid & 31, rg = tid >> 5;
          double acc = 0.0;
          if (c < nb)
#pragma unroll 4
            for (int i = r0 + rg; i < n; i += 8) acc = fma(S[(size_t)i * ld + j0 + c], v[i], acc);
          sh_w[rg * NB + c] = acc;
        }
        __syncthreads();
        if (wv == 0) {
          double reg = 0.0;
          if (lane < nb) {
            double acc = sh_w[lane];
#pragma unroll
            for (int rg = 1; rg < 8; rg++) acc += sh_w[rg * NB + lane];
            reg = v[j0 + lane] / dd[j0 + lane] - acc;
          }
          for (int j = nb - 1; j > 0; j--) {
            const double xj = __shfl(reg, j, 64);
            if (lane < j) reg = fma(-sh_t[j * TD + lane], xj, reg);
          }
          if (lane < nb) v[j0 + lane] = reg;
        }
        __syncthreads();
      }
      for (int i = tid; i < n; i += 256) xh[i] += v[i];
      for (int r = wv; r < M; r += 4) {
        if (cur[r] == 0) continue;  // (uniform over the wavefront)
        const double av = a_row(r, v);
        if (lane == 0) yh[r] += inv_delta * (av - r2[r]);
      }
      __syncthreads();
    }
    if (k == 0) {
      reason0 = judge(xh, yh);
      pri_r0 = j_pri;
      dua_r0 = j_dua;
      obj_r0 = j_obj;
    }
    // the revision: an equality row stays; an active row whose multiplier has the wrong sign leaves; an inactive row
    // violated by more than the tolerance joins on that side
    judged = k;
    for (int r = wv; r < M; r += 4) {
      const signed char c = cur[r];
      const double z = c == 0 ? a_row(r, xh) : 0.0;  // (uniform over the wavefront)
      if (lane == 0) {
        const double l = lg[r], u = ug[r], y = yh[r];
        signed char cn = c;
        if (l != u) {
          if (c < 0) cn = y > POLG_TOL ? 0 : c;
          else if (c > 0) cn = y < -POLG_TOL ? 0 : c;
          else if (l > -POLG_INFTY && l - z > POLG_TOL) cn = -1;
          else if (u < POLG_INFTY && z - u > POLG_TOL) cn = 1;
        }
        nxt[r] = cn;
      }
    }
    __syncthreads();
    int c4 = 0, c5 = 0;
    for (int r = tid; r < M; r += 256) {
      const signed char c = cur[r], cn = nxt[r];
      c4 += cn != c && c == 0;
      c5 += cn != c && c != 0;
    }
    c4 = polg_block_count(c4, red, tid);
    c5 = polg_block_count(c5, red, tid);
    added += c4;
    dropped += c5;
    if (c4 + c5 == 0) break;
    if (k == a.repair_iter) {
      stop = 1;
      break;
    }
    // the next round on the revised set from xh = yh = 0; this round's point is kept
    for (int i = tid; i < n; i += 256) {
      xk[i] = xh[i];
      xh[i] = 0.0;
    }
    for (int r = tid; r < M; r += 256) {
      yk[r] = yh[r];
      yh[r] = 0.0;
    }
    k++;
    __syncthreads();
  }
  const int rounds = k;

  // ---- 4. the point the loop ended with, the decision, the record
  const double *X = stop == 2 ? xk : xh, *Y = stop == 2 ? yk : yh;
  int reason = reason0;
  double pri1 = pri_r0, dua1 = dua_r0, obj = obj_r0;
  if (broke0) {
    reason = 1;
    pri1 = dua1 = obj = __builtin_nan("");
  } else if (rounds > 0) {
    reason = judge(X, Y);
    pri1 = j_pri;
    dua1 = j_dua;
    obj = j_obj;
  }
  const signed char *fin = clsbuf[judged & 1];
  int c_lo = 0, c_up = 0;
  for (int r = tid; r < M; r += 256) {
    c_lo += fin[r] < 0;
    c_up += fin[r] > 0;
  }
  const int n_lower = polg_block_count(c_lo, red, tid), n_upper = polg_block_count(c_up, red, tid);
  if (tid == 0) {
    PolManyRec r;
    r.accepted = reason == 0;
    r.reason = reason;
    r.n_lower = n_lower;
    r.n_upper = n_upper;
    r.rounds = rounds;
    r.stop = stop;
    r.n_added = added;
    r.n_dropped = dropped;
    r.accepted0 = reason0 == 0;
    r.reason0 = reason0;
    r.pad[0] = r.pad[1] = 0;
    r.pri_before = pri0;
    r.dua_before = dua0;
    r.pri_after = pri1;
    r.dua_after = dua1;
    r.obj = obj;
    *(PolManyRec *)out = r;
  }
  double *xo = out + POLM_REC_DOUBLES, *yo = xo + n;
  signed char *co = (signed char *)(yo + M);
  const bool take = reason == 0;
  for (int i = tid; i < n; i += 256) xo[i] = take ? X[i] : xg[i];
  for (int r = tid; r < M; r += 256) {
    yo[r] = take ? Y[r] : yg[r];
    co[r] = fin[r];
  }
  __syncthreads();  // (the slab is the next instance's)
