// part of polish_many.hip (included there, not compiled alone): the body of k_pol_many and of k_pol_many_m, as text in
// both entries (a shared __forceinline__ function moves the register allocation, DESIGN 3l).  The entry defines before it:
//   polm_lds (the dynamic LDS), a (const PolManyArgs &, final pointers or the launch's), inst (the instance's index
//   behind a's pointers), POLM_TABLE (constexpr bool: the table entry, whose y may be NULL) and polm_tau (its guess's size)
  const int n = a.n, M = a.M, lda = n | 1, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const PolmLds o = polm_layout(n, M);
  double *S = polm_lds + o.S, *Ad = polm_lds + o.Ad, *q = polm_lds + o.q, *xh = polm_lds + o.xh, *t = polm_lds + o.t;
  double *v = polm_lds + o.v, *px = polm_lds + o.px, *xk = polm_lds + o.xk, *lo = polm_lds + o.l, *up = polm_lds + o.u;
  double *yh = polm_lds + o.yh, *r2 = polm_lds + o.r2, *yk = polm_lds + o.yk, *red = polm_lds + o.red;
  int *act = (int *)(polm_lds + o.act);
  signed char *clsbuf[2] = {(signed char *)(polm_lds + o.cls), (signed char *)(polm_lds + o.cls) + M};
  const double *qg = a.q ? a.q + inst * n : a.q_engine;
  const double *lg = a.l + inst * M, *ug = a.u + inst * M, *xg = a.x + inst * n, *yg = a.y + inst * M;
  const double delta = a.delta, inv_delta = a.inv_delta;
  const int ntri = (n * (n + 1)) / 2;

  // P vec -> px, one wavefront per row of the full symmetric P (lanes stride the row, an xor butterfly: the sums of the
  // single polish); the caller puts a barrier behind it
  auto p_times = [&](const double *vec) {
    for (int i = wv; i < n; i += 4) {
      double acc = 0.0;
      for (int k = a.pr_ptr[i] + lane; k < a.pr_ptr[i + 1]; k += 64) acc = fma(a.pr_val[k], vec[a.pr_idx[k]], acc);
      acc = polm_wave_sum(acc);
      if (lane == 0) px[i] = acc;
    }
  };
  // row `r` of A times vec, by one thread in ascending order of the variables
  auto a_row = [&](int r, const double *vec) {
    const double *row = Ad + r * lda;
    double acc = 0.0;
    for (int i = 0; i < n; i++) acc = fma(row[i], vec[i], acc);
    return acc;
  };

  // ---- 1. the instance's vectors and the dense image of A (pads repeat a row's last column with a zero: skipped)
  for (int i = tid; i < n; i += 256) {
    q[i] = qg[i];
    xk[i] = xg[i];  // (the input sits where the kept point will: it is needed only before the first round)
    xh[i] = 0.0;
  }
  for (int r = tid; r < M; r += 256) {
    lo[r] = lg[r];
    up[r] = ug[r];
    if constexpr (POLM_TABLE) yk[r] = yg ? yg[r] : 0.0;  // (no y: stage 2 guesses it)
    else yk[r] = yg[r];
    yh[r] = 0.0;
  }
  for (int e = tid; e < M * lda; e += 256) Ad[e] = 0.0;
  __syncthreads();
  for (int r = wv; r < M; r += 4) {
    const int k0 = a.pc_ptr[r], k1 = a.pc_ptr[r + 1];
    for (int k = k0 + lane; k < k1; k += 64) {
      const int i = a.pc_idx[k];
      if (k > k0 && a.pc_idx[k - 1] == i) continue;
      Ad[r * lda + i] = a.A[k];
    }
  }
  p_times(xk);
  __syncthreads();

  // ---- 2. the set guessed from (x, y) and the input's residuals
  double pri0, dua0;
  {
    double pr = 0.0;
    if (tid < M) {
      const int r = tid;
      const double z = a_row(r, xk), l = lo[r], u = up[r];
      double y = yk[r];
      if constexpr (POLM_TABLE) {
        if (!yg) {  // a tree returns no y: the side of the nearer bound, tau in size; this is the y a rejection returns
          y = (l == u || (l <= -POLM_INFTY && u >= POLM_INFTY)) ? 0.0 : (z - l < u - z ? -polm_tau : polm_tau);
          yk[r] = y;
          (a.out + inst * polm_out_stride(n, M) + POLM_REC_DOUBLES + n)[r] = y;
        }
      }
      signed char c = 0;
      if (l > -POLM_INFTY && (l == u || z - l < -y)) c = -1;
      else if (u < POLM_INFTY && u - z < y) c = 1;
      clsbuf[0][r] = c;
      pr = polm_max(polm_max(0.0, l - z), z - u);
    }
    pri0 = polm_block_max(pr, red, tid);
    double du = 0.0;
    if (tid < n) {
      double a0 = 0.0;
      for (int r = 0; r < M; r++) a0 = fma(Ad[r * lda + tid], yk[r], a0);
      du = fabs((px[tid] + q[tid]) + a0);
    }
    dua0 = polm_block_max(du, red, tid);
  }

  // the residuals and the objective of a point (X, Y) in LDS, over ALL rows (every thread gets them)
  double j_pri = 0.0, j_dua = 0.0, j_obj = 0.0;
  auto judge = [&](const double *X, const double *Y) {
    p_times(X);
    double pr = 0.0;
    if (tid < M) {
      const double z = a_row(tid, X);
      pr = polm_max(polm_max(0.0, lo[tid] - z), z - up[tid]);
    }
    j_pri = polm_block_max(pr, red, tid);  // (its barriers also publish px)
    double du = 0.0, ob = 0.0;
    if (tid < n) {
      double a1 = 0.0;
      for (int r = 0; r < M; r++) a1 = fma(Ad[r * lda + tid], Y[r], a1);
      du = fabs((px[tid] + q[tid]) + a1);
      ob = X[tid] * fma(0.5, px[tid], q[tid]);
    }
    j_dua = polm_block_max(du, red, tid);
    j_obj = polm_block_sum(ob, red, tid);
    const int reason = !(j_pri <= fmax(pri0, 1e-10)) ? 2 : !(j_dua <= fmax(dua0, 1e-10)) ? 3 : 0;
    return reason;
  };

  // ---- 3, 4. the rounds
  int k = 0, judged = 0, stop = 0, added = 0, dropped = 0, reason0 = 1;
  bool broke0 = false;
  double pri_r0 = 0.0, dua_r0 = 0.0, obj_r0 = 0.0;
  for (;;) {
    const signed char *cur = clsbuf[k & 1];
    signed char *nxt = clsbuf[(k + 1) & 1];
    // the active rows in ascending order, by the first wavefront
    int na = 0;
    for (int c0 = 0; c0 < M; c0 += 64) {
      const int r = c0 + lane;
      const bool on = r < M && cur[r] != 0;
      const unsigned long long mask = __ballot(on);
      if (wv == 0 && on) act[na + __popcll(mask & ((1ull << lane) - 1ull))] = r;
      na += __popcll(mask);
    }
    // S: zeros, P's entries (lower triangle; a pad repeats the row's last column), delta, then the active rows
    for (int e = tid; e < ntri; e += 256) S[e] = 0.0;
    __syncthreads();
    for (int i1 = wv; i1 < n; i1 += 4) {
      const int k0 = a.pr_ptr[i1], k1 = a.pr_ptr[i1 + 1];
      for (int kk = k0 + lane; kk < k1; kk += 64) {
        const int i2 = a.pr_idx[kk];
        if (i2 > i1 || (kk > k0 && a.pr_idx[kk - 1] == i2)) continue;
        S[polm_tri(i1) + i2] += a.pr_val[kk];
      }
    }
    __syncthreads();
    if (tid < n) S[polm_tri(tid) + tid] += delta;
    __syncthreads();
    for (int e = tid; e < ntri; e += 256) {
      int i1 = (int)((sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
      while (polm_tri(i1) > e) i1--;
      while (polm_tri(i1 + 1) <= e) i1++;
      const int i2 = e - polm_tri(i1);
      double acc = S[e];
      for (int s = 0; s < na; s++) {
        const double *row = Ad + act[s] * lda;
        acc = fma(inv_delta * row[i1], row[i2], acc);
      }
      S[e] = acc;
    }
    __syncthreads();
    // LDL^T in place, right-looking: column j over its pivot goes to a buffer, the trailing rows take
    // S[i][k] -= S[i][j] * L[k][j], and L's column j replaces S's one step later (its old values are still being read)
    bool broke = false;
    for (int j = 0; j < n; j++) {
      const double d = S[polm_tri(j) + j];
      if (!(d > 0.0)) {  // (uniform: every thread reads the same pivot)
        broke = true;
        break;
      }
      double *cb = (j & 1) ? v : t;
      const double *cbp = (j & 1) ? t : v;
      {
        const int i = j + tid;
        if (i < n) {
          if (j > 0) S[polm_tri(i) + j - 1] = cbp[i];
          if (i > j) cb[i] = S[polm_tri(i) + j] / d;
        }
      }
      __syncthreads();
      for (int i = j + 1 + wv; i < n; i += 4) {
        const double sij = S[polm_tri(i) + j];
        double *row = S + polm_tri(i);
        for (int c = j + 1 + lane; c <= i; c += 64) row[c] = fma(-sij, cb[c], row[c]);
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
      if (it > 0) p_times(xh);
      if (tid < M) {
        const signed char c = cur[tid];
        double r = 0.0;
        if (c != 0) r = (c < 0 ? lo[tid] : up[tid]) - (it > 0 ? a_row(tid, xh) : 0.0);
        r2[tid] = r;
      }
      __syncthreads();
      if (tid < n) {
        double aty = 0.0, atr = 0.0;
        for (int s = 0; s < na; s++) {
          const int r = act[s];
          const double av = Ad[r * lda + tid];
          aty = fma(av, yh[r], aty);
          atr = fma(av, inv_delta * r2[r], atr);
        }
        const double r1 = (-q[tid] - (it > 0 ? px[tid] : 0.0)) - aty;
        t[tid] = r1 + atr;
      }
      __syncthreads();
      if (wv == 0) {
        // L D L^T dx = t by the first wavefront, entry i = lane + 64 s in register s: a column at a time, forward
        // through L (column j below the diagonal), the pivots, back through L^T (row j left of the diagonal)
        double reg[3];
#pragma unroll
        for (int s = 0; s < 3; s++) reg[s] = lane + 64 * s < n ? t[lane + 64 * s] : 0.0;
#pragma unroll
        for (int sg = 0; sg < 3; sg++) {
          for (int jj = 0; jj < 64; jj++) {
            const int j = sg * 64 + jj;
            if (j >= n) break;
            const double vj = __shfl(reg[sg], jj, 64);
#pragma unroll
            for (int s = sg; s < 3; s++) {
              const int i = lane + 64 * s;
              if (i > j && i < n) reg[s] = fma(-S[polm_tri(i) + j], vj, reg[s]);
            }
          }
        }
#pragma unroll
        for (int s = 0; s < 3; s++) {
          const int i = lane + 64 * s;
          if (i < n) reg[s] /= S[polm_tri(i) + i];
        }
#pragma unroll
        for (int sg = 2; sg >= 0; sg--) {
          for (int jj = 63; jj >= 0; jj--) {
            const int j = sg * 64 + jj;
            if (j >= n) continue;
            const double xj = __shfl(reg[sg], jj, 64);
            const double *row = S + polm_tri(j);
#pragma unroll
            for (int s = 0; s <= sg; s++) {
              const int i = lane + 64 * s;
              if (i < j) reg[s] = fma(-row[i], xj, reg[s]);
            }
          }
        }
#pragma unroll
        for (int s = 0; s < 3; s++) {
          const int i = lane + 64 * s;
          if (i < n) {
            v[i] = reg[s];
            xh[i] += reg[s];
          }
        }
      }
      __syncthreads();
      if (tid < M && cur[tid] != 0) yh[tid] += inv_delta * (a_row(tid, v) - r2[tid]);
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
    bool add = false, drop = false;
    if (tid < M) {
      const double z = a_row(tid, xh), l = lo[tid], u = up[tid], y = yh[tid];
      const signed char c = cur[tid];
      signed char cn = c;
      if (l != u) {
        if (c < 0) cn = y > POLM_TOL ? 0 : c;
        else if (c > 0) cn = y < -POLM_TOL ? 0 : c;
        else if (l > -POLM_INFTY && l - z > POLM_TOL) cn = -1;
        else if (u < POLM_INFTY && z - u > POLM_TOL) cn = 1;
      }
      nxt[tid] = cn;
      add = cn != c && c == 0;
      drop = cn != c && c != 0;
    }
    const int c4 = polm_block_count(add, red, tid), c5 = polm_block_count(drop, red, tid);
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

  // ---- 5. the point the loop ended with, the decision, the record
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
  const int n_lower = polm_block_count(tid < M && fin[tid] < 0, red, tid);
  const int n_upper = polm_block_count(tid < M && fin[tid] > 0, red, tid);
  double *out = a.out + inst * polm_out_stride(n, M);
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
    if constexpr (POLM_TABLE) {
      if (take) yo[r] = Y[r];
      else if (yg) yo[r] = yg[r];  // (a guessed y is there already, written by this thread in stage 2)
    } else {
      yo[r] = take ? Y[r] : yg[r];
    }
    co[r] = fin[r];
  }
