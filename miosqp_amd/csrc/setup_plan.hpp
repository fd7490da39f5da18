// Set-up of many small models in one launch (miosqp_qp_setup_models): the host logic that needs neither an engine nor the
// device -- the argument checks that refuse a call before anything is queued, which model the launch takes, and where
// every array of every model lies in the call's device arena and its pinned slab.
// Plain C++ (no HIP): engine.hip includes it, and so does the stand-alone sanitized program under tests/.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "setup_models_body.hpp"  // eligible_shape, lds_doubles, Record (plain C++ too)
#include "setup_models_large_body.hpp"  // eligible_shape_large, lds_doubles_large: the launch for models beyond n + M = 192
#include "prepare_models_body.hpp"  // lds_doubles of k_prepare_models, Scalars

namespace miosqp {
namespace setup_models {

constexpr int ERR_ARG = -1;          // MIOSQP_EARG
constexpr int ERR_UNSUPPORTED = -5;  // MIOSQP_EUNSUPPORTED
constexpr size_t ALIGN = 256;        // every array starts on a multiple of this (what the engine's pool hands out)
constexpr size_t SLACK = 64;         // elements behind an array that tile loads may touch (dupload keeps the same)
constexpr size_t CTRL_BYTES = 128;   // room of one control block (engine.hip: Ctrl is 120 bytes)

// one model as the entry point receives it (pointers are only tested against NULL here, l and u are read)
struct Args {
  int n = 0, M = 0;
  const void *Pp = nullptr, *Pi = nullptr, *Px = nullptr, *Ap = nullptr, *Ai = nullptr, *Ax = nullptr, *q = nullptr;
  const double *l = nullptr, *u = nullptr;
  const void *settings = nullptr;
  double rho = 0, sigma = 0, alpha = 0;
  int max_iter = 0, rho_auto = 0, coop = -1, resident = -1, fold = -1, setup_on_device = -1, pers = -1;
  int n_int = -1, m_orig = 0;  // n_int < 0: no integer rows in the descriptor
  const void *i_idx = nullptr;
  const double *l_root = nullptr, *u_root = nullptr;
};

// settings under which miosqp_qp_setup would choose resident + fold + W at a fixed rho for an eligible shape;
// rho_auto_in_launch (miosqp_qp_setup_models_auto): rho_auto = 1 is taken too, the launch chooses rho itself
inline bool eligible_settings(const Args &a, bool rho_auto_in_launch = false) {
  return (a.rho_auto == 0 || (rho_auto_in_launch && a.rho_auto == 1)) && a.coop != 1 && a.resident != 0 && a.fold != 0 &&
         a.setup_on_device != 1;
}
// the size rule of the launch that chooses rho: the probing iterations' vectors fit the LDS as well.  The same set of
// shapes as eligible_shape (the stand-alone program under tests/ walks the whole grid).
inline bool eligible_shape_auto(int n, int M) {
  return eligible_shape(n, M) && lds_doubles_auto(n, M) * sizeof(double) <= LDS_LIMIT;
}

// A model beyond n + M = 192 (miosqp_qp_setup_models_large) comes out as the engine miosqp_qp_setup builds with coop = 0,
// resident = 0, fold = 1, pers = 0: settings that ask for another form keep it out.  rho is fixed: choosing it for such
// a model inside the launch is the opt-in of miosqp_qp_setup_models_large_auto (large_rho_auto: rho_auto = 1 is taken
// too; its size rule is eligible_shape_large_auto).
inline bool eligible_settings_large(const Args &a, bool large_rho_auto = false) {
  return (a.rho_auto == 0 || (large_rho_auto && a.rho_auto == 1)) && a.setup_on_device != 1 && a.fold != 0 && a.coop != 1 &&
         a.resident != 1 && a.pers <= 0;
}

// The launch writes the dense copies of Abar and Pbar entry by entry where the per-model set-up sums what a matrix stores
// twice: a column whose row indices do not ascend strictly (an entry twice, or unsorted) keeps its model out of the launch.
inline bool csc_strictly_ascending(int cols, const int32_t *ptr, const int32_t *idx) {
  for (int j = 0; j < cols; j++)
    for (int32_t p = ptr[j] + 1; p < ptr[j + 1]; p++)
      if (idx[p] <= idx[p - 1]) return false;
  return true;
}

// 0, or the error code with `err` naming the model's position.  large (miosqp_qp_setup_models_large): a model that the
// small launch does not take for its SIZE is judged by the rules of the large one.  large_rho_auto
// (miosqp_qp_setup_models_large_auto): such a model with rho_auto = 1 is taken where the probing iterations' vectors fit.
inline int check_args(int32_t B, const Args *a, const void *out, const void *stats, std::string &err,
                      bool rho_auto_in_launch = false, bool large = false, bool large_rho_auto = false) {
  const std::string who = "setup_models: ";
  if (B < 1) {
    err = who + "B must be at least 1";
    return ERR_ARG;
  }
  if (!a || !out || !stats) {
    err = who + "a NULL argument";
    return ERR_ARG;
  }
  for (int b = 0; b < B; b++) {
    const Args &m = a[b];
    const std::string at = " (model " + std::to_string(b) + ")";
    if (m.n <= 0 || m.M <= 0) {
      err = who + "n and M must be at least 1" + at;
      return ERR_ARG;
    }
    if (!m.Pp || !m.Ap || !m.q || !m.l || !m.u || !m.settings) {
      err = who + "a NULL pointer" + at;
      return ERR_ARG;
    }
    if (!(m.rho > 0) || !(m.sigma > 0) || !(m.alpha > 0 && m.alpha < 2) || m.max_iter <= 0) {
      err = who + "settings out of range" + at;
      return ERR_ARG;
    }
    if (m.n_int >= 0 && (m.n_int > m.n || m.m_orig < 0 || m.m_orig + m.n_int != m.M || (m.n_int > 0 && !m.i_idx))) {
      err = who + "integer rows: need m_orig + n_int == M" + at;
      return ERR_ARG;
    }
    if ((m.l_root || m.u_root) && (!m.l_root || !m.u_root || m.n_int < 0)) {
      err = who + "a root needs both bounds and the integer rows" + at;
      return ERR_ARG;
    }
    for (int i = 0; i < m.M; i++)
      if (m.l[i] > m.u[i]) {
        err = who + "lower bound above upper bound" + at;
        return ERR_ARG;
      }
    if (large && !eligible_shape(m.n, m.M)) {
      if (!eligible_shape_large(m.n, m.M)) {
        err = who + "neither launch takes this model: the packed triangle of n variables within " +
              std::to_string(LDS_LIMIT / 1024) + " KB of LDS (n <= 198) and n + M <= " + std::to_string(MAX_NM_LARGE) + at;
        return ERR_UNSUPPORTED;
      }
      if (m.rho_auto != 0 && !large_rho_auto) {
        err = who + "rho_auto = 1 beyond n + M = " + std::to_string(MAX_NM) + ": the large launch builds a fixed rho only" + at;
        return ERR_UNSUPPORTED;
      }
      if (m.rho_auto != 0 && !eligible_shape_large_auto(m.n, m.M)) {
        err = who + "rho_auto = 1 beyond the large launch that chooses rho: the packed triangle of n variables and the "
                    "probing iterations' n + 3 M + 8 doubles within " + std::to_string(LDS_LIMIT / 1024) + " KB of LDS (n <= 197)" + at;
        return ERR_UNSUPPORTED;
      }
      if (!eligible_settings_large(m, large_rho_auto)) {
        err = who + "the large launch does not take this model: it builds the engine of coop = 0, resident = 0, fold = 1, "
                    "pers = 0 on the host's set-up path (setup_on_device != 1)" + at;
        return ERR_UNSUPPORTED;
      }
      continue;
    }
    if (!eligible_shape(m.n, m.M) || !eligible_settings(m, rho_auto_in_launch) ||
        (rho_auto_in_launch && m.rho_auto && !eligible_shape_auto(m.n, m.M))) {
      err = who + "the launch does not take this model: n + M <= " + std::to_string(MAX_NM) +
            (rho_auto_in_launch ? ", rho fixed or rho_auto = 1" : ", a fixed rho") +
            ", and settings that lead to the LDS-resident form with the explicit inverse" + at;
      return ERR_UNSUPPORTED;
    }
  }
  return 0;
}

constexpr int FORM_SMALL = 0;  // k_setup_models / k_setup_models_auto
constexpr int FORM_LARGE = 1;  // k_setup_models_large / k_setup_models_large_auto

struct Shape {
  int n = 0, M = 0;
  size_t nv = 0, nc = 0, npb = 0, npr = 0;  // lengths of the packed rows as stored (padding included): by variable, by
                                            // constraint, Pbar, Praw
  int rho_auto = 0;                         // 1: the launch chooses this model's rho (LDS for the probing iterations)
  int form = FORM_SMALL;                    // which launch builds it (FORM_LARGE: no W, no Kc, the large LDS rule)
  int prepare = 0;                          // 1: k_prepare_models builds the packed rows and the scalings from the raw problem
  size_t nnzP = 0, nnzA = 0;                // prepare: entries of P as given and of A (the raw CSC goes up instead of the rows)
};

// the arrays of one model, in the order they lie in the arena
enum Part {
  // uploaded
  PV_PTR, PV_IDX, PV_L, PV_AT, PC_PTR, PC_IDX, PC_L, PC_A, PB_PTR, PB_IDX, PB_VAL, PR_PTR, PR_IDX, PR_VAL, D_, DINV, E_, EINV,
  Q, QRAW, RAW,  // RAW: raw_l | raw_u | raw_x | raw_y
  // products of the launch
  LINV, LINVT, D2INV, F_ROWS, F_GMT, F_AD, F_ATD, F_PD, W_, KC,
  // iterates and staging
  L_, U_, X_, Z_, Y_, WH, CV, UT, XT, DX, DY, SM, SN, XI, XIS, ROOT_L, ROOT_U, CTRL, OUT, I_IDX,
  // left to the engine's pool: int_pos, f_rows2 and a_int of miosqp_qp_set_integer_rows, the guard's scratch, slack
  RESERVE,
  NPARTS
};
constexpr int FIRST_PRODUCT = LINV, FIRST_ITERATE = L_;
// the raw problem of a model that k_prepare_models prepares: uploaded in place of the packed rows
enum RawPart { RAW_PP, RAW_PI, RAW_PX, RAW_AP, RAW_AI, RAW_AX, NRAW };
// of the parts before FIRST_PRODUCT a prepared model still uploads these; the others the device writes
inline bool prepared_uploads(int k) { return k == PV_PTR || k == PC_PTR || k == PB_PTR || k == PR_PTR || k == QRAW || k == RAW; }

struct Span {
  size_t off = 0, bytes = 0;  // from the arena's base
};

struct Slot {
  Span part[NPARTS];
  size_t rec = 0;  // this model's Record
  size_t entry = 0;  // its place in the table: small models first, then the large ones, each in the caller's order
  // the pinned slab: h_in (in_cap doubles), h_out (out_cap doubles), h_ctrl, h_ctrl2 (two control blocks)
  size_t pin_in = 0, pin_out = 0, pin_ctrl = 0, pin_ctrl2 = 0, in_cap = 0, out_cap = 0;
  Span raw[NRAW];  // a prepared model: its raw CSC in the upload; no bytes otherwise
  Span scal;       // ... and the scalars of its equilibration (c, cinv) among the device-written parts
};

// [ table | uploaded arrays of every model | products, iterates, reserve of every model | records ]: the first two parts
// go up in ONE copy out of the pinned slab (which holds their image at the same offsets), the records come back in ONE.
struct Plan {
  std::vector<Slot> slot;
  size_t table_bytes = 0;
  size_t up_bytes = 0;             // [0, up_bytes) is staged and uploaded
  size_t rec_off = 0, rec_bytes = 0;
  size_t total_bytes = 0;          // the arena
  size_t pin_bytes = 0;            // the slab: max(upload image, the engines' staging) + records
  size_t pin_rec = 0;              // where the records land in the slab
  size_t lds_bytes = 0;            // dynamic LDS of the launch: the largest model's
  size_t n_small = 0, n_large = 0; // table entries [0, n_small) go to the small launch, [n_small, n_small + n_large) to the large one
  size_t lds_bytes_large = 0;      // dynamic LDS of the large launch
  // With prepared models the arena is [ table | table of k_prepare_models | uploaded | device-written rows and scalings
  // of the prepared models | records | products, iterates, reserve ]: the fourth and fifth part come back in ONE copy
  // (the host's mirrors are filled from it) and land in the slab at pin_prep, the records behind them at pin_rec.
  size_t n_prepare = 0;
  size_t ptab_off = 0, ptab_bytes = 0;
  size_t prep_off = 0, prep_bytes = 0;
  size_t pin_prep = 0;
  size_t lds_bytes_prepare = 0;    // dynamic LDS of k_prepare_models
};

inline size_t round_up(size_t v, size_t to) { return (v + to - 1) / to * to; }
inline size_t arr(size_t count, size_t elem) { return round_up((count + SLACK) * elem, ALIGN); }

// bytes of every part of one model
inline void part_bytes(const Shape &s, size_t (&by)[NPARTS]) {
  const size_t n = (size_t)s.n, M = (size_t)s.M, N = n + M;
  const size_t ld = (n + 15) & ~(size_t)15, ldf = (N + 15) & ~(size_t)15, ldn = ld, ldm = (M + 15) & ~(size_t)15,
               ldw = (N + 7) & ~(size_t)7;
  const size_t I = sizeof(int32_t), F = sizeof(double);
  by[PV_PTR] = arr(n + 1, I); by[PV_IDX] = arr(s.nv, I); by[PV_L] = arr(s.nv, F); by[PV_AT] = arr(s.nv, F);
  by[PC_PTR] = arr(M + 1, I); by[PC_IDX] = arr(s.nc, I); by[PC_L] = arr(s.nc, F); by[PC_A] = arr(s.nc, F);
  by[PB_PTR] = arr(n + 1, I); by[PB_IDX] = arr(s.npb, I); by[PB_VAL] = arr(s.npb, F);
  by[PR_PTR] = arr(n + 1, I); by[PR_IDX] = arr(s.npr, I); by[PR_VAL] = arr(s.npr, F);
  by[D_] = arr(n, F); by[DINV] = arr(n, F); by[E_] = arr(M, F); by[EINV] = arr(M, F);
  by[Q] = arr(n, F); by[QRAW] = arr(n, F); by[RAW] = arr(3 * M + n, F);
  by[LINV] = arr(n * ld, F); by[LINVT] = arr(n * ld, F); by[D2INV] = arr(n, F);
  by[F_ROWS] = arr(n * ldf, F); by[F_GMT] = arr(M * ldn, F); by[F_AD] = arr(M * ldn, F); by[F_ATD] = arr(n * ldm, F);
  by[F_PD] = arr(n * ldn, F);
  const bool w = s.form != FORM_LARGE;  // (the large form builds neither: 2 x 1.7 MB at n + M = 470)
  by[W_] = w ? arr(N * ldw, F) : 0; by[KC] = w ? arr(N * ldw, F) : 0;
  by[L_] = arr(M, F); by[U_] = arr(M, F); by[X_] = arr(n, F); by[Z_] = arr(M, F); by[Y_] = arr(M, F); by[WH] = arr(N, F);
  by[CV] = arr(n, F); by[UT] = arr(n, F); by[XT] = arr(n, F); by[DX] = arr(n, F); by[DY] = arr(M, F);
  by[SM] = arr(8 * M, F); by[SN] = arr(10 * n, F); by[XI] = arr(n, F); by[XIS] = arr(n, F);
  by[ROOT_L] = arr(M, F); by[ROOT_U] = arr(M, F); by[CTRL] = round_up(CTRL_BYTES, ALIGN); by[OUT] = arr(N, F);
  by[I_IDX] = arr(n, I);
  by[RESERVE] = arr(n, I) + arr(n * ldf, F) + arr(n, F) + arr(3 * N + 8, F) + arr(8, F) + 4096;
}

inline Plan plan(const std::vector<Shape> &sh, size_t entry_bytes, size_t prepare_entry_bytes = 0) {
  Plan P;
  const size_t B = sh.size();
  P.slot.resize(B);
  P.table_bytes = round_up(B * entry_bytes, ALIGN);
  size_t at = P.table_bytes;
  for (size_t b = 0; b < B; b++) P.n_prepare += sh[b].prepare ? 1 : 0;
  if (P.n_prepare) {  // (one entry per model of the call, by position: the launch reads those of the prepared ones)
    P.ptab_off = at;
    P.ptab_bytes = round_up(B * prepare_entry_bytes, ALIGN);
    at += P.ptab_bytes;
  }
  std::vector<size_t> by((size_t)NPARTS * B);
  for (size_t b = 0; b < B; b++) {
    size_t one[NPARTS];
    part_bytes(sh[b], one);
    for (int k = 0; k < NPARTS; k++) by[b * NPARTS + k] = one[k];
    for (int k = 0; k < FIRST_PRODUCT; k++) {
      if (sh[b].prepare && !prepared_uploads(k)) continue;
      P.slot[b].part[k] = Span{at, one[k]};
      at += one[k];
    }
    if (sh[b].prepare) {
      const size_t n1 = (size_t)sh[b].n + 1, I = sizeof(int32_t), F = sizeof(double);
      const size_t raw[NRAW] = {arr(n1, I), arr(sh[b].nnzP, I), arr(sh[b].nnzP, F), arr(n1, I), arr(sh[b].nnzA, I), arr(sh[b].nnzA, F)};
      for (int k = 0; k < NRAW; k++) {
        P.slot[b].raw[k] = Span{at, raw[k]};
        at += raw[k];
      }
      const size_t lds = prepare_models::lds_doubles(sh[b].n, sh[b].M) * sizeof(double);
      if (lds > P.lds_bytes_prepare) P.lds_bytes_prepare = lds;
    }
    if (sh[b].form == FORM_LARGE) {
      const size_t lds = (sh[b].rho_auto ? lds_doubles_large_auto(sh[b].n, sh[b].M) : lds_doubles_large(sh[b].n, sh[b].M)) * sizeof(double);
      if (lds > P.lds_bytes_large) P.lds_bytes_large = lds;
      P.n_large++;
    } else {
      const size_t lds = (sh[b].rho_auto ? lds_doubles_auto(sh[b].n, sh[b].M) : lds_doubles(sh[b].n, sh[b].M)) * sizeof(double);
      if (lds > P.lds_bytes) P.lds_bytes = lds;
      P.n_small++;
    }
  }
  for (size_t b = 0, s = 0, l = P.n_small; b < B; b++) P.slot[b].entry = sh[b].form == FORM_LARGE ? l++ : s++;
  P.up_bytes = at;
  if (P.n_prepare) {
    P.prep_off = at;
    for (size_t b = 0; b < B; b++) {
      if (!sh[b].prepare) continue;
      for (int k = 0; k < FIRST_PRODUCT; k++) {
        if (prepared_uploads(k)) continue;
        P.slot[b].part[k] = Span{at, by[b * NPARTS + k]};
        at += by[b * NPARTS + k];
      }
      P.slot[b].scal = Span{at, ALIGN};
      at += ALIGN;
    }
    P.prep_bytes = at - P.prep_off;
    P.rec_off = at;
    P.rec_bytes = round_up(B * sizeof(Record), ALIGN);
    at += P.rec_bytes;
  }
  for (size_t b = 0; b < B; b++)
    for (int k = FIRST_PRODUCT; k < NPARTS; k++) {
      P.slot[b].part[k] = Span{at, by[b * NPARTS + k]};
      at += by[b * NPARTS + k];
    }
  if (!P.n_prepare) {
    P.rec_off = at;
    P.rec_bytes = round_up(B * sizeof(Record), ALIGN);
    at += P.rec_bytes;
  }
  for (size_t b = 0; b < B; b++) P.slot[b].rec = P.rec_off + b * sizeof(Record);
  P.total_bytes = at;
  // the slab: while the call runs it holds the upload's image; afterwards the same bytes are the engines' staging
  size_t pin = 0;
  for (size_t b = 0; b < B; b++) {
    const size_t n = (size_t)sh[b].n, M = (size_t)sh[b].M;
    Slot &s = P.slot[b];
    s.in_cap = round_up(3 * M + 2 * n + 8, 8);  // bounds | x, y or q (miosqp_qp_set_integer_rows stages n_int + n ints and n doubles)
    s.out_cap = round_up(n + M + 1, 8);
    s.pin_in = pin;
    pin += round_up(s.in_cap * sizeof(double), ALIGN);
    s.pin_out = pin;
    pin += round_up(s.out_cap * sizeof(double), ALIGN);
    s.pin_ctrl = pin;
    pin += round_up(CTRL_BYTES, ALIGN);
    s.pin_ctrl2 = pin;
    pin += round_up(2 * CTRL_BYTES, ALIGN);
  }
  P.pin_rec = round_up(pin > P.up_bytes ? pin : P.up_bytes, ALIGN);
  if (P.n_prepare) {  // (the download is one copy: rows and scalings, then the records)
    P.pin_prep = P.pin_rec;
    P.pin_rec = P.pin_prep + P.prep_bytes;
  }
  P.pin_bytes = P.pin_rec + P.rec_bytes;
  return P;
}

}  // namespace setup_models
}  // namespace miosqp
