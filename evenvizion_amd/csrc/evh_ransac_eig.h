// evh_ransac_eig.h -- internal to evh_ransac.hip (layer 2 of 4): the three Jacobi eigen-solvers and the 8x8 LDL^T
#pragma once
#include "evh_ransac_wave.h"
#include <stddef.h>
#include <type_traits>
namespace {
#define MS 9           // row stride (doubles) of the matrices held in LDS, for N = 8 and N = 9

struct RowMat {          // one eigen-problem: A full symmetric, V eigenvectors as rows, W eigenvalues, sort order
  double A[MS * MS];
  double V[MS * MS];     // directly behind A: jacobi_one addresses both through one element index
  double W[MS];
  int ord[12];           // ord[p] = index of the p-th largest eigenvalue (selection-sort order of the reference)
};
static_assert(offsetof(RowMat, V) == sizeof(double) * MS * MS, "V must follow A");

// Order of the eigenvalues (descending) into M.ord, rows of a wave in parallel; `active` is row-uniform.  Distinct
// values: position = number of larger ones.  Equal values (degenerate input): replay the reference's selection sort
// on the index list.
template <int N>
__device__ __forceinline__ void eig_order(RowMat& M, int lane, bool active) {
  const int gl = lane & 15;
  double* Wd = M.W;
  int gt = 0, eq = 0;
  if (active && gl < N) {
    const double w = Wd[gl];
#pragma unroll
    for (int i = 0; i < N; i++) { const double wi = Wd[i]; gt += wi > w ? 1 : 0; eq += wi == w ? 1 : 0; }
  }
  const unsigned long long tie = __ballot(active && gl < N && eq != 1);   // != 1 also catches NaN
  const bool row_tie = ((tie >> (lane & 48)) & 0xFFFFull) != 0ull;
  if (active && gl < N && !row_tie) M.ord[gt] = gl;
  if (active && row_tie && gl == 0) {
    for (int i = 0; i < N; i++) M.ord[i] = i;
    for (int a = 0; a < N - 1; a++) {
      int mm = a;
      for (int i = a + 1; i < N; i++) if (Wd[M.ord[mm]] < Wd[M.ord[i]]) mm = i;
      const int tmp = M.ord[a]; M.ord[a] = M.ord[mm]; M.ord[mm] = tmp;
    }
  }
  WSYNC();
}

// Symmetric eigen-solver (Jacobi with largest-pivot selection; eigenvalues sorted descending through M.ord), one
// matrix per 16-lane row, up to four rows of a wavefront at once.  Arithmetic and pivot order are those of the
// serial algorithm (first maximum in the scan order R0..R(N-2), C1..C(N-1); indR / indC rescanned only for the two
// rotated indices).  Lane roles inside a row (half = lanes 0-7 / 8-15, m = lane & 7):
//   half 0: rotation index m,     owner of the column candidate C(m+1) = A[indC[m+1]][m+1], column rescans (i < K)
//   half 1: rotation index m + 1, owner of the row candidate R(m) = A[m][indR[m]],         row rescans (j > K)
// A is held as a full symmetric matrix (both mirrors written), so A[own][cidx] addresses either kind of candidate.
// The diagonal of A is dead after W is taken from it (lanes k and l park their unused products there).
// Must be called by all 64 lanes; `active` is row-uniform.
template <int N>
__device__ __forceinline__ int jacobi_rows(RowMat& M, int lane, bool active) {
  const int gl = lane & 15, half = gl >> 3, m = gl & 7;
  const int idx = half ? m + 1 : m;
  const bool idx_ok = idx < N;
  const int idx_c = idx_ok ? idx : 0;
  const int own = half ? m : m + 1;
  const bool own_ok = m <= N - 2;
  const int own_c = own_ok ? own : 1;
  const unsigned prio = half ? m : 8 + m;
  const int vc = gl < N ? gl : 0;
  const int sgn = half ? 1 : -1, sidx = idx_ok ? sgn * idx : -64;
  double* A = M.A;
  double* V = M.V;
  double* Wd = M.W;
  unsigned amax = 0;                            // largest high word of |a_ij|: decides once whether the short divide /
  if (active) {                                 // square-root sequences are safe for the whole solve (see below)
    for (int e = gl; e < N * N; e += GL) {
      const int i = e / N, j = e - i * N;
      V[i * MS + j] = i == j ? 1.0 : 0.0;
      amax = max(amax, hi32(A[i * MS + j]) & 0x7FFFFFFFu);
    }
    if (gl < N) Wd[gl] = A[gl * MS + gl];
  }
  // Rotations preserve the Frobenius norm, so with every |a_ij| < 2^300 all later entries, eigenvalue estimates and
  // the hypotenuses built from them stay below 2^310: no operand of the unscaled sequences can leave their range.
  // Anything larger (or NaN) sends the whole wave through the plain `/` and sqrt() forms.
  const bool plain = __ballot(active && rmax16(amax) >= 0x52B00000u) != 0ull;
  // initial indR[own] / indC[own]: first maximum of the row right of / the column above the diagonal
  int cidx = half ? own_c + 1 : 0;
  double cval = 0;
  if (active && own_ok) {
    double mv = -1.0;
#pragma unroll
    for (int j = 0; j < N; j++) {
      const bool in = half ? j > own : j < own;
      const double v = fabs(A[own * MS + j]);
      if (in && mv < v) mv = v, cidx = j;
    }
    cval = A[own * MS + cidx];
  }
  WSYNC();
  bool act = active;
  const int maxIters = N * N * 30;
  int iters = 0;
  auto sweep = [&](auto plain_tag) {
  constexpr bool PLAIN = decltype(plain_tag)::value;
  for (; iters < maxIters; iters++) {
    if (__ballot(act) == 0ull) break;
    // ---- pivot: first maximum of |candidate| over the row's 2N-2 owners, in the order R0.., C1..
    const bool cv = act && own_ok;
    const unsigned ch = cv ? hi32(cval) & 0x7FFFFFFFu : 0u, cl = cv ? lo32(cval) : 0u;
    const unsigned mh = rmax16(ch);
    const unsigned ml = rmax16(ch == mh ? cl : 0u);
    const bool win = cv && ch == mh && cl == ml;
    const unsigned pack = (prio << 12) | ((hi32(cval) >> 31) << 8) | ((half ? own : cidx) << 4) | (half ? cidx : own);
    const unsigned pk = rmin16(win ? pack : 0xFFFFFFFFu);
    const double pabs = mk64(mh, ml);
    if (pabs <= DBL_EPSILON) act = false;
    const int k = act ? (pk >> 4) & 15 : 0, l = act ? pk & 15 : 1;
    const double p = (pk >> 8) & 1 ? -pabs : pabs;
    // ---- operands of this rotation (independent of c, s: issued before the scalar chain)
    const double wk = Wd[k], wl = Wd[l];
    const double a0 = A[idx_c * MS + k], b0 = A[idx_c * MS + l];
    const double va = V[k * MS + vc], vb = V[l * MS + vc];
    double c = 1, s = 0, t = 0;
    if (PLAIN) { const Cst r = rotation_scalars_plain(p, wk, wl); c = r.c; s = r.s; t = r.t; }
    else rotation_scalars(p, wk, wl, c, s, t);
    double u = a0 * c - b0 * s, v = a0 * s + b0 * c;
    if (idx == l) u = 0;                        // A[k][l] = 0
    if (idx == k) v = 0;
    const double nva = va * c - vb * s, nvb = va * s + vb * c;
    if (act) {
      if (idx_ok) { A[idx * MS + k] = u; A[k * MS + idx] = u; A[idx * MS + l] = v; A[l * MS + idx] = v; }
      if (gl < N) { V[k * MS + gl] = nva; V[l * MS + gl] = nvb; }
      if (gl == 0) { Wd[k] = wk - t; Wd[l] = wl + t; }
    }
    WSYNC();
    // ---- candidates: every owner re-reads its element (its index may be stale, its value never is) ...
    const double fresh = A[own_c * MS + cidx];
    // ---- ... and the owners of k and l rescan: half 0 the column above, half 1 the row right of the diagonal,
    //      straight from the rotated values in registers (u = new A[idx][k], v = new A[idx][l])
    const bool inu = sidx - sgn * k > 0;        // half 1: idx > k, half 0: idx < k (never for a lane without index)
    const bool inv = sidx - sgn * l > 0;
    const unsigned uh = inu ? hi32(u) & 0x7FFFFFFFu : 0u, ul = inu ? lo32(u) : 0u;
    const unsigned vh = inv ? hi32(v) & 0x7FFFFFFFu : 0u, vl = inv ? lo32(v) : 0u;
    const unsigned muh = rmax8(uh), mvh = rmax8(vh);
    const unsigned mul_ = rmax8(uh == muh ? ul : 0u), mvl = rmax8(vh == mvh ? vl : 0u);
    const unsigned pu = rmin8(inu && uh == muh && ul == mul_ ? (unsigned)(idx << 1) | (hi32(u) >> 31) : 0xFFFFFFFFu);
    const unsigned pv = rmin8(inv && vh == mvh && vl == mvl ? (unsigned)(idx << 1) | (hi32(v) >> 31) : 0xFFFFFFFFu);
    {
      const bool tk = act && own == k, tl = act && own == l;
      cidx = (int)vsel(tk, (pu >> 1) & 15, vsel(tl, (pv >> 1) & 15, (unsigned)cidx));
      const unsigned nh = vsel(tk, muh | (pu << 31), vsel(tl, mvh | (pv << 31), hi32(fresh)));
      const unsigned nl = vsel(tk, mul_, vsel(tl, mvl, lo32(fresh)));
      cval = mk64(nh, nl);
    }
  }
  };
  if (plain) sweep(std::true_type{}); else sweep(std::false_type{});
  WSYNC();
  eig_order<N>(M, lane, active);
  return iters;
}

// The same solver for ONE matrix served by the whole wavefront (refit, LM solves): the pivot (k, l, p) and the
// eigenvalues it needs travel through SGPRs (v_readfirstlane / v_readlane), the rotations of A and V are one
// instruction stream (rows 0-1 of the wave rotate A pairs, row 2 the V pairs), the rescans for k and for l run side
// by side (row 0 / row 1) and row 1's results reach the candidate owners in row 0 by v_permlane16_swap.  W lives in
// registers (lane j holds W[j]) and is stored to M.W at the end.  Same arithmetic, same pivot order, same result.
template <int N>
__device__ __forceinline__ int jacobi_one(RowMat& M, int lane) {
  const int row = lane >> 4, gl = lane & 15, half = gl >> 3, m = gl & 7;
  const int idx = half ? m + 1 : m;
  const bool a_lane = row < 2 && idx < N;
  const bool a_writer = row == 0 && idx < N;
  const bool v_lane = row == 2 && gl < N;
  const int own = half ? m : m + 1;
  const bool own_ok = row == 0 && m <= N - 2;
  const int own_c = m <= N - 2 ? own : 1;
  const unsigned prio = half ? m : 8 + m;
  const int sgn = half ? 1 : -1, sidx = a_lane ? sgn * idx : -64;
  const int zidx = a_lane ? idx : 99;
  // element index of this lane's pair inside M.A (V behind it): e0 = ebase + k * emult, e1 = ebase + l * emult
  const int ebase = a_lane ? idx * MS : v_lane ? MS * MS + gl : 0;
  const int emult = a_lane ? 1 : v_lane ? MS : 0;
  double* D = M.A;
  unsigned amax = 0;
  for (int e = lane; e < N * N; e += NL) {
    const int i = e / N, j = e - i * N;
    M.V[i * MS + j] = i == j ? 1.0 : 0.0;
    amax = max(amax, hi32(D[i * MS + j]) & 0x7FFFFFFFu);
  }
  const bool plain = __ballot(amax >= 0x52B00000u) != 0ull;     // see jacobi_rows
  double wreg = lane < N ? D[lane * MS + lane] : 0.0;
  int cidx = half ? own_c + 1 : 0;
  double cval = 0;
  if (own_ok) {
    double mv = -1.0;
#pragma unroll
    for (int j = 0; j < N; j++) {
      const bool in = half ? j > own : j < own;
      const double v = fabs(D[own * MS + j]);
      if (in && mv < v) mv = v, cidx = j;
    }
    cval = D[own * MS + cidx];
  }
  WSYNC();
  const int maxIters = N * N * 30;
  int iters = 0;
  auto sweep = [&](auto plain_tag) {
  constexpr bool PLAIN = decltype(plain_tag)::value;
  for (; iters < maxIters; iters++) {
    // ---- pivot (row 0 holds the candidates; the other rows reduce zeros)
    const unsigned ch = own_ok ? hi32(cval) & 0x7FFFFFFFu : 0u, cl = own_ok ? lo32(cval) : 0u;
    const unsigned mh = rmax16(ch);
    const unsigned ml = rmax16(ch == mh ? cl : 0u);
    const bool win = own_ok && ch == mh && cl == ml;
    const unsigned pack = (prio << 12) | ((hi32(cval) >> 31) << 8) | ((half ? own : cidx) << 4) | (half ? cidx : own);
    const unsigned pk = rmin16(win ? pack : 0xFFFFFFFFu);
    const unsigned spk = (unsigned)__builtin_amdgcn_readfirstlane((int)pk);
    const double pabs = mk64((unsigned)__builtin_amdgcn_readfirstlane((int)mh), (unsigned)__builtin_amdgcn_readfirstlane((int)ml));
    if (pabs <= DBL_EPSILON) break;
    const int k = (spk >> 4) & 15, l = spk & 15;
    const double p = (spk >> 8) & 1 ? -pabs : pabs;
    const double wk = mk64((unsigned)__builtin_amdgcn_readlane((int)hi32(wreg), k), (unsigned)__builtin_amdgcn_readlane((int)lo32(wreg), k));
    const double wl = mk64((unsigned)__builtin_amdgcn_readlane((int)hi32(wreg), l), (unsigned)__builtin_amdgcn_readlane((int)lo32(wreg), l));
    const int e0 = ebase + k * emult, e1 = ebase + l * emult;
    const double a0 = D[e0], b0 = D[e1];
    double c = 1, s = 0, t = 0;
    if (PLAIN) { const Cst r = rotation_scalars_plain(p, wk, wl); c = r.c; s = r.s; t = r.t; }
    else rotation_scalars(p, wk, wl, c, s, t);
    double x0 = a0 * c - b0 * s, x1 = a0 * s + b0 * c;
    if (zidx == l) x0 = 0;                      // A[k][l] = 0
    if (zidx == k) x1 = 0;
    if (a_writer || v_lane) { D[e0] = x0; D[e1] = x1; }
    if (a_writer) { D[k * MS + idx] = x0; D[l * MS + idx] = x1; }
    {
      const double wm = wreg - t, wp = wreg + t;
      wreg = lane == k ? wm : lane == l ? wp : wreg;
    }
    WSYNC();
    const double fresh = D[own_c * MS + cidx];
    // ---- rescans: row 0 for k on the first components, row 1 for l on the second ones
    const double xs = row == 1 ? x1 : x0;
    const int Ks = row == 1 ? l : k;
    const bool inr = sidx - sgn * Ks > 0;
    const unsigned xh = inr ? hi32(xs) & 0x7FFFFFFFu : 0u, xl = inr ? lo32(xs) : 0u;
    const unsigned m8h = rmax8(xh);
    const unsigned m8l = rmax8(xh == m8h ? xl : 0u);
    const unsigned pw = rmin8(inr && xh == m8h && xl == m8l ? (unsigned)(idx << 1) | (hi32(xs) >> 31) : 0xFFFFFFFFu);
    const unsigned o_pw = __builtin_amdgcn_permlane16_swap(pw, pw, false, false)[1];     // row 0 <- row 1
    const unsigned o_h = __builtin_amdgcn_permlane16_swap(m8h, m8h, false, false)[1];
    const unsigned o_l = __builtin_amdgcn_permlane16_swap(m8l, m8l, false, false)[1];
    {
      const bool tk = own == k, tl = own == l;
      cidx = (int)vsel(tk, (pw >> 1) & 15, vsel(tl, (o_pw >> 1) & 15, (unsigned)cidx));
      const unsigned nh = vsel(tk, m8h | (pw << 31), vsel(tl, o_h | (o_pw << 31), hi32(fresh)));
      const unsigned nl = vsel(tk, m8l, vsel(tl, o_l, lo32(fresh)));
      cval = mk64(nh, nl);
    }
  }
  };
  if (plain) sweep(std::true_type{}); else sweep(std::false_type{});
  if (lane < N) M.W[lane] = wreg;
  WSYNC();
  eig_order<N>(M, lane, lane < GL);
  return iters;
}

// ---- one 9x9 eigen-problem PER LANE (fixed-iteration RANSAC: thousands of hypotheses, throughput matters, latency does
// not): the serial algorithm as it stands, 64 problems side by side.  A and W of every lane live in LDS as
// [element][lane] (512 bytes between elements: whatever element a lane picks, it stays on its own banks): 0..35 upper
// off-diagonal of A (row i starts at i(17-i)/2), 36..44 W.  V (81 elements per lane, written and read only by its own
// lane, never on the pivot's critical path) lives in a global scratch of the same [element][lane] shape -- it stays in
// L2 -- so that four waves fit a compute unit instead of two; its loads are issued before the rotation scalars.  indR / indC are
// one register per index.  The rescans of indR / indC for the two rotated indices run inside the
// rotation loop on the freshly rotated values (ascending index, strict '<': the first maximum, as the reference).
#define LM_ELEMS 45
#define LM_W 36
#define LV_ELEMS 81
__device__ __forceinline__ int lm_arow(int i) { return (i * (17 - i)) >> 1; }          // first element of row i (j = i+1)
__device__ __forceinline__ int lm_a(int i, int j) { return lm_arow(i) + j - i - 1; }     // i < j
// L = this lane's column: element e at L[e * 64].  A (upper) and W (diagonal) hold the input.  Returns the row of V
// that belongs to the smallest eigenvalue under the reference's selection sort.
__device__ __forceinline__ int jacobi_lanes9(double* L, double* Vg, bool active) {
  const int N = 9;
#define EL(e) L[(e) * NL]
#define VL(e) Vg[(e) * NL]
  if (active) {
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
      for (int j = 0; j < N; j++) VL(i * N + j) = i == j ? 1.0 : 0.0;
  }
  int indR[9], indC[9];                // one register each (static index in every loop below)
#pragma unroll
  for (int k = 0; k < N; k++) { indR[k] = k < N - 1 ? k + 1 : 0; indC[k] = 0; }
  if (active) {
#pragma unroll
    for (int k = 0; k < N; k++) {
      if (k < N - 1) {
        int m = k + 1; double mv = fabs(EL(lm_a(k, k + 1)));
#pragma unroll
        for (int i = k + 2; i < N; i++) { const double v = fabs(EL(lm_a(k, i))); if (mv < v) mv = v, m = i; }
        indR[k] = m;
      }
      if (k > 0) {
        int m = 0; double mv = fabs(EL(lm_a(0, k)));
#pragma unroll
        for (int i = 1; i < k; i++) { const double v = fabs(EL(lm_a(i, k))); if (mv < v) mv = v, m = i; }
        indC[k] = m;
      }
    }
  }
  // the short divide / square-root sequences need every |a_ij| < 2^300 (see jacobi_rows); one lane out of range sends
  // the wave through the plain forms
  unsigned amax = 0;
  if (active) {
#pragma unroll
    for (int e = 0; e < LM_ELEMS; e++) amax = max(amax, hi32(EL(e)) & 0x7FFFFFFFu);
  }
  const bool plain = __ballot(active && amax >= 0x52B00000u) != 0ull;
  bool act = active;
  for (int iters = 0; iters < N * N * 30; iters++) {
    if (__ballot(act) == 0ull) break;
    // pivot: rows 0..7 through indR, then columns 1..8 through indC; first maximum.  All sixteen candidates are
    // loaded first (one LDS latency), then compared in order.
    int ci[16]; double cvv[16];
#pragma unroll
    for (int i = 0; i < N - 1; i++) { ci[i] = indR[i]; cvv[i] = EL(lm_arow(i) + ci[i] - i - 1); }
#pragma unroll
    for (int i = 1; i < N; i++) { ci[7 + i] = indC[i]; cvv[7 + i] = EL(lm_arow(ci[7 + i]) + i - ci[7 + i] - 1); }
    int k = 0, l = ci[0];
    double p = cvv[0], mv = fabs(p);
#pragma unroll
    for (int i = 1; i < N - 1; i++) {
      const bool b = mv < fabs(cvv[i]);
      mv = b ? fabs(cvv[i]) : mv; p = b ? cvv[i] : p; k = b ? i : k; l = b ? ci[i] : l;
    }
#pragma unroll
    for (int i = 1; i < N; i++) {
      const bool b = mv < fabs(cvv[7 + i]);
      mv = b ? fabs(cvv[7 + i]) : mv; p = b ? cvv[7 + i] : p; k = b ? ci[7 + i] : k; l = b ? i : l;
    }
    if (mv <= DBL_EPSILON) act = false;
    k = act ? k : 0; l = act ? l : 1;
    const int rowk = lm_arow(k), rowl = lm_arow(l);
    // operands of the rotation: the pairs of A (dummy element 0 for i == k, l) and of V, loaded before the scalars
    int e1[9], e2[9];
    double a0[9], b0[9], va[9], vb[9];
#pragma unroll
    for (int i = 0; i < N; i++) {
      const bool rot = i != k && i != l;
      e1[i] = rot ? (i < k ? lm_arow(i) + k - i - 1 : rowk + i - k - 1) : 0;
      e2[i] = rot ? (i < l ? lm_arow(i) + l - i - 1 : rowl + i - l - 1) : 0;
      a0[i] = EL(e1[i]); b0[i] = EL(e2[i]);
      va[i] = VL(k * N + i); vb[i] = VL(l * N + i);
    }
    const double wk = EL(LM_W + k), wl = EL(LM_W + l);
    double c = 1, sn = 0, t = 0;
    if (plain) { const Cst r = rotation_scalars_plain(p, wk, wl); c = r.c; sn = r.s; t = r.t; }
    else rotation_scalars(p, wk, wl, c, sn, t);
    // rotate; the rescans of indR / indC for k and l run on the fresh values: row k right of the diagonal holds
    // A[k][l] = 0 at index l, column l above the diagonal holds it at index k
    int mRk = 0, mCk = 0, mRl = 0, mCl = 0;
    double vRk = -1, vCk = -1, vRl = -1, vCl = -1;
#pragma unroll
    for (int i = 0; i < N; i++) {
      const bool rot = i != k && i != l;
      const double u = rot ? a0[i] * c - b0[i] * sn : 0.0, v = rot ? a0[i] * sn + b0[i] * c : 0.0;
      if (act && rot) { EL(e1[i]) = u; EL(e2[i]) = v; }
      const double au = fabs(u), av = fabs(v);
      const bool rk = i > k && vRk < au, ck = i < k && vCk < au, rl = i > l && vRl < av, cl = i < l && vCl < av;
      vRk = rk ? au : vRk; mRk = rk ? i : mRk;
      vCk = ck ? au : vCk; mCk = ck ? i : mCk;
      vRl = rl ? av : vRl; mRl = rl ? i : mRl;
      vCl = cl ? av : vCl; mCl = cl ? i : mCl;
    }
    if (act) {
      EL(rowk + l - k - 1) = 0.0;
      EL(LM_W + k) = wk - t; EL(LM_W + l) = wl + t;
#pragma unroll
      for (int i = 0; i < N; i++) {
        VL(k * N + i) = va[i] * c - vb[i] * sn;
        VL(l * N + i) = va[i] * sn + vb[i] * c;
      }
    }
    // indR / indC of the two rotated indices (row N-1 has no indR, column 0 no indC: those registers are never read)
#pragma unroll
    for (int i = 0; i < N; i++) {
      indR[i] = act && i == k ? mRk : act && i == l ? mRl : indR[i];
      indC[i] = act && i == k ? mCk : act && i == l ? mCl : indC[i];
    }
  }
  // selection sort (descending) on the index list: only the row that ends last is needed
  double w[9]; int pm[9];
#pragma unroll
  for (int i = 0; i < N; i++) { w[i] = active ? EL(LM_W + i) : 0.0; pm[i] = i; }
#pragma unroll
  for (int a = 0; a < N - 1; a++) {
    double bv = w[a]; int bi = a, bp = pm[a];
#pragma unroll
    for (int i = a + 1; i < N; i++) if (bv < w[i]) bv = w[i], bi = i, bp = pm[i];
#pragma unroll
    for (int i = a + 1; i < N; i++) if (i == bi) { w[i] = w[a]; pm[i] = pm[a]; }
    w[a] = bv; pm[a] = bp;
  }
  return pm[N - 1];
#undef EL
#undef VL
}

// ---- tolerance mode of the LM refinement (EVH_SOLVER_FAST).  cv::solve(Ap, v, d, DECOMP_EIG) costs ~100 dependent Jacobi
// rotations of ~1 400 cycles each; the same 8x8 symmetric positive definite system by LDL^T in one lane is ~3 000 cycles.
// These systems are graded over ~14 orders of magnitude (raw pixel coordinates: smallest eigenvalue ~5 x the eigen-solve's
// truncation threshold), so along the weakest direction the two solvers differ in the leading digits of the step and, LM being
// cut after 10 iterations, H ends up to ~6e-4 px (corners) away from OpenCV's -- an opt-in mode (include/evhip.h); the RANSAC
// draw, the inlier masks and the refit are untouched.  Returns false when a pivot is not positive (the
// caller then takes the exact path), so nothing is ever solved with a factorisation that does not exist; min_rel_pivot > 0
// also refuses pivots at or below that fraction of their diagonal entry (numerically singular: the refit's h33 = 1 system).
__device__ bool ldl8_factor(const double* A /*LDS, symmetric 8x8*/, double (&Lm)[28], double (&Dinv)[8], double min_rel_pivot) {
  double Dd[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    double dj = A[j * 8 + j];
#pragma unroll
    for (int k = 0; k < j; k++) { const double l = Lm[(j * (j - 1)) / 2 + k]; dj -= l * l * Dd[k]; }
    if (!(dj > 0) || dj <= min_rel_pivot * A[j * 8 + j]) return false;
    Dd[j] = dj;
    Dinv[j] = 1.0 / dj;
#pragma unroll
    for (int i = j + 1; i < 8; i++) {
      double t = A[i * 8 + j];
#pragma unroll
      for (int k = 0; k < j; k++) t -= Lm[(i * (i - 1)) / 2 + k] * Lm[(j * (j - 1)) / 2 + k] * Dd[k];
      Lm[(i * (i - 1)) / 2 + j] = t * Dinv[j];
    }
  }
  return true;
}
__device__ void ldl8_solve(const double (&Lm)[28], const double (&Dinv)[8], const double (&b)[8], double (&x)[8]) {
  double y[8];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    double t = b[i];
#pragma unroll
    for (int k = 0; k < i; k++) t -= Lm[(i * (i - 1)) / 2 + k] * y[k];
    y[i] = t;
  }
#pragma unroll
  for (int i = 7; i >= 0; i--) {
    double t = y[i] * Dinv[i];
#pragma unroll
    for (int k = i + 1; k < 8; k++) t -= Lm[(k * (k - 1)) / 2 + i] * x[k];
    x[i] = t;
  }
}
// lane 0: x = A^-1 b (b != null) or x[0] = max_i |(A^-1)_ii| (b == null); flag in ok (LDS int)
__device__ void fast_solve8(int lane, const double* A, const double* b, double* x, int* ok, double min_rel_pivot = 0.0) {
  if (lane == 0) {
    double Lm[28], Dinv[8];
    bool good = ldl8_factor(A, Lm, Dinv, min_rel_pivot);
    if (good) {
      if (b) {
        double bb[8], xx[8];
#pragma unroll
        for (int i = 0; i < 8; i++) bb[i] = b[i];
        ldl8_solve(Lm, Dinv, bb, xx);
#pragma unroll
        for (int i = 0; i < 8; i++) x[i] = xx[i];
      } else {
        double mv = 0;
        for (int c = 0; c < 8; c++) {
          double e[8], col[8];
#pragma unroll
          for (int i = 0; i < 8; i++) e[i] = i == c ? 1.0 : 0.0;
          ldl8_solve(Lm, Dinv, e, col);
          double dc = 0;
#pragma unroll
          for (int i = 0; i < 8; i++) dc = i == c ? col[i] : dc;
          mv = fmax(mv, fabs(dc));
        }
        x[0] = mv;
      }
    }
    *ok = good ? 1 : 0;
  }
}
}  // namespace
