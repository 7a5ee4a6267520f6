// evh_ransac_dlt.h -- internal to evh_ransac.hip (layer 3 of 4): the four forms of the normalised DLT, SolveLds
#pragma once
#include "evh_ransac_eig.h"
namespace {
#define TS 11          // stride (doubles) of one point's terms in the LDS tile
#define TT (NL + 2)    // term-major tiles ([term][point], the single-problem stages): doubles between two terms' rows; 528
                       // bytes, so that 16-byte reads of different terms fall on different bank slots

// de-normalise the smallest-eigenvalue eigenvector into H (runKernel's tail)
__device__ __forceinline__ void dlt_finish_from(const double* H0, double cmx, double cmy, double smx, double smy, double cMx,
                                                double cMy, double sMx, double sMy, double* H) {
  const double invHnorm[9] = {1. / smx, 0, cmx, 0, 1. / smy, cmy, 0, 0, 1};
  const double Hnorm2[9] = {sMx, 0, -cMx * sMx, 0, sMy, -cMy * sMy, 0, 0, 1};
  double Ht[9], H1[9];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++)
      Ht[3 * r + c] = (invHnorm[3 * r] * H0[c] + invHnorm[3 * r + 1] * H0[3 + c]) + invHnorm[3 * r + 2] * H0[6 + c];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++)
      H1[3 * r + c] = (Ht[3 * r] * Hnorm2[c] + Ht[3 * r + 1] * Hnorm2[3 + c]) + Ht[3 * r + 2] * Hnorm2[6 + c];
  double inv = 1. / H1[8];
#pragma unroll
  for (int i = 0; i < 9; i++) H[i] = H1[i] * inv;
}
__device__ __forceinline__ void dlt_finish(const RowMat& M, double cmx, double cmy, double smx, double smy, double cMx,
                                           double cMy, double sMx, double sMy, double* H) {
  double H0[9];
  const int r8 = M.ord[8];
#pragma unroll
  for (int i = 0; i < 9; i++) H0[i] = M.V[r8 * MS + i];
  dlt_finish_from(H0, cmx, cmy, smx, smy, cMx, cMy, sMx, sMy, H);
}

// one entry (j, k) of L^T L contributed by a normalised correspondence (x, y) <- (X, Y)
__device__ __forceinline__ double ltl_term(int j, int k, double x, double y, double X, double Y) {
  const double nxX = -x * X, nxY = -x * Y, nyX = -y * X, nyY = -y * Y;
  // Lx = {X, Y, 1, 0, 0, 0, -xX, -xY, -x}; Ly = {0, 0, 0, X, Y, 1, -yX, -yY, -y}
#define LXS(q) ((q) == 0 ? X : (q) == 1 ? Y : (q) == 2 ? 1.0 : (q) < 6 ? 0.0 : (q) == 6 ? nxX : (q) == 7 ? nxY : -x)
#define LYS(q) ((q) < 3 ? 0.0 : (q) == 3 ? X : (q) == 4 ? Y : (q) == 5 ? 1.0 : (q) == 6 ? nyX : (q) == 7 ? nyY : -y)
  return LXS(j) * LXS(k) + LYS(j) * LYS(k);
#undef LXS
#undef LYS
}
// upper-triangle entry number e (0..44, row-major) of a 9x9 -> (j, k), j <= k
__device__ __forceinline__ void tri9(int e, int& j, int& k) {
  j = 0;
  while (e >= 9 - j) { e -= 9 - j; j++; }
  k = j + e;
}
__device__ __forceinline__ void tri8(int e, int& i, int& j) {
  i = 0;
  while (e >= 8 - i) { e -= 8 - i; i++; }
  j = i + e;
}

// normalised DLT of each row's own 4 correspondences (M -> m): every lane of a row holds the same 4 points.
// `valid` is row-uniform; returns (row-uniform) whether a model was produced; H valid on every lane of the row.
__device__ __forceinline__ bool dlt4_rows(RowMat& M, int lane, bool valid, const float* Mx, const float* My,
                                          const float* mx, const float* my, double* H) {
  const int gl = lane & 15;
  double cMx = 0, cMy = 0, cmx = 0, cmy = 0, sMx = 0, sMy = 0, smx = 0, smy = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) { cmx += mx[i]; cmy += my[i]; cMx += Mx[i]; cMy += My[i]; }
  cmx /= 4; cmy /= 4; cMx /= 4; cMy /= 4;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    smx += fabs(mx[i] - cmx); smy += fabs(my[i] - cmy);
    sMx += fabs(Mx[i] - cMx); sMy += fabs(My[i] - cMy);
  }
  const bool ok = valid && !(fabs(smx) < DBL_EPSILON || fabs(smy) < DBL_EPSILON || fabs(sMx) < DBL_EPSILON ||
                             fabs(sMy) < DBL_EPSILON);
  if (ok) {
    smx = 4 / smx; smy = 4 / smy; sMx = 4 / sMx; sMy = 4 / sMy;
    for (int e = gl; e < 45; e += GL) {          // L^T L upper triangle, entry e <-> (j, k), points summed in order
      int j, k;
      tri9(e, j, k);
      double acc = 0;
#pragma unroll
      for (int i = 0; i < 4; i++)
        acc += ltl_term(j, k, (mx[i] - cmx) * smx, (my[i] - cmy) * smy, (Mx[i] - cMx) * sMx, (My[i] - cMy) * sMy);
      M.A[j * MS + k] = acc;
      M.A[k * MS + j] = acc;
    }
  }
  WSYNC();
  jacobi_rows<9>(M, lane, ok);
  if (ok) dlt_finish(M, cmx, cmy, smx, smy, cMx, cMy, sMx, sMy, H);
  return ok;
}

// normalised DLT of this LANE's own 4 correspondences (M -> m); returns whether a model was produced
__device__ __forceinline__ bool dlt4_lane(double* L, double* Vg, bool valid, const float* Mx, const float* My, const float* mx,
                                          const float* my, double* H) {
  double cMx = 0, cMy = 0, cmx = 0, cmy = 0, sMx = 0, sMy = 0, smx = 0, smy = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) { cmx += mx[i]; cmy += my[i]; cMx += Mx[i]; cMy += My[i]; }
  cmx /= 4; cmy /= 4; cMx /= 4; cMy /= 4;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    smx += fabs(mx[i] - cmx); smy += fabs(my[i] - cmy);
    sMx += fabs(Mx[i] - cMx); sMy += fabs(My[i] - cMy);
  }
  const bool ok = valid && !(fabs(smx) < DBL_EPSILON || fabs(smy) < DBL_EPSILON || fabs(sMx) < DBL_EPSILON ||
                             fabs(sMy) < DBL_EPSILON);
  if (ok) {
    smx = 4 / smx; smy = 4 / smy; sMx = 4 / sMx; sMy = 4 / sMy;
    double x[4], y[4], X[4], Y[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      x[i] = (mx[i] - cmx) * smx; y[i] = (my[i] - cmy) * smy; X[i] = (Mx[i] - cMx) * sMx; Y[i] = (My[i] - cMy) * sMy;
    }
#pragma unroll
    for (int j = 0; j < 9; j++)
#pragma unroll
      for (int k = j; k < 9; k++) {
        double acc = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) acc += ltl_term(j, k, x[i], y[i], X[i], Y[i]);
        L[(j == k ? LM_W + j : lm_a(j, k)) * NL] = acc;
      }
  }
  const int r8 = jacobi_lanes9(L, Vg, ok);
  if (ok) {
    double H0[9];
#pragma unroll
    for (int i = 0; i < 9; i++) H0[i] = Vg[(r8 * 9 + i) * NL];
    dlt_finish_from(H0, cmx, cmy, smx, smy, cMx, cMy, sMx, sMy, H);
  }
  return ok;
}

struct SolveLds {        // scratch of the single-problem stages (refit, LM): used by wave 0 only
  double bestH[9];
  double H[9];           // result of the last single-problem DLT / LM
  double x[8], xd[8], v[8], d[8], D[8], tmpd[8], A8[64], Ap[64], Inv[64];
  double sc[8];          // scalars: S, Sd, lambda, lc, nu, rmax ...
  int ib[8];             // ints: proceed flags, counts
  int fast;              // EvhRansacArgs::fast_solver (set by the kernels before any solve)
  alignas(16) double T[NL * TS];     // the 64-point tile (16-byte LDS accesses: ds_read_b128 costs a quarter of the 8-byte forms)
  double P2[NL / 2 + 2]; // lm_eval: squared residuals of a tile, summed per pair of points (+ the two terms of an odd last point)
};

// ---- tolerance mode (EVH_SOLVER_FAST) of the refit's sums: lane-strided partial sums + a butterfly instead of the point-order
// chains (see lm_eval_fast).  With a = (X, Y, 1): Lx = (a, 0, -x a), Ly = (0, a, -y a), so L^T L needs sum a_i a_j, sum x a_i a_j,
// sum y a_i a_j and sum (x^2 + y^2) a_i a_j -- 24 sums instead of 45 chains.  The eigen-solve and the de-normalisation are shared.
__device__ __forceinline__ bool dlt_rows_fast(SolveLds& S, RowMat& M, int lane, const float* rows, int count, double* Hout /* LDS */,
                                              unsigned long long* prof) {
  double c0 = 0, c1 = 0, c2 = 0, c3 = 0;
  for (int i = lane; i < count; i += NL) {
    const float4 r = *reinterpret_cast<const float4*>(rows + 4 * i);
    c0 += r.z; c1 += r.w; c2 += r.x; c3 += r.y;
  }
  const double cmx = wave_sum_f64(c0) / count, cmy = wave_sum_f64(c1) / count, cMx = wave_sum_f64(c2) / count, cMy = wave_sum_f64(c3) / count;
  c0 = c1 = c2 = c3 = 0;
  for (int i = lane; i < count; i += NL) {
    const float4 r = *reinterpret_cast<const float4*>(rows + 4 * i);
    c0 += fabs(r.z - cmx); c1 += fabs(r.w - cmy); c2 += fabs(r.x - cMx); c3 += fabs(r.y - cMy);
  }
  double smx = wave_sum_f64(c0), smy = wave_sum_f64(c1), sMx = wave_sum_f64(c2), sMy = wave_sum_f64(c3);
  if (fabs(smx) < DBL_EPSILON || fabs(smy) < DBL_EPSILON || fabs(sMx) < DBL_EPSILON || fabs(sMy) < DBL_EPSILON) return false;
  smx = count / smx; smy = count / smy; sMx = count / sMx; sMy = count / sMy;
  double aa[6] = {0, 0, 0, 0, 0, 0}, xa[6] = {0, 0, 0, 0, 0, 0}, ya[6] = {0, 0, 0, 0, 0, 0}, qa[6] = {0, 0, 0, 0, 0, 0};
  for (int i = lane; i < count; i += NL) {
    const float4 r = *reinterpret_cast<const float4*>(rows + 4 * i);
    const double x = (r.z - cmx) * smx, y = (r.w - cmy) * smy;
    const double X = (r.x - cMx) * sMx, Y = (r.y - cMy) * sMy;
    const double p[6] = {X * X, X * Y, X, Y * Y, Y, 1.0};           // a_i a_j for (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
    const double q = x * x + y * y;
#pragma unroll
    for (int k = 0; k < 6; k++) { aa[k] += p[k]; xa[k] += x * p[k]; ya[k] += y * p[k]; qa[k] += q * p[k]; }
  }
#pragma unroll
  for (int k = 0; k < 6; k++) { aa[k] = wave_sum_f64(aa[k]); xa[k] = wave_sum_f64(xa[k]); ya[k] = wave_sum_f64(ya[k]); qa[k] = wave_sum_f64(qa[k]); }
  if (lane == 0) {
    for (int i = 0; i < 9; i++) for (int j = 0; j < 9; j++) M.A[i * MS + j] = 0.0;
    const int ui[6] = {0, 0, 0, 1, 1, 2}, uj[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const int i = ui[k], j = uj[k];
      M.A[i * MS + j] = aa[k]; M.A[j * MS + i] = aa[k];
      M.A[(3 + i) * MS + 3 + j] = aa[k]; M.A[(3 + j) * MS + 3 + i] = aa[k];
      M.A[(6 + i) * MS + 6 + j] = qa[k]; M.A[(6 + j) * MS + 6 + i] = qa[k];
      M.A[i * MS + 6 + j] = -xa[k]; M.A[j * MS + 6 + i] = -xa[k]; M.A[(6 + j) * MS + i] = -xa[k]; M.A[(6 + i) * MS + j] = -xa[k];
      M.A[(3 + i) * MS + 6 + j] = -ya[k]; M.A[(3 + j) * MS + 6 + i] = -ya[k]; M.A[(6 + j) * MS + 3 + i] = -ya[k]; M.A[(6 + i) * MS + 3 + j] = -ya[k];
    }
  }
  WSYNC();
  // The refit only seeds the LM refinement, so in this mode the smallest eigenvector of L^T L (117 Jacobi rotations) gives way
  // to the inhomogeneous least-squares solution with h33 = 1 in the normalised frame: one 8x8 LDL^T.  A pivot that is not
  // positive, or a solution that is not finite, falls back to the eigen-solve.  So does a pivot at or below 1e-10 of its
  // diagonal entry: when the horizon of H passes through the source centroid, h33 = 0 in the normalised frame, the 8x8
  // block is singular and its last pivot is rounding noise of either sign -- a positive one used to go through with a
  // solution of ordinary size that is noise over noise, a seed LM could not repair (tests/solver_families.py, f6_horizon).
  // A pivot ratio of 1e-10 means |h33| below ~1e-5 of the null vector in the normalised frame.
  if (lane == 0) {
    for (int i = 0; i < 8; i++) {
      for (int j = 0; j < 8; j++) S.Ap[i * 8 + j] = M.A[i * MS + j];
      S.tmpd[i] = -M.A[i * MS + 8];
    }
  }
  WSYNC();
  fast_solve8(lane, S.Ap, S.tmpd, S.d, &S.ib[2], 1e-10);
  WSYNC();
  bool direct = S.ib[2] != 0;
  if (direct) {
    double mx = 0;
    for (int i = 0; i < 8; i++) mx = fmax(mx, fabs(S.d[i]));
    direct = mx < 1e12;                                   // (NaN compares false)
  }
  if (direct) {
    if (lane == 0) {
      double H0[9], H[9];
      for (int i = 0; i < 8; i++) H0[i] = S.d[i];
      H0[8] = 1.0;
      dlt_finish_from(H0, cmx, cmy, smx, smy, cMx, cMy, sMx, sMy, H);
      for (int i = 0; i < 9; i++) Hout[i] = H[i];
    }
    WSYNC();
    return true;
  }
  pf_add(prof, PF_ROT9, jacobi_one<9>(M, lane));
  if (lane == 0) {
    double H[9];
    dlt_finish(M, cmx, cmy, smx, smy, cMx, cMy, sMx, sMy, H);
    for (int i = 0; i < 9; i++) Hout[i] = H[i];
  }
  WSYNC();
  return true;
}

// ---- single-problem normalised DLT on `count` rows (ax,ay,bx,by): sums in row order, one lane per sum; wave 0 ------
__device__ __forceinline__ bool dlt_rows(SolveLds& S, RowMat& M, int lane, const float* rows, int count, double* Hout /* LDS */,
                                         unsigned long long* prof = nullptr) {
  if (S.fast && count > 4) return dlt_rows_fast(S, M, lane, rows, count, Hout, prof);
  double* T = S.T;
  // centroids: lanes 0..3 own cm.x, cm.y, cM.x, cM.y  (m = b columns, M = a columns)
  double acc = 0;
  const float4 first_rows = lane < count ? *reinterpret_cast<const float4*>(rows + 4 * lane) : make_float4(0, 0, 0, 0);
  float4 rnext = first_rows;
  for (int c0 = 0; c0 < count; c0 += NL) {
    const int i = c0 + lane;
    const float4 r = rnext;                       // requested one tile ahead
    if (i + NL < count) rnext = *reinterpret_cast<const float4*>(rows + 4 * (i + NL));
    if (i < count) {
      T[lane] = r.z; T[TT + lane] = r.w; T[2 * TT + lane] = r.x; T[3 * TT + lane] = r.y;
    }
    WSYNC();
    const int cnt = min(NL, count - c0);
    if (lane < 4) {
      int j = 0;
      for (; j + 16 <= cnt; j += 16) {
        d2_t v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = *reinterpret_cast<const d2_t*>(T + lane * TT + j + 2 * u);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 8; u++) { acc += v[u].x; acc += v[u].y; }
      }
      for (; j < cnt; j++) acc += T[lane * TT + j];
    }
    WSYNC();
  }
  if (lane < 4) acc /= count;
  const double cmx = __shfl(acc, 0), cmy = __shfl(acc, 1), cMx = __shfl(acc, 2), cMy = __shfl(acc, 3);
  double dev = 0;
  const double mycen = lane == 0 ? cmx : lane == 1 ? cmy : lane == 2 ? cMx : cMy;
  rnext = first_rows;
  for (int c0 = 0; c0 < count; c0 += NL) {
    const int i = c0 + lane;
    const float4 r = rnext;                       // requested one tile ahead
    if (i + NL < count) rnext = *reinterpret_cast<const float4*>(rows + 4 * (i + NL));
    if (i < count) {
      T[lane] = r.z; T[TT + lane] = r.w; T[2 * TT + lane] = r.x; T[3 * TT + lane] = r.y;
    }
    WSYNC();
    const int cnt = min(NL, count - c0);
    if (lane < 4) {
      int j = 0;
      for (; j + 16 <= cnt; j += 16) {
        d2_t v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = *reinterpret_cast<const d2_t*>(T + lane * TT + j + 2 * u);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 8; u++) { dev += fabs(v[u].x - mycen); dev += fabs(v[u].y - mycen); }
      }
      for (; j < cnt; j++) dev += fabs(T[lane * TT + j] - mycen);
    }
    WSYNC();
  }
  double smx = __shfl(dev, 0), smy = __shfl(dev, 1), sMx = __shfl(dev, 2), sMy = __shfl(dev, 3);
  if (fabs(smx) < DBL_EPSILON || fabs(smy) < DBL_EPSILON || fabs(sMx) < DBL_EPSILON || fabs(sMy) < DBL_EPSILON)
    return false;
  smx = count / smx; smy = count / smy; sMx = count / sMx; sMy = count / sMy;
  // L^T L upper triangle: lane e <-> entry (j,k), sequential over the points.  A point's terms in the tile:
  // 0:X 1:Y 2:1 3:0 4:-xX 5:-xY 6:-x 7:-yX 8:-yY 9:-y ; Lx = {0,1,2,3,3,3,4,5,6}, Ly = {3,3,3,0,1,2,7,8,9}
  int ej = 0, ek = 0;
  if (lane < 45) tri9(lane, ej, ek);
  const int lxj = ej < 3 ? ej : ej < 6 ? 3 : ej - 2, lxk = ek < 3 ? ek : ek < 6 ? 3 : ek - 2;
  const int lyj = ej < 3 ? 3 : ej < 6 ? ej - 3 : ej + 1, lyk = ek < 3 ? 3 : ek < 6 ? ek - 3 : ek + 1;
  double s = 0;
  rnext = first_rows;
  for (int c0 = 0; c0 < count; c0 += NL) {
    const int i = c0 + lane;
    const float4 r = rnext;
    if (i + NL < count) rnext = *reinterpret_cast<const float4*>(rows + 4 * (i + NL));
    if (i < count) {
      const double x = (r.z - cmx) * smx, y = (r.w - cmy) * smy;
      const double X = (r.x - cMx) * sMx, Y = (r.y - cMy) * sMy;
      double* t = T + lane;                                 // term j of this point at t[j * TT]
      t[0] = X; t[TT] = Y; t[2 * TT] = 1.0; t[3 * TT] = 0.0; t[4 * TT] = -x * X; t[5 * TT] = -x * Y; t[6 * TT] = -x;
      t[7 * TT] = -y * X; t[8 * TT] = -y * Y; t[9 * TT] = -y;
    }
    WSYNC();
    const int cnt = min(NL, count - c0);
    if (lane < 45) {
      // four points' operands requested before the first product: the compiler otherwise waits for the LDS after every
      // point (measured on lm_eval_mw's loops: one round trip per read group, 3x the time)
      int j = 0;
      for (; j + 8 <= cnt; j += 8) {                        // eight points: four 16-byte reads per operand row
        d2_t a[4], b[4], c[4], d[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
          a[u] = *reinterpret_cast<const d2_t*>(T + lxj * TT + j + 2 * u); b[u] = *reinterpret_cast<const d2_t*>(T + lxk * TT + j + 2 * u);
          c[u] = *reinterpret_cast<const d2_t*>(T + lyj * TT + j + 2 * u); d[u] = *reinterpret_cast<const d2_t*>(T + lyk * TT + j + 2 * u);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 4; u++) { s += a[u].x * b[u].x + c[u].x * d[u].x; s += a[u].y * b[u].y + c[u].y * d[u].y; }
      }
      for (; j < cnt; j++) s += T[lxj * TT + j] * T[lxk * TT + j] + T[lyj * TT + j] * T[lyk * TT + j];
    }
    WSYNC();
  }
  if (lane < 45) { M.A[ej * MS + ek] = s; M.A[ek * MS + ej] = s; }
  WSYNC();
  pf_add(prof, PF_ROT9, jacobi_one<9>(M, lane));
  if (lane == 0) {
    double H[9];
    dlt_finish(M, cmx, cmy, smx, smy, cMx, cMy, sMx, sMy, H);
    for (int i = 0; i < 9; i++) Hout[i] = H[i];
  }
  WSYNC();
  return true;
}
}  // namespace
