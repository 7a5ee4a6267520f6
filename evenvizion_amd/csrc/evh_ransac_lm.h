// evh_ransac_lm.h -- internal to evh_ransac.hip (layer 4 of 4): the LM refinement, its three evaluation forms, BlockLds
#pragma once
#include "evh_ransac_dlt.h"
namespace {
// ---- symmetric solve / inverse through the eigen-decomposition (cv::solve / cv::invert, DECOMP_EIGEN) -------------
// all 64 lanes of wave 0; Ain / b / x live in LDS.  Back-substitution keeps the serial summation orders: lane i forms
// s_i = (sum_j u_i[j] b[j]) / w_i, lane j accumulates x[j] += s_i u_i[j] over i ascending.
__device__ __forceinline__ void eig_solve8_wave(RowMat& M, int lane, const double* Ain /*LDS 64*/, const double* b /*LDS 8 or null*/,
                                double* x /*LDS 8 or 64*/, unsigned long long* prof = nullptr) {
  const unsigned long long pt0 = pf_now_if(prof);
  {
    const int i = lane >> 3, j = lane & 7;
    M.A[i * MS + j] = Ain[min(i, j) * 8 + max(i, j)];
  }
  WSYNC();
  pf_add(prof, PF_ROT8, jacobi_one<8>(M, lane));
  double threshold = 0;
  for (int i = 0; i < 8; i++) threshold += M.W[M.ord[i]];
  threshold *= DBL_EPSILON * 2;
  if (b) {
    // s_i on lane i (0 for skipped eigenvalues is NOT equivalent to skipping: keep a flag)
    double si = 0; bool use = false;
    if (lane < 8) {
      const int r = M.ord[lane];
      double wi = M.W[r];
      if (!(fabs(wi) <= threshold)) {
        use = true;
        wi = 1 / wi;
        double acc = 0;
        for (int j = 0; j < 8; j++) acc += M.V[r * MS + j] * b[j];
        si = acc * wi;
      }
    }
    double xj = 0;
    for (int i = 0; i < 8; i++) {
      const double s_i = __shfl(si, i);
      const int u_i = __shfl((int)use, i);
      if (u_i && lane < 8) xj = xj + s_i * M.V[M.ord[i] * MS + lane];
    }
    if (lane < 8) x[lane] = xj;
  } else {
    // inverse: x[r][j] += u_i[r] * (u_i[j] / w_i) over i ascending; lane = r*8 + j
    const int r = lane >> 3, j = lane & 7;
    double acc = 0;
    for (int i = 0; i < 8; i++) {
      const int ri = M.ord[i];
      double wi = M.W[ri];
      if (fabs(wi) <= threshold) continue;
      wi = 1 / wi;
      const double sj = M.V[ri * MS + j] * wi;
      acc = acc + M.V[ri * MS + r] * sj;
    }
    x[r * 8 + j] = acc;
  }
  WSYNC();
  pf_add(prof, PF_SOLVE8, pf_now_if(prof) - pt0);
}

// acc + v[0] + v[1] + ... + v[n-1] in that order, the words requested sixteen at a time (the compiler alone waits for the
// LDS after every single read of such a chain)
__device__ __forceinline__ double add_in_order(double acc, const double* v, int n) {
  int g = 0;
  for (; g + 16 <= n; g += 16) {
    double w[16];
#pragma unroll
    for (int u = 0; u < 16; u++) w[u] = v[g + u];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 16; u++) acc += w[u];
  }
  for (; g < n; g++) acc += v[g];
  return acc;
}

// One pass of the refinement callback over the rows at parameters h[0..7] (LDS): S.sc[slotS] = sum of squared
// residuals (groups of four, as cv::norm), S.sc[slotR] = max |residual|; with J also S.A8 = J^T J (mirrored) and
// S.v = J^T r (four interleaved partial sums).  Wave 0, all 64 lanes.  A point's terms in the tile:
// 0:Mx*ww 1:My*ww 2:ww 3:0 4:-Mx*ww*xi 5:-My*ww*xi 6:-Mx*ww*yi 7:-My*ww*yi 8:xi-mx 9:yi-my
//   x-row of J = {0,1,2,3,3,3,4,5}, y-row = {3,3,3,0,1,2,6,7}
__device__ __forceinline__ void lm_eval(SolveLds& S, int lane, const float* rows, int count, const double* h, bool withJ, int slotS,
                        int slotR) {
  double* T = S.T;
  const double h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3], h4 = h[4], h5 = h[5], h6 = h[6], h7 = h[7];
  int ei = 0, ej = 0;
  if (lane < 36) tri8(lane, ei, ej);
  const int jxi = ei < 3 ? ei : ei < 6 ? 3 : ei - 2, jxj = ej < 3 ? ej : ej < 6 ? 3 : ej - 2;
  const int jyi = ei < 3 ? 3 : ei < 6 ? ei - 3 : ei, jyj = ej < 3 ? 3 : ej < 6 ? ej - 3 : ej;
  const int vi = lane - 36;                      // lanes 36..43: J^T r entry vi
  const int vx = vi < 3 ? vi : vi < 6 ? 3 : vi - 2, vy = vi < 3 ? 3 : vi < 6 ? vi - 3 : vi;
  double s = 0, s0 = 0, s1 = 0, s2 = 0, s3 = 0, nrm = 0, rmax = 0;
  // role of this lane in the sums: 1 = one J^T J entry (lanes 0..35), 2 = one J^T r entry (36..43), 3 = the squared norm (44)
  const int role = withJ && lane < 36 ? 1 : withJ && lane < 44 ? 2 : lane == 44 ? 3 : 0;
  const int pa = role == 1 ? jxi : role == 2 ? vx : 8, pb = role == 1 ? jxj : 8;
  const int pc = role == 1 ? jyi : role == 2 ? vy : 9, pd = role == 1 ? jyj : 9;
  // the rows of the NEXT tile are requested before this tile is worked on (a tile used to start with a full memory round trip)
  float4 rnext = lane < count ? *reinterpret_cast<const float4*>(rows + 4 * lane) : make_float4(0, 0, 0, 0);
  for (int c0 = 0; c0 < count; c0 += NL) {
    const int i = c0 + lane;
    double q0 = 0, q1 = 0;
    const float4 r = rnext;
    if (i + NL < count) rnext = *reinterpret_cast<const float4*>(rows + 4 * (i + NL));
    if (i < count) {
      const double Mx = r.x, My = r.y;
      double ww = h6 * Mx + h7 * My + 1.;
      ww = fabs(ww) > DBL_EPSILON ? 1. / ww : 0;
      const double xi = (h0 * Mx + h1 * My + h2) * ww;
      const double yi = (h3 * Mx + h4 * My + h5) * ww;
      const double rx = xi - r.z, ry = yi - r.w;
      double* t = T + lane * TS;
      t[8] = rx; t[9] = ry;
      if (withJ) {
        t[0] = Mx * ww; t[1] = My * ww; t[2] = ww; t[3] = 0.0;
        t[4] = -Mx * ww * xi; t[5] = -My * ww * xi; t[6] = -Mx * ww * yi; t[7] = -My * ww * yi;
      }
      rmax = fmax(rmax, fabs(rx));
      rmax = fmax(rmax, fabs(ry));
      q0 = rx * rx; q1 = ry * ry;
    }
    // the squared norm goes in groups of four like cv::norm: ((rx_j^2 + ry_j^2) + rx_{j+1}^2) + ry_{j+1}^2 per PAIR of
    // points.  The pair sums are formed in parallel (the even lane takes its neighbour's squares), one lane then adds the
    // <= 32 of them in order -- 48 instructions per tile instead of a 512-instruction walk by one lane
    const int cnt = min(NL, count - c0);
    {
      const double n0 = __shfl_down(q0, 1), n1 = __shfl_down(q1, 1);
      if (!(lane & 1)) {
        if (lane + 1 < cnt) S.P2[lane >> 1] = ((q0 + q1) + n0) + n1;
        else if (lane < cnt) { S.P2[NL / 2] = q0; S.P2[NL / 2 + 1] = q1; }      // odd last point: two separate additions
      }
    }
    WSYNC();
    // One instruction stream for the two kinds of matrix sums (round 3; with the norm they were three divergent
    // branches, i.e. three passes of the wave over the tile): every lane forms the same four products per PAIR of points
    // from its own four term indices (pa, pb, pc, pd) -- J^T J entry: (jxi, jxj, jyi, jyj), J^T r entry: (vx, 8, vy, 9) --
    // and only the additions differ: one running sum in point order / four interleaved partial sums.
    if (role == 1 || role == 2) {
      int j = 0;
      for (; j + 3 < cnt; j += 4) {               // two pairs of points per trip, their sixteen operands requested together
        const double* t = T + j * TS;
        double a[4], b[4], c[4], d[4];
#pragma unroll
        for (int u = 0; u < 4; u++) { a[u] = t[u * TS + pa]; b[u] = t[u * TS + pb]; c[u] = t[u * TS + pc]; d[u] = t[u * TS + pd]; }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 4; u += 2) {
          const double P0 = a[u] * b[u], P1 = c[u] * d[u], P2 = a[u + 1] * b[u + 1], P3 = c[u + 1] * d[u + 1];
          if (role == 1) { s += P0; s += P1; s += P2; s += P3; }
          else { s0 += P0; s1 += P1; s2 += P2; s3 += P3; }
        }
      }
      for (; j + 1 < cnt; j += 2) {
        const double* t = T + j * TS;
        const double P0 = t[pa] * t[pb], P1 = t[pc] * t[pd], P2 = t[TS + pa] * t[TS + pb], P3 = t[TS + pc] * t[TS + pd];
        if (role == 1) { s += P0; s += P1; s += P2; s += P3; }
        else { s0 += P0; s1 += P1; s2 += P2; s3 += P3; }
      }
      if (j < cnt) {                              // only at the very end (tiles hold an even number of points)
        const double* t = T + j * TS;
        const double P0 = t[pa] * t[pb], P1 = t[pc] * t[pd];
        if (role == 1) { s += P0; s += P1; }
        else { s0 += P0; s0 += P1; }
      }
    } else if (role == 3) {
      nrm = add_in_order(nrm, S.P2, cnt >> 1);
      if (cnt & 1) { nrm += S.P2[NL / 2]; nrm += S.P2[NL / 2 + 1]; }
    }
    WSYNC();
  }
  for (int sft = 32; sft > 0; sft >>= 1) rmax = fmax(rmax, __shfl_xor(rmax, sft));
  if (withJ && lane < 36) { S.A8[ei * 8 + ej] = s; S.A8[ej * 8 + ei] = s; }
  if (withJ && lane >= 36 && lane < 44) S.v[vi] = (s0 + s1 + s2 + s3) * 1.0;
  if (lane == 44) { S.sc[slotS] = nrm; S.sc[slotR] = rmax; }
  WSYNC();
}

// ---- tolerance mode (EVH_SOLVER_FAST): the same sums WITHOUT the operator's point order.  Every lane of wave 0 takes the
// points lane, lane + 64, ... and keeps its own partial sums in registers, a butterfly over the wave adds them: the 2N-long
// dependent chains of the exact form (8.4 cycles per addition, 0.7 M cycles per pair on the default detector list) become
// N / 64 independent steps and a 6-level tree.  J's rows are (t0 t1 t2 0 0 0 t4 t5) and (0 0 0 t0 t1 t2 t6 t7): 21 distinct
// entries of J^T J (the (3..5, 3..5) block repeats the (0..2, 0..2) block), 8 of J^T r, the squared norm, max |r|.
// Results differ from the exact form in the last digits (tests/test_gpu_parity.py::test_fast_solver_mode states the bars).
__device__ __forceinline__ void lm_eval_fast(SolveLds& S, int lane, const float* rows, int count, const double* h, bool withJ, int slotS,
                                             int slotR) {
  const double h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3], h4 = h[4], h5 = h[5], h6 = h[6], h7 = h[7];
  double xx[6] = {0, 0, 0, 0, 0, 0};        // sum t_i t_j, (i, j) = (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
  double xh[6] = {0, 0, 0, 0, 0, 0};        // sum t_i t4, t_i t5        (rows 0..2 against columns 6, 7)
  double yh[6] = {0, 0, 0, 0, 0, 0};        // sum t_i t6, t_i t7        (rows 3..5 against columns 6, 7)
  double hh[3] = {0, 0, 0};                 // (6,6) (6,7) (7,7)
  double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  double nrm = 0, rmax = 0;
  for (int i = lane; i < count; i += NL) {
    const float4 r = *reinterpret_cast<const float4*>(rows + 4 * i);
    const double Mx = r.x, My = r.y;
    double ww = h6 * Mx + h7 * My + 1.;
    ww = fabs(ww) > DBL_EPSILON ? 1. / ww : 0;
    const double xi = (h0 * Mx + h1 * My + h2) * ww;
    const double yi = (h3 * Mx + h4 * My + h5) * ww;
    const double rx = xi - r.z, ry = yi - r.w;
    rmax = fmax(rmax, fmax(fabs(rx), fabs(ry)));
    nrm += rx * rx + ry * ry;
    if (withJ) {
      const double t0 = Mx * ww, t1 = My * ww, t2 = ww;
      const double t4 = -t0 * xi, t5 = -t1 * xi, t6 = -t0 * yi, t7 = -t1 * yi;
      xx[0] += t0 * t0; xx[1] += t0 * t1; xx[2] += t0 * t2; xx[3] += t1 * t1; xx[4] += t1 * t2; xx[5] += t2 * t2;
      xh[0] += t0 * t4; xh[1] += t0 * t5; xh[2] += t1 * t4; xh[3] += t1 * t5; xh[4] += t2 * t4; xh[5] += t2 * t5;
      yh[0] += t0 * t6; yh[1] += t0 * t7; yh[2] += t1 * t6; yh[3] += t1 * t7; yh[4] += t2 * t6; yh[5] += t2 * t7;
      hh[0] += t4 * t4 + t6 * t6; hh[1] += t4 * t5 + t6 * t7; hh[2] += t5 * t5 + t7 * t7;
      v[0] += t0 * rx; v[1] += t1 * rx; v[2] += t2 * rx; v[3] += t0 * ry; v[4] += t1 * ry; v[5] += t2 * ry;
      v[6] += t4 * rx + t6 * ry; v[7] += t5 * rx + t7 * ry;
    }
  }
  nrm = wave_sum_f64(nrm);
  for (int sft = 32; sft > 0; sft >>= 1) rmax = fmax(rmax, __shfl_xor(rmax, sft));
  if (withJ) {
#pragma unroll
    for (int k = 0; k < 6; k++) { xx[k] = wave_sum_f64(xx[k]); xh[k] = wave_sum_f64(xh[k]); yh[k] = wave_sum_f64(yh[k]); }
#pragma unroll
    for (int k = 0; k < 3; k++) hh[k] = wave_sum_f64(hh[k]);
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = wave_sum_f64(v[k]);
    if (lane == 0) {
      double* A = S.A8;
      for (int k = 0; k < 64; k++) A[k] = 0.0;
      const int ui[6] = {0, 0, 0, 1, 1, 2}, uj[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
      for (int k = 0; k < 6; k++) {
        A[ui[k] * 8 + uj[k]] = xx[k]; A[uj[k] * 8 + ui[k]] = xx[k];
        A[(3 + ui[k]) * 8 + 3 + uj[k]] = xx[k]; A[(3 + uj[k]) * 8 + 3 + ui[k]] = xx[k];
      }
#pragma unroll
      for (int i = 0; i < 3; i++) {
        A[i * 8 + 6] = xh[2 * i]; A[6 * 8 + i] = xh[2 * i]; A[i * 8 + 7] = xh[2 * i + 1]; A[7 * 8 + i] = xh[2 * i + 1];
        A[(3 + i) * 8 + 6] = yh[2 * i]; A[6 * 8 + 3 + i] = yh[2 * i]; A[(3 + i) * 8 + 7] = yh[2 * i + 1]; A[7 * 8 + 3 + i] = yh[2 * i + 1];
      }
      A[6 * 8 + 6] = hh[0]; A[6 * 8 + 7] = hh[1]; A[7 * 8 + 6] = hh[1]; A[7 * 8 + 7] = hh[2];
#pragma unroll
      for (int k = 0; k < 8; k++) S.v[k] = v[k];
    }
  }
  if (lane == 0) { S.sc[slotS] = nrm; S.sc[slotR] = rmax; }
  WSYNC();
}

__device__ __forceinline__ double dot8(const double* a, const double* b) {
  double r = 0;
  r += a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
  r += a[4] * b[4] + a[5] * b[5] + a[6] * b[6] + a[7] * b[7];
  return r;
}

// Levenberg-Marquardt refinement of S.H[0..7] over `count` rows (<= 10 iterations). Returns iterations.  Wave 0.
// S.sc: 0 = S, 1 = rmax of the kept point, 2 = lambda, 3 = lc, 4 = nu, 5 = Sd, 6 = rmax of the trial point
// evalJ(): the pass WITH the Jacobian at S.x into S.sc[0], S.sc[1], S.A8, S.v -- lm_eval by this wave alone, or the
// four-wave form (lm_eval_mw) where the workgroup has helper waves.
template <typename EvalJ, typename EvalN>
__device__ __forceinline__ int lm_refine(SolveLds& S, RowMat& M, int lane, const float* rows, int count,
                                         unsigned long long* prof, EvalJ evalJ, EvalN evalN /* residuals at S.xd -> sc[5], sc[6] */) {
  const int maxIters = 10;
  const double epsx = FLT_EPSILON, epsf = FLT_EPSILON;
  if (lane < 8) S.x[lane] = S.H[lane];
  WSYNC();
  unsigned long long pe = pf_now_if(prof);
  evalJ();
  pf_add(prof, PF_EVAL, pf_now_if(prof) - pe);
  if (lane < 8) S.D[lane] = S.A8[lane * 8 + lane];
  if (lane == 0) { S.sc[2] = 1; S.sc[3] = 0.75; }  // lambda, lc
  WSYNC();
  int iter = 0;
  for (;;) {
    {
      const int i = lane >> 3, j = lane & 7;                 // Ap = A + lambda * diag(D)
      S.Ap[lane] = i == j ? S.A8[lane] + S.sc[2] * S.D[i] : S.A8[lane];
    }
    WSYNC();
    bool solved = false;
    if (S.fast) {
      const unsigned long long pt0 = pf_now_if(prof);
      fast_solve8(lane, S.Ap, S.v, S.d, &S.ib[2]);
      WSYNC();
      solved = S.ib[2] != 0;
      pf_add(prof, PF_SOLVE8, pf_now_if(prof) - pt0);
    }
    if (!solved) eig_solve8_wave(M, lane, S.Ap, S.v, S.d, prof);
    if (lane < 8) S.xd[lane] = S.x[lane] - S.d[lane];
    WSYNC();
    pe = pf_now_if(prof);
    evalN();
    pf_add(prof, PF_EVAL, pf_now_if(prof) - pe);
    // trial residual -> Sd, gain ratio R; lane 0 decides, the (rare) inverse is done by the whole wave
    if (lane == 0) {
      const double Rlo = 0.25, Rhi = 0.75;
      double Sc = S.sc[0];
      double Sd = S.sc[5];
      for (int i = 0; i < 8; i++) {  // tmpd = -A*d + 2*v  (four interleaved partial sums per row)
        const double* a = S.A8 + i * 8;
        const double* d = S.d;
        double s0 = a[0] * d[0] + a[4] * d[4], s1 = a[1] * d[1] + a[5] * d[5], s2 = a[2] * d[2] + a[6] * d[6],
               s3 = a[3] * d[3] + a[7] * d[7];
        S.tmpd[i] = (s0 + s1 + s2 + s3) * -1.0 + S.v[i] * 2.0;
      }
      double dS = dot8(S.d, S.tmpd);
      double R = (Sc - Sd) / (fabs(dS) > DBL_EPSILON ? dS : 1);
      double lambda = S.sc[2], lc = S.sc[3];
      int need_inv = 0;
      double nu = 0;
      if (R > Rhi) {
        lambda *= 0.5;
        if (lambda < lc) lambda = 0;
      } else if (R < Rlo) {
        double t = dot8(S.d, S.v);
        nu = (Sd - Sc) / (fabs(t) > DBL_EPSILON ? t : 1) + 2;
        nu = fmin(fmax(nu, 2.), 10.);
        if (lambda == 0) need_inv = 1;
        else lambda *= nu;
      }
      S.sc[2] = lambda; S.sc[3] = lc; S.sc[4] = nu;
      S.ib[1] = need_inv;
    }
    WSYNC();
    if (S.ib[1]) {
      bool inverted = false;
      if (S.fast) {
        fast_solve8(lane, S.A8, nullptr, S.Inv, &S.ib[2]);      // S.Inv[0] = max |diag(A^-1)|
        WSYNC();
        inverted = S.ib[2] != 0;
        if (inverted && lane == 0) { const double mv = S.Inv[0]; for (int i = 0; i < 8; i++) S.Inv[i * 8 + i] = mv; }
        WSYNC();
      }
      if (!inverted) eig_solve8_wave(M, lane, S.A8, nullptr, S.Inv, prof);
      if (lane == 0) {
        double maxval = DBL_EPSILON;
        for (int i = 0; i < 8; i++) maxval = fmax(maxval, fabs(S.Inv[i * 8 + i]));
        const double lam = 1. / maxval;
        S.sc[3] = lam;                       // lc
        S.sc[2] = lam * (S.sc[4] * 0.5);     // lambda = lc; nu *= 0.5; lambda *= nu
      }
      WSYNC();
    }
    const bool accepted = S.sc[5] < S.sc[0];
    WSYNC();
    if (accepted) {
      if (lane < 8) { const double t = S.x[lane]; S.x[lane] = S.xd[lane]; S.xd[lane] = t; }
      WSYNC();
      pe = pf_now_if(prof);
      evalJ();                                          // residuals / Jacobian at the accepted point (S = Sd again)
      pf_add(prof, PF_EVAL, pf_now_if(prof) - pe);
    }
    iter++;
    // norm(r, INF) of the kept residual, norm(d, INF)
    const double rmax = S.sc[1];
    double dmax = 0;
    for (int i = 0; i < 8; i++) dmax = fmax(dmax, fabs(S.d[i]));
    const bool proceed = iter < maxIters && dmax >= epsx && rmax >= epsf;
    WSYNC();
    if (!proceed) break;
  }
  if (lane < 8) S.H[lane] = S.x[lane];
  WSYNC();
  return iter;
}

#define HB 2048        // displacement-histogram bins held in LDS (larger displacements take the quadratic path)

// LANES: the hypothesis phase gives every LANE its own hypothesis (jacobi_lanes9) instead of every 16-lane row -- the
// fixed-iteration mode, where thousands of hypotheses are evaluated and throughput counts; 23 KB of LDS per wave.
template <int NW, bool LANES>
struct alignas(16) BlockLds {
  RowMat m[LANES ? 1 : NW][NG];
  SolveLds s;
  int hyp[2][LANES ? NW * NL : NW * NG];    // per hypothesis of a chunk: valid << 31 | model << 30 | inlier count (double-buffered)
  double Hsup[9], Hprev[9], Hcur[9];
  int have_prev, gate;
  union {
    struct { unsigned hist[HB]; } h;                       // static filter: population of every displacement bin
    double lmat[LANES ? NW * LM_ELEMS * NL : 1];            // the per-lane matrices (dead when the static filter runs)
  } u;
  unsigned long long red[NW];
};

// ---- lm_eval with the Jacobian, all four waves of the workgroup (round 3).  The sums of J^T J and J^T r are strictly
// sequential over the points (the operator's order), but only their ADDITIONS are: the products are formed ahead by
// another wave.  And most of the products are structural zeros: the x-row of J is (t0 t1 t2 0 0 0 t4 t5), the y-row
// (0 0 0 t0 t1 t2 t6 t7), so of the 36 entries (i <= j) of J^T J  9 have no nonzero product at all, 24 have ONE per
// point (x or y) and only (6,6), (6,7), (7,7) have both.  Adding +-0.0 to a running sum that started at +0.0 never
// changes a bit of it (x + +-0 = x for x != 0, and +0 + -0 = +0), so the zero products are neither formed nor added:
// 46 products per point instead of 88, 16 dependent additions per step instead of 32 for the 24 single entries.
// (Finite terms assumed: 0 * inf would be NaN.  The terms are products of the rows, 1/w and the current parameters;
// parameters that large have already failed the residual tests.)
// Steps of 16 points, one workgroup barrier per step, everything double-buffered:
//   wave 1  terms of the next 64-point tile (every fourth step; its rows are requested one step ahead), max |r| and the
//           pair sums of the squared residuals of that tile
//   wave 2  the 46 products (lane = product) for the 16 points of the NEXT step: all lanes read the same point's terms
//           (10 words: no bank conflict) and write prod[point][46]: 24 singles, then (x, y) of 11 pair entries
//   wave 0  this step's additions of the 24 single entries (lane = entry, one running sum in point order) and, every
//           fourth step, the squared norm (lane 44)
//   wave 3  this step's additions of the pair entries: (6,6), (6,7), (7,7) of J^T J (s += x; s += y) and the 8 entries of
//           J^T r (four interleaved partial sums; their structural zeros are formed and added like any other value)
// Same operations in the same order on every sum.  LDS: the buffers live in what is dead during the refinement -- the
// hypothesis matrices of the other rows / waves and the static filter's histogram.
#define MW_SUB 16                        // points per step
#define MW_NS 24                         // single entries of J^T J
#define MW_NP 11                         // pair entries: 3 of J^T J + 8 of J^T r
#define MW_NPR (MW_NS + 2 * MW_NP)       // products per point
#define MW_PSTR (MW_SUB + 2)              // doubles between two products' rows: [product][point], 144 bytes -> ds_*_b128 of
                                         // neighbouring lanes fall on different bank slots
#define MW_PROD (MW_PSTR * MW_NPR)       // doubles per product buffer
#define MW_MIN_ROWS 512                   // fewer inlier rows: wave 0 alone (measured break-even ~300 rows)
__device__ __forceinline__ int mw_jx(int k) { return k < 3 ? k : k < 6 ? 3 : k - 2; }   // term index of J's x-row, column k
__device__ __forceinline__ int mw_jy(int k) { return k < 3 ? 3 : k < 6 ? k - 3 : k; }   // ... y-row
// the `which`-th entry (i <= j, tri8 order) of the given kind: 1 = x only, 2 = y only (both kinds enumerated together as
// "single"), 0 = none; returns false when there is no such entry
__device__ __forceinline__ bool mw_entry(int which, bool single, int& ei, int& ej, bool& yrow) {
  int cnt = 0;
  bool found = false;
  for (int e = 0; e < 36; e++) {
    int i, j;
    tri8(e, i, j);
    const bool cx = !(i >= 3 && i < 6) && !(j >= 3 && j < 6), cy = i >= 3 && j >= 3;
    const bool is_single = cx != cy, is_none = !cx && !cy;
    if (single ? is_single : is_none) {
      if (cnt == which) { ei = i; ej = j; yrow = cy; found = true; }
      cnt++;
    }
  }
  return found;
}
template <int NW, bool LANES>
__device__ __forceinline__ void lm_eval_mw(BlockLds<NW, LANES>& B, int wave, int lane, const float* rows, int count,
                                           unsigned long long* prof) {
  static_assert(NW == 4 && !LANES, "helper waves: the four-wave row form only");
  static_assert(sizeof(RowMat) * (NW * NG - 1) >= sizeof(double) * (MW_PROD + NL * TS) + 16, "buffer 0 + second tile");
  static_assert(sizeof(B.u) >= sizeof(double) * MW_PROD + 16, "buffer 1");
  static_assert(NL * TS >= 10 * TT, "a tile of terms, term-major");
  static_assert(alignof(BlockLds<NW, LANES>) >= 16, "16-byte LDS accesses below");
  SolveLds& S = B.s;
  // (selects, not arrays of pointers: an indexed pointer array loses the LDS address space and turns every access into
  // a FLAT instruction -- measured 3x slower)
  // every buffer starts on a 16-byte boundary (the struct is 16-byte aligned; an odd multiple of 8 is skipped by one double)
  typedef BlockLds<NW, LANES> BL;
  double* const prod0 = reinterpret_cast<double*>(&B.m[0][1]) + ((offsetof(BL, m) + sizeof(RowMat)) % 16 ? 1 : 0);
  double* const prod1 = reinterpret_cast<double*>(&B.u) + (offsetof(BL, u) % 16 ? 1 : 0);
  double* const Tb0 = S.T + ((offsetof(BL, s) + offsetof(SolveLds, T)) % 16 ? 1 : 0);
  double* const Tb1 = prod0 + MW_PROD;
  static_assert(MW_PROD % 2 == 0 && MW_PSTR % 2 == 0 && TT % 2 == 0 && MW_SUB % 2 == 0, "16-byte rows");
#define MW_PRODBUF(i) (((i) & 1) ? prod1 : prod0)
#define MW_TERMBUF(i) (((i) & 1) ? Tb1 : Tb0)
  const int nsub = (count + MW_SUB - 1) / MW_SUB;
  double h0 = 0, h1 = 0, h2 = 0, h3 = 0, h4 = 0, h5 = 0, h6 = 0, h7 = 0;
  if (wave == 1) { h0 = S.x[0]; h1 = S.x[1]; h2 = S.x[2]; h3 = S.x[3]; h4 = S.x[4]; h5 = S.x[5]; h6 = S.x[6]; h7 = S.x[7]; }
  // wave 2: the two term indices of this lane's product.  wave 0: where this lane's sum goes in A8 (lanes 24..32: the
  // entries that are zero by structure).  wave 3: lanes 0..2 = (6,6), (6,7), (7,7); lanes 3..10 = J^T r entry lane - 3.
  int ia = 3, ib = 3, a8i = -1, a8j = -1;
  if (wave == 2) {
    if (lane < MW_NS) {
      int ei = 0, ej = 0; bool yrow = false;
      mw_entry(lane, true, ei, ej, yrow);
      ia = yrow ? mw_jy(ei) : mw_jx(ei); ib = yrow ? mw_jy(ej) : mw_jx(ej);
    } else if (lane < MW_NPR) {
      const int u = (lane - MW_NS) >> 1;
      const bool yrow = (lane - MW_NS) & 1;
      if (u < 3) {
        const int ei = u == 2 ? 7 : 6, ej = u == 0 ? 6 : 7;
        ia = yrow ? mw_jy(ei) : mw_jx(ei); ib = yrow ? mw_jy(ej) : mw_jx(ej);
      } else {
        ia = yrow ? mw_jy(u - 3) : mw_jx(u - 3); ib = yrow ? 9 : 8;
      }
    }
  } else if (wave == 0) {
    bool yrow = false;
    if (lane < MW_NS) mw_entry(lane, true, a8i, a8j, yrow);
    else if (lane < MW_NS + 9) mw_entry(lane - MW_NS, false, a8i, a8j, yrow);
  } else if (wave == 3 && lane < 3) {
    a8i = lane == 2 ? 7 : 6; a8j = lane == 0 ? 6 : 7;
  }
  double s = 0, s0 = 0, s1 = 0, s2 = 0, s3 = 0, nrm = 0, rmax = 0;
  float4 rnext = make_float4(0, 0, 0, 0);
  unsigned long long pf_busy = 0, pf_wait = 0;       // cycle accounting: summed in registers, one atomic per pass
  for (int k = -2; k < nsub; k++) {
    const unsigned long long pm0 = pf_now_if(prof);
    if (wave == 1) {
      // rows of the tile whose terms are due at the next step (or now, for the first tile)
      if (k == -2 || ((k + 3) & 3) == 0) {
        const int i = ((k + 3) >> 2) * NL + lane;
        if (i < count) rnext = *reinterpret_cast<const float4*>(rows + 4 * i);
      }
      if (((k + 2) & 3) == 0 && ((k + 2) >> 2) * NL < count) {
        const int n = (k + 2) >> 2, c0 = n * NL, i = c0 + lane;
        double q0 = 0, q1 = 0;
        if (i < count) {
          const float4 r = rnext;
          const double Mx = r.x, My = r.y;
          double ww = h6 * Mx + h7 * My + 1.;
          ww = fabs(ww) > DBL_EPSILON ? 1. / ww : 0;
          const double xi = (h0 * Mx + h1 * My + h2) * ww;
          const double yi = (h3 * Mx + h4 * My + h5) * ww;
          const double rx = xi - r.z, ry = yi - r.w;
          double* t = MW_TERMBUF(n) + lane;                          // term j of this point at t[j * TT]
          t[8 * TT] = rx; t[9 * TT] = ry;
          t[0] = Mx * ww; t[TT] = My * ww; t[2 * TT] = ww; t[3 * TT] = 0.0;
          t[4 * TT] = -Mx * ww * xi; t[5 * TT] = -My * ww * xi; t[6 * TT] = -Mx * ww * yi; t[7 * TT] = -My * ww * yi;
          rmax = fmax(rmax, fabs(rx));
          rmax = fmax(rmax, fabs(ry));
          q0 = rx * rx; q1 = ry * ry;
        }
        const int cnt = min(NL, count - c0);
        const double n0 = __shfl_down(q0, 1), n1 = __shfl_down(q1, 1);
        if (!(lane & 1)) {
          if (lane + 1 < cnt) S.P2[lane >> 1] = ((q0 + q1) + n0) + n1;
          else if (lane < cnt) { S.P2[NL / 2] = q0; S.P2[NL / 2 + 1] = q1; }
        }
      }
    } else if (wave == 0) {
      if (k >= 0 && lane < MW_NS) {
        const double* r = MW_PRODBUF(k) + lane * MW_PSTR;               // this entry's products of the step's 16 points
        const int cnt = min(MW_SUB, count - k * MW_SUB);
        if (cnt == MW_SUB) {
          // all words requested before the first addition (left alone the compiler waits for every read in turn); two
          // points per ds_read_b128 (a quarter of the LDS cycles of the 8-byte reads: this loop was LDS-issue bound)
          d2_t v[MW_SUB / 2];
#pragma unroll
          for (int q = 0; q < MW_SUB / 2; q++) v[q] = *reinterpret_cast<const d2_t*>(r + 2 * q);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int q = 0; q < MW_SUB / 2; q++) { s += v[q].x; s += v[q].y; }
        } else {
          for (int q = 0; q < cnt; q++) s += r[q];
        }
      }
      // the squared norm of tile n (pair sums left by wave 1 one step ago), in order, by a lane with nothing else to do
      if (((k + 1) & 3) == 0 && ((k + 1) >> 2) * NL < count && lane == 44) {
        const int cnt = min(NL, count - ((k + 1) >> 2) * NL);
        nrm = add_in_order(nrm, S.P2, cnt >> 1);
        if (cnt & 1) { nrm += S.P2[NL / 2]; nrm += S.P2[NL / 2 + 1]; }
      }
    } else if (wave == 3) {
      if (k >= 0 && lane < MW_NP) {
        const double* rx = MW_PRODBUF(k) + (MW_NS + 2 * lane) * MW_PSTR;  // x products of the 16 points; y: the next row
        const double* ry = rx + MW_PSTR;
        const int cnt = min(MW_SUB, count - k * MW_SUB);
        if (cnt == MW_SUB) {
          d2_t vx[MW_SUB / 2], vy[MW_SUB / 2];
#pragma unroll
          for (int q = 0; q < MW_SUB / 2; q++) { vx[q] = *reinterpret_cast<const d2_t*>(rx + 2 * q); vy[q] = *reinterpret_cast<const d2_t*>(ry + 2 * q); }
          __builtin_amdgcn_sched_barrier(0);
          if (lane < 3) {
#pragma unroll
            for (int q = 0; q < MW_SUB / 2; q++) { s += vx[q].x; s += vy[q].x; s += vx[q].y; s += vy[q].y; }
          } else {
#pragma unroll
            for (int q = 0; q < MW_SUB / 2; q++) { s0 += vx[q].x; s1 += vy[q].x; s2 += vx[q].y; s3 += vy[q].y; }
          }
        } else {
          int q = 0;
          for (; q + 1 < cnt; q += 2) {
            const double a = rx[q], b = ry[q], c = rx[q + 1], d = ry[q + 1];
            if (lane < 3) { s += a; s += b; s += c; s += d; }
            else { s0 += a; s1 += b; s2 += c; s3 += d; }
          }
          if (q < cnt) {
            const double a = rx[q], b = ry[q];
            if (lane < 3) { s += a; s += b; }
            else { s0 += a; s0 += b; }
          }
        }
      }
    } else {
      const int sub = k + 1;
      if (sub >= 0 && sub < nsub && lane < MW_NPR) {
        const double* t = MW_TERMBUF(sub >> 2) + (sub & 3) * MW_SUB;     // term j of the step's point q at t[j * TT + q]
        double* out = MW_PRODBUF(sub) + lane * MW_PSTR;
        const int cnt = min(MW_SUB, count - sub * MW_SUB);
        if (cnt == MW_SUB) {
          d2_t va[MW_SUB / 2], vb[MW_SUB / 2];
#pragma unroll
          for (int q = 0; q < MW_SUB / 2; q++) {
            va[q] = *reinterpret_cast<const d2_t*>(t + ia * TT + 2 * q);
            vb[q] = *reinterpret_cast<const d2_t*>(t + ib * TT + 2 * q);
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int q = 0; q < MW_SUB / 2; q++) {
            d2_t pr; pr.x = va[q].x * vb[q].x; pr.y = va[q].y * vb[q].y;
            *reinterpret_cast<d2_t*>(out + 2 * q) = pr;
          }
        } else {
          for (int q = 0; q < cnt; q++) out[q] = t[ia * TT + q] * t[ib * TT + q];
        }
      }
    }
    const unsigned long long pm1 = pf_now_if(prof);
    __syncthreads();
    pf_busy += pm1 - pm0; pf_wait += pf_now_if(prof) - pm1;
  }
  pf_add_wave(prof, PF_MW_W0 + wave, pf_busy);
  if (wave == 0) { pf_add(prof, PF_MW_WAIT, pf_wait); pf_add(prof, PF_MW_STEPS, nsub + 2); }
  if (wave == 0 && a8i >= 0) { S.A8[a8i * 8 + a8j] = s; S.A8[a8j * 8 + a8i] = s; }      // (s = 0 for the structural zeros)
  if (wave == 0 && lane == 44) S.sc[0] = nrm;
  if (wave == 3 && lane < 3) { S.A8[a8i * 8 + a8j] = s; S.A8[a8j * 8 + a8i] = s; }
  if (wave == 3 && lane >= 3 && lane < MW_NP) S.v[lane - 3] = (s0 + s1 + s2 + s3) * 1.0;
  if (wave == 1) {
    for (int sft = 32; sft > 0; sft >>= 1) rmax = fmax(rmax, __shfl_xor(rmax, sft));
    if (lane == 44) S.sc[1] = rmax;
  }
  __syncthreads();
#undef MW_PRODBUF
#undef MW_TERMBUF
}

// ---- the pass WITHOUT the Jacobian (the trial point of every LM iteration: squared norm and max |r| only) on two waves:
// wave 1 computes the residuals of the next 64-point tile and their pair sums (rows requested a tile ahead), wave 0's
// lane 44 adds the pair sums of the present tile in order; one workgroup barrier per tile, two pair-sum buffers.
template <int NW, bool LANES>
__device__ __forceinline__ void lm_eval_noj_mw(BlockLds<NW, LANES>& B, int wave, int lane, const float* rows, int count) {
  static_assert(NW == 4 && !LANES, "helper waves: the four-wave row form only");
  SolveLds& S = B.s;
  double* const Pa = S.P2;
  double* const Pb = reinterpret_cast<double*>(&B.m[0][1]);         // dead during the refinement (see lm_eval_mw)
#define MW_P2BUF(i) (((i) & 1) ? Pb : Pa)
  const int ntile = (count + NL - 1) / NL;
  double h0 = 0, h1 = 0, h2 = 0, h3 = 0, h4 = 0, h5 = 0, h6 = 0, h7 = 0;
  if (wave == 1) { h0 = S.xd[0]; h1 = S.xd[1]; h2 = S.xd[2]; h3 = S.xd[3]; h4 = S.xd[4]; h5 = S.xd[5]; h6 = S.xd[6]; h7 = S.xd[7]; }
  double nrm = 0, rmax = 0;
  float4 rnext = make_float4(0, 0, 0, 0);
  if (wave == 1 && lane < count) rnext = *reinterpret_cast<const float4*>(rows + 4 * lane);
  for (int n = -1; n < ntile; n++) {
    if (wave == 1 && n + 1 < ntile) {
      const int c0 = (n + 1) * NL, i = c0 + lane;
      const float4 r = rnext;
      if (i + NL < count) rnext = *reinterpret_cast<const float4*>(rows + 4 * (i + NL));
      double q0 = 0, q1 = 0;
      if (i < count) {
        const double Mx = r.x, My = r.y;
        double ww = h6 * Mx + h7 * My + 1.;
        ww = fabs(ww) > DBL_EPSILON ? 1. / ww : 0;
        const double xi = (h0 * Mx + h1 * My + h2) * ww;
        const double yi = (h3 * Mx + h4 * My + h5) * ww;
        const double rx = xi - r.z, ry = yi - r.w;
        rmax = fmax(rmax, fabs(rx));
        rmax = fmax(rmax, fabs(ry));
        q0 = rx * rx; q1 = ry * ry;
      }
      const int cnt = min(NL, count - c0);
      const double n0 = __shfl_down(q0, 1), n1 = __shfl_down(q1, 1);
      double* P = MW_P2BUF(n + 1);
      if (!(lane & 1)) {
        if (lane + 1 < cnt) P[lane >> 1] = ((q0 + q1) + n0) + n1;
        else if (lane < cnt) { P[NL / 2] = q0; P[NL / 2 + 1] = q1; }
      }
    } else if (wave == 0 && n >= 0 && lane == 44) {
      const int cnt = min(NL, count - n * NL);
      const double* P = MW_P2BUF(n);
      nrm = add_in_order(nrm, P, cnt >> 1);
      if (cnt & 1) { nrm += P[NL / 2]; nrm += P[NL / 2 + 1]; }
    }
    __syncthreads();
  }
#undef MW_P2BUF
  if (wave == 0 && lane == 44) S.sc[5] = nrm;
  if (wave == 1) {
    for (int sft = 32; sft > 0; sft >>= 1) rmax = fmax(rmax, __shfl_xor(rmax, sft));
    if (lane == 44) S.sc[6] = rmax;
  }
  __syncthreads();
}

// The helper waves (1..NW-1) of a workgroup while wave 0 refines: they sleep at the workgroup barrier until wave 0 posts a
// command in S.ib[4] (1: one lm_eval_mw pass over S.ib[5] rows of `crow`; 2: one lm_eval_noj_mw pass; 0: done).
template <int NW, bool LANES>
__device__ __forceinline__ void lm_helper_loop(BlockLds<NW, LANES>& B, int wave, int lane, const float* crow, unsigned long long* prof) {
  if constexpr (NW == 4 && !LANES) {
    for (;;) {
      __syncthreads();
      const int cmd = B.s.ib[4];
      if (cmd == 0) break;
      if (cmd == 1) lm_eval_mw<NW, LANES>(B, wave, lane, crow, B.s.ib[5], prof);
      else lm_eval_noj_mw<NW, LANES>(B, wave, lane, crow, B.s.ib[5]);
    }
  }
}
}  // namespace
