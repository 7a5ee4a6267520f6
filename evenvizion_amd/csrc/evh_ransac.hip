// evh_ransac.hip -- RANSAC + DLT + Levenberg-Marquardt homography estimation and the reference's point filters
// around it, for gfx950.  Replaces cv2.findHomography(a, b, cv2.RANSAC, 3.0) (reference call sites
// evenvizion/processing/matching.py:156-157 and utils.py:356-358) and the glue find_point_displacement /
// get_largest_group_points (utils.py:258-325), compute_homography (utils.py:328-363), matrix_superposition
// (utils.py:118-145).
//
// Shape of the computation.  One workgroup of NW wavefronts per frame pair (or per stream in the sequential scan).
// * RANSAC hypotheses are evaluated a chunk at a time: every 16-lane row of every wave owns one 4-point hypothesis
//   (4 * NW per chunk), or -- when the caller forces the iteration count -- every LANE does (64 * NW per chunk).  The
//   sample sequence of the fixed-seed multiply-with-carry generator is advanced by every lane identically (scalar
//   code), each owner keeps its own quadruple, solves its normalised DLT (9x9 Jacobi eigen-solver, f64) and counts its
//   inliers; a sequential replay in sample order then applies "strictly more inliers wins" and the adaptive iteration
//   bound exactly like a serial RANSAC (over-evaluated hypotheses are simply ignored).
// * The eigen-solver is the latency-critical piece: measured on this part (tools/ubench/lat.hip) a dependent f64 divide
//   costs 69 cycles, a square root 106, an LDS round trip 65-125 and a lone wave issues one instruction per ~5 cycles.
//   Three forms of the same arithmetic (same pivot order, bit-identical results):
//     jacobi_rows  -- one matrix per 16-lane row, four per wave (hypothesis chunks): pivot candidates in registers,
//                     pivot search and the four index rescans as DPP integer reductions on the raw bits of |a_ij|,
//                     rotated values rescanned before they leave registers;
//     jacobi_one   -- one matrix for the whole wave (refit, LM solves): pivot through SGPRs, W in registers, the two
//                     rescans side by side, results exchanged by v_permlane16_swap;
//     jacobi_lanes9 -- one matrix per lane (fixed-iteration mode): the serial algorithm, A and W in LDS as
//                     [element][lane], V in an L2-resident global scratch.
//   The c/s/t scalars of a rotation use the exact divide / square-root instruction sequences without the range
//   scaling they cannot need here (one check per solve; out-of-range input takes a plain-arithmetic sweep).
// * Sums over points (centroids, L^T L, J^T J, J^T r, residual norms) keep the serial summation order of the operator
//   being replaced: the points go through a 64-point LDS tile (all lanes compute their own point's terms), then one
//   lane per output entry adds the tile's terms in point order.
// All floating-point sums keep a fixed order (-ffp-contract=off); f64 throughout the solves, f32 for the
// reprojection error, as the operator being replaced.
// One translation unit in layers, each header including only the one before it: evh_ransac_wave.h (wave primitives),
// _eig.h (Jacobi forms, LDL^T), _dlt.h (DLT forms), _lm.h (LM refinement, BlockLds); this file: sampling, block routines,
// kernels, launchers.
#include "evh_devmath.h"
#include "evh_internal.h"
#include "evh_ransac.h"
#include "evh_ransac_lm.h"
#include <stdio.h>
#include <stdlib.h>

namespace {

struct Rng {  // multiply-with-carry generator, seeded with all ones for every findHomography call
  unsigned long long state;
  __device__ Rng() : state(0xFFFFFFFFFFFFFFFFull) {}
  __device__ unsigned next() {
    state = (unsigned long long)(unsigned)state * 4164903690u + (unsigned)(state >> 32);
    return (unsigned)state;
  }
};
// x % n for 32-bit x through the 64-bit reciprocal M = ceil(2^64 / n): floor(x * M / 2^64) == x / n for every 32-bit x
struct FastMod {
  unsigned n, mlo, mhi;
  __device__ explicit FastMod(unsigned n_) : n(n_) {
    const unsigned long long M = 0xFFFFFFFFFFFFFFFFull / n_ + 1ull;
    mlo = (unsigned)M; mhi = (unsigned)(M >> 32);
  }
  __device__ __forceinline__ unsigned mod(unsigned x) const {
    const unsigned long long t = (unsigned long long)x * mhi + __umulhi(x, mlo);
    return x - (unsigned)(t >> 32) * n;
  }
};
// four distinct indices, a duplicate is redrawn (getSubset's inner loop, straight-line)
__device__ __forceinline__ int4 draw_quad(Rng& rng, const FastMod& fm) {
  const int q0 = (int)fm.mod(rng.next());
  int q1, q2, q3;
  do q1 = (int)fm.mod(rng.next()); while (q1 == q0);
  do q2 = (int)fm.mod(rng.next()); while (q2 == q0 || q2 == q1);
  do q3 = (int)fm.mod(rng.next()); while (q3 == q0 || q3 == q1 || q3 == q2);
  return make_int4(q0, q1, q2, q3);
}

__device__ __forceinline__ bool have_collinear4(const float* px, const float* py) {
  const int i = 3;
  for (int j = 0; j < i; j++) {
    double dx1 = px[j] - px[i];
    double dy1 = py[j] - py[i];
    for (int k = 0; k < j; k++) {
      double dx2 = px[k] - px[i];
      double dy2 = py[k] - py[i];
      if (fabs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2))) return true;
    }
  }
  return false;
}

__device__ __forceinline__ double det3(const float* px, const float* py, int t0, int t1, int t2) {
  double a00 = px[t0], a01 = py[t0], a02 = 1., a10 = px[t1], a11 = py[t1], a12 = 1., a20 = px[t2], a21 = py[t2],
         a22 = 1.;
  return a00 * (a11 * a22 - a21 * a12) - a01 * (a10 * a22 - a20 * a12) + a02 * (a10 * a21 - a20 * a11);
}

__device__ __forceinline__ bool check_subset4(const float* Mx, const float* My, const float* mx, const float* my) {
  if (have_collinear4(Mx, My) || have_collinear4(mx, my)) return false;
  const int tt[4][3] = {{0, 1, 2}, {1, 2, 3}, {0, 2, 3}, {0, 1, 3}};
  int negative = 0;
#pragma unroll
  for (int i = 0; i < 4; i++)
    negative += (det3(Mx, My, tt[i][0], tt[i][1], tt[i][2]) * det3(mx, my, tt[i][0], tt[i][1], tt[i][2]) < 0) ? 1 : 0;
  return negative == 0 || negative == 4;
}

__device__ __forceinline__ bool is_inlier(const float* Hf, float Mx, float My, float mx, float my, float t) {
  float ww = 1.f / ((Hf[6] * Mx + Hf[7] * My) + 1.f);
  float dx = ((Hf[0] * Mx + Hf[1] * My) + Hf[2]) * ww - mx;
  float dy = ((Hf[3] * Mx + Hf[4] * My) + Hf[5]) * ww - my;
  float err = dx * dx + dy * dy;
  return err <= t;
}

__device__ int update_num_iters(double p, double ep, int modelPoints, int maxIters) {
  p = fmax(p, 0.); p = fmin(p, 1.);
  ep = fmax(ep, 0.); ep = fmin(ep, 1.);
  double num = fmax(1. - p, DBL_MIN);
  double denom = 1. - pow(1. - ep, (double)modelPoints);
  if (denom < DBL_MIN) return 0;
  num = log(num);
  denom = log(denom);
  return denom >= 0 || -num >= maxIters * (-denom) ? maxIters : (int)__builtin_rint(num / denom);
}

// result word of one evaluated sample: valid << 31 | model << 30 | inlier count (the readers return the bits as they are,
// not bool: with bool the replay loop of find_homography_block compiled to different code)
__device__ __forceinline__ unsigned hyp_pack(bool valid, bool model, int count) { return (valid ? 0x80000000u : 0u) | (model ? 0x40000000u : 0u) | (unsigned)count; }
__device__ __forceinline__ unsigned hyp_valid(unsigned e) { return e >> 31; }
__device__ __forceinline__ unsigned hyp_model(unsigned e) { return (e >> 30) & 1u; }
__device__ __forceinline__ unsigned hyp_count(unsigned e) { return e & 0x3FFFFFFFu; }

// Hypotheses of one RANSAC call that were evaluated ahead of it by other workgroups (k_scan_hyp: the fixed-iteration
// stream scan spreads the 2000 samples of a pair over ~140 workgroups; only the replay below is serial).
struct ScanPre {
  const int* hyp;                  // [count] result words (hyp_pack), in sample order
  const double* H;                 // [count][9] the models
  int count;                       // < 10000
  unsigned long long rng_after;    // generator state after `count` quadruples
};

// ---- cv2.findHomography(a, b, RANSAC, thr) on `n` rows; result in B.s.H (LDS), mask[n] in global.  All NW*64
// threads of the workgroup call this; the return value is uniform.  scratch: crow = float rows [n][4] for the
// compacted inliers.  Ends with a workgroup barrier.
template <int NW, bool LANES>
__device__ __forceinline__ bool find_homography_block(BlockLds<NW, LANES>& B, const float* rows, int n, double thr, int maxItersArg, double conf,
                                      int force_max, uint8_t* mask, float* crow, int* info, unsigned long long* prof,
                                      double* lane_v /* LANES: this workgroup's NW * 81 * 64 doubles of global scratch */,
                                      const ScanPre* pre = nullptr /* force_max only */) {
  const unsigned long long pf0 = pf_now_if(prof);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, row = lane >> 4, gl = lane & 15;
  SolveLds& S = B.s;
  if (info && tid < 3) info[tid] = 0;
  for (int i = tid; i < n; i += NW * NL) mask[i] = 0;
  if (thr <= 0) thr = 3;
  if (n < 4) { __threadfence_block(); __syncthreads(); return false; }
  if (n == 4) {
    if (wave == 0) {
      const bool ok = dlt_rows(S, B.m[0][0], lane, rows, 4, S.H);
      if (lane == 0) S.ib[2] = ok ? 1 : 0;
      if (ok && lane < 4) mask[lane] = 1;
      if (ok && info && lane == 0) info[1] = 4;
    }
    __threadfence_block();
    __syncthreads();
    return S.ib[2] != 0;
  }
  const float t = (float)(thr * thr);
  constexpr int HC = LANES ? NW * NL : NW * NG;             // hypotheses per chunk
  const int myh = LANES ? wave * NL + lane : wave * NG + row;
  Rng rng;
  const FastMod fm((unsigned)n);
  int niters = max(maxItersArg, 1), maxGood = 0, iter = 0, run = 0, chunk = 0;
  bool stop = false;
  if (pre) {
    // Replay of the samples evaluated ahead, 64 at a time.  With the iteration count fixed the serial rule of the
    // chunk loop below reduces to: the samples that count are the valid ones among the first `niters` valid ones, the
    // winner is the FIRST of them with the largest inlier count (> 3); `run` = trailing rejected samples.
    int lastvalid = -1;
    unsigned long long bestkey = 0ull;
    for (int c0 = 0; c0 < pre->count; c0 += NL) {
      const int h = c0 + lane;
      const unsigned e = h < pre->count ? (unsigned)pre->hyp[h] : 0u;
      const bool v = hyp_valid(e) != 0u;
      const unsigned long long vb = __ballot(v);
      const int before = iter + __popcll(vb & ((1ull << lane) - 1ull));
      if (v && before < niters && hyp_model(e) && hyp_count(e) > 3u) {
        const unsigned long long key = ((unsigned long long)hyp_count(e) << 32) | (0xFFFFFFFFu - (unsigned)h);
        bestkey = key > bestkey ? key : bestkey;
      }
      if (__ballot(v && before >= niters) != 0ull) stop = true;
      iter = min(iter + (int)__popcll(vb), niters);
      if (vb) lastvalid = c0 + 63 - __clzll((long long)vb);
    }
    bestkey = wave_max_u64(bestkey);
    run = pre->count - 1 - lastvalid;
    if (bestkey) {
      maxGood = (int)(bestkey >> 32);
      const int bh = (int)(0xFFFFFFFFu - (unsigned)bestkey);
      if (tid < 9) S.bestH[tid] = pre->H[9 * (int64_t)bh + tid];
    }
    rng.state = pre->rng_after;
  }
  while (!stop && iter < niters) {
    // every lane advances the generator identically through HC quadruples; the lanes of hypothesis h keep quadruple #h
    const unsigned long long pr0 = pf_now_if(prof);
    int my[4] = {0, 1, 2, 3};
    for (int h = 0; h < HC; h++) {
      const int4 q = draw_quad(rng, fm);
      if (h == myh) { my[0] = q.x; my[1] = q.y; my[2] = q.z; my[3] = q.w; }
    }
    float Mx[4], My[4], mx[4], my_[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const float4 r = *reinterpret_cast<const float4*>(rows + 4 * my[i]);
      Mx[i] = r.x; My[i] = r.y; mx[i] = r.z; my_[i] = r.w;
    }
    const bool valid = check_subset4(Mx, My, mx, my_);
    double H[9];
    const unsigned long long ps0 = pf_now_if(prof);
    pf_add(prof, PF_RNG, ps0 - pr0);
    bool ok;
    if constexpr (LANES) ok = dlt4_lane(B.u.lmat + (wave * LM_ELEMS * NL + lane), lane_v + (wave * LV_ELEMS * NL + lane), valid, Mx, My, mx, my_, H);
    else ok = dlt4_rows(B.m[wave][row], lane, valid, Mx, My, mx, my_, H);
    const unsigned long long ps1 = pf_now_if(prof);
    pf_add(prof, PF_SETUP, ps1 - ps0);
    int good = 0;
    {
      float Hf[8];
#pragma unroll
      for (int i = 0; i < 8; i++) Hf[i] = ok ? (float)H[i] : 0.f;
      if constexpr (LANES) {   // every lane walks all points (same addresses across the wave: one transaction each)
        if (__ballot(ok) != 0ull) {
#pragma unroll 4
          for (int i = 0; i < n; i++) {
            const float4 r = *reinterpret_cast<const float4*>(rows + 4 * i);
            good += is_inlier(Hf, r.x, r.y, r.z, r.w, t) ? 1 : 0;
          }
        }
        if (!ok) good = 0;
      } else {
        if (ok) {   // the 16 lanes of the row split the points; integer count, order-free
#pragma unroll 4
          for (int i = gl; i < n; i += GL) {
            const float4 r = *reinterpret_cast<const float4*>(rows + 4 * i);
            good += is_inlier(Hf, r.x, r.y, r.z, r.w, t) ? 1 : 0;
          }
        }
        good = rsum16(good);
      }
    }
    int* hyp = B.hyp[chunk & 1];
    if (LANES || gl == 0) hyp[myh] = hyp_pack(valid, ok, good);
    const unsigned long long ps2 = pf_now_if(prof);
    pf_add(prof, PF_COUNT, ps2 - ps1);
    __syncthreads();
    const unsigned long long ps3 = pf_now_if(prof);
    pf_add(prof, PF_BARRIER, ps3 - ps2);
    // sequential replay in sample order (every thread, identically); the chunk's entries are fetched once into
    // registers (lane j holds entries j, j + 64, ...) and walked with v_readlane instead of one LDS round trip each
    constexpr int NSEG = (HC + NL - 1) / NL;
    unsigned er[NSEG];
#pragma unroll
    for (int sg = 0; sg < NSEG; sg++) er[sg] = sg * NL + lane < HC ? (unsigned)hyp[sg * NL + lane] : 0u;
    int best_h = -1;
#pragma unroll
    for (int sg = 0; sg < NSEG; sg++)
    for (int hj = 0; hj < (HC - sg * NL < NL ? HC - sg * NL : NL) && !stop; hj++) {
      const int h = sg * NL + hj;
      const unsigned e = (unsigned)__builtin_amdgcn_readlane((int)er[sg], hj);
      if (!hyp_valid(e)) {  // rejected sample: counts towards the 10000-attempt bound of one draw
        if (++run >= 10000) { stop = true; break; }
        continue;
      }
      run = 0;
      if (iter >= niters) { stop = true; break; }
      iter++;
      if (!hyp_model(e)) continue;
      const int g = (int)hyp_count(e);
      if (g > max(maxGood, 3)) {
        maxGood = g;
        best_h = h;
        if (!force_max) niters = update_num_iters(conf, (double)(n - g) / n, 4, niters);
      }
    }
    if (best_h == myh && (LANES || gl == 0)) {
#pragma unroll
      for (int i = 0; i < 9; i++) S.bestH[i] = H[i];
    }
    chunk++;
    pf_add(prof, PF_REPLAY, pf_now_if(prof) - ps3);
  }
  __threadfence_block();
  __syncthreads();
  const unsigned long long pf1 = pf_now_if(prof);
  pf_add(prof, PF_CALLS, 1); pf_add(prof, PF_HYP, pf1 - pf0); pf_add(prof, PF_CHUNKS, chunk);
  if (info && tid == 0) { info[0] = iter; info[1] = maxGood; }
  if (maxGood <= 0) return false;
  if (wave == 0) {
    // inlier mask of the winning hypothesis + ordered compaction of its inliers
    float Hf[8];
#pragma unroll
    for (int i = 0; i < 8; i++) Hf[i] = (float)S.bestH[i];
    int ni = 0;
    for (int c0 = 0; c0 < n; c0 += NL) {
      const int i = c0 + lane;
      bool in = false;
      float4 r = make_float4(0, 0, 0, 0);
      if (i < n) {
        r = *reinterpret_cast<const float4*>(rows + 4 * i);
        in = is_inlier(Hf, r.x, r.y, r.z, r.w, t);
        mask[i] = in ? 1 : 0;
      }
      const unsigned long long mm = __ballot(in);
      if (in) *reinterpret_cast<float4*>(crow + 4 * (ni + __popcll(mm & ((1ull << lane) - 1ull)))) = r;
      ni += __popcll(mm);
    }
    __threadfence_block();
    WSYNC();
    if (lane < 9) S.H[lane] = S.bestH[lane];
    WSYNC();
    const unsigned long long pf2 = pf_now_if(prof);
    pf_add(prof, PF_COMPACT, pf2 - pf1);
    if (ni > 0) {
      dlt_rows(S, B.m[0][0], lane, crow, ni, S.H, prof);  // keeps the RANSAC model when the refit is degenerate
      const unsigned long long pf3 = pf_now_if(prof);
      pf_add(prof, PF_REFIT, pf3 - pf2);
      int it;
      if constexpr (NW == 4 && !LANES) {
        // the passes with the Jacobian run on all four waves: post the command, meet the helpers at the barrier
        // (from MW_MIN_ROWS rows on: below that the extra barriers cost what the helpers save)
        it = lm_refine(S, B.m[0][0], lane, crow, ni, prof, [&]() {
          if (S.fast) { lm_eval_fast(S, lane, crow, ni, S.x, true, 0, 1); return; }
          if (ni < MW_MIN_ROWS) { lm_eval(S, lane, crow, ni, S.x, true, 0, 1); return; }
          if (lane == 0) { S.ib[4] = 1; S.ib[5] = ni; }
          __threadfence_block();
          __syncthreads();
          lm_eval_mw<NW, LANES>(B, 0, lane, crow, ni, prof);
        }, [&]() {
          if (S.fast) { lm_eval_fast(S, lane, crow, ni, S.xd, false, 5, 6); return; }
          if (ni < MW_MIN_ROWS) { lm_eval(S, lane, crow, ni, S.xd, false, 5, 6); return; }
          if (lane == 0) { S.ib[4] = 2; S.ib[5] = ni; }
          __threadfence_block();
          __syncthreads();
          lm_eval_noj_mw<NW, LANES>(B, 0, lane, crow, ni);
        });
      } else {
        it = lm_refine(S, B.m[0][0], lane, crow, ni, prof,
                       [&]() { if (S.fast) lm_eval_fast(S, lane, crow, ni, S.x, true, 0, 1); else lm_eval(S, lane, crow, ni, S.x, true, 0, 1); },
                       [&]() { if (S.fast) lm_eval_fast(S, lane, crow, ni, S.xd, false, 5, 6); else lm_eval(S, lane, crow, ni, S.xd, false, 5, 6); });
      }
      pf_add(prof, PF_LM, pf_now_if(prof) - pf3); pf_add(prof, PF_LM_ITERS, it);
      if (info && lane == 0) info[2] = it;
    }
    if constexpr (NW == 4 && !LANES) {
      if (lane == 0) S.ib[4] = 0;                          // release the helpers
      __threadfence_block();
      __syncthreads();
    }
  } else {
    lm_helper_loop<NW, LANES>(B, wave, lane, crow, prof);
  }
  __threadfence_block();
  __syncthreads();
  pf_add(prof, PF_TOTAL, pf_now_if(prof) - pf0);
  return true;
}

// find_point_displacement + get_largest_group_points; rbin = scratch of 16 bytes per row (global, 8-byte aligned): an int
// bin per row and, behind them, the rounded displacement per row as a double for the quadratic path; returns kept count
// (uniform).  All threads of the workgroup; ends with a workgroup barrier.
template <int NW, bool LANES>
__device__ __forceinline__ int static_filter_block(BlockLds<NW, LANES>& B, const double* H /*LDS*/, const float* rows, int n, int* rbin,
                                   float* out) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, NT = NW * NL;
  for (int i = tid; i < HB; i += NT) B.u.h.hist[i] = 0u;
  __syncthreads();
  // round(displacement) of row i: Python round(), half to even, as a double -- a Python int has no upper bound, and a
  // point that H sends next to its line at infinity is displaced by more than any int holds
  auto rounded = [&](int i) {
    double tx, ty, tw;
    hdot(H, (double)rows[4 * i], (double)rows[4 * i + 1], &tx, &ty, &tw);
    double dx = tx / tw - (double)rows[4 * i + 2], dy = ty / tw - (double)rows[4 * i + 3];
    return __builtin_rint(sqrt(dx * dx + dy * dy));
  };
  int big = 0;
  for (int i = tid; i < n; i += NT) {
    const double rd = rounded(i);
    // HB: every displacement beyond the histogram.  A NaN displacement (0 / 0 where tw == 0; the reference raises there)
    // converts to bin 0 on this device, as before; in the quadratic path it equals nothing and is in no group
    const int r = rd >= (double)HB ? HB : (int)rd;
    rbin[i] = r;
    if (r < HB) atomicAdd(&B.u.h.hist[r], 1u);
    else big = 1;
  }
  __threadfence_block();
  big = __syncthreads_or(big);
  if (n == 0) return 0;
  // most populated bin; ties -> the bin whose first member comes first.  key = population << 32 | (0x7FFFFFFF - first
  // member): the largest key over the POINTS (a point carries the population of its own bin) is the largest over the
  // bins -- no per-bin "first member" table is needed (it cost 8 KB of LDS in every solver workgroup)
  unsigned long long bestkey = 0;
  double* rwide = reinterpret_cast<double*>(rbin + ((n + 1) & ~1));     // 4 (n + 1) + 8 n <= 16 n bytes
  if (!big) {
    for (int i = tid; i < n; i += NT) {
      const unsigned long long key = ((unsigned long long)B.u.h.hist[rbin[i]] << 32) | (unsigned)(0x7FFFFFFF - i);
      bestkey = key > bestkey ? key : bestkey;
    }
  } else {
    // some displacement is 2048 or more: bins are compared as the rounded doubles themselves, which keeps apart every
    // pair of values an int would saturate together (above 2^31)
    for (int i = tid; i < n; i += NT) rwide[i] = rounded(i);
    __threadfence_block();
    __syncthreads();
    for (int i = tid; i < n; i += NT) {
      const double r = rwide[i];
      bool first = true;
      int cnt = 0;
      for (int j = 0; j < n; j++) {
        if (rwide[j] == r) { cnt++; if (j < i) first = false; }
      }
      if (first) {
        unsigned long long key = ((unsigned long long)cnt << 32) | (unsigned)(0x7FFFFFFF - i);
        bestkey = key > bestkey ? key : bestkey;
      }
    }
  }
  bestkey = wave_max_u64(bestkey);
  if (lane == 0) B.red[wave] = bestkey;
  __syncthreads();
  for (int w = 0; w < NW; w++) { const unsigned long long o = B.red[w]; bestkey = o > bestkey ? o : bestkey; }
  const int ibest = 0x7FFFFFFF - (int)(bestkey & 0xFFFFFFFFull);
  const int rbest = rbin[ibest];
  const double wbest = big ? rwide[ibest] : 0.0;
  int mcount = 0;
  if (wave == 0) {
    for (int c0 = 0; c0 < n; c0 += NL) {
      const int i = c0 + lane;
      const bool f = i < n && (big ? rwide[i] == wbest : rbin[i] == rbest);
      const unsigned long long b = __ballot(f);
      if (f) *reinterpret_cast<float4*>(out + 4 * (mcount + __popcll(b & ((1ull << lane) - 1ull)))) =
          *reinterpret_cast<const float4*>(rows + 4 * i);
      mcount += __popcll(b);
    }
    if (lane == 0) B.s.ib[3] = mcount;
  }
  __threadfence_block();
  __syncthreads();
  return B.s.ib[3];
}

// the rows in the fixed plane: both points of every row through Hsup (f64 -> f32); `nthreads` threads of a workgroup
__device__ __forceinline__ void to_fixed_plane(const double* Hsup /*LDS*/, const float* rows, int n, float* trow, int nthreads) {
  for (int i = threadIdx.x; i < n; i += nthreads) {
    double tx, ty, tw;
    hdot(Hsup, (double)rows[4 * i], (double)rows[4 * i + 1], &tx, &ty, &tw);
    float ax = (float)(tx / tw), ay = (float)(ty / tw);
    hdot(Hsup, (double)rows[4 * i + 2], (double)rows[4 * i + 3], &tx, &ty, &tw);
    float bx = (float)(tx / tw), by = (float)(ty / tw);
    *reinterpret_cast<float4*>(trow + 4 * i) = make_float4(ax, ay, bx, by);
  }
}

// compute_homography (utils.py:351-362): optional pre-transform by Hsup (f64 -> f32), RANSAC #2, 0.7 gate.
// All threads; uniform result; ends with a workgroup barrier.
template <int NW, bool LANES>
__device__ __forceinline__ int compute_homography_block(BlockLds<NW, LANES>& B, const float* rows, int n, const double* Hsup /*LDS|null*/,
                                        const EvhRansacArgs& A, uint8_t* mask, float* trow, float* crow, int* info,
                                        const ScanPre* pre = nullptr) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* use = rows;
  if (Hsup) {
    to_fixed_plane(Hsup, rows, n, trow, NW * NL);
    __threadfence_block();
    __syncthreads();
    use = trow;
  }
  const bool found = find_homography_block<NW, LANES>(B, use, n, A.thr, A.max_iters, A.conf, A.force_max, mask, crow, info, A.prof, A.lane_v ? A.lane_v + (int64_t)blockIdx.x * (NW * LV_ELEMS * NL) : nullptr, pre);
  if (wave == 0) {
    int s = 0;
    for (int i = lane; i < n; i += NL) s += mask[i];
    s = wave_sum(s);
    if (lane == 0) B.gate = (double)s < 0.7 * (double)n ? 1 : 0;
  }
  __syncthreads();
  if (B.gate) return EVH_PAIR_LOW_INLIER_RATIO;
  if (!found) return EVH_PAIR_NO_FINAL_H;
  return EVH_PAIR_OK;
}

template <int NW, bool LANES>
__device__ __forceinline__ BlockLds<NW, LANES>& block_lds() {
  __shared__ BlockLds<NW, LANES> g;
  return g;
}

// ... with the solver mode posted (read after the first barrier of the solve).  The value, not the argument block: a
// kernel that hands its EvhRansacArgs on by reference reads all of it up front (k_ransac_static changed its code)
template <int NW, bool LANES>
__device__ __forceinline__ BlockLds<NW, LANES>& block_lds(int fast_solver) {
  BlockLds<NW, LANES>& B = block_lds<NW, LANES>();
  if (threadIdx.x == 0) B.s.fast = fast_solver;
  return B;
}

// generic single-problem entry (evh_find_homography_ransac)
template <int NW, bool LANES>
__global__ __launch_bounds__(NW * NL) void k_find_homography(EvhRansacArgs A) {
  BlockLds<NW, LANES>& B = block_lds<NW, LANES>(A.fast_solver);
  const int tid = threadIdx.x;
  const int n = A.n_fixed;
  const bool found = find_homography_block<NW, LANES>(B, A.pts, n, A.thr, A.max_iters, A.conf, A.force_max, A.mask, A.crow, A.info, A.prof, A.lane_v);
  if (tid < 9) A.H[tid] = found ? B.s.H[tid] : 0.0;
  if (tid == 0) A.found[0] = found ? 1 : 0;
}

// generic static filter entry
template <int NW, bool LANES>
__global__ __launch_bounds__(NW * NL) void k_static_filter(const double* H, const float* rows, int n, int* rbin,
                                                           float* out, int* count) {
  BlockLds<NW, LANES>& B = block_lds<NW, LANES>();
  const int tid = threadIdx.x;
  if (tid < 9) B.s.H[tid] = H[tid];
  __syncthreads();
  const int m = static_filter_block<NW, LANES>(B, B.s.H, rows, n, rbin, out);
  if (tid == 0) count[0] = m;
}

// phase 1 of a pair: RANSAC #1 on the matched rows, then the static-point filter (matching.py:152-163)
template <int NW, bool LANES>
__global__ __launch_bounds__(NW * NL) void k_ransac_static(EvhRansacArgs A) {
  BlockLds<NW, LANES>& B = block_lds<NW, LANES>(A.fast_solver);
  const int p = blockIdx.x, tid = threadIdx.x;
  if (A.status[p] != EVH_PAIR_OK) { if (tid == 0) A.npts2[p] = 0; return; }
  const int n = A.npts[p];
  const float* rows = A.pts + (int64_t)p * A.row_stride * 4;
  float* out = A.pts2 + (int64_t)p * A.row_stride * 4;
  uint8_t* mask = A.mask + (int64_t)p * A.row_stride;
  float* crow = A.crow + (int64_t)p * A.row_stride * 4;
  int* rbin = reinterpret_cast<int*>(A.lm + (int64_t)p * A.row_stride * 4);
  int* info = A.info ? A.info + 8 * p : nullptr;
  const bool found = find_homography_block<NW, LANES>(B, rows, n, A.thr, A.max_iters, A.conf, A.force_max, mask, crow, info, A.prof, A.lane_v ? A.lane_v + (int64_t)blockIdx.x * (NW * LV_ELEMS * NL) : nullptr);
  if (!found) {
    if (tid == 0) { A.status[p] = EVH_PAIR_NO_PROVISIONAL_H; A.npts2[p] = 0; }
    return;
  }
  if (A.H1 && tid < 9) A.H1[9 * p + tid] = B.s.H[tid];
  const int m = static_filter_block<NW, LANES>(B, B.s.H, rows, n, rbin, out);
  if (tid == 0) A.npts2[p] = m;
}

// phase 2: compute_homography.  Independent pairs: one workgroup per pair, Hsup = None.
template <int NW, bool LANES>
__global__ __launch_bounds__(NW * NL) void k_ransac_final_pairs(EvhRansacArgs A) {
  BlockLds<NW, LANES>& B = block_lds<NW, LANES>(A.fast_solver);
  const int p = blockIdx.x, tid = threadIdx.x;
  int st = A.status[p];
  if (st == EVH_PAIR_OK) {
    const int n = A.npts2[p];
    const float* rows = A.pts2 + (int64_t)p * A.row_stride * 4;
    st = compute_homography_block<NW, LANES>(B, rows, n, nullptr, A, A.mask + (int64_t)p * A.row_stride,
                                      A.pts + (int64_t)p * A.row_stride * 4 /* matched rows are dead: scratch */,
                                      A.crow + (int64_t)p * A.row_stride * 4, A.info ? A.info + 8 * p + 4 : nullptr);
  }
  if (tid < 9) A.H[9 * p + tid] = st == EVH_PAIR_OK ? B.s.H[tid] : 0.0;
  if (tid == 0) A.out_status[p] = st;
}

// the end of one step of the scan: status, H of the pair (a failed pair repeats the previous H, none_H_processing=True),
// running superposition.  All threads; returns true when the scan stops here (uniform); ends with a workgroup barrier.
template <int NW, bool LANES>
__device__ __forceinline__ bool scan_step_tail(BlockLds<NW, LANES>& B, int st, int p, int npairs, double* Hout, int* stout, bool first) {
  const int tid = threadIdx.x;
  if (tid == 0) stout[p] = st;
  if (st != EVH_PAIR_OK && !B.have_prev) {
    // the reference raises here (None.tolist()); mark the pair and stop the scan
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    for (int q = p + 1 + tid; q < npairs; q += NW * NL) stout[q] = st;
    for (int q = 9 * p + tid; q < 9 * npairs; q += NW * NL) Hout[q] = nan;
    return true;
  }
  if (tid < 9) B.Hcur[tid] = st == EVH_PAIR_OK ? B.s.H[tid] : B.Hprev[tid];
  __syncthreads();
  if (tid < NL) {                          // wave 0
    if (tid < 9) { Hout[9 * p + tid] = B.Hcur[tid]; B.Hprev[tid] = B.Hcur[tid]; }
    // matrix_superposition (utils.py:139-145); np.dot(3x3,3x3) = forward FMA chain (pinned by fixtures)
    double P = 0;
    if (!first && tid < 9) {
      const int r = tid / 3, c = tid - 3 * r;
      P = fma(B.Hcur[3 * r + 2], B.Hsup[6 + c], fma(B.Hcur[3 * r + 1], B.Hsup[3 + c], B.Hcur[3 * r] * B.Hsup[c]));
    }
    const double P8 = __shfl(P, 8);
    WSYNC();
    if (tid < 9) B.Hsup[tid] = first ? B.Hcur[tid] : P / P8;
    if (tid == 0) B.have_prev = 1;
  }
  __syncthreads();
  return false;
}

// phase 2, stream semantics (video_processing.py:83-105): sequential scan over the pairs of one stream with the
// running superposition; a failed pair repeats the previous H (none_H_processing=True).
template <int NW, bool LANES>
__global__ __launch_bounds__(NW * NL) void k_ransac_final_stream(EvhRansacArgs A, int npairs, int pitch) {
  // one workgroup per stream: block s scans the npairs pairs whose per-pair slots start at s * pitch (several streams
  // of one batch sit `pitch` pair slots apart); H / status are written compactly at s * npairs + p
  BlockLds<NW, LANES>& B = block_lds<NW, LANES>(A.fast_solver);
  const int tid = threadIdx.x, s = blockIdx.x;
  const double* Hsup0 = A.Hsup0 ? A.Hsup0 + 18 * s : nullptr;
  const double* Hprev0 = A.Hprev0 ? A.Hprev0 + 18 * s : nullptr;
  const int64_t slot0 = (int64_t)s * pitch;                 // first pair slot of this stream; also its scratch slot
  double* Hout = A.H + (int64_t)9 * s * npairs;
  int* stout = A.out_status + (int64_t)s * npairs;
  if (tid == 0) B.have_prev = Hprev0 ? 1 : 0;
  if (tid < 9 && Hsup0) B.Hsup[tid] = Hsup0[tid];
  if (tid < 9 && Hprev0) B.Hprev[tid] = Hprev0[tid];
  __syncthreads();
  bool first = Hsup0 == nullptr;
  for (int p = 0; p < npairs; p++) {
    int st = A.status[slot0 + p];
    if (st == EVH_PAIR_OK) {
      const int n = A.npts2[slot0 + p];
      const float* rows = A.pts2 + (slot0 + p) * A.row_stride * 4;
      // the scan is sequential: one pair's worth of scratch (the stream's first slot) serves all its pairs
      st = compute_homography_block<NW, LANES>(B, rows, n, first ? nullptr : B.Hsup, A, A.mask + slot0 * A.row_stride,
                                        A.pts + slot0 * A.row_stride * 4, A.crow + slot0 * A.row_stride * 4,
                                        A.info ? A.info + 8 * (slot0 + p) + 4 : nullptr);
    }
    if (scan_step_tail<NW, LANES>(B, st, p, npairs, Hout, stout, first)) return;
    first = false;
  }
  if (A.state_out && tid < 9) { A.state_out[18 * s + tid] = B.Hsup[tid]; A.state_out[18 * s + 9 + tid] = B.Hprev[tid]; }
}

// ---- fixed-iteration stream scan (force_max): the samples of a pair are independent, only the replay and the
// refinement are serial, so every pair takes two launches: k_scan_hyp (one 16-hypothesis chunk per workgroup, ~140
// workgroups) and k_scan_finish (one workgroup: replay, inlier mask, refit, LM, superposition).  The state of the scan
// lives in global memory between the launches.
struct ScanState { double Hsup[9], Hprev[9]; int have_prev, first, aborted, pad; };
struct ScanWs {
  ScanState* state;                // [nstreams]
  unsigned long long* rng_after;   // [nstreams * npairs] generator state after the table of the pair
  ushort4* quads;                  // [nstreams * npairs][hmax] the sample table: depends on the row count of the pair alone
  int* hyp;                        // [nstreams][hmax]
  double* hypH;                    // [nstreams][hmax][9]
  int hmax;
};

__global__ __launch_bounds__(NL) void k_scan_init(EvhRansacArgs A, ScanWs W) {
  const int s = blockIdx.x, tid = threadIdx.x;
  ScanState& T = W.state[s];
  if (tid < 9) { T.Hsup[tid] = A.Hsup0 ? A.Hsup0[18 * s + tid] : 0.0; T.Hprev[tid] = A.Hprev0 ? A.Hprev0[18 * s + tid] : 0.0; }
  if (tid == 0) { T.have_prev = A.Hprev0 ? 1 : 0; T.first = A.Hsup0 ? 0 : 1; T.aborted = 0; T.pad = 0; }
}

// the sample quadruples of every pair of the batch, all pairs at once (getSubset: they depend on the row count only, so
// they can be drawn before the scan reaches the pair)
__global__ __launch_bounds__(NL) void k_scan_quads(EvhRansacArgs A, int npairs, int pitch, ScanWs W, int phase1) {
  // phase1: the tables of RANSAC #1 of independent pairs (row counts in A.npts, one "stream" of one pair per block)
  const int b = blockIdx.x, s = b / npairs, p = b - s * npairs, lane = threadIdx.x;
  const int64_t slot = (int64_t)s * pitch + p;
  if (A.status[slot] != EVH_PAIR_OK) return;
  const int n = phase1 ? A.npts[slot] : A.npts2[slot];
  if (n <= 4) return;
  Rng rng;
  const FastMod fm((unsigned)n);
  ushort4* out = W.quads + (int64_t)b * W.hmax;
  unsigned long long after = 0ull;
  for (int h0 = 0; h0 < W.hmax; h0 += NL) {
    int m0 = 0, m1 = 0, m2 = 0, m3 = 0;
    for (int j = 0; j < NL; j++) {
      const int4 q = draw_quad(rng, fm);
      if (j == lane) { m0 = q.x; m1 = q.y; m2 = q.z; m3 = q.w; }
      if (h0 + j + 1 == W.hmax) after = rng.state;
    }
    if (h0 + lane < W.hmax) out[h0 + lane] = make_ushort4((unsigned short)m0, (unsigned short)m1, (unsigned short)m2, (unsigned short)m3);
  }
  if (lane == 0) W.rng_after[b] = after;
}

// LDS of the hypothesis kernels: the 16 row matrices and nothing else (23 KB: seven workgroups per compute unit; the
// full BlockLds of the finishing kernels would allow three)
struct HypLds { RowMat m[4][NG]; double Hsup[9]; };

// one chunk of 16 hypotheses (a 16-lane row each) per workgroup, blockIdx.x = chunk: samples of table `table` of W.quads on
// the n > 4 rows `use`, result words and models into table `slot` of W.hyp / W.hypH
__device__ __forceinline__ void hyp_chunk(HypLds& B, const EvhRansacArgs& A, const ScanWs& W, const float* use, int n, int64_t table,
                                          int64_t slot) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, row = lane >> 4, gl = lane & 15;
  double thr = A.thr;
  if (thr <= 0) thr = 3;
  const float t = (float)(thr * thr);
  const int hg = blockIdx.x * (4 * NG) + wave * NG + row;
  const ushort4 q = W.quads[table * W.hmax + hg];
  const int my[4] = {q.x, q.y, q.z, q.w};
  float Mx[4], My[4], mx[4], my_[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const float4 r = *reinterpret_cast<const float4*>(use + 4 * my[i]);
    Mx[i] = r.x; My[i] = r.y; mx[i] = r.z; my_[i] = r.w;
  }
  const bool valid = check_subset4(Mx, My, mx, my_);
  double H[9];
  const bool ok = dlt4_rows(B.m[wave][row], lane, valid, Mx, My, mx, my_, H);
  int good = 0;
  if (ok) {
    float Hf[8];
#pragma unroll
    for (int i = 0; i < 8; i++) Hf[i] = (float)H[i];
#pragma unroll 4
    for (int i = gl; i < n; i += GL) {
      const float4 r = *reinterpret_cast<const float4*>(use + 4 * i);
      good += is_inlier(Hf, r.x, r.y, r.z, r.w, t) ? 1 : 0;
    }
  }
  good = rsum16(good);
  if (gl == 0) {
    W.hyp[slot * W.hmax + hg] = (int)hyp_pack(valid, ok, good);
    double* Ho = W.hypH + (slot * W.hmax + hg) * 9;
#pragma unroll
    for (int i = 0; i < 9; i++) Ho[i] = ok ? H[i] : 0.0;
  }
}

// the chunks of pair p of every stream, rows in the fixed plane; grid (hmax / 16, nstreams)
__global__ __launch_bounds__(4 * NL) void k_scan_hyp(EvhRansacArgs A, int p, int npairs, int pitch, ScanWs W) {
  __shared__ HypLds B;
  const int tid = threadIdx.x, s = blockIdx.y;
  const ScanState& T = W.state[s];
  if (T.aborted) return;
  const int64_t slot0 = (int64_t)s * pitch, slot = slot0 + p;
  if (A.status[slot] != EVH_PAIR_OK) return;
  const int n = A.npts2[slot];
  if (n <= 4) return;
  const float* use = A.pts2 + slot * A.row_stride * 4;
  if (!T.first) {
    // the rows in the fixed plane (compute_homography_block's transform).  Every workgroup of the pair writes the same
    // values to the stream's one scratch slot and reads back what it wrote itself -- identical bits from every writer.
    float* trow = A.pts + slot0 * A.row_stride * 4;
    if (tid < 9) B.Hsup[tid] = T.Hsup[tid];
    __syncthreads();
    to_fixed_plane(B.Hsup, use, n, trow, 4 * NL);
    __threadfence_block();
    __syncthreads();
    use = trow;
  }
  hyp_chunk(B, A, W, use, n, (int64_t)s * npairs + p, s);
}

// the serial part of pair p: replay of the hypotheses, refinement, step of the scan; grid = nstreams
__global__ __launch_bounds__(4 * NL) void k_scan_finish(EvhRansacArgs A, int p, int npairs, int pitch, ScanWs W) {
  BlockLds<4, false>& B = block_lds<4, false>(A.fast_solver);
  const int tid = threadIdx.x, s = blockIdx.x;
  ScanState& T = W.state[s];
  if (T.aborted) return;
  const int64_t slot0 = (int64_t)s * pitch;
  double* Hout = A.H + (int64_t)9 * s * npairs;
  int* stout = A.out_status + (int64_t)s * npairs;
  const bool first = T.first != 0;
  if (tid == 0) B.have_prev = T.have_prev;
  if (tid < 9) { B.Hsup[tid] = T.Hsup[tid]; B.Hprev[tid] = T.Hprev[tid]; }
  __syncthreads();
  int st = A.status[slot0 + p];
  if (st == EVH_PAIR_OK) {
    const int n = A.npts2[slot0 + p];
    const float* rows = A.pts2 + (slot0 + p) * A.row_stride * 4;
    const ScanPre pre{W.hyp + (int64_t)s * W.hmax, W.hypH + (int64_t)s * W.hmax * 9, W.hmax, n > 4 ? W.rng_after[(int64_t)s * npairs + p] : 0ull};
    st = compute_homography_block<4, false>(B, rows, n, first ? nullptr : B.Hsup, A, A.mask + slot0 * A.row_stride,
                                            A.pts + slot0 * A.row_stride * 4, A.crow + slot0 * A.row_stride * 4,
                                            A.info ? A.info + 8 * (slot0 + p) + 4 : nullptr, n > 4 ? &pre : nullptr);
  }
  if (scan_step_tail<4, false>(B, st, p, npairs, Hout, stout, first)) {
    if (tid == 0) T.aborted = 1;
    return;
  }
  if (tid < 9) { T.Hsup[tid] = B.Hsup[tid]; T.Hprev[tid] = B.Hprev[tid]; }
  if (tid == 0) { T.have_prev = 1; T.first = 0; }
  if (p == npairs - 1 && A.state_out && tid < 9) { A.state_out[18 * s + tid] = B.Hsup[tid]; A.state_out[18 * s + 9 + tid] = B.Hprev[tid]; }
}

// ---- ragged batches (evh_streams_homography_batch): the scans above and below once more with the streams taken from a segment
// table.  The existing entries keep their own kernels (k_ransac_final_stream, k_scan_*): with the layout folded into them their
// prologues changed and bench.py --config 3 fell outside the parent's run-to-run spread (profiles/r07_streams_ragged.txt).
// KEEP IN STEP: k_ransac_final_ragged, k_scan_init_ragged, k_scan_hyp_ragged, k_scan_finish_ragged and launch_forced_ragged are
// copies of k_ransac_final_stream, k_scan_init, k_scan_hyp, k_scan_finish and launch_forced_scan that differ only in where a
// stream's slots, rows and start flag come from; a change to the scan goes into both.  tests/test_gpu_streams_ragged.py is what
// holds them together: per stream it demands the bits of the single-stream entries, adaptive and forced, carried state included.
// at(s) = stream s: its first pair slot (also its scratch slot), the first row of its
// status and the first double of its H, its pair count, and whether it reads its row of the entering state (A.Hsup0 /
// A.Hprev0, when the launch has them).
struct StreamAt { int64_t slot0, out0, h0; int npairs; bool carried; };
// a ragged batch (evh_streams_homography_batch): stream s owns the consecutive frames of segs[s]; pair k of it reads pair slot
// first_frame + k and writes row first_frame + k; a segment with `start` set begins its stream whatever the state pointers hold
struct RaggedStreams {
  const evh_stream_seg* segs;
  __device__ __forceinline__ StreamAt at(int s) const {
    const int4 g = *reinterpret_cast<const int4*>(segs + s);     // first_frame, nframes, start, reserved
    return {(int64_t)g.x, (int64_t)g.x, (int64_t)9 * g.x, g.y - 1, g.z == 0};
  }
};

// phase 2, stream semantics (video_processing.py:83-105): sequential scan over the pairs of one stream with the
// running superposition; a failed pair repeats the previous H (none_H_processing=True).
// One workgroup per stream: block s scans the pairs of stream s (StreamAt).  (The arguments by value, the body in the kernel
// itself: handed on by reference the argument block is read up front, see block_lds.)
template <int NW, bool LANES>
__global__ __launch_bounds__(NW * NL) void k_ransac_final_ragged(EvhRansacArgs A, RaggedStreams lay) {
  BlockLds<NW, LANES>& B = block_lds<NW, LANES>(A.fast_solver);
  const int tid = threadIdx.x, s = blockIdx.x;
  const StreamAt T = lay.at(s);
  const double* Hsup0 = A.Hsup0 && T.carried ? A.Hsup0 + 18 * s : nullptr;
  const double* Hprev0 = A.Hprev0 && T.carried ? A.Hprev0 + 18 * s : nullptr;
  const int64_t slot0 = T.slot0;                            // first pair slot of this stream; also its scratch slot
  const int npairs = T.npairs;
  double* Hout = A.H + T.h0;
  int* stout = A.out_status + T.out0;
  if (tid == 0) B.have_prev = Hprev0 ? 1 : 0;
  if (tid < 9 && Hsup0) B.Hsup[tid] = Hsup0[tid];
  if (tid < 9 && Hprev0) B.Hprev[tid] = Hprev0[tid];
  __syncthreads();
  bool first = Hsup0 == nullptr;
  for (int p = 0; p < npairs; p++) {
    int st = A.status[slot0 + p];
    if (st == EVH_PAIR_OK) {
      const int n = A.npts2[slot0 + p];
      const float* rows = A.pts2 + (slot0 + p) * A.row_stride * 4;
      // the scan is sequential: one pair's worth of scratch (the stream's first slot) serves all its pairs
      st = compute_homography_block<NW, LANES>(B, rows, n, first ? nullptr : B.Hsup, A, A.mask + slot0 * A.row_stride,
                                        A.pts + slot0 * A.row_stride * 4, A.crow + slot0 * A.row_stride * 4,
                                        A.info ? A.info + 8 * (slot0 + p) + 4 : nullptr);
    }
    if (scan_step_tail<NW, LANES>(B, st, p, npairs, Hout, stout, first)) return;
    first = false;
  }
  if (A.state_out && tid < 9) { A.state_out[18 * s + tid] = B.Hsup[tid]; A.state_out[18 * s + 9 + tid] = B.Hprev[tid]; }
}
__global__ __launch_bounds__(NL) void k_scan_init_ragged(EvhRansacArgs A, ScanWs W, RaggedStreams lay) {
  const int s = blockIdx.x, tid = threadIdx.x;
  ScanState& T = W.state[s];
  const bool carried = lay.at(s).carried;
  const double* Hsup0 = carried ? A.Hsup0 : nullptr;
  const double* Hprev0 = carried ? A.Hprev0 : nullptr;
  if (tid < 9) { T.Hsup[tid] = Hsup0 ? Hsup0[18 * s + tid] : 0.0; T.Hprev[tid] = Hprev0 ? Hprev0[18 * s + tid] : 0.0; }
  if (tid == 0) { T.have_prev = Hprev0 ? 1 : 0; T.first = Hsup0 ? 0 : 1; T.aborted = 0; T.pad = 0; }
}


// the chunks of pair p of every stream that has one, rows in the fixed plane; grid (hmax / 16, nstreams)
__global__ __launch_bounds__(4 * NL) void k_scan_hyp_ragged(EvhRansacArgs A, int p, RaggedStreams lay, ScanWs W) {
  __shared__ HypLds B;
  const int tid = threadIdx.x, s = blockIdx.y;
  const ScanState& T = W.state[s];
  const StreamAt at = lay.at(s);
  if (p >= at.npairs || T.aborted) return;
  const int64_t slot0 = at.slot0, slot = slot0 + p;
  if (A.status[slot] != EVH_PAIR_OK) return;
  const int n = A.npts2[slot];
  if (n <= 4) return;
  const float* use = A.pts2 + slot * A.row_stride * 4;
  if (!T.first) {
    // the rows in the fixed plane (compute_homography_block's transform).  Every workgroup of the pair writes the same
    // values to the stream's one scratch slot and reads back what it wrote itself -- identical bits from every writer.
    float* trow = A.pts + slot0 * A.row_stride * 4;
    if (tid < 9) B.Hsup[tid] = T.Hsup[tid];
    __syncthreads();
    to_fixed_plane(B.Hsup, use, n, trow, 4 * NL);
    __threadfence_block();
    __syncthreads();
    use = trow;
  }
  hyp_chunk(B, A, W, use, n, at.slot0 + p, s);
}

// the serial part of pair p: replay of the hypotheses, refinement, step of the scan; grid = nstreams (a stream with fewer
// pairs has left)
__global__ __launch_bounds__(4 * NL) void k_scan_finish_ragged(EvhRansacArgs A, int p, RaggedStreams lay, ScanWs W) {
  BlockLds<4, false>& B = block_lds<4, false>(A.fast_solver);
  const int tid = threadIdx.x, s = blockIdx.x;
  ScanState& T = W.state[s];
  const StreamAt at = lay.at(s);
  const int npairs = at.npairs;
  if (p >= npairs || T.aborted) return;
  const int64_t slot0 = at.slot0;
  double* Hout = A.H + at.h0;
  int* stout = A.out_status + at.out0;
  const bool first = T.first != 0;
  if (tid == 0) B.have_prev = T.have_prev;
  if (tid < 9) { B.Hsup[tid] = T.Hsup[tid]; B.Hprev[tid] = T.Hprev[tid]; }
  __syncthreads();
  int st = A.status[slot0 + p];
  if (st == EVH_PAIR_OK) {
    const int n = A.npts2[slot0 + p];
    const float* rows = A.pts2 + (slot0 + p) * A.row_stride * 4;
    const ScanPre pre{W.hyp + (int64_t)s * W.hmax, W.hypH + (int64_t)s * W.hmax * 9, W.hmax, n > 4 ? W.rng_after[at.slot0 + p] : 0ull};
    st = compute_homography_block<4, false>(B, rows, n, first ? nullptr : B.Hsup, A, A.mask + slot0 * A.row_stride,
                                            A.pts + slot0 * A.row_stride * 4, A.crow + slot0 * A.row_stride * 4,
                                            A.info ? A.info + 8 * (slot0 + p) + 4 : nullptr, n > 4 ? &pre : nullptr);
  }
  if (scan_step_tail<4, false>(B, st, p, npairs, Hout, stout, first)) {
    if (tid == 0) T.aborted = 1;
    return;
  }
  if (tid < 9) { T.Hsup[tid] = B.Hsup[tid]; T.Hprev[tid] = B.Hprev[tid]; }
  if (tid == 0) { T.have_prev = 1; T.first = 0; }
  if (p == npairs - 1 && A.state_out && tid < 9) { A.state_out[18 * s + tid] = B.Hsup[tid]; A.state_out[18 * s + 9 + tid] = B.Hprev[tid]; }
}

// ---- fixed-iteration RANSAC #1 of a SMALL batch of pairs (a stream chunk): the same split -- k_static_hyp evaluates one
// 16-hypothesis chunk per workgroup (grid: chunks x pairs), k_static_finish replays, refines and runs the static filter.
// (One workgroup per pair with per-lane solvers is the throughput form for hundreds of pairs; alone it takes 4.8 ms.)
__global__ __launch_bounds__(4 * NL) void k_static_hyp(EvhRansacArgs A, ScanWs W) {
  __shared__ HypLds B;
  const int p = blockIdx.y;
  if (A.status[p] != EVH_PAIR_OK) return;
  const int n = A.npts[p];
  if (n <= 4) return;
  const float* use = A.pts + (int64_t)p * A.row_stride * 4;
  hyp_chunk(B, A, W, use, n, p, p);
}

__global__ __launch_bounds__(4 * NL) void k_static_finish(EvhRansacArgs A, ScanWs W) {
  BlockLds<4, false>& B = block_lds<4, false>(A.fast_solver);
  const int p = blockIdx.x, tid = threadIdx.x;
  if (A.status[p] != EVH_PAIR_OK) { if (tid == 0) A.npts2[p] = 0; return; }
  const int n = A.npts[p];
  const float* rows = A.pts + (int64_t)p * A.row_stride * 4;
  float* out = A.pts2 + (int64_t)p * A.row_stride * 4;
  uint8_t* mask = A.mask + (int64_t)p * A.row_stride;
  float* crow = A.crow + (int64_t)p * A.row_stride * 4;
  int* rbin = reinterpret_cast<int*>(A.lm + (int64_t)p * A.row_stride * 4);
  int* info = A.info ? A.info + 8 * p : nullptr;
  const ScanPre pre{W.hyp + (int64_t)p * W.hmax, W.hypH + (int64_t)p * W.hmax * 9, W.hmax, n > 4 ? W.rng_after[p] : 0ull};
  const bool found = find_homography_block<4, false>(B, rows, n, A.thr, A.max_iters, A.conf, A.force_max, mask, crow, info, A.prof,
                                                     nullptr, n > 4 ? &pre : nullptr);
  if (!found) {
    if (tid == 0) { A.status[p] = EVH_PAIR_NO_PROVISIONAL_H; A.npts2[p] = 0; }
    return;
  }
  if (A.H1 && tid < 9) A.H1[9 * p + tid] = B.s.H[tid];
  const int m = static_filter_block<4, false>(B, B.s.H, rows, n, rbin, out);
  if (tid == 0) A.npts2[p] = m;
}

// waves per workgroup: enough rows to cover the handful of hypotheses an adaptive RANSAC needs in one chunk when the
// launch is small (latency), one wave per pair when the launch fills the chip anyway (throughput); with the iteration
// count forced, four waves of lane-per-hypothesis solvers (256 hypotheses per chunk)
int waves_for(int nblocks, int force_max) {
  if (force_max) return 0;      // the LANES form
  return nblocks >= 512 ? 1 : 4;
}

// workspace of the fixed-iteration stream scan, grown on demand
int scan_ws(evh_ctx* c, int nstreams, size_t slots /* sample tables */, int hmax, ScanWs* W) {
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t o_state = 0, o_rng = o_state + up(sizeof(ScanState) * nstreams), o_quads = o_rng + up(8 * slots),
               o_hyp = o_quads + up(sizeof(ushort4) * slots * hmax), o_H = o_hyp + up(sizeof(int) * (size_t)nstreams * hmax),
               total = o_H + up(sizeof(double) * 9 * (size_t)nstreams * hmax);
  if (int rc = grow(c, &c->d_scan_ws, &c->scan_ws_bytes, total)) return rc;
  char* b = c->d_scan_ws;
  W->state = reinterpret_cast<ScanState*>(b + o_state); W->rng_after = reinterpret_cast<unsigned long long*>(b + o_rng);
  W->quads = reinterpret_cast<ushort4*>(b + o_quads); W->hyp = reinterpret_cast<int*>(b + o_hyp);
  W->hypH = reinterpret_cast<double*>(b + o_H); W->hmax = hmax;
  return EVH_SUCCESS;
}

// enough 16-hypothesis chunks for max_iters counted samples plus 1/8 of rejected ones; a pair that needs more continues
// inside the finishing kernel with the ordinary chunk loop
int forced_chunks(const EvhRansacArgs& A) {
  const int iters = A.max_iters > 0 ? A.max_iters : 1;
  int chunks = (iters + iters / 8 + 4 * NG - 1) / (4 * NG) + 1;
  if (const char* e = getenv("EVH_SCAN_CHUNKS")) chunks = atoi(e) > 0 ? atoi(e) : chunks;   // tests: a short table, the rest in the finishing kernel
  return chunks > 608 ? 608 : chunks;                               // < 10000 samples (ScanPre)
}

int launch_forced_static(evh_ctx* c, const EvhRansacArgs& A, int npairs) {
  if (A.row_stride > 65536) return evh_fail(c, EVH_ERR_INVALID, "fixed-iteration RANSAC: more than 65536 rows per pair");
  const int chunks = forced_chunks(A);
  ScanWs W;
  int rc = scan_ws(c, npairs, (size_t)npairs, chunks * 4 * NG, &W);
  if (rc) return rc;
  hipLaunchKernelGGL(k_scan_quads, dim3(npairs), dim3(NL), 0, c->stream, A, 1, 1, W, 1);
  hipLaunchKernelGGL(k_static_hyp, dim3(chunks, npairs), dim3(4 * NL), 0, c->stream, A, W);
  hipLaunchKernelGGL(k_static_finish, dim3(npairs), dim3(4 * NL), 0, c->stream, A, W);
  return EVH_SUCCESS;
}

int launch_forced_scan(evh_ctx* c, const EvhRansacArgs& A, int npairs, int nstreams, int pitch) {
  if (A.row_stride > 65536) return evh_fail(c, EVH_ERR_INVALID, "fixed-iteration scan: more than 65536 rows per pair");
  const int chunks = forced_chunks(A);
  ScanWs W;
  int rc = scan_ws(c, nstreams, (size_t)nstreams * npairs, chunks * 4 * NG, &W);
  if (rc) return rc;
  hipLaunchKernelGGL(k_scan_init, dim3(nstreams), dim3(NL), 0, c->stream, A, W);
  hipLaunchKernelGGL(k_scan_quads, dim3(nstreams * npairs), dim3(NL), 0, c->stream, A, npairs, pitch, W, 0);
  for (int p = 0; p < npairs; p++) {
    hipLaunchKernelGGL(k_scan_hyp, dim3(chunks, nstreams), dim3(4 * NL), 0, c->stream, A, p, npairs, pitch, W);
    hipLaunchKernelGGL(k_scan_finish, dim3(nstreams), dim3(4 * NL), 0, c->stream, A, p, npairs, pitch, W);
  }
  return EVH_SUCCESS;
}

// npairs: the pairs of the longest stream (the per-pair launches run that far).  The sample tables: one per pair of every
// stream (quad_streams x quad_pairs of them, `pitch` slots apart) -- a ragged batch draws them for all its pair slots as one
// run (1 x slots), the straddling ones included
int launch_forced_ragged(evh_ctx* c, const EvhRansacArgs& A, int npairs, int nstreams, const RaggedStreams& lay, int quad_streams,
                       int quad_pairs, int pitch) {
  if (A.row_stride > 65536) return evh_fail(c, EVH_ERR_INVALID, "fixed-iteration scan: more than 65536 rows per pair");
  const int chunks = forced_chunks(A);
  ScanWs W;
  int rc = scan_ws(c, nstreams, (size_t)quad_streams * quad_pairs, chunks * 4 * NG, &W);
  if (rc) return rc;
  hipLaunchKernelGGL(k_scan_init_ragged, dim3(nstreams), dim3(NL), 0, c->stream, A, W, lay);
  hipLaunchKernelGGL(k_scan_quads, dim3(quad_streams * quad_pairs), dim3(NL), 0, c->stream, A, quad_pairs, pitch, W, 0);
  for (int p = 0; p < npairs; p++) {
    hipLaunchKernelGGL(k_scan_hyp_ragged, dim3(chunks, nstreams), dim3(4 * NL), 0, c->stream, A, p, lay, W);
    hipLaunchKernelGGL(k_scan_finish_ragged, dim3(nstreams), dim3(4 * NL), 0, c->stream, A, p, lay, W);
  }
  return EVH_SUCCESS;
}

int check_lane_scratch(evh_ctx* c, const EvhRansacArgs& A) {
  return A.force_max && !A.lane_v ? evh_fail(c, EVH_ERR_HIP, "fixed-iteration RANSAC: the per-lane scratch could not be allocated") : EVH_SUCCESS;
}
// the tail of every launcher: a launch that did not go out is reported here
int launched(evh_ctx* c) { EVH_HIP(c, hipGetLastError()); return EVH_SUCCESS; }

}  // namespace

#define EVH_LAUNCH_NW(nw, kernel, grid, stream, ...)                                                               \
  do {                                                                                                            \
    if ((nw) == 0) hipLaunchKernelGGL((kernel<4, true>), dim3(grid), dim3(4 * NL), 0, stream, __VA_ARGS__);        \
    else if ((nw) == 4) hipLaunchKernelGGL((kernel<4, false>), dim3(grid), dim3(4 * NL), 0, stream, __VA_ARGS__);  \
    else hipLaunchKernelGGL((kernel<1, false>), dim3(grid), dim3(NL), 0, stream, __VA_ARGS__);                     \
  } while (0)

int evh_launch_find_homography(evh_ctx* c, const EvhRansacArgs& A) {
  if (int rc = check_lane_scratch(c, A)) return rc;
  EVH_LAUNCH_NW(waves_for(1, A.force_max), k_find_homography, 1, c->stream, A);
  return launched(c);
}
int evh_launch_static_filter(evh_ctx* c, const double* d_H, const float* d_rows, int n, int* d_rbin, float* d_out,
                             int* d_count) {
  hipLaunchKernelGGL((k_static_filter<4, false>), dim3(1), dim3(4 * NL), 0, c->stream, d_H, d_rows, n, d_rbin, d_out, d_count);
  return launched(c);
}
int evh_launch_ransac_static(evh_ctx* c, const EvhRansacArgs& A, int npairs) {
  if (npairs <= 0) return EVH_SUCCESS;
  if (int rc = check_lane_scratch(c, A)) return rc;
  if (A.force_max && npairs <= 256 && !getenv("EVH_SCAN_ONE_WG")) {        // a stream chunk: spread the samples of every pair
    if (int rc = launch_forced_static(c, A, npairs)) return rc;
    return launched(c);
  }
  EVH_LAUNCH_NW(waves_for(npairs, A.force_max), k_ransac_static, npairs, c->stream, A);
  return launched(c);
}
int evh_launch_ransac_final(evh_ctx* c, const EvhRansacArgs& A_, const EvhSolveLayout& L) {
  if (L.npairs <= 0) return EVH_SUCCESS;
  EvhRansacArgs A = A_;
  if (int rc = check_lane_scratch(c, A)) return rc;
  static const bool want_prof = getenv("EVH_RANSAC_PROF") != nullptr;   // debugging aid: cycle accounting to stderr
  unsigned long long* d_prof = nullptr;
  if (want_prof) {
    EVH_HIP(c, hipMalloc(&d_prof, sizeof(unsigned long long) * PF_NSLOTS));
    if (hipMemsetAsync(d_prof, 0, sizeof(unsigned long long) * PF_NSLOTS, c->stream) != hipSuccess) {
      (void)hipFree(d_prof);
      return evh_fail(c, EVH_ERR_HIP, "EVH_RANSAC_PROF: hipMemsetAsync failed");
    }
    A.prof = d_prof;
  }
  const bool ragged = L.kind == EvhSolveLayout::RAGGED;
  if (L.kind != EvhSolveLayout::PAIRS && A.force_max && !getenv("EVH_SCAN_ONE_WG")) {
    const int fr = ragged ? launch_forced_ragged(c, A, L.max_pairs, L.nstreams, RaggedStreams{L.d_segs}, 1, L.npairs, 0)
                          : launch_forced_scan(c, A, L.npairs, L.nstreams, L.pitch);
    if (fr) { if (d_prof) (void)hipFree(d_prof); return fr; }
  } else if (ragged) EVH_LAUNCH_NW(waves_for(L.nstreams, A.force_max), k_ransac_final_ragged, L.nstreams, c->stream, A, RaggedStreams{L.d_segs});
  else if (L.kind == EvhSolveLayout::STREAMS) EVH_LAUNCH_NW(waves_for(L.nstreams, A.force_max), k_ransac_final_stream, L.nstreams, c->stream, A, L.npairs, L.pitch);
  else EVH_LAUNCH_NW(waves_for(L.npairs, A.force_max), k_ransac_final_pairs, L.npairs, c->stream, A);
  {
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) { if (d_prof) (void)hipFree(d_prof); return evh_fail(c, EVH_ERR_HIP, std::string("k_ransac_final: ") + hipGetErrorString(le)); }
  }
  if (d_prof) {
    unsigned long long h[PF_NSLOTS];
    hipError_t pe = hipStreamSynchronize(c->stream);
    if (pe == hipSuccess) pe = hipMemcpy(h, d_prof, sizeof(h), hipMemcpyDeviceToHost);
    (void)hipFree(d_prof);                       // released on every path
    if (pe != hipSuccess) return evh_fail(c, EVH_ERR_HIP, std::string("EVH_RANSAC_PROF read-back: ") + hipGetErrorString(pe));
    const double n = h[PF_CALLS] ? (double)h[PF_CALLS] : 1.0;
    fprintf(stderr, "[evh ransac_final prof] calls %llu | per call (cycles): total %.0f hyp %.0f (chunks %.2f, dlt4+jacobi %.0f) "
            "compact %.0f refit %.0f lm %.0f (iters %.2f, solve8 %.0f, eval %.0f) | rotations: 9x9 %.1f 8x8 %.1f | chunk loop: rng %.0f "
            "count %.0f barrier %.0f replay %.0f | 4-wave eval: steps %.1f, busy per step wave0 (singles) %.0f wave1 (terms) %.0f wave2 (products) %.0f wave3 (pairs) %.0f, wave0 at the barrier %.0f\n",
            h[PF_CALLS], h[PF_TOTAL] / n, h[PF_HYP] / n, h[PF_CHUNKS] / n, h[PF_SETUP] / n, h[PF_COMPACT] / n,
            h[PF_REFIT] / n, h[PF_LM] / n, h[PF_LM_ITERS] / n, h[PF_SOLVE8] / n, h[PF_EVAL] / n, h[PF_ROT9] / n,
            h[PF_ROT8] / n, h[PF_RNG] / n, h[PF_COUNT] / n, h[PF_BARRIER] / n, h[PF_REPLAY] / n, h[PF_MW_STEPS] / n,
            h[PF_MW_W0] / (double)(h[PF_MW_STEPS] ? h[PF_MW_STEPS] : 1), h[PF_MW_W1] / (double)(h[PF_MW_STEPS] ? h[PF_MW_STEPS] : 1),
            h[PF_MW_W2] / (double)(h[PF_MW_STEPS] ? h[PF_MW_STEPS] : 1), h[PF_MW_W3] / (double)(h[PF_MW_STEPS] ? h[PF_MW_STEPS] : 1),
            h[PF_MW_WAIT] / (double)(h[PF_MW_STEPS] ? h[PF_MW_STEPS] : 1));
  }
  return EVH_SUCCESS;
}
