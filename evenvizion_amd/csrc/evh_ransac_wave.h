// evh_ransac_wave.h -- internal to evh_ransac.hip (layer 1 of 4): lane / row constants, wave-level primitives, cycle accounting
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
namespace {
#define NL 64          // lanes of a wavefront
#define NG 4           // 16-lane rows per wavefront: one eigen-problem (one RANSAC hypothesis) per row
#define GL 16          // lanes per row
typedef double d2_t __attribute__((ext_vector_type(2)));

// Ordering point between a cross-lane write and read of LDS / global scratch INSIDE one wavefront.  DS (and VMEM)
// operations of one wave execute in order, so no wait is needed: this only pins the compiler's ordering.
#define WSYNC()                                                \
  do {                                                         \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");     \
    __builtin_amdgcn_wave_barrier();                           \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");     \
  } while (0)

// ---- cross-lane reductions inside a 16-lane row (or one of its 8-lane halves) as DPP-fused integer min / max ------
#define DPP_XOR1 0xB1          // quad_perm [1,0,3,2]
#define DPP_XOR2 0x4E          // quad_perm [2,3,0,1]
#define DPP_HALF_MIRROR 0x141
#define DPP_ROW_MIRROR 0x140
template <int CTRL>
__device__ __forceinline__ unsigned dmax(unsigned v) {
  return max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true));
}
template <int CTRL>
__device__ __forceinline__ unsigned dmin(unsigned v) {
  return min(v, (unsigned)__builtin_amdgcn_update_dpp(-1, (int)v, CTRL, 0xF, 0xF, false));
}
template <int CTRL>
__device__ __forceinline__ int dadd(int v) { return v + __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true); }
__device__ __forceinline__ unsigned rmax8(unsigned v) { return dmax<DPP_HALF_MIRROR>(dmax<DPP_XOR2>(dmax<DPP_XOR1>(v))); }
__device__ __forceinline__ unsigned rmin8(unsigned v) { return dmin<DPP_HALF_MIRROR>(dmin<DPP_XOR2>(dmin<DPP_XOR1>(v))); }
__device__ __forceinline__ unsigned rmax16(unsigned v) { return dmax<DPP_ROW_MIRROR>(rmax8(v)); }
__device__ __forceinline__ unsigned rmin16(unsigned v) { return dmin<DPP_ROW_MIRROR>(rmin8(v)); }
__device__ __forceinline__ int rsum16(int v) {
  return dadd<DPP_ROW_MIRROR>(dadd<DPP_HALF_MIRROR>(dadd<DPP_XOR2>(dadd<DPP_XOR1>(v))));
}
// c ? a : b as one v_cndmask_b32 (the optimiser otherwise turns the candidate updates into exec-mask branches)
__device__ __forceinline__ unsigned vsel(bool c, unsigned a, unsigned b) {
  unsigned r;
  const unsigned long long m = __builtin_amdgcn_ballot_w64(c);
  asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(b), "v"(a), "s"(m));
  return r;
}
__device__ __forceinline__ unsigned hi32(double v) { return (unsigned)__double2hiint(v); }
__device__ __forceinline__ unsigned lo32(double v) { return (unsigned)__double2loint(v); }
__device__ __forceinline__ double mk64(unsigned hi, unsigned lo) { return __hiloint2double((int)hi, (int)lo); }

// ---- exact f64 divide / square root without the range scaling (same instruction sequences the compiler emits for
//      `/` and sqrt(), minus v_div_scale / v_div_fixup / v_ldexp): bit-identical whenever no intermediate leaves the
//      normal range, which the callers guarantee (and check) ------------------------------------------------------
struct Recip { double den, r; };
__device__ __forceinline__ Recip recip_refined(double den) {
  double r = __builtin_amdgcn_rcp(den);
  double e = fma(-den, r, 1.0);
  r = fma(r, e, r);
  e = fma(-den, r, 1.0);
  r = fma(r, e, r);
  return Recip{den, r};
}
__device__ __forceinline__ double div_by(double num, const Recip& R) {
  const double q = num * R.r;
  const double rem = fma(-R.den, q, num);
  return fma(rem, R.r, q);
}
__device__ __forceinline__ double sqrt_1_2(double x) {  // x in [1, 2]
  const double y = __builtin_amdgcn_rsq(x);
  double g = x * y, h = y * 0.5;
  const double r = fma(-h, g, 0.5);
  g = fma(g, r, g);
  h = fma(h, r, h);
  double d = fma(-g, g, x);
  g = fma(d, h, g);
  d = fma(-g, g, x);
  g = fma(d, h, g);
  return g;
}

__device__ __forceinline__ double hyp(double a, double b) {
  a = fabs(a); b = fabs(b);
  if (a > b) { b /= a; return a * sqrt(1 + b * b); }
  if (b > 0) { a /= b; return b * sqrt(1 + a * a); }
  return 0;
}
// the rotation scalars of one Jacobi step, plain form (reference order of operations)
struct Cst { double c, s, t; };
__device__ __forceinline__ Cst rotation_scalars_plain(double p, double wk, double wl) {
  const double y = (wl - wk) * 0.5;
  double tt = fabs(y) + hyp(p, y);
  double sn = hyp(p, tt);
  Cst r;
  r.c = tt / sn;
  sn = p / sn; tt = (p / tt) * p;
  if (y < 0) sn = -sn, tt = -tt;
  r.s = sn; r.t = tt;
  return r;
}
// the same values with the short sequences: |p| > DBL_EPSILON is given, so hyp(p, y) >= |p| > 0, t >= |p| and the
// second hyp() always takes its "b >= a" branch; (p / t) * p == (|p| / t) * |p| because IEEE division and
// multiplication are sign-symmetric.  The caller has checked that no operand can be too large for the unscaled
// sequences (small ones are harmless: a quotient that loses its last bits is one whose square vanishes against 1).
__device__ __forceinline__ void rotation_scalars(double p, double wk, double wl, double& c, double& s, double& t) {
  const double y = (wl - wk) * 0.5;
  const double ap = fabs(p), ay = fabs(y);
  const bool pg = ap > ay;
  const double hi = pg ? ap : ay;
  const double lo = pg ? ay : ap;             // (a quotient too small for the short divide also vanishes against 1)
  const double q = div_by(lo, recip_refined(hi));
  const double h = hi * sqrt_1_2(1.0 + q * q);
  const double tt = ay + h;
  const double q2 = div_by(ap, recip_refined(tt));
  const double sn = tt * sqrt_1_2(1.0 + q2 * q2);
  const Recip rs = recip_refined(sn);
  c = div_by(tt, rs);
  double ss = div_by(p, rs);
  double t2 = q2 * ap;
  if (y < 0) ss = -ss, t2 = -t2;
  s = ss; t = t2;
}

__device__ __forceinline__ int wave_sum(int v) {
  for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
  return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int sft = 32; sft > 0; sft >>= 1) v += __shfl_xor(v, sft);
  return v;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
  for (int sft = 32; sft > 0; sft >>= 1) { const unsigned long long o = __shfl_xor(v, sft); v = o > v ? o : v; }
  return v;
}

// optional in-kernel cycle accounting (EVH_RANSAC_PROF=1): slots of A.prof, accumulated by thread 0
enum { PF_CALLS = 0, PF_HYP, PF_CHUNKS, PF_COMPACT, PF_REFIT, PF_LM, PF_LM_ITERS, PF_SOLVE8, PF_EVAL, PF_TOTAL, PF_ROT9,
       PF_ROT8, PF_SETUP, PF_RNG, PF_COUNT, PF_BARRIER, PF_REPLAY, PF_MW_W0, PF_MW_W1, PF_MW_W2, PF_MW_W3, PF_MW_WAIT, PF_MW_STEPS, PF_NSLOTS };
__device__ __forceinline__ unsigned long long pf_now() { return __builtin_readcyclecounter(); }
// inside loops: s_memtime is a scalar memory instruction -- its result is waited for with lgkmcnt(0), which also drains every
// LDS read in flight -- so the counter is read only when the accounting is on (prof is wave-uniform)
__device__ __forceinline__ unsigned long long pf_now_if(const unsigned long long* prof) { return prof ? __builtin_readcyclecounter() : 0ull; }
__device__ __forceinline__ void pf_add(unsigned long long* prof, int slot, unsigned long long v) {
  if (prof && threadIdx.x == 0) atomicAdd(prof + slot, v);
}
__device__ __forceinline__ void pf_add_wave(unsigned long long* prof, int slot, unsigned long long v) {   // lane 0 of any wave
  if (prof && (threadIdx.x & 63) == 0) atomicAdd(prof + slot, v);
}
}  // namespace
