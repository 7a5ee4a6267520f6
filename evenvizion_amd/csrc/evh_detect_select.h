// evh_detect_select.h -- internal to evh_detect.hip (stage 3 of 5): canonical selection, key-point records
#pragma once
#include "evh_detect_fast.h"
namespace {
// K4: per frame, per level: retainBest(2*quota) by FAST score (all ties with the cut kept), Harris response,
// retainBest(quota) by Harris (ties kept), canonical order (y, x); writes keypoint records.
struct SelectArgs {
  EvhLevel lv[EVH_NLEVELS];
  const uint8_t* pyr; int64_t pyr_frame_bytes;
  const uint32_t* cand; int64_t cand_frame_entries;
  const int* cand_count;
  float* kp_xy; uint32_t* kp_meta; float* kp_resp; int* kp_count; int* frame_flags;
  uint32_t* tmp_meta; float* tmp_resp; int* lvl_count;   // per-level staging (segments at EvhLevel.kp_base)
  int kcap;
  int k1cap, k2cap;   // LDS capacities of k_select (stage-1 / stage-2 survivors of one level)
  int nframes;        // real frame count (the grid of k_select is padded, xcd_grid)
};

__device__ __forceinline__ float harris_response(const uint8_t* img, int stride, int x0, int y0) {
  // the 9 x 9 window (x0-4 .. x0+4, y0-4 .. y0+4) as three aligned dwords per row, realigned in registers:
  // 27 dword loads per key point instead of ~190 scattered byte loads (the texture-address path was the limit).
  // Integer sums are order-independent, the float tail below is unchanged.
  const int xa = (x0 - 4) & ~3;
  const uint32_t sh = (uint32_t)((x0 - 4) - xa);
  const uint32_t* base = reinterpret_cast<const uint32_t*>(img + (int64_t)(y0 - 4) * stride + xa);
  const int sd = stride >> 2;
  uint32_t w0[9], w1[9], w2[9];
#pragma unroll
  for (int r = 0; r < 9; r++) {
    const uint32_t d0 = base[r * sd], d1 = base[r * sd + 1], d2 = base[r * sd + 2];
    w0[r] = __builtin_amdgcn_alignbyte(d1, d0, sh);      // bytes x0-4 .. x0-1
    w1[r] = __builtin_amdgcn_alignbyte(d2, d1, sh);      // bytes x0 .. x0+3
    w2[r] = d2 >> (8 * sh);                              // byte x0+4 in bits 0..7
  }
#define HB(r, c) ((c) < 4 ? (int)((w0[r] >> (8 * (c))) & 0xFFu) : (c) < 8 ? (int)((w1[r] >> (8 * ((c) - 4))) & 0xFFu) : (int)(w2[r] & 0xFFu))
  int a = 0, b = 0, c = 0;
#pragma unroll
  for (int i = 1; i <= 7; i++) {          // window row i = y0 - 4 + i
#pragma unroll
    for (int j = 1; j <= 7; j++) {        // window column j = x0 - 4 + j
      const int Ix = (HB(i, j + 1) - HB(i, j - 1)) * 2 + (HB(i - 1, j + 1) - HB(i - 1, j - 1)) + (HB(i + 1, j + 1) - HB(i + 1, j - 1));
      const int Iy = (HB(i + 1, j) - HB(i - 1, j)) * 2 + (HB(i + 1, j - 1) - HB(i - 1, j - 1)) + (HB(i + 1, j + 1) - HB(i - 1, j + 1));
      a = mad24s(Ix, Ix, a); b = mad24s(Iy, Iy, b); c = mad24s(Ix, Iy, c);   // |Ix|, |Iy| <= 1020
    }
  }
#undef HB
  const float scale = 1.f / (4 * 7 * 255.f);
  const float scale_sq_sq = scale * scale * scale * scale;
  float fa = (float)a, fb = (float)b, fc = (float)c;
  float t1 = fa * fb;
  float t2 = fc * fc;
  float s = fa + fb;
  float t3 = (0.04f * s) * s;
  return ((t1 - t2) - t3) * scale_sq_sq;
}

__device__ __forceinline__ uint32_t f32_order_key(float v) {
  uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// All 256 threads: the largest bin d whose inclusive suffix sum (bins d..255) reaches `target`, and the sum of the bins
// above d.  Equals the serial scan "from 255 down, stop at the first bin where the running sum reaches target".
// hist must be complete (barrier before the call); the caller guarantees that the total reaches target.  sh: int[12].
__device__ __forceinline__ int block_suffix_cut(const uint32_t* hist, int target, int* sh, int& above) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int v = (int)hist[tid];
  int s = v;                                    // inclusive suffix sum inside the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_down(s, o); if (lane + o < 64) s += t; }
  if (lane == 0) sh[wv] = s;
  __syncthreads();
  int hi = 0;
  for (int w = wv + 1; w < 4; w++) hi += sh[w];
  const int suf = s + hi;
  const unsigned long long m = __ballot(suf >= target);
  if (lane == 0) sh[4 + wv] = m ? (wv * 64 + 63 - (int)__clzll(m)) : -1;
  __syncthreads();
  const int d = max(max(sh[4], sh[5]), max(max(sh[6], sh[7]), 0));
  if (tid == d) sh[8] = suf - v;
  __syncthreads();
  above = sh[8];
  return d;
}

// one workgroup per (level, frame): both retainBest stages + Harris + canonical order; results go to the level's
// segment of the frame's staging arrays, k_pack then concatenates the eight segments.
__global__ __launch_bounds__(256, 6) void k_select(SelectArgs A) {   // 75 VGPRs: 6 instead of 4 waves per SIMD, 0.42 -> 0.39 ms
  // dynamic LDS, sized by the launcher from the key-point budget: keys[k1cap] | resp[k1cap] | sel[k2cap] | selr[k2cap]
  extern __shared__ uint32_t sel_dyn[];
  const int K1CAP = A.k1cap, K2CAP = A.k2cap;
  uint32_t* keys = sel_dyn;
  float* resp = reinterpret_cast<float*>(keys + K1CAP);
  uint32_t* sel = reinterpret_cast<uint32_t*>(resp + K1CAP);
  float* selr = reinterpret_cast<float*>(sel + K2CAP);
  __shared__ uint32_t hist[256];
  __shared__ int sh_i[8];  // 1: k1, 2: k2
  __shared__ int sh_cut[12];
  int l, f;                      // the eight levels of a frame on one XCD: 0.54 -> 0.45 ms
  xcd_order(l, f);
  if (f >= A.nframes) return;    // grid padding (workgroup-uniform)
  const int tid = threadIdx.x;
  const EvhLevel L = A.lv[l];
  const uint32_t* cand = A.cand + (int64_t)f * A.cand_frame_entries + L.cand_off;
  const int n_raw = A.cand_count[f * EVH_NLEVELS + l];
  bool overflow = n_raw > L.cand_cap;
  const int n = min(n_raw, L.cand_cap);
  const int q = L.quota;
  int k2 = 0;
  if (n > 0 && q > 0) {
    // ---- stage 1: cut on the integer FAST score through a 256-bin histogram
    hist[tid] = 0;
    if (tid < 8) sh_i[tid] = 0;
    __syncthreads();
    if (n > 2 * q)
      for (int i = tid; i < n; i += 256) atomicAdd(&hist[cand_score(cand[i])], 1u);
    __syncthreads();
    uint32_t cut = 0;
    if (n > 2 * q) { int above; cut = (uint32_t)block_suffix_cut(hist, 2 * q, sh_cut, above); }   // workgroup-uniform branch
    for (int i = tid; i < n; i += 256) {
      uint32_t c = cand[i];
      if (cand_score(c) >= cut) {
        int slot = atomicAdd(&sh_i[1], 1);
        if (slot < K1CAP) keys[slot] = c;
      }
    }
    __syncthreads();
    const int k1 = sh_i[1];
    // retainBest keeps EVERY tie at the cut, so k1 has no bound but n (saturated / binary content ties massively on the
    // integer score).  More survivors than the LDS list holds: spill path -- nothing is stored, the survivors are
    // re-read from the candidate list and their Harris responses recomputed in each pass (same values, same cut).
    const bool spill = k1 > K1CAP;                       // workgroup-uniform
    const uint8_t* img = A.pyr + (int64_t)f * A.pyr_frame_bytes + L.off;
    // ---- Harris response of every stage-1 survivor
    if (!spill) {
      for (int j = tid; j < k1; j += 256) {
        uint32_t c = keys[j];
        resp[j] = harris_response(img, L.stride, cand_x(c), cand_y(c));
      }
    }
    __syncthreads();
    // every stage-1 survivor with its Harris response: from the LDS lists, or (spill) re-read and recomputed
    auto for_survivors = [&](auto body) {
      if (!spill) {
        for (int j = tid; j < k1; j += 256) body(keys[j], resp[j]);
      } else {
        for (int i = tid; i < n; i += 256) {
          const uint32_t c = cand[i];
          if (cand_score(c) < cut) continue;
          body(c, harris_response(img, L.stride, cand_x(c), cand_y(c)));
        }
      }
    };
    // ---- stage 2: value of the q-th largest response by a 4 x 8-bit radix select on order-preserving keys
    float cutf = -INFINITY;
    if (k1 > q) {
      uint32_t prefix = 0;
      int rem = q;
      for (int pass = 0; pass < 4; pass++) {
        const int shift = 24 - 8 * pass;
        hist[tid] = 0;
        __syncthreads();
        for_survivors([&](uint32_t, float r) {
          uint32_t u = f32_order_key(r);
          bool in = pass == 0 ? true : ((u >> (shift + 8)) == (prefix >> (shift + 8)));
          if (in) atomicAdd(&hist[(u >> shift) & 0xFFu], 1u);
        });
        __syncthreads();
        int above;
        const int d = block_suffix_cut(hist, rem, sh_cut, above);
        rem -= above;
        prefix |= (uint32_t)d << shift;
      }
      uint32_t u = (prefix & 0x80000000u) ? (prefix & 0x7FFFFFFFu) : ~prefix;
      cutf = __uint_as_float(u);
    }
    for_survivors([&](uint32_t c, float r) {
      if (r >= cutf) {
        int slot = atomicAdd(&sh_i[2], 1);
        if (slot < K2CAP) { sel[slot] = c; selr[slot] = r; }
      }
    });
    __syncthreads();
    k2 = sh_i[2];
    // the one hard bound left: a level cannot deliver more key points than a frame's slot holds (K2CAP == kcap);
    // such a frame is flagged (EVH_PAIR_CAPACITY for its pairs), never truncated silently
    if (k2 > K2CAP) { overflow = true; k2 = K2CAP; }
    // ---- canonical order inside the level: ascending (y, x) by rank counting
    for (int j = tid; j < k2; j += 256) {
      uint32_t kj = sel[j] & 0xFFFFFFu;
      int pos = 0;
      for (int i = 0; i < k2; i++) pos += ((sel[i] & 0xFFFFFFu) < kj) ? 1 : 0;
      int64_t o = ((int64_t)f * EVH_NLEVELS + l) * A.kcap + pos;
      A.tmp_meta[o] = ((uint32_t)l << 24) | kj;
      A.tmp_resp[o] = selr[j];
    }
  }
  if (tid == 0) {
    A.lvl_count[f * EVH_NLEVELS + l] = k2;
    if (overflow) atomicOr(&A.frame_flags[f], 1);
  }
}

// concatenates the per-level segments of one frame (canonical order = level, y, x) and derives kp.pt; a frame whose
// levels together hold more than kcap key points is flagged (its slot keeps the first kcap)
__global__ __launch_bounds__(256) void k_pack(SelectArgs A) {
  const int f = blockIdx.x, tid = threadIdx.x;
  int base = 0;
  for (int l = 0; l < EVH_NLEVELS; l++) {
    const EvhLevel L = A.lv[l];
    const int n = min(A.lvl_count[f * EVH_NLEVELS + l], A.kcap - base);
    if (n < A.lvl_count[f * EVH_NLEVELS + l] && tid == 0) atomicOr(&A.frame_flags[f], 1);
    for (int j = tid; j < n; j += 256) {
      const int64_t si = ((int64_t)f * EVH_NLEVELS + l) * A.kcap + j, o = (int64_t)f * A.kcap + base + j;
      const uint32_t m = A.tmp_meta[si];
      A.kp_meta[o] = m;
      A.kp_resp[o] = A.tmp_resp[si];
      A.kp_xy[2 * o] = (float)cand_x(m) * L.scale;          // keypoint.pt *= layerScale
      A.kp_xy[2 * o + 1] = (float)cand_y(m) * L.scale;
    }
    base += n;
  }
  if (tid == 0) A.kp_count[f] = base;
}

__device__ __forceinline__ float f32_from_order_key(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
}  // namespace
