// evh_detect_describe.h -- internal to evh_detect.hip (stage 5 of 5): orientation and steered BRIEF
#pragma once
#include "evh_devmath.h"
#include "evh_detect_pyr.h"
namespace {
// K5 + K6: one wavefront per keypoint.  The 45x45 raw neighbourhood is staged in LDS once (16-byte loads) and serves the
// intensity-centroid orientation (radius-15 disc), the 7x7 sigma-2 fixed-point Gaussian (only the 39x39 region
// the steered taps can reach) and the 256 rotated BRIEF tests (4 x 64-lane ballots = the 32 descriptor bytes).
struct DescribeArgs {
  EvhLevel lv[EVH_NLEVELS];
  const uint8_t* pyr; int64_t pyr_frame_bytes;
  const float* kp_xy; const uint32_t* kp_meta; const int* kp_count;
  float* kp_angle; uint8_t* desc;
  int kcap;
};

__constant__ int8_t c_pattern[256 * 4] = {
#include "orb_pattern.inc"
};
// byte masks of the radius-15 disc: c_omask[|v|][d] selects the bytes c = 4d..4d+3 of patch row v with |c - 22| <= umax[|v|]
__constant__ uint32_t c_omask[16][10] = {
  {0x00000000u, 0xFF000000u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x0000FFFFu},
  {0x00000000u, 0xFF000000u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x0000FFFFu},
  {0x00000000u, 0xFF000000u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x0000FFFFu},
  {0x00000000u, 0xFF000000u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x0000FFFFu},
  {0x00000000u, 0x00000000u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x000000FFu},
  {0x00000000u, 0x00000000u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x000000FFu},
  {0x00000000u, 0x00000000u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x000000FFu},
  {0x00000000u, 0x00000000u, 0xFFFFFF00u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x00000000u},
  {0x00000000u, 0x00000000u, 0xFFFFFF00u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x00000000u},
  {0x00000000u, 0x00000000u, 0xFFFF0000u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x00FFFFFFu, 0x00000000u},
  {0x00000000u, 0x00000000u, 0xFF000000u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x0000FFFFu, 0x00000000u},
  {0x00000000u, 0x00000000u, 0x00000000u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x000000FFu, 0x00000000u},
  {0x00000000u, 0x00000000u, 0x00000000u, 0xFFFFFF00u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x00000000u, 0x00000000u},
  {0x00000000u, 0x00000000u, 0x00000000u, 0xFFFF0000u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x00FFFFFFu, 0x00000000u, 0x00000000u},
  {0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x000000FFu, 0x00000000u, 0x00000000u},
  {0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0xFF000000u, 0xFFFFFFFFu, 0x0000FFFFu, 0x00000000u, 0x00000000u, 0x00000000u}};

#define DP_R 22                 // raw neighbourhood radius
#define DP_N (2 * DP_R + 1)     // 45
#define DP_STRIDE4 17           // dwords per staged row: 16 loaded + 1 (odd dword stride: row-per-lane reads are conflict-free)
#define DB_R 19                 // blurred radius reachable by steered taps
#define DB_N (2 * DB_R + 1)     // 39
#define DH_STRIDE 41            // u16 per row of the horizontal-pass buffer (odd: conflict-free row-per-lane writes)
#define DW_PER_BLOCK 4

// 7-tap sigma-2 kernel, symmetric: 18 34 49 55 49 34 18 (byte / 16-bit dot products in k_describe)
__global__ __launch_bounds__(64 * DW_PER_BLOCK, 8) void k_describe(DescribeArgs A) {
  // ONE LDS region per wave (3.7 KB), used in turn as the raw patch (45 x 68 B), the horizontal-pass buffer
  // (45 x 41 u16) and the blurred patch (39 x 39 B): every pass first loads all it needs into registers, a
  // wave-level fence follows, only then does it store the next form over the same words.  14.8 KB per workgroup.
  __shared__ uint32_t patch32[DW_PER_BLOCK][(DP_N * DH_STRIDE + 2) / 2 + 1];
  static_assert(DP_N * DP_STRIDE4 <= (DP_N * DH_STRIDE + 2) / 2 + 1 && DB_N * DB_N <= 4 * ((DP_N * DH_STRIDE + 2) / 2 + 1), "forms share one region");
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t* raw = patch32[wv];
  uint16_t* hb = reinterpret_cast<uint16_t*>(patch32[wv]);
  uint8_t* blurp = reinterpret_cast<uint8_t*>(patch32[wv]);
  const int f = blockIdx.y;      // (XCD order measured 2 % slower here)
  const int k = blockIdx.x * DW_PER_BLOCK + wv;
  if (k >= A.kp_count[f]) return;  // whole wave exits; only wave-level synchronisation is used below
  const int64_t o = (int64_t)f * A.kcap + k;
  const uint32_t meta = A.kp_meta[o];
  const int l = (int)(meta >> 24);
  const EvhLevel L = A.lv[l];
  // centre exactly as computeOrbDescriptors recovers it from kp.pt
  const float inv = 1.f / L.scale;
  const int cx = (int)rintf(A.kp_xy[2 * o] * inv), cy = (int)rintf(A.kp_xy[2 * o + 1] * inv);
  const uint8_t* img = A.pyr + (int64_t)f * A.pyr_frame_bytes + L.off;
  // the 45-byte patch rows lie inside the 64 bytes from the 16-byte boundary below their first pixel: each row is
  // four aligned 16-byte loads (180 per patch = 3 per lane, no division), stored with a 17-dword row stride
  // (odd: the row-per-lane reads below are conflict-free).  A key point is >= 31 px from every border of its level
  // and rows are padded to 64 bytes, so the window never leaves the level's rows.
  const int xs = cx - DP_R, xa = xs & ~15, shq = (xs - xa) >> 2;
  const uint32_t sh = (uint32_t)(xs & 3);
  {
    // 45 rows x 4 cells = 180 cells, lane = (row & 15, cell) three times over; the third round covers rows 32..47: its
    // loads are clamped to row 44 and its stores of rows 45..47 land in the part of the wave's region the raw form does
    // not use -- no predicate, so all three requests are in flight before the first store (the predicated form
    // compiled to two loads, wait, third load, wait)
    static_assert(47 * DP_STRIDE4 + 16 <= (DP_N * DH_STRIDE + 2) / 2 + 1, "rows 45..47 fit behind the raw patch");
    const uint4* src = reinterpret_cast<const uint4*>(img + xa);
    const int stride16 = L.stride >> 4;
    const int r0 = lane >> 2, c = lane & 3;
    uint4 v[3];
#pragma unroll
    for (int k = 0; k < 3; k++)
      v[k] = src[mad24((uint32_t)(cy - DP_R + min(r0 + 16 * k, DP_N - 1)), (uint32_t)stride16, (uint32_t)c)];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      uint32_t* d = raw + (r0 + 16 * k) * DP_STRIDE4 + c * 4;
      d[0] = v[k].x; d[1] = v[k].y; d[2] = v[k].z; d[3] = v[k].w;
    }
  }
  WAVE_LDS_SYNC();
  // ---- one lane per patch row: realign the row to the patch origin, then (a) orientation moments over the
  //      radius-15 disc and (b) the horizontal 7-tap pass with a sliding window
  int m10 = 0, m01 = 0;
  uint32_t w[12];
  if (lane < DP_N) {
    const uint32_t* rp = raw + lane * DP_STRIDE4 + shq;
#pragma unroll
    for (int j = 0; j < 12; j++) w[j] = __builtin_amdgcn_alignbyte(rp[j + 1], rp[j], sh);
  }
  WAVE_LDS_SYNC();      // every row is in registers: the region may now take the horizontal-pass values
  if (lane < DP_N) {
    const int v = lane - DP_R;
    // intensity-centroid moments over the disc as byte dot products: row bytes masked by the disc's extent in this
    // row, s0 = sum I, s1 = sum (u + 15) I - 15 s0 with u = c - 22 (weights 0..30 fit a byte); same integers as the
    // per-pixel sums
    int s0 = 0, s1 = 0;
    if (abs(v) <= 15) {
      const uint32_t* mk = c_omask[abs(v)];
      uint32_t a0 = 0, a1 = 0;
#pragma unroll
      for (int d = 1; d <= 9; d++) {               // bytes 4 .. 39 cover c = 7 .. 37
        const uint32_t x = w[d] & mk[d];
        const int u0 = 4 * d - DP_R + 15;          // weight of the dword's first byte; bytes outside 0..30 are masked off
        const uint32_t wt = ((uint32_t)(u0 & 0xFF)) | ((uint32_t)((u0 + 1) & 0xFF) << 8) | ((uint32_t)((u0 + 2) & 0xFF) << 16) |
                            ((uint32_t)((u0 + 3) & 0xFF) << 24);
        a0 = __builtin_amdgcn_udot4(x, 0x01010101u, a0, false);
        a1 = __builtin_amdgcn_udot4(x, wt, a1, false);
      }
      s0 = (int)a0; s1 = (int)a1 - 15 * (int)a0;
    }
    m10 = s1; m01 = v * s0;
    // horizontal 7-tap pass as byte dot products: X(c) = the dword of bytes c..c+3 of the realigned row (every fourth
    // one is a register as it stands, the others one v_alignbyte), h(c) = dot4(X(c), {18,34,49,55}) +
    // dot4(X(c+4), {49,34,18,0}) -- the same integer as gauss7 on the seven bytes
    uint16_t* hrow = hb + lane * DH_STRIDE;
    uint32_t X[DB_N + 4];
#pragma unroll
    for (int c = 0; c < DB_N + 4; c++)
      X[c] = (c & 3) == 0 ? w[c >> 2] : __builtin_amdgcn_alignbyte(w[(c >> 2) + 1], w[c >> 2], (uint32_t)(c & 3));
    const uint32_t W0 = 18u | (34u << 8) | (49u << 16) | (55u << 24), W1 = 49u | (34u << 8) | (18u << 16);
#pragma unroll
    for (int c = 0; c < DB_N; c++)
      hrow[c] = (uint16_t)__builtin_amdgcn_udot4(X[c + 4], W1, __builtin_amdgcn_udot4(X[c], W0, 0u, false), false);
  }
  for (int s = 32; s > 0; s >>= 1) { m10 += __shfl_xor(m10, s); m01 += __shfl_xor(m01, s); }
  const float angle = fast_atan2_deg((float)m01, (float)m10);
  WAVE_LDS_SYNC();
  // ---- one lane per blurred column: vertical 7-tap pass down the 45 rows.  The column is held as PAIRS of
  //      consecutive rows (h[2j] | h[2j+1] << 16: the second ds_read_u16 of a pair lands in the high half of the same
  //      register), an output row is then four v_dot2_u32_u16 with the tap pairs (18,34)(49,55)(49,34)(18,0) or
  //      (0,18)(34,49)(55,49)(34,18) -- the same integer as gauss7 on the seven values, 4 instead of 9 operations
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  u16x2 P[(DP_N + 1) / 2];
  if (lane < DB_N) {
    const uint16_t* hc = hb + lane;
#pragma unroll
    for (int j = 0; j < DP_N / 2; j++) { P[j].x = hc[(2 * j) * DH_STRIDE]; P[j].y = hc[(2 * j + 1) * DH_STRIDE]; }
    P[DP_N / 2].x = hc[(DP_N - 1) * DH_STRIDE]; P[DP_N / 2].y = 0;       // row 45 does not exist (its tap weight is 0)
  }
  WAVE_LDS_SYNC();      // every column is in registers: the region may now take the blurred patch
  if (lane < DB_N) {
    const u16x2 WE[4] = {{18, 34}, {49, 55}, {49, 34}, {18, 0}}, WO[4] = {{0, 18}, {34, 49}, {55, 49}, {34, 18}};
#pragma unroll
    for (int r = 0; r < DB_N; r++) {              // output row r = taps on rows r .. r + 6 of the 45
      uint32_t sum = 32768u;
#pragma unroll
      for (int q = 0; q < 4; q++) sum = __builtin_amdgcn_udot2(P[(r >> 1) + q], (r & 1) ? WO[q] : WE[q], sum, false);
      blurp[r * DB_N + lane] = (uint8_t)(min(sum, 0x00FFFFFFu) >> 16);   // saturating store: 255 * 257 * 257 + 32768 >> 16 = 257
    }
  }
  WAVE_LDS_SYNC();
  // ---- steered BRIEF
  const float ang = angle * (float)(3.14159265358979323846 / 180.f);
  double sd, cd;
  det_sincos((double)ang, &sd, &cd);
  const float a = (float)cd, b = (float)sd;
  unsigned long long bits[4];
#pragma unroll
  for (int m = 0; m < 4; m++) {
    const int8_t* p = c_pattern + (lane + 64 * m) * 4;
    float px0 = (float)p[0], py0 = (float)p[1], px1 = (float)p[2], py1 = (float)p[3];
    float fx0 = px0 * a - py0 * b, fy0 = px0 * b + py0 * a;
    float fx1 = px1 * a - py1 * b, fy1 = px1 * b + py1 * a;
    int t0 = blurp[((int)rintf(fy0) + DB_R) * DB_N + (int)rintf(fx0) + DB_R];
    int t1 = blurp[((int)rintf(fy1) + DB_R) * DB_N + (int)rintf(fx1) + DB_R];
    bits[m] = __ballot(t0 < t1);
  }
  if (lane < 4) reinterpret_cast<unsigned long long*>(A.desc + o * 32)[lane] = bits[lane];
  if (lane == 0) A.kp_angle[o] = angle;
}
}  // namespace
