// evh_detect_pyr.h -- internal to evh_detect.hip (stage 1 of 5): gray conversion, the pyramid kernels, XCD workgroup order
#pragma once
#include "evh_internal.h"
namespace {
__device__ __forceinline__ uint32_t gdot4(uint32_t a, uint32_t b, uint32_t acc) {
  return __builtin_amdgcn_udot4(a, b, acc, false);
}
// 4 gray pixels from 12 BGR bytes in three dwords: B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
__device__ __forceinline__ uint32_t gray_bgr12(uint32_t w0, uint32_t w1, uint32_t w2) {
  // weights split in bytes (1868 = 7*256 + 76, 9617 = 37*256 + 145, 4899 = 19*256 + 35): two v_dot4_u32_u8 per
  // pixel on the dword that holds its B,G,R (the fourth byte meets a zero weight); same integers as the scalar form
  const uint32_t WL = 76u | (145u << 8) | (35u << 16), WH = 7u | (37u << 8) | (19u << 16);
  const uint32_t p1 = __builtin_amdgcn_alignbyte(w1, w0, 3), p2 = __builtin_amdgcn_alignbyte(w2, w1, 2);
  const uint32_t y0 = (gdot4(w0, WL, 8192u) + (gdot4(w0, WH, 0u) << 8)) >> 14;
  const uint32_t y1 = (gdot4(p1, WL, 8192u) + (gdot4(p1, WH, 0u) << 8)) >> 14;
  const uint32_t y2 = (gdot4(p2, WL, 8192u) + (gdot4(p2, WH, 0u) << 8)) >> 14;
  const uint32_t y3 = (gdot4(w2, WL << 8, 8192u) + (gdot4(w2, WH << 8, 0u) << 8)) >> 14;
  return __builtin_amdgcn_perm(y1, y0, 0x0C0C0400u) | __builtin_amdgcn_perm(y3, y2, 0x04000C0Cu);
}
// 4 gray pixels (n < 4 at the right edge) from `s`: Y = (B*1868 + G*9617 + R*4899 + 8192) >> 14, or a plain copy
__device__ __forceinline__ uint32_t gray_quad(const uint8_t* __restrict__ s, int channels, int n, int aligned4) {
  uint32_t out = 0;
  if (aligned4 && n == 4) {
    if (channels == 1) out = *reinterpret_cast<const uint32_t*>(s);
    else {
      const uint32_t* s4 = reinterpret_cast<const uint32_t*>(s);
      out = gray_bgr12(s4[0], s4[1], s4[2]);
    }
  } else if (channels == 1) {
    for (int i = 0; i < n; i++) out |= (uint32_t)s[i] << (8 * i);
  } else {
    for (int i = 0; i < n; i++) {
      uint32_t b = s[3 * i], g = s[3 * i + 1], r = s[3 * i + 2];
      out |= ((b * 1868u + g * 9617u + r * 4899u + 8192u) >> 14) << (8 * i);
    }
  }
  return out;
}

// ------------------------------------------------------------------------------------------------------------
// K1: BGR -> gray (Y = (B*1868 + G*9617 + R*4899 + 8192) >> 14) or gray copy, into pyramid level 0.
// One thread = 4 output pixels: three aligned dword loads (12 BGR bytes) -> one dword store; grid.y = frame.
__global__ void k_gray_level0(const uint8_t* __restrict__ src, int channels, int64_t row_stride, int64_t frame_stride,
                              uint8_t* __restrict__ pyr, int64_t pyr_frame_bytes, int w, int h, int dst_stride,
                              int aligned4) {
  const int f = blockIdx.y;
  const int qpr = (w + 3) >> 2;
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= qpr * h) return;
  const int y = q / qpr, x = (q - y * qpr) * 4;
  const uint8_t* s = src + (int64_t)f * frame_stride + (int64_t)y * row_stride + (int64_t)x * channels;
  uint8_t* d = pyr + (int64_t)f * pyr_frame_bytes + (int64_t)y * dst_stride + x;
  const uint32_t out = gray_quad(s, channels, min(4, w - x), aligned4);
  *reinterpret_cast<uint32_t*>(d) = out;  // rows are 64-byte aligned and padded, a full dword is always in range
}

// ------------------------------------------------------------------------------------------------------------
// K2: pyramid level l from level l-1, resize(INTER_LINEAR_EXACT): 8.8 fixed-point weights per axis,
// out = ((c0*s00 + c1*s01)*m0 + (c0*s10 + c1*s11)*m1 + 32768) >> 16.  Tables (host-computed): per dst column
// (xofs, xc1), per dst row (yofs, yc1); edge replication is encoded in the tables.
// Workgroup = 128 x 64 output pixels (PDN_H); the source footprint (<= 176 x 82 bytes at scale 1.2) is staged in LDS
// with 16-byte loads, each thread then produces 8 rows x 4 pixels from LDS bytes and stores one dword per row.
__device__ __forceinline__ uint32_t mad24(uint32_t a, uint32_t b, uint32_t c) {   // a*b + c, a,b < 2^24 (half-rate VALU;
  uint32_t r; asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r;   // v_mul_lo_u32 / v_mad_u64_u32 are far slower)
}
// NEVER feed a v_dot4 result to these asm forms: a VALU read of a DOT result needs three wait states on gfx950 and the
// hazard recogniser does not look inside an asm statement (measured in round 2: stale reads, wrong pixels).
__device__ __forceinline__ int mad24s(int a, int b, int c) {   // signed a*b + c, |a|,|b| < 2^23
  int r; asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r;
}
// XCD-aware workgroup order.  The dispatcher deals workgroups round-robin to the 8 XCDs (linear id n -> XCD n % 8),
// each with its own L2: neighbouring tiles of one image then sit on eight different L2s, every shared cache line is
// fetched (and every partial line written back) once per XCD and DRAM sees eight interleaved walks.  Remapped, XCD k
// works through one contiguous eighth of the frames, tile after tile.  Measured with tools/ubench/bw_tile.hip on the
// shape of k_gray_pyr1 (480 B x 40 rows): 3.8 -> 5.2 TB/s; on 240 B x 80 rows: 2.5 -> 4.8 TB/s.
// Division-free: BOTH grid dimensions are launched rounded up to a multiple of 8 (xcd_grid), so XCD = blockIdx.x & 7,
// and the caller drops the (tile, frame) pairs past the real counts.
__device__ __forceinline__ void xcd_order(int& tile, int& frame) {
  const uint32_t x = blockIdx.x, y = blockIdx.y;
  tile = (int)((y & 7u) * (gridDim.x >> 3) + (x >> 3));
  frame = (int)((x & 7u) * (gridDim.y >> 3) + (y >> 3));
}
// q = v / d for v * d < 2^20 (tile index / tiles per row), magic = floor(2^20 / d) + 1 from the host
__device__ __forceinline__ int div_magic20(int v, int magic) { return (int)(((uint32_t)v * (uint32_t)magic) >> 20); }
// this workgroup's frame and tile (tx, ty) in XCD order and the tile's origin; false: grid padding (workgroup-uniform)
template <int W, int H>
__device__ __forceinline__ bool pyr_tile_origin(int tiles_x, int tx_magic, int ntiles, int nframes, int& f, int& tx, int& ty,
                                                int& x0, int& y0) {
  int bt;
  xcd_order(bt, f);
  if (bt >= ntiles || f >= nframes) return false;
  ty = div_magic20(bt, tx_magic); tx = bt - ty * tiles_x;
  x0 = tx * W; y0 = ty * H;
  return true;
}
// ordering point between LDS writes and reads of different lanes INSIDE one wave (the other waves are not waited for)
#define WAVE_LDS_SYNC()                                    \
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   \
  __builtin_amdgcn_wave_barrier();                         \
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup")
#define PD_W 128
#define PD_H 32
#define PD_SW 192   // staged source row bytes (multiple of 16, >= 1.2*128 + 4 + 15 of slack and alignment)
#define PD_SH 44    // staged source rows (>= 1.2*32 + 5)
// k_pyr_down: output rows per tile.  64 amortises the per-workgroup set-up (tap tables, footprint, ~160 scalar and
// vector instructions) and the two halo rows over twice the pixels: 2.18 -> 1.95 ms for the six launches; 48 rows
// 2.02, 96 rows 2.13, 128 rows 2.5 (LDS then allows 5 workgroups per CU).  k_gray_pyr1 keeps PD_H = 32: its BGR
// staging lives in registers.
#define PDN_H 64
#define PDN_SH (PDN_H * 121 / 100 + 5)   // staged source rows
// the output loop shared by k_pyr_down and k_gray_pyr1: a ROWS x 128 tile from its staged source rows (PITCH bytes apart) and
// the tile's tap tables in LDS; each thread produces ROWS / 8 rows x 4 pixels and stores one dword per row
template <int ROWS, int PITCH>
__device__ __forceinline__ void pyr_rows_from_tile(const uint8_t* tile, const int* xo_s, const int* xc_s, const int* yo_s,
                                                   const int* yc_s, uint8_t* dimg, int dst_stride, int x0, int y0, int dw,
                                                   int dh) {
  const int qx = threadIdx.x & 31, qy = threadIdx.x >> 5;     // 32 quads across, 8 groups of ROWS / 8 rows down
  const int x = x0 + qx * 4;
  if (x >= dw) return;
#pragma unroll
  for (int rr = 0; rr < ROWS / 8; rr++) {
    const int y = y0 + qy * (ROWS / 8) + rr;
    if (y >= dh) break;
    const uint8_t* r0 = tile + yo_s[qy * (ROWS / 8) + rr] * PITCH;
    const uint8_t* r1 = r0 + PITCH;
    const int m1 = yc_s[qy * (ROWS / 8) + rr];
    // (c0*a + c1*b)*m0 + (c0*a' + c1*b')*m1 + 32768, c0 = 256 - c1, m0 = 256 - m1: 24-bit multiply-adds only (a
    // multiply-add costs the same issue slot as a shift here); the result byte sits in bits 16..23 of v[i] and two
    // v_perm_b32 gather the four of them
    const uint32_t m0 = 256u - (uint32_t)m1;
    uint32_t v[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int o = xo_s[qx * 4 + i];
      const uint32_t c1 = (uint32_t)xc_s[qx * 4 + i], c0 = 256u - c1;
      const uint32_t a0 = r0[o], b0 = r0[o + 1], a1 = r1[o], b1 = r1[o + 1];
      const uint32_t h0 = mad24(a0, c0, mad24(b0, c1, 0u));
      const uint32_t h1 = mad24(a1, c0, mad24(b1, c1, 0u));
      v[i] = mad24(h0, m0, mad24(h1, (uint32_t)m1, 32768u));
    }
    const uint32_t out = __builtin_amdgcn_perm(v[1], v[0], 0x0C0C0602u) | __builtin_amdgcn_perm(v[3], v[2], 0x06020C0Cu);
    reinterpret_cast<uint32_t*>(dimg)[mad24((uint32_t)y, (uint32_t)(dst_stride >> 2), (uint32_t)(x >> 2))] = out;
  }
}

__global__ __launch_bounds__(256) void k_pyr_down(uint8_t* __restrict__ pyr, int64_t pyr_frame_bytes, int64_t src_off,
                                                  int src_stride, int64_t dst_off, int dst_stride, int dw,
                                                  int dh, int tiles_x, int tx_magic, int ntiles, int nframes,
                                                  const int* __restrict__ xofs, const int* __restrict__ xc1,
                                                  const int* __restrict__ yofs, const int* __restrict__ yc1) {
  __shared__ uint32_t tile32[PDN_SH * PD_SW / 4];
  __shared__ int xo_s[PD_W]; __shared__ int xc_s[PD_W]; __shared__ int yo_s[PDN_H]; __shared__ int yc_s[PDN_H];
  int f, tx, ty, x0, y0;
  if (!pyr_tile_origin<PD_W, PDN_H>(tiles_x, tx_magic, ntiles, nframes, f, tx, ty, x0, y0)) return;
  const int x1 = min(x0 + PD_W, dw) - 1, y1 = min(y0 + PDN_H, dh) - 1;
  // source footprint straight from the tap tables (scalar loads; a right / bottom edge tap is encoded as
  // (size - 2, weight 256), so ofs + 1 is always inside the source)
  const int sx0 = xofs[x0] & ~15, sy0 = yofs[y0];
  const int ex = xofs[x1] + 1, ey = yofs[y1] + 1;
  const int ncol16 = (ex - sx0) / 16 + 1, nrow = ey - sy0 + 1;     // <= PD_SW/16 = 11, <= PDN_SH
  uint8_t* base = pyr + (int64_t)f * pyr_frame_bytes;   // wave-uniform 64-bit bases; per-lane offsets stay 32-bit
  const uint8_t* simg = base + src_off + sx0;
  uint8_t* dimg = base + dst_off;
  // exact taps of this tile's 128 columns / PDN_H rows from the host tables (independent of the staging loads)
  if (threadIdx.x < PD_W) {
    const int xi = min(x0 + (int)threadIdx.x, dw - 1);
    xo_s[threadIdx.x] = xofs[xi] - sx0; xc_s[threadIdx.x] = xc1[xi];
  } else if (threadIdx.x < PD_W + PDN_H) {
    const int r = threadIdx.x - PD_W, yi = min(y0 + r, dh - 1);
    yo_s[r] = yofs[yi] - sy0; yc_s[r] = yc1[yi];
  }
  {
    // 16-byte loads: a thread moves one (row, 16-byte column) cell; 16 threads cover a source row of <= 176 bytes
    const int c16 = threadIdx.x & 15;
    if (c16 < ncol16) {
      const uint4* col = reinterpret_cast<const uint4*>(simg) + c16;
      const int stride16 = src_stride >> 4;
      for (int r = threadIdx.x >> 4; r < nrow; r += 16)
        *reinterpret_cast<uint4*>(&tile32[r * (PD_SW / 4) + c16 * 4]) =
            col[mad24((uint32_t)(sy0 + r), (uint32_t)stride16, 0u)];
    }
  }
  __syncthreads();
  pyr_rows_from_tile<PDN_H, PD_SW>(reinterpret_cast<const uint8_t*>(tile32), xo_s, xc_s, yo_s, yc_s, dimg, dst_stride, x0, y0, dw, dh);
}

// K2, row-walking form (round 3).  Same arithmetic as k_pyr_down, different work split: a workgroup owns a 256 x 32 output
// tile, a WAVE owns 8 consecutive output rows of it and a lane 4 output columns.  At scale 1.2 consecutive output rows
// share a source row five times out of six: the wave walks down its rows keeping the horizontal pass h(row) of the two
// source rows in registers and recomputes only the row that is new (10.6 horizontal row-passes per 8 output rows
// instead of 16; the row index is wave-uniform, so the reuse test is a scalar branch and the y tables come through
// scalar loads).  VALU slots per output quad 52 -> 41, LDS byte reads 16 -> 10.6; results bit-identical.
#define PW_W 256
#define PW_H 32
#define PW_SW 352                        // staged source row bytes: >= 1.21*256 + 15 + 2, multiple of 16
#define PW_SH (PW_H * 121 / 100 + 5)     // staged source rows
__global__ __launch_bounds__(256) void k_pyr_walk(uint8_t* __restrict__ pyr, int64_t pyr_frame_bytes, int64_t src_off,
                                                  int src_stride, int64_t dst_off, int dst_stride, int dw, int dh,
                                                  int tiles_x, int tx_magic, int ntiles, int nframes,
                                                  const int* __restrict__ xofs, const int* __restrict__ xc1,
                                                  const int* __restrict__ yofs, const int* __restrict__ yc1) {
  __shared__ uint32_t tile32[PW_SH * PW_SW / 4];
  int f, tx, ty, x0, y0;
  if (!pyr_tile_origin<PW_W, PW_H>(tiles_x, tx_magic, ntiles, nframes, f, tx, ty, x0, y0)) return;
  const int x1 = min(x0 + PW_W, dw) - 1, y1 = min(y0 + PW_H, dh) - 1;
  const int sx0 = xofs[x0] & ~15, sy0 = yofs[y0];
  const int ex = xofs[x1] + 1, ey = yofs[y1] + 1;
  const int ncol16 = (ex - sx0) / 16 + 1, nrow = ey - sy0 + 1;     // <= PW_SW/16 = 22, <= PW_SH
  uint8_t* base = pyr + (int64_t)f * pyr_frame_bytes;
  const uint8_t* simg = base + src_off + sx0;
  uint8_t* dimg = base + dst_off;
  // this lane's four columns: tap offset inside the staged row and the right-tap weight
  const int lane = threadIdx.x & 63;
  const int x = x0 + lane * 4;
  int o[4]; uint32_t c1[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int xi = min(x + i, dw - 1);
    o[i] = xofs[xi] - sx0; c1[i] = (uint32_t)xc1[xi];
  }
  // this wave's eight output rows: source row and bottom-tap weight, fetched (scalar loads: the row index is
  // wave-uniform) before the staging loads so that the row loop below never waits on memory
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int yb = y0 + w * (PW_H / 4);
  int yo[PW_H / 4]; uint32_t ym[PW_H / 4];
#pragma unroll
  for (int rr = 0; rr < PW_H / 4; rr++) {
    const int yi = min(yb + rr, dh - 1);
    yo[rr] = yofs[yi] - sy0; ym[rr] = (uint32_t)yc1[yi];
  }
  {
    // 32 threads per source row, <= 22 of them move a 16-byte cell; ALL of a thread's cells (<= 6 rows, 8 apart) are
    // requested before the first is stored: one memory round trip per workgroup
    const int c16 = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    const int stride16 = src_stride >> 4;
    // (clamped addresses, unconditional loads: the six values stay in registers; the stores carry the bounds)
    const uint4* colc = reinterpret_cast<const uint4*>(simg) + min(c16, ncol16 - 1);
    uint4 v0, v1, v2, v3, v4, v5;
    static_assert((PW_SH + 7) / 8 == 6, "six staged rows per thread");
#define PW_LD(k) colc[mad24((uint32_t)(sy0 + min(r0 + 8 * (k), nrow - 1)), (uint32_t)stride16, 0u)]
    v0 = PW_LD(0); v1 = PW_LD(1); v2 = PW_LD(2); v3 = PW_LD(3); v4 = PW_LD(4); v5 = PW_LD(5);
#undef PW_LD
    if (c16 < ncol16) {
      uint4* d = reinterpret_cast<uint4*>(&tile32[r0 * (PW_SW / 4) + c16 * 4]);
      if (r0 < nrow) d[0] = v0;
      if (r0 + 8 < nrow) d[8 * (PW_SW / 16)] = v1;
      if (r0 + 16 < nrow) d[16 * (PW_SW / 16)] = v2;
      if (r0 + 24 < nrow) d[24 * (PW_SW / 16)] = v3;
      if (r0 + 32 < nrow) d[32 * (PW_SW / 16)] = v4;
      if (r0 + 40 < nrow) d[40 * (PW_SW / 16)] = v5;
    }
  }
  __syncthreads();
  const uint8_t* tile = reinterpret_cast<const uint8_t*>(tile32);
  uint32_t h0[4] = {0, 0, 0, 0}, h1[4] = {0, 0, 0, 0};
  auto hpass = [&](int r, uint32_t (&h)[4]) {           // horizontal pass of staged source row r on this lane's columns
    const uint8_t* row = tile + r * PW_SW;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const uint32_t a = row[o[i]], b = row[o[i] + 1];
      h[i] = mad24(a, 256u - c1[i], mad24(b, c1[i], 0u));
    }
  };
  int prev = -9;
#pragma unroll
  for (int rr = 0; rr < PW_H / 4; rr++) {
    const int y = yb + rr;
    if (y >= dh) break;                                  // wave-uniform
    const int r = yo[rr];
    const uint32_t m1 = ym[rr], m0 = 256u - m1;
    if (r == prev + 1) {
#pragma unroll
      for (int i = 0; i < 4; i++) h0[i] = h1[i];
      hpass(r + 1, h1);
    } else if (r != prev) {
      hpass(r, h0); hpass(r + 1, h1);
    }
    prev = r;
    uint32_t v[4];
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = mad24(h0[i], m0, mad24(h1[i], m1, 32768u));
    const uint32_t out = __builtin_amdgcn_perm(v[1], v[0], 0x0C0C0602u) | __builtin_amdgcn_perm(v[3], v[2], 0x06020C0Cu);
    if (x < dw) reinterpret_cast<uint32_t*>(dimg)[mad24((uint32_t)y, (uint32_t)(dst_stride >> 2), (uint32_t)(x >> 2))] = out;
  }
}

// K1+K2 fused for level 1: a workgroup owns one 128 x 32 tile of level 1. It converts the level-0 footprint of that
// tile straight from the BGR/gray input into LDS (gray never re-read from HBM), writes the level-0 pixels it OWNS
// (columns [xofs[x0] & ~3, xofs[x0 + 128] & ~3), rows [yofs[y0], yofs[y0 + 32]); the monotone tap tables make these
// ranges a partition of level 0) and then produces its level-1 tile from LDS exactly as k_pyr_down does.
#define GP_SW 176   // LDS gray row bytes (>= 1.21*128 + 7, multiple of 4)
#define GP_SH 44    // LDS gray rows      (>= 1.21*32 + 3)
// BGR4 = 3-channel input, 4-byte aligned rows, width a multiple of 4: every quad is 12 aligned bytes, and ALL of a
// thread's quads (<= 8, one global_load_dwordx3 each) are issued before the first is converted -- one memory round
// trip per workgroup instead of seven (measured -0.13 ms of 2.2 on 2048 720p frames, on top of the XCD order).
template <bool BGR4>
__global__ __launch_bounds__(256) void k_gray_pyr1(const uint8_t* __restrict__ src, int channels, int64_t row_stride,
                                                   int64_t frame_stride, int aligned4, uint8_t* __restrict__ pyr,
                                                   int64_t pyr_frame_bytes, int s_stride, int sw, int sh, int64_t dst_off,
                                                   int dst_stride, int dw, int dh, int tiles_x, int tiles_y,
                                                   int tx_magic, int nframes,
                                                   const int* __restrict__ xofs, const int* __restrict__ xc1,
                                                   const int* __restrict__ yofs, const int* __restrict__ yc1) {
  __shared__ uint32_t tile32[GP_SH * GP_SW / 4];
  __shared__ int xo_s[PD_W]; __shared__ int xc_s[PD_W]; __shared__ int yo_s[PD_H]; __shared__ int yc_s[PD_H];
  int f, tx, ty, x0, y0;
  if (!pyr_tile_origin<PD_W, PD_H>(tiles_x, tx_magic, tiles_x * tiles_y, nframes, f, tx, ty, x0, y0)) return;
  const int x1 = min(x0 + PD_W, dw) - 1, y1 = min(y0 + PD_H, dh) - 1;
  const int rx0 = xofs[x0] & ~3, ry0 = yofs[y0];
  const int own_x1 = (tx == tiles_x - 1) ? ((sw + 3) & ~3) : (xofs[x0 + PD_W] & ~3);
  const int own_y1 = (ty == tiles_y - 1) ? sh : yofs[y0 + PD_H];
  const int rx1 = max(own_x1, min(xofs[x1] + 2, sw)), ry1 = max(own_y1, min(yofs[y1] + 2, sh));   // exclusive
  const int nqx = (rx1 - rx0 + 3) >> 2, nr = ry1 - ry0;                                             // <= 44, <= 44
  auto stage_taps = [&]() {
    if (threadIdx.x < PD_W) {
      const int xi = min(x0 + (int)threadIdx.x, dw - 1);
      xo_s[threadIdx.x] = xofs[xi] - rx0; xc_s[threadIdx.x] = xc1[xi];
    } else if (threadIdx.x < PD_W + PD_H) {
      const int r = threadIdx.x - PD_W, yi = min(y0 + r, dh - 1);
      yo_s[r] = yofs[yi] - ry0; yc_s[r] = yc1[yi];
    }
  };
  const uint8_t* sframe = src + (int64_t)f * frame_stride;
  uint8_t* base = pyr + (int64_t)f * pyr_frame_bytes;
  const float inv = 1.0f / (float)nqx;
  auto quad_rc = [&](int q, int& r, int& qx) {   // quad q of the footprint -> its staged row and its quad in that row
    r = (int)(((float)q + 0.5f) * inv);           // exact: q + 0.5 is at least 0.5 away from a multiple of nqx
    qx = q - (int)mad24((uint32_t)r, (uint32_t)nqx, 0u);
  };
  // gray quad g of staged row r, quad qx = level-0 pixels (x .. x+3, y): into the LDS tile, and to level 0 where this tile owns it
  auto store_own = [&](int r, int qx, int x, int y, uint32_t g) {
    tile32[r * (GP_SW / 4) + qx] = g;
    if (x < own_x1 && y < own_y1)
      *reinterpret_cast<uint32_t*>(base + mad24((uint32_t)y, (uint32_t)s_stride, (uint32_t)x)) = g;
  };
  if constexpr (BGR4) {
    constexpr int GP_IT = (GP_SH * (GP_SW / 4) + 255) / 256;     // 8
    const int nq = nqx * nr;
    uint32_t w0[GP_IT], w1[GP_IT], w2[GP_IT];
#pragma unroll
    for (int it = 0; it < GP_IT; it++) {
      const int q = min((int)threadIdx.x + 256 * it, nq - 1);     // clamped: no load behind a branch
      int r, qx; quad_rc(q, r, qx);
      const uint32_t so = mad24((uint32_t)(ry0 + r), (uint32_t)row_stride, 3u * (uint32_t)(rx0 + 4 * qx));
      const uint32_t* s4 = reinterpret_cast<const uint32_t*>(sframe + so);
      w0[it] = s4[0]; w1[it] = s4[1]; w2[it] = s4[2];
    }
    stage_taps();
#pragma unroll
    for (int it = 0; it < GP_IT; it++) {
      const int q = (int)threadIdx.x + 256 * it;
      if (q < nq) {
        int r, qx; quad_rc(q, r, qx);
        const int x = rx0 + 4 * qx, y = ry0 + r;
        const uint32_t g = gray_bgr12(w0[it], w1[it], w2[it]);
        store_own(r, qx, x, y, g);
      }
    }
  } else {
  stage_taps();
  for (int q = threadIdx.x; q < nqx * nr; q += 256) {
    int r, qx; quad_rc(q, r, qx);
    const int x = rx0 + 4 * qx, y = ry0 + r;
    if (x >= sw) continue;                             // padding quad: never read by a tap, never stored
    // per-lane offsets stay 32-bit (frames are < 4096 x 4096 x 3 bytes)
    const uint32_t so = mad24((uint32_t)y, (uint32_t)row_stride, channels == 1 ? (uint32_t)x : 3u * (uint32_t)x);
    const uint32_t g = gray_quad(sframe + so, channels, min(4, sw - x), aligned4);
    store_own(r, qx, x, y, g);
  }
  }
  __syncthreads();
  uint8_t* dimg = base + dst_off;
  pyr_rows_from_tile<PD_H, GP_SW>(reinterpret_cast<const uint8_t*>(tile32), xo_s, xc_s, yo_s, yc_s, dimg, dst_stride, x0, y0, dw, dh);
}

// host side of xcd_order / div_magic20
dim3 xcd_grid(int tiles, int frames) { return dim3((unsigned)((tiles + 7) & ~7), (unsigned)((frames + 7) & ~7)); }
int magic20(int d) { return (1 << 20) / d + 1; }   // exact for v * d < 2^20: at most 4095 / 128 x 4095 / 32 tiles
}  // namespace
