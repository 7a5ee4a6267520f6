// evh_jpeg.hip -- pictures encoded where they lie: evh_jpeg_encode writes baseline JFIF files of gray or BGR pictures, so that only
// compressed bytes cross the host link; evh_jpeg_header and evh_jpeg_bound are its host parts.  include/evhip.h states the
// arithmetic, tests/jpeg_checks.py restates it; a file is a pure function of the pixels and the tables: everything is integer,
// the restart interval is one MCU row, so a row's bits depend on its own pixels only, and the bits of neighbouring blocks meet
// in shared words by atomicOr on DISJOINT bits, which no order of arrival changes.  A wave is a block throughout: lane k holds
// coefficient k of the zig-zag order, a ballot of the non-zero lanes gives every lane its run of zeros.
// Kernels first, then the head, then check() -- every refusal comes before anything is enqueued -- and launch().
#include "evh_internal.h"

namespace {

// ---- T.81 Annex K.3: code lengths and symbols, [0] luminance, [1] chrominance ----
constexpr uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
constexpr uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};
// a symbol's code word: length << 16 | code (Annex C: codes of a length count up, a longer length appends a 0); 0 = no such symbol
struct Huff { uint32_t dc[2][12]; uint32_t ac[2][256]; };
constexpr Huff make_huff() {
  Huff H{};
  for (int t = 0; t < 2; t++) {
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; len++) {
      for (int i = 0; i < kDcBits[t][len - 1]; i++) H.dc[t][k++] = (unsigned)len << 16 | code++;     // DC symbols are 0..11 in order
      code <<= 1;
    }
    code = 0; k = 0;
    for (int len = 1; len <= 16; len++) {
      for (int i = 0; i < kAcBits[t][len - 1]; i++) H.ac[t][kAcVals[t][k++]] = (unsigned)len << 16 | code++;
      code <<= 1;
    }
  }
  return H;
}
__constant__ Huff kHuff = make_huff();
// natural (row-major) index of zig-zag position k
#define EVH_ZIGZAG                                                                                                                   \
  {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,   \
   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}
constexpr uint8_t kZigHost[64] = EVH_ZIGZAG;
__constant__ uint8_t kZig[64] = EVH_ZIGZAG;
// T[u][x] of include/evhip.h
__constant__ int kDct[64] = {2896, 2896,  2896,  2896,  2896,  2896,  2896,  2896,  4017, 3406,  2276,  799,   -799,  -2276, -3406, -4017,
                             3784, 1567,  -1567, -3784, -3784, -1567, 1567,  3784,  3406, -799,  -4017, -2276, 2276,  4017,  799,   -3406,
                             2896, -2896, -2896, 2896,  2896,  -2896, -2896, 2896,  2276, -4017, 799,   3406,  -3406, -799,  4017,  -2276,
                             1567, -3784, 3784,  -1567, -1567, 3784,  -3784, 1567,  799,  -2276, 3406,  -4017, 4017,  -3406, 2276,  -799};

#define JPEG_HEAD_MAX 640
#define JPEG_BLOCK_BITS 1658          // 20 of DC, 63 * 26 of AC: include/evhip.h, BOUND
// what the host hands over per call: both tables in natural order, the head
struct JpegTabs { uint16_t q[2][64]; int hlen; uint8_t head[JPEG_HEAD_MAX]; };
// blocks of a picture are numbered row by row, inside a row MCU by MCU in scan order: block = row * bpr + mcu * bpm + k
struct JpegGeom { int w, h, bpm, mcus_x, rows, bpr, row_words; int64_t blocks_pp; };

// the component (0 Y, 1 Cb, 2 Cr) of block k of an MCU of bpm blocks
__device__ __forceinline__ int component_of(int bpm, int k) { return bpm == 1 ? 0 : bpm == 3 ? k : k < 4 ? 0 : k - 3; }
// the previous block of the same component inside the row, negative: none -- the DC prediction starts at 0
__device__ __forceinline__ int pred_of(int bpm, int i, int k) { return bpm == 1 ? i - 1 : bpm == 3 ? i - 3 : k == 0 ? i - 3 : k < 4 ? i - 1 : i - 6; }
__device__ __forceinline__ int bit_length(int v) { return 32 - __clz(v < 0 ? -v : v); }     // of |v|; 0 for 0
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
// component `comp` of a BGR pixel, 0..255
__device__ __forceinline__ int ycc(int comp, const uint8_t* __restrict__ px) {
  const int b = px[0], g = px[1], r = px[2];
  if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
  return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}
// the AC part of lane k's code: its zeros' ZRLs, the (run, size) code, the value bits; needs q != 0, k > 0
__device__ __forceinline__ void ac_code(int tab, int lane, int q, unsigned long long mask, unsigned long long& code, int& len) {
  const unsigned long long below = mask & ((1ull << lane) - 1ull);
  const int prev = below ? 63 - __clzll(below) : 0, run = lane - 1 - prev, size = bit_length(q);
  const uint32_t zrl = kHuff.ac[tab][0xF0], sym = kHuff.ac[tab][(run & 15) << 4 | size];
  code = 0; len = 0;
  for (int z = 0; z < (run >> 4); z++) { code = code << (zrl >> 16) | (zrl & 0xffffu); len += (int)(zrl >> 16); }
  code = code << (sym >> 16) | (sym & 0xffffu);
  code = code << size | (unsigned)((q < 0 ? q - 1 : q) & ((1 << size) - 1));
  len += (int)(sym >> 16) + size;
}

// grid = (four blocks, picture), a wave per block: the samples of the block -- converted, for 4:2:0 chroma averaged, edge pixels
// repeated -- to LDS, the row pass, the column pass straight into zig-zag order, the division.  The wave leaves its 64
// coefficients and the bits its AC codes (EOB included) will take; the DC code waits for the previous block (k_jpeg_scan).
template <int CN, int SUB>
__global__ __launch_bounds__(256) void k_jpeg_blocks(const uint8_t* __restrict__ pics, int64_t row_stride, int64_t pic_stride, JpegGeom G,
                                                     int pic0, const JpegTabs* __restrict__ tabs, int16_t* __restrict__ coef,
                                                     int32_t* __restrict__ acbits) {
  __shared__ int sT[64], S[4][64], A[4][64];
  constexpr int BPM = CN == 1 ? 1 : SUB ? 6 : 3;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, p = pic0 + (int)blockIdx.y;
  const int64_t blk_raw = (int64_t)blockIdx.x * 4 + wv;
  const bool live = blk_raw < G.blocks_pp;
  const int64_t blk = live ? blk_raw : G.blocks_pp - 1;            // a spare wave repeats the last block and stores nothing
  const int row = (int)(blk / G.bpr), i = (int)(blk - (int64_t)row * G.bpr), mx = i / BPM, k = i - mx * BPM;
  const int comp = component_of(BPM, k), tab = comp ? 1 : 0;
  const uint8_t* pic = pics + (int64_t)p * pic_stride;
  const int ly = lane >> 3, lx = lane & 7;
  int s;
  if (SUB && comp > 0) {
    int acc = 0;
#pragma unroll
    for (int dy = 0; dy < 2; dy++)
#pragma unroll
      for (int dx = 0; dx < 2; dx++) {
        const int x = min(16 * mx + 2 * lx + dx, G.w - 1), y = min(16 * row + 2 * ly + dy, G.h - 1);
        acc += ycc(comp, pic + (int64_t)y * row_stride + 3 * (int64_t)x);
      }
    s = ((acc + 2) >> 2) - 128;
  } else {
    const int x = min((SUB ? 16 * mx + 8 * (k & 1) : 8 * mx) + lx, G.w - 1), y = min((SUB ? 16 * row + 8 * (k >> 1) : 8 * row) + ly, G.h - 1);
    const uint8_t* px = pic + (int64_t)y * row_stride + (int64_t)CN * x;
    s = (CN == 1 ? (int)px[0] : ycc(comp, px)) - 128;
  }
  if (t < 64) sT[t] = kDct[t];
  S[wv][lane] = s;
  __syncthreads();
  int a = 0;                                                       // rows: lane = (y, u)
#pragma unroll
  for (int x = 0; x < 8; x++) a += sT[lx * 8 + x] * S[wv][ly * 8 + x];
  A[wv][lane] = (a + 128) >> 8;
  __syncthreads();
  const int nat = kZig[lane], v = nat >> 3, u = nat & 7;           // columns: lane = zig-zag position
  int f = 0;
#pragma unroll
  for (int y = 0; y < 8; y++) f += sT[v * 8 + y] * A[wv][y * 8 + u];
  const int F = (f + (1 << 17)) >> 18, Q = tabs->q[tab][nat];
  const int mag = ((F < 0 ? -F : F) + (Q >> 1)) / Q, q = F < 0 ? -mag : mag;
  const bool nz = lane > 0 && q != 0;
  const unsigned long long mask = __ballot(nz);
  int bits = 0;
  if (nz) {
    unsigned long long code;
    ac_code(tab, lane, q, mask, code, bits);
  } else if (lane == 63) bits = (int)(kHuff.ac[tab][0] >> 16);     // EOB: coefficient 63 is zero
  bits = wave_sum(bits);
  if (live) {
    const int64_t gb = (int64_t)p * G.blocks_pp + blk;
    coef[gb * 64 + lane] = (int16_t)q;
    if (lane == 0) acbits[gb] = bits;
  }
}

// grid = (MCU row, picture): every block's DC code length from the block before it, and the running sum of the row's code
// lengths -- 256 blocks at a time, shuffles inside a wave, the waves' totals through LDS -- gives each block its first bit.
template <int BPM>
__global__ __launch_bounds__(256) void k_jpeg_scan(JpegGeom G, int pic0, const int16_t* __restrict__ coef, const int32_t* __restrict__ acbits,
                                                   int32_t* __restrict__ bitoff, int32_t* __restrict__ rowbits) {
  __shared__ int wtot[4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, row = blockIdx.x, p = pic0 + (int)blockIdx.y;
  const int64_t base = (int64_t)p * G.blocks_pp + (int64_t)row * G.bpr;
  int running = 0;
  for (int b0 = 0; b0 < G.bpr; b0 += 256) {
    const int i = b0 + t;
    int bits = 0;
    if (i < G.bpr) {
      const int k = i % BPM, pred = pred_of(BPM, i, k), tab = component_of(BPM, k) ? 1 : 0;
      const int d = (int)coef[(base + i) * 64] - (pred >= 0 ? (int)coef[(base + pred) * 64] : 0), cat = bit_length(d);
      bits = (int)(kHuff.dc[tab][cat] >> 16) + cat + acbits[base + i];
    }
    int incl = bits;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
      const int o = __shfl_up(incl, m, 64);
      if (lane >= m) incl += o;
    }
    if (lane == 63) wtot[wv] = incl;
    __syncthreads();
    int off = running;
    for (int j = 0; j < wv; j++) off += wtot[j];
    if (i < G.bpr) bitoff[base + i] = off + incl - bits;
    running += wtot[0] + wtot[1] + wtot[2] + wtot[3];
    __syncthreads();
  }
  if (t == 0) rowbits[(int64_t)p * G.rows + row] = running;
}

// grid = (four blocks, picture), a wave per block: every lane forms its code again (at most 59 bits: three ZRLs of 11, a code of
// 16, 10 value bits), a scan of the lengths gives its first bit, and the code is ORed into the row's words, most significant
// bit first.  A code spans at most three words; words it leaves zero are not touched, so nothing past the row's last bit is.
template <int BPM>
__global__ __launch_bounds__(256) void k_jpeg_pack(JpegGeom G, int pic0, const int16_t* __restrict__ coef, const int32_t* __restrict__ bitoff,
                                                   uint32_t* __restrict__ words) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, p = pic0 + (int)blockIdx.y;
  const int64_t blk = (int64_t)blockIdx.x * 4 + wv;
  if (blk >= G.blocks_pp) return;                                  // the whole wave: no barrier follows
  const int row = (int)(blk / G.bpr), i = (int)(blk - (int64_t)row * G.bpr), k = i % BPM;
  const int tab = component_of(BPM, k) ? 1 : 0, pred = pred_of(BPM, i, k);
  const int64_t gb = (int64_t)p * G.blocks_pp + blk;
  const int q = coef[gb * 64 + lane];
  const bool nz = lane > 0 && q != 0;
  const unsigned long long mask = __ballot(nz);
  unsigned long long code = 0;
  int len = 0;
  if (lane == 0) {
    const int d = q - (pred >= 0 ? (int)coef[(gb - i + pred) * 64] : 0), cat = bit_length(d);
    const uint32_t sym = kHuff.dc[tab][cat];
    code = (unsigned long long)(sym & 0xffffu) << cat | (unsigned)((d < 0 ? d - 1 : d) & ((1 << cat) - 1));
    len = (int)(sym >> 16) + cat;
  } else if (nz) ac_code(tab, lane, q, mask, code, len);
  else if (lane == 63) { code = kHuff.ac[tab][0] & 0xffffu; len = (int)(kHuff.ac[tab][0] >> 16); }
  int incl = len;
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const int o = __shfl_up(incl, m, 64);
    if (lane >= m) incl += o;
  }
  if (len == 0) return;
  const int pos = bitoff[gb] + incl - len, o = pos & 31, w0 = pos >> 5;
  const unsigned long long val = code << (64 - len), hi = val >> o;
  const uint32_t part[3] = {(uint32_t)(hi >> 32), (uint32_t)hi, o ? (uint32_t)((val << (64 - o)) >> 32) : 0u};
  uint32_t* dst = words + ((int64_t)p * G.rows + row) * G.row_words;
#pragma unroll
  for (int j = 0; j < 3; j++)
    if (part[j] && w0 + j < G.row_words) atomicOr(dst + w0 + j, part[j]);
}

// byte i of a row's bit buffer
__device__ __forceinline__ int row_byte(const uint32_t* __restrict__ words, int i) { return (int)(words[i >> 2] >> (24 - 8 * (i & 3))) & 255; }

// grid = (MCU row, picture): the 1-bits that pad the row to a byte go into its last word, and the row's bytes in the file are
// counted: its data bytes, a 0x00 for each 0xFF among them, and the RST marker unless the row is the last.
__global__ __launch_bounds__(256) void k_jpeg_row_bytes(JpegGeom G, int pic0, const int32_t* __restrict__ rowbits, uint32_t* __restrict__ words,
                                                        int32_t* __restrict__ rowbytes) {
  __shared__ int wtot[4];
  const int t = threadIdx.x, row = blockIdx.x, p = pic0 + (int)blockIdx.y;
  const int64_t pr = (int64_t)p * G.rows + row;
  uint32_t* wd = words + pr * G.row_words;
  const int nbits = rowbits[pr], nb = (nbits + 7) >> 3, pad = (8 - (nbits & 7)) & 7, last = nb - 1;
  int count = 0;
#pragma unroll 1
  for (int j = t; 4 * j < nb; j += 256) {
    uint32_t v = wd[j];
    if (j == (last >> 2) && pad) { v |= ((1u << pad) - 1u) << (24 - 8 * (last & 3)); wd[j] = v; }
#pragma unroll
    for (int b = 0; b < 4; b++) count += (4 * j + b < nb && ((v >> (24 - 8 * b)) & 255u) == 255u) ? 1 : 0;
  }
  count = wave_sum(count);
  if ((t & 63) == 0) wtot[t >> 6] = count;
  __syncthreads();
  if (t == 0) rowbytes[pr] = nb + wtot[0] + wtot[1] + wtot[2] + wtot[3] + (row < G.rows - 1 ? 2 : 0);
}

// grid = (MCU row, picture): the row's place in the file is the head and the rows before it; its bytes go there with their
// stuffing -- 256 at a time, a ballot of the 0xFF bytes places each --, then RSTm or, after the last row, EOI and the length.
// Row 0 also writes the head.  Nothing is stored at or past out_cap.
__global__ __launch_bounds__(256) void k_jpeg_assemble(JpegGeom G, int pic0, const JpegTabs* __restrict__ tabs, const int32_t* __restrict__ rowbits,
                                                       const int32_t* __restrict__ rowbytes, const uint32_t* __restrict__ words,
                                                       uint8_t* __restrict__ d_out, int64_t out_stride, int64_t out_cap,
                                                       int64_t* __restrict__ d_out_bytes) {
  __shared__ long long wsum[4];
  __shared__ int wtot[4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, row = blockIdx.x, p = pic0 + (int)blockIdx.y;
  const int64_t pr = (int64_t)p * G.rows + row;
  const uint32_t* wd = words + pr * G.row_words;
  uint8_t* out = d_out + (int64_t)p * out_stride;
  const int hlen = tabs->hlen;
  long long before = 0;
  for (int r = t; r < row; r += 256) before += rowbytes[(int64_t)p * G.rows + r];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) before += __shfl_xor(before, m, 64);
  if (lane == 0) wsum[wv] = before;
  __syncthreads();
  const int64_t off = hlen + wsum[0] + wsum[1] + wsum[2] + wsum[3];
  if (row == 0)
    for (int i = t; i < hlen; i += 256)
      if (i < out_cap) out[i] = tabs->head[i];
  const int nb = (rowbits[pr] + 7) >> 3;
  int running = 0;
  for (int b0 = 0; b0 < nb; b0 += 256) {
    const int i = b0 + t;
    const bool have = i < nb;
    const int byte = have ? row_byte(wd, i) : 0;
    const bool ff = have && byte == 255;
    const unsigned long long m = __ballot(ff);
    if (lane == 0) wtot[wv] = __popcll(m);
    __syncthreads();
    int extra = running + __popcll(m & ((1ull << lane) - 1ull));
    for (int j = 0; j < wv; j++) extra += wtot[j];
    const int64_t pos = off + i + extra;
    if (have && pos < out_cap) out[pos] = (uint8_t)byte;
    if (ff && pos + 1 < out_cap) out[pos + 1] = 0;
    running += wtot[0] + wtot[1] + wtot[2] + wtot[3];
    __syncthreads();
  }
  if (t == 0) {
    const int64_t end = off + nb + running;
    if (end < out_cap) out[end] = 0xFF;
    if (end + 1 < out_cap) out[end + 1] = (uint8_t)(row < G.rows - 1 ? 0xD0 + (row & 7) : 0xD9);
    if (row == G.rows - 1) d_out_bytes[p] = end + 2;
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
struct JpegArgs {
  const uint8_t* pics; int n, w, h; int64_t row_stride, pic_stride; int channels, sub; const uint16_t* qtab; uint8_t* out;
  int64_t out_stride, out_cap; int64_t* out_bytes;
};
// the layout and the tables evh_jpeg_encode takes; `why` names what it refuses
bool layout_ok(int w, int h, int channels, int sub, const char** why) {
  if (w < 1 || w > 65535 || h < 1 || h > 65535) { *why = "w and h must lie in 1..65535"; return false; }
  if (channels != 1 && channels != 3) { *why = "channels must be 1 or 3"; return false; }
  if (sub != EVH_JPEG_444 && sub != EVH_JPEG_420) { *why = "subsampling must be EVH_JPEG_444 or EVH_JPEG_420"; return false; }
  if (sub == EVH_JPEG_420 && channels == 1) { *why = "EVH_JPEG_420 needs three channels"; return false; }
  return true;
}
bool tables_ok(const uint16_t* qtab) {
  for (int i = 0; i < 128; i++)
    if (qtab[i] < 1 || qtab[i] > 255) return false;
  return true;
}
JpegGeom geometry(int w, int h, int channels, int sub) {
  JpegGeom G{};
  const int mcu = sub == EVH_JPEG_420 ? 16 : 8;
  G.w = w; G.h = h; G.bpm = channels == 1 ? 1 : sub == EVH_JPEG_420 ? 6 : 3;
  G.mcus_x = (w + mcu - 1) / mcu; G.rows = (h + mcu - 1) / mcu; G.bpr = G.mcus_x * G.bpm;
  G.row_words = (int)(((int64_t)G.bpr * JPEG_BLOCK_BITS + 31) / 32);
  G.blocks_pp = (int64_t)G.rows * G.bpr;
  return G;
}
int head_length(int channels) { return channels == 1 ? 550 : 629; }
// SOI .. SOS of include/evhip.h, FILE; the caller has checked the layout and the tables
int write_head(int w, int h, int channels, int sub, const uint16_t* qtab, uint8_t* out) {
  uint8_t* o = out;
  auto put = [&](std::initializer_list<int> bytes) { for (int b : bytes) *o++ = (uint8_t)b; };
  put({0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
  for (int t = 0; t < (channels == 1 ? 1 : 2); t++) {
    put({0xFF, 0xDB, 0, 67, t});
    for (int k = 0; k < 64; k++) *o++ = (uint8_t)qtab[64 * t + kZigHost[k]];
  }
  put({0xFF, 0xC0, 0, 8 + 3 * channels, 8, h >> 8, h & 255, w >> 8, w & 255, channels});
  for (int c = 0; c < channels; c++) put({c + 1, c == 0 && sub == EVH_JPEG_420 ? 0x22 : 0x11, c ? 1 : 0});
  for (int t = 0; t < 2; t++) {
    put({0xFF, 0xC4, 0, 19 + 12, t});
    for (int i = 0; i < 16; i++) *o++ = kDcBits[t][i];
    for (int i = 0; i < 12; i++) *o++ = (uint8_t)i;
    put({0xFF, 0xC4, 0, 19 + 162, 0x10 | t});
    for (int i = 0; i < 16; i++) *o++ = kAcBits[t][i];
    for (int i = 0; i < 162; i++) *o++ = kAcVals[t][i];
  }
  const int mcu = sub == EVH_JPEG_420 ? 16 : 8, dri = (w + mcu - 1) / mcu;
  put({0xFF, 0xDD, 0, 4, dri >> 8, dri & 255});
  put({0xFF, 0xDA, 0, 6 + 2 * channels, channels});
  for (int c = 0; c < channels; c++) put({c + 1, c ? 0x11 : 0x00});
  put({0, 63, 0});
  return (int)(o - out);
}

int check(evh_ctx* c, const JpegArgs& A) {
  const std::string W = "evh_jpeg_encode: ";
  if (!A.pics || !A.qtab || !A.out || !A.out_bytes) return evh_fail(c, EVH_ERR_INVALID, W + "NULL argument");
  if (A.n < 0) return evh_fail(c, EVH_ERR_INVALID, W + "negative n");
  const char* why = "";
  if (!layout_ok(A.w, A.h, A.channels, A.sub, &why)) return evh_fail(c, EVH_ERR_INVALID, W + why);
  if (!tables_ok(A.qtab)) return evh_fail(c, EVH_ERR_INVALID, W + "every table entry must lie in 1..255");
  if (A.row_stride < (int64_t)A.w * A.channels) return evh_fail(c, EVH_ERR_INVALID, W + "row_stride shorter than a row");
  if (A.out_cap < 0) return evh_fail(c, EVH_ERR_INVALID, W + "negative out_cap");
  if (A.out_stride < A.out_cap) return evh_fail(c, EVH_ERR_INVALID, W + "out_stride smaller than out_cap");
  return EVH_SUCCESS;
}

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

template <int CN, int SUB>
void launch_kernels(evh_ctx* c, const JpegArgs& A, const JpegGeom& G, int p0, int np, const JpegTabs* tabs, int16_t* coef, int32_t* acbits,
                    int32_t* bitoff, int32_t* rowbits, int32_t* rowbytes, uint32_t* words) {
  constexpr int BPM = CN == 1 ? 1 : SUB ? 6 : 3;
  const dim3 per_block((unsigned)((G.blocks_pp + 3) / 4), (unsigned)np), per_row((unsigned)G.rows, (unsigned)np);
  hipLaunchKernelGGL((k_jpeg_blocks<CN, SUB>), per_block, dim3(256), 0, c->stream, A.pics, A.row_stride, A.pic_stride, G, p0, tabs, coef, acbits);
  hipLaunchKernelGGL((k_jpeg_scan<BPM>), per_row, dim3(256), 0, c->stream, G, p0, coef, acbits, bitoff, rowbits);
  hipLaunchKernelGGL((k_jpeg_pack<BPM>), per_block, dim3(256), 0, c->stream, G, p0, coef, bitoff, words);
  hipLaunchKernelGGL(k_jpeg_row_bytes, per_row, dim3(256), 0, c->stream, G, p0, rowbits, words, rowbytes);
  hipLaunchKernelGGL(k_jpeg_assemble, per_row, dim3(256), 0, c->stream, G, p0, tabs, rowbits, rowbytes, words, A.out, A.out_stride, A.out_cap,
                     A.out_bytes);
}

// the tables and the head go up first, the bit buffers are cleared, then the five kernels per 65535 pictures (grid.y's range)
int launch(evh_ctx* c, const JpegArgs& A) {
  const JpegGeom G = geometry(A.w, A.h, A.channels, A.sub);
  const size_t nb = (size_t)A.n * (size_t)G.blocks_pp, nr = (size_t)A.n * (size_t)G.rows;
  const size_t o_coef = up256(sizeof(JpegTabs)), o_ac = o_coef + up256(nb * 128), o_off = o_ac + up256(nb * 4), o_bits = o_off + up256(nb * 4),
               o_bytes = o_bits + up256(nr * 4), o_words = o_bytes + up256(nr * 4), words_bytes = nr * (size_t)G.row_words * 4;
  if (int rc = grow(c, &c->d_jpeg_ws, &c->jpeg_ws_bytes, o_words + words_bytes)) return rc;
  char* ws = c->d_jpeg_ws;
  JpegTabs T{};
  for (int i = 0; i < 128; i++) T.q[i >> 6][i & 63] = A.qtab[i];
  T.hlen = write_head(A.w, A.h, A.channels, A.sub, A.qtab, T.head);
  EVH_HIP(c, hipMemcpyAsync(ws, &T, sizeof(T), hipMemcpyHostToDevice, c->stream));      // pageable: staged before the call returns
  EVH_HIP(c, hipMemsetAsync(ws + o_words, 0, words_bytes, c->stream));
  const JpegTabs* tabs = reinterpret_cast<const JpegTabs*>(ws);
  int16_t* coef = reinterpret_cast<int16_t*>(ws + o_coef);
  int32_t *acbits = reinterpret_cast<int32_t*>(ws + o_ac), *bitoff = reinterpret_cast<int32_t*>(ws + o_off),
          *rowbits = reinterpret_cast<int32_t*>(ws + o_bits), *rowbytes = reinterpret_cast<int32_t*>(ws + o_bytes);
  uint32_t* words = reinterpret_cast<uint32_t*>(ws + o_words);
  for (int p0 = 0; p0 < A.n; p0 += 65535) {
    const int np = std::min(65535, A.n - p0);
    if (A.channels == 1) launch_kernels<1, 0>(c, A, G, p0, np, tabs, coef, acbits, bitoff, rowbits, rowbytes, words);
    else if (A.sub == EVH_JPEG_420) launch_kernels<3, 1>(c, A, G, p0, np, tabs, coef, acbits, bitoff, rowbits, rowbytes, words);
    else launch_kernels<3, 0>(c, A, G, p0, np, tabs, coef, acbits, bitoff, rowbits, rowbytes, words);
  }
  EVH_HIP(c, hipGetLastError());
  return EVH_SUCCESS;
}

}  // namespace

extern "C" {

int64_t evh_jpeg_bound(int w, int h, int channels, int subsampling) {
  const char* why;
  if (!layout_ok(w, h, channels, subsampling, &why)) return -1;
  const JpegGeom G = geometry(w, h, channels, subsampling);
  return head_length(channels) + (int64_t)G.rows * (2 * (((int64_t)G.bpr * JPEG_BLOCK_BITS + 7) / 8) + 2) + 2;
}

int evh_jpeg_header(int w, int h, int channels, int subsampling, const uint16_t* qtab, uint8_t* out, int cap) {
  const char* why;
  if (!qtab || !out || !layout_ok(w, h, channels, subsampling, &why) || !tables_ok(qtab) || cap < head_length(channels)) return EVH_ERR_INVALID;
  return write_head(w, h, channels, subsampling, qtab, out);
}

int evh_jpeg_encode(evh_ctx* c, const uint8_t* d_pictures, int n, int w, int h, int64_t row_stride, int64_t picture_stride, int channels,
                    int subsampling, const uint16_t* qtab, uint8_t* d_out, int64_t out_stride, int64_t out_cap, int64_t* d_out_bytes) {
  if (!c) return EVH_ERR_INVALID;
  const JpegArgs A{d_pictures, n, w, h, row_stride, picture_stride, channels, subsampling, qtab, d_out, out_stride, out_cap, d_out_bytes};
  if (int rc = check(c, A)) return rc;
  return n == 0 ? EVH_SUCCESS : launch(c, A);
}

}  // extern "C"
