// evh_detect_fast.h -- internal to evh_detect.hip (stage 2 of 5): FAST-9/16 dense and lifted, corner score, NMS, candidate lists
#pragma once
#include "evh_detect_pyr.h"
namespace {
// K3: FAST-9/16 + corner score + 3x3 NMS + 31-px border filter, all pyramid levels of all frames in one launch.
// Workgroup = 128 x 28 output tile (FT_W x FT_H); the tile plus a halo of 4 rows and 8 columns is staged in LDS (16-byte
// loads), the corner score of tile+1 halo is computed into an LDS score plane, NMS + emission read that plane.
// score = max over the 16 arcs of 9 contiguous ring pixels of min(+-(centre - ring)) - 1; corner iff that max
// exceeds the threshold (equivalent to the ">= 9 contiguous strictly brighter/darker" definition).
struct FastArgs {
  EvhLevel lv[EVH_NLEVELS];
  uint8_t* pyr; int64_t pyr_frame_bytes;
  uint32_t* cand; int64_t cand_frame_entries;
  int* cand_count;
  // threshold lifting (k_fast_sample .. k_fast_redo): per (frame, level) score threshold, sampled score histogram, redo flags
  int* thr;            // [F][8]
  unsigned* shist;     // [F][8][256]
  int* redo;           // [1 + F*8]: count, then the (frame * 8 + level) entries to redo densely
  uint32_t* tdesc;     // reference order: [F][total_tiles][8] per-tile burst descriptor (offset in the level's list, 28 row counts)
  int total_tiles;
  int lift_base;       // 1: k_fast_main scores through the pre-test + queue machinery at the base threshold too (reference order)
  int samp_start[EVH_NLEVELS], samp_mod[EVH_NLEVELS];   // sampling lattice of k_fast_sample
  // consecutive frames of one video look alike: with share_group = F > 0 the frames of a call form groups of F
  // consecutive frames and a frame at an odd position of its group takes the sampled score histogram of the frame
  // before it instead of sampling itself (any threshold is exact; a wrong guess only costs the dense redo)
  int share_group;
  // threshold hint carried from the previous detect call of this context (per level: the lower-quartile lifted
  // threshold over the frames of that call, 0 = none): the sample pass then scores its tiles with the lifted machinery at 5/8 of the hint instead
  // of densely -- the histogram is exact above that floor, which is where the new threshold will lie
  const int* hint_in; int* hint_out;
  unsigned* hint_hist;   // [8][256] votes of this call: the lifted threshold of every frame that sampled (bin 0: a failed level)
};

#define FT_W 128                 // output tile width (pixels)
#define FT_H 28                  // output tile height (30 score rows x 34 quads = 1020 quads = 4 full passes of 256)
#define FR_DW ((FT_W + 16) / 4)  // staged raw row: x0-8 .. x0+135, 36 dwords
#define FR_H (FT_H + 8)          // staged raw rows: y0-4 .. y0+FT_H+3
#define FS_DW ((FT_W + 8) / 4)   // score row: x0-4 .. x0+131, 34 quads (dwords of 4 byte scores)
#define FS_H (FT_H + 2)          // score rows: y0-1 .. y0+FT_H
#define FSC_CAP 512              // scored-pixel list of the lifted path

// byte B (relative to the quad's own dword M; -4..-1 = left neighbour dword, 4..7 = right neighbour dword)
template <int B>
__device__ __forceinline__ int rbyte(uint32_t L, uint32_t M, uint32_t R) {
  if constexpr (B < 0) return (int)((L >> (8 * (4 + B))) & 0xFFu);
  else if constexpr (B < 4) return (int)((M >> (8 * B)) & 0xFFu);
  else return (int)((R >> (8 * (B - 4))) & 0xFFu);
}
// THE ring of FAST-9/16: (dx, dy) of ring pixel k, once round from (0, +3).  The byte form and the register form below take their
// offsets from here; corner16_pass4 cuts the same ring out of row dwords (its comments give the ring indices of every row).
constexpr int FAST_RING[16][2] = {{0, 3},  {1, 3},   {2, 2},   {3, 1},   {3, 0},  {3, -1}, {2, -2}, {1, -3},
                                  {0, -3}, {-1, -3}, {-2, -2}, {-3, -1}, {-3, 0}, {-3, 1}, {-2, 2}, {-1, 3}};
// byte form: the 16 ring bytes of the pixel at p in a byte plane of PITCH bytes per row
template <int PITCH>
__device__ __forceinline__ void fast_ring(const uint8_t* p, uint32_t (&ring)[16]) {
#pragma unroll
  for (int k = 0; k < 16; k++) ring[k] = p[FAST_RING[k][1] * PITCH + FAST_RING[k][0]];
}
// register form: centre - ring of pixel J (0..3) of a quad; L/M/R[0..6] = the three dwords of rows y-3 .. y+3. Branch-free.
template <int J>
__device__ __forceinline__ void fast_diffs_px(const uint32_t (&L)[7], const uint32_t (&M)[7], const uint32_t (&R)[7],
                                              short (&d)[16]) {
  const int v = rbyte<J>(L[3], M[3], R[3]);
#define FD(K) d[K] = (short)(v - rbyte<J + FAST_RING[K][0]>(L[3 + FAST_RING[K][1]], M[3 + FAST_RING[K][1]], R[3 + FAST_RING[K][1]]))
  FD(0); FD(1); FD(2); FD(3); FD(4); FD(5); FD(6); FD(7); FD(8); FD(9); FD(10); FD(11); FD(12); FD(13); FD(14); FD(15);
#undef FD
}

// 16-bit VALU min/max issue at full rate on gfx950 (measured: 2 cycles per wave64 instruction), the 32-bit and
// 3-input forms at half rate; the differences centre-ring fit int16, so the score trees run on the low halves.
typedef short i16;
__device__ __forceinline__ i16 mn16(i16 a, i16 b) { return a < b ? a : b; }
__device__ __forceinline__ i16 mx16(i16 a, i16 b) { return a > b ? a : b; }
__device__ __forceinline__ int sext16(i16 a) { return (int)a; }

// Exact corner score from the 16 differences d[k] = centre - ring[k] (low 16 bits significant):
// max over the 16 circular arcs of 9 of min(d) (darker) and of min(-d) (brighter).  Sliding minimum by block
// prefix/suffix scans (blocks 0..7 and 8..15; arc k = 8b+r is suffix_b[r] joined with prefix_{b^1}[r]).
__device__ __forceinline__ int fast_score_from_d(const i16 (&d)[16]) {
  i16 Pn[2][8], Sn[2][8], Px[2][8], Sx[2][8];
#pragma unroll
  for (int b = 0; b < 2; b++) {
    Pn[b][0] = d[8 * b]; Px[b][0] = d[8 * b];
    Sn[b][7] = d[8 * b + 7]; Sx[b][7] = d[8 * b + 7];
#pragma unroll
    for (int r = 1; r < 8; r++) {
      Pn[b][r] = mn16(Pn[b][r - 1], d[8 * b + r]);
      Px[b][r] = mx16(Px[b][r - 1], d[8 * b + r]);
      Sn[b][7 - r] = mn16(Sn[b][8 - r], d[8 * b + 7 - r]);
      Sx[b][7 - r] = mx16(Sx[b][8 - r], d[8 * b + 7 - r]);
    }
  }
  i16 a = mn16(Sn[0][0], Pn[1][0]);   // max over arcs of min(d)
  i16 m = mx16(Sx[0][0], Px[1][0]);   // min over arcs of max(d)
#pragma unroll
  for (int b = 0; b < 2; b++)
#pragma unroll
    for (int r = 0; r < 8; r++) {
      if (b == 0 && r == 0) continue;
      a = mx16(a, mn16(Sn[b][r], Pn[b ^ 1][r]));
      m = mn16(m, mx16(Sx[b][r], Px[b ^ 1][r]));
    }
  const int best = max(sext16(a), -sext16(m));
  return best > EVH_FAST_THR ? best - 1 : 0;
}

// Score byte of a pixel the segment test has already found to be a corner, from the raw bytes: v = centre, p[k] = ring,
// m = 0xFF where the ring is the brighter side, 0 where it is the darker one.  A corner has exactly one polarity (two
// 9-arcs of a 16-ring overlap, so a ring cannot hold nine pixels below centre - T and nine above centre + T), and on
// the other side every arc then holds a pixel of the winning arc, whose difference has the wrong sign by more than T:
// that side's candidate is below -T and never wins the max of fast_score_from_d.  The score is therefore one-sided,
// best = max over arcs of min(v - p) = v - min over arcs of max(p) for a darker ring, and the same with every byte
// complemented (v ^ 0xFF = 255 - v keeps the differences, swaps their sign) for a brighter one.  No subtraction per
// ring pixel, unsigned 16-bit max / min only (the full-rate forms).  best > T is what the segment test proved, so
// the byte best - 1 is returned without the comparison.  Same block prefix / suffix scans as fast_score_from_d.
typedef unsigned short u16;
__device__ __forceinline__ u16 mnu16(u16 a, u16 b) { return a < b ? a : b; }
__device__ __forceinline__ u16 mxu16(u16 a, u16 b) { return a > b ? a : b; }
__device__ __forceinline__ int fast_score_one_sided(uint32_t v, const uint32_t (&p)[16], uint32_t m) {
  u16 q[16], Px[2][8], Sx[2][8];
#pragma unroll
  for (int k = 0; k < 16; k++) q[k] = (u16)(p[k] ^ m);
#pragma unroll
  for (int b = 0; b < 2; b++) {
    Px[b][0] = q[8 * b];
    Sx[b][7] = q[8 * b + 7];
#pragma unroll
    for (int r = 1; r < 8; r++) {
      Px[b][r] = mxu16(Px[b][r - 1], q[8 * b + r]);
      Sx[b][7 - r] = mxu16(Sx[b][8 - r], q[8 * b + 7 - r]);
    }
  }
  u16 lo = mxu16(Sx[0][0], Px[1][0]);   // min over arcs of max(ring)
#pragma unroll
  for (int b = 0; b < 2; b++)
#pragma unroll
    for (int r = 0; r < 8; r++) {
      if (b == 0 && r == 0) continue;
      lo = mnu16(lo, mxu16(Sx[b][r], Px[b ^ 1][r]));
    }
  return (int)(v ^ m) - (int)lo - 1;
}

#define FQ_PITCH (FS_DW * 4)   // score plane pitch in bytes (136)

// bit 7 of byte j set for the pixels xq + j of a quad that lie in [lo_x, hi_x)
__device__ __forceinline__ uint32_t quad_range_mask(int xq, int lo_x, int hi_x) {
  const int lo = min(max(lo_x - xq, 0), 4), hi = max(min(hi_x - xq, 4), 0);   // valid pixels j in [lo, hi)
  return lo < hi ? (0x80808080u << (8 * lo)) & (0x80808080u >> (8 * (4 - hi))) : 0u;
}
// candidate word of a corner, the entry of a level's candidate list: score << 24 | y << 12 | x (level coordinates, < 4096).
// The key-point word of k_select* / k_pack keeps y and x in place and puts the level where the score was.
__device__ __forceinline__ uint32_t fast_cand(uint32_t s, int y, int x) { return (s << 24) | ((uint32_t)y << 12) | (uint32_t)x; }
__device__ __forceinline__ int cand_x(uint32_t c) { return (int)(c & 0xFFFu); }
__device__ __forceinline__ int cand_y(uint32_t c) { return (int)((c >> 12) & 0xFFFu); }
__device__ __forceinline__ uint32_t cand_score(uint32_t c) { return c >> 24; }

struct FastLds {
  alignas(16) uint32_t raw[FR_H * FR_DW];   // 36 rows x 36 dwords: rows y0-4.., columns x0-8.. (16-byte staging stores)
  alignas(16) uint32_t score[FS_H * FS_DW];   // 30 x 34 quads of byte scores: rows y0-1.., columns x0-4..
  // lst: NMS output, at most one corner per 2x2 block (896 entries).  The lifted path uses the same words first as
  // its queue of quads with a pixel that passes the pre-test (<= 1020 entries, quad index | pass bits << 16): the
  // queue is dead before NMS writes the list.
  uint32_t lst[FS_H * FS_DW + 4];
  // lifted path: pixels whose exact score reached T.  A few dozen per tile; a tile with more than FSC_CAP takes the
  // full-plane NMS instead (fast_nms_collect), so the list can be short: 17.0 -> 14.5 KB of LDS per workgroup lets 11
  // instead of 9 workgroups sit on a compute unit while some of them are down to their tail wave
  uint16_t scored[FSC_CAP];
  alignas(16) uint32_t sink[4];      // target of the second staging store of threads that have no second item
  int lcnt, gbase, qcnt, scnt;
  int wtot[4];                       // ordered collection: survivors per wave of the current pass
  uint32_t rowcnt[8];                // ordered collection: survivors per tile row, one byte each (FT_H = 28 rows)
};

// stage rows y0-4 .. y0+FT_H+3, columns x0-8 .. x0+135 with 16-byte loads (data outside the image reads as 0: it
// only feeds pixels whose centre is outside the testable range, which are never scored); clears the counters
__device__ __forceinline__ void fast_stage(FastLds& S, const uint8_t* img, const EvhLevel& L, int x0, int y0) {
  if (threadIdx.x == 0) { S.lcnt = 0; S.qcnt = 0; S.scnt = 0; }
  if (threadIdx.x >= 8 && threadIdx.x < 16) S.rowcnt[threadIdx.x - 8] = 0;
  // 16-byte items (x0 - 8 = 16 + 128 tx is 16-byte aligned, a staged row is 9 of them): item i = (row i / 9,
  // column i % 9), 324 items = 2 per thread at most; +256 items = +28 rows +4 columns.  Rows are padded to 64 bytes,
  // so an item is wholly inside [0, stride) or wholly outside.
  static_assert(FR_DW % 4 == 0 && ((EVH_FAST_OX - 8) % 16) == 0 && (FT_W % 16) == 0, "16-byte staging");
  constexpr int C16 = FR_DW / 4;
  constexpr int NITEM = FR_H * C16;                     // 324 items: two per thread at most
  static_assert(NITEM > 256 && NITEM <= 512, "two staging items per thread");
  const int stride16 = L.stride >> 4;
  // workgroup-uniform: every staged byte exists (all tiles but those on the right / bottom edge of a level)
  const bool inside = y0 >= 4 && y0 + FT_H + 4 <= L.h && x0 >= 8 && x0 + FT_W + 8 <= L.stride;
  const int ra = (int)threadIdx.x / C16, ca = (int)threadIdx.x - ra * C16;
  int rb = ra + 256 / C16, cb = ca + 256 % C16;
  if (cb >= C16) { cb -= C16; rb++; }
  const bool has_b = (int)threadIdx.x + 256 < NITEM;
  if (!has_b) { rb = ra; cb = ca; }      // no second item: request the first one again (same line, no extra traffic)
  const uint4* img16 = reinterpret_cast<const uint4*>(img);
  // BOTH items are requested before either is stored (clamped addresses, unconditional loads: one memory round trip
  // per workgroup -- the predicated form compiled to load, wait, store, load, wait, store)
  const int ya = y0 - 4 + ra, xa = x0 - 8 + ca * 16, yb = y0 - 4 + rb, xb = x0 - 8 + cb * 16;
  const int xmax = L.stride - 16;
  const uint4 la = img16[mad24s(min(max(ya, 0), L.h - 1), stride16, min(max(xa, 0), xmax) >> 4)];
  const uint4 lb = img16[mad24s(min(max(yb, 0), L.h - 1), stride16, min(max(xb, 0), xmax) >> 4)];
  // straight-line stores (a thread without a second item writes it to a sink word): nothing between the two loads and
  // the two stores for the compiler to sink a load into
  uint4* da = reinterpret_cast<uint4*>(&S.raw[ra * FR_DW + ca * 4]);
  uint4* db = has_b ? reinterpret_cast<uint4*>(&S.raw[rb * FR_DW + cb * 4]) : reinterpret_cast<uint4*>(S.sink);
  *da = la;
  *db = lb;
  if (!inside) {                                          // edge tiles (workgroup-uniform): what lies outside the level reads as 0
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    if (!(xa >= 0 && xa < L.stride && ya >= 0 && ya < L.h)) *da = z;
    if (has_b && !(xb >= 0 && xb < L.stride && yb >= 0 && yb < L.h)) *db = z;
  }
}

// dense path: exact scores (threshold 20) of rows y0-1 .. y0+FT_H, quads x0-4 .. x0+131; one thread = 4 adjacent
// pixels, ring bytes taken straight out of the row dwords (SDWA), branch-free
__device__ __forceinline__ void fast_dense_scores(FastLds& S, const EvhLevel& L, int x0, int y0) {
  for (int i = threadIdx.x; i < FS_H * FS_DW; i += 256) {
    const int sr = i / FS_DW, sq = i - sr * FS_DW;
    const int y = y0 - 1 + sr, xq = x0 - 4 + sq * 4;
    uint32_t out = 0;
    if (y >= 3 && y < L.h - 3 && xq + 3 >= 3 && xq < L.w - 3) {      // wave-divergent only at image borders
      uint32_t Lr[7], Mr[7], Rr[7];
      const uint32_t* p = S.raw + sr * FR_DW + sq;                    // row (y-3), dword of x = xq-4
#pragma unroll
      for (int r = 0; r < 7; r++) { Lr[r] = p[r * FR_DW]; Mr[r] = p[r * FR_DW + 1]; Rr[r] = p[r * FR_DW + 2]; }
      i16 d[16];
      fast_diffs_px<0>(Lr, Mr, Rr, d); int s0 = fast_score_from_d(d);
      fast_diffs_px<1>(Lr, Mr, Rr, d); int s1 = fast_score_from_d(d);
      fast_diffs_px<2>(Lr, Mr, Rr, d); int s2 = fast_score_from_d(d);
      fast_diffs_px<3>(Lr, Mr, Rr, d); int s3 = fast_score_from_d(d);
      if (xq < 3 || xq >= L.w - 3) s0 = 0;
      if (xq + 1 < 3 || xq + 1 >= L.w - 3) s1 = 0;
      if (xq + 2 < 3 || xq + 2 >= L.w - 3) s2 = 0;
      if (xq + 3 < 3 || xq + 3 >= L.w - 3) s3 = 0;
      out = (uint32_t)s0 | ((uint32_t)s1 << 8) | ((uint32_t)s2 << 16) | ((uint32_t)s3 << 24);
    }
    S.score[i] = out;
  }
}

// 4-point pre-test, byte-parallel (4 pixels per dword).  Bit 7 of each result byte is set where the pixel PASSES:
// centre - ring > T for two adjacent compass points (D), or ring - centre > T for two adjacent ones (B).
// Adjacent pairs of a 4-cycle: (D0&D4)|(D4&D8)|(D8&D12)|(D12&D0) == (D0|D8)&(D4|D12).  K4 = (T+1) * 0x01010101, T+1 <= 127.
// swar_ge: bit 7 of every byte = (a >= b), from the 7-bit difference t = (a|H) - (b&~H) which never borrows.
// Three-input boolean ops are spelled as v_bitop3_b32 explicitly: it issues at the full VALU rate on gfx950 while
// v_or3 / v_and_or (what the compiler picks for the same expressions) issue at half rate
// (profiles/r01_valu_issue_rates.txt).  Truth table = the expression evaluated on (0xF0, 0xCC, 0xAA).
template <class F>
constexpr uint32_t tt3(F f) { return f(0xF0u, 0xCCu, 0xAAu) & 0xFFu; }
#define BITOP3(a, b, c, EXPR) \
  __builtin_amdgcn_bitop3_b32((a), (b), (c), tt3([](uint32_t A, uint32_t B, uint32_t C) { return (EXPR); }))
__device__ __forceinline__ uint32_t swar_ge(uint32_t aH, uint32_t a, uint32_t b, uint32_t bL) {
  const uint32_t t = aH - bL;
  return BITOP3(a, b, t, (A & ~B) | (~(A ^ B) & C));
}
// the same with the 7-bit difference handed in: for the brighter compare (ring | H) - chL = (ring & Lm) + (H - chL) per byte,
// no carry or borrow (chL <= 127), ring & Lm is what the darker compare needs anyway and H - chL is one value per quad
__device__ __forceinline__ uint32_t swar_ge_t(uint32_t a, uint32_t b, uint32_t t) {
  return BITOP3(a, b, t, (A & ~B) | (~(A ^ B) & C));
}
__device__ __forceinline__ uint32_t pretest_pass4(uint32_t c, uint32_t rd, uint32_t rr, uint32_t ru, uint32_t rl, uint32_t K4) {
  const uint32_t H = 0x80808080u, Lm = 0x7F7F7F7Fu;
  const uint32_t t = (c | H) - K4;                          // 128 + (c & 127) - K per byte
  const uint32_t cl = BITOP3(t, c, Lm, A & (B | C));        // c - K where c >= K;          bit 7 of (c | t): c >= K
  const uint32_t u = (c & Lm) + K4;                         // (c & 127) + K <= 254 per byte
  const uint32_t ch = BITOP3(u, c, H, A | (B & C));         // c + K where it fits a byte;  bit 7 of ~(c & u): it does
  const uint32_t clH = cl | H, chL = ch & Lm;
  const uint32_t D0 = swar_ge(clH, cl, rd, rd & Lm), D4 = swar_ge(clH, cl, rr, rr & Lm);
  const uint32_t D8 = swar_ge(clH, cl, ru, ru & Lm), D12 = swar_ge(clH, cl, rl, rl & Lm);
  const uint32_t B0 = swar_ge(rd | H, rd, ch, chL), B4 = swar_ge(rr | H, rr, ch, chL);
  const uint32_t B8 = swar_ge(ru | H, ru, ch, chL), B12 = swar_ge(rl | H, rl, ch, chL);
  const uint32_t Dx = D0 | D8, Bx = B0 | B8;
  const uint32_t Dy = BITOP3(D4, D12, Dx, (A | B) & C), By = BITOP3(B4, B12, Bx, (A | B) & C);
  const uint32_t Dm = BITOP3(Dy, c, t, A & (B | C));        // & (c >= K)
  const uint32_t Bm = BITOP3(By, c, u, A & ~(B & C));       // & (c + K <= 255)
  return BITOP3(Dm, Bm, H, (A | B) & C);
}

// The segment test itself, byte-parallel: bit 7 of byte j = pixel j of the quad IS a corner at threshold T (nine contiguous
// ring pixels all darker than centre - T or all brighter than centre + T), K4 = (T + 1) * 0x01010101.  p = the quad's centre row
// in the staged tile (p[0], p[1], p[2] = the dwords of x-4.., x.., x+4..); ring byte k of the four pixels = one dword, taken
// straight (dx = 0) or cut out of two neighbours with v_alignbyte.  Contiguity of 9 out of 16 (cyclic) with three-input ANDs:
// A3[k] = M[k] & M[k+1] & M[k+2], A9[k] = A3[k] & A3[k+3] & A3[k+6], any = OR_k A9[k] -- 40 v_bitop3 per polarity.
// Used where every corner at the base threshold is wanted (reference key-point order): the exact score is then computed for the
// corners only (~10 % of the pixels of a textured frame) instead of for every pixel.
// The result is already masked with cmask (bit 7 of the bytes of the testable pixels) and carries the polarity: bit 6 of a corner's
// byte is set where its arc is the brighter side (Bm), clear where it is the darker one (Dm) -- never both, two 9-arcs of a 16-ring
// overlap.  The scorer of the queued corners evaluates that side only (fast_score_one_sided).
// The brighter compare takes its 7-bit difference as (ring & Lm) + (H - chL): ring & Lm is shared with the darker compare and
// H - chL is one value per quad, so a ring dword costs AND, SUB, ADD and two v_bitop3 for both compares (an OR less than swar_ge twice).
__device__ __forceinline__ uint32_t corner16_pass4(const uint32_t* p, uint32_t K4, uint32_t cmask) {
  const uint32_t H = 0x80808080u, Lm = 0x7F7F7F7Fu;
  const uint32_t c = p[1];
  const uint32_t t = (c | H) - K4;
  const uint32_t cl = BITOP3(t, c, Lm, A & (B | C));
  const uint32_t u = (c & Lm) + K4;
  const uint32_t ch = BITOP3(u, c, H, A | (B & C));
  const uint32_t clH = cl | H;
  uint32_t cB = H - (ch & Lm);
  asm volatile("" : "+v"(cB));     // pinned: left alone the compiler folds (ring & Lm) + (H - chL) back into an add and a subtract per ring pixel
  uint32_t r[16];
  {
    const uint32_t* q = p + 3 * FR_DW;                       // row y + 3: ring 15, 0, 1
    const uint32_t l = q[0], m = q[1], rr = q[2];
    r[0] = m; r[1] = __builtin_amdgcn_alignbyte(rr, m, 1); r[15] = __builtin_amdgcn_alignbyte(m, l, 3);
  }
  {
    const uint32_t* q = p + 2 * FR_DW;                       // row y + 2: ring 14, 2
    r[2] = __builtin_amdgcn_alignbyte(q[2], q[1], 2); r[14] = __builtin_amdgcn_alignbyte(q[1], q[0], 2);
  }
  {
    const uint32_t* q = p + FR_DW;                           // row y + 1: ring 13, 3
    r[3] = __builtin_amdgcn_alignbyte(q[2], q[1], 3); r[13] = __builtin_amdgcn_alignbyte(q[1], q[0], 1);
  }
  r[4] = __builtin_amdgcn_alignbyte(p[2], c, 3); r[12] = __builtin_amdgcn_alignbyte(c, p[0], 1);   // row y: ring 12, 4
  {
    const uint32_t* q = p - FR_DW;                           // row y - 1: ring 11, 5
    r[5] = __builtin_amdgcn_alignbyte(q[2], q[1], 3); r[11] = __builtin_amdgcn_alignbyte(q[1], q[0], 1);
  }
  {
    const uint32_t* q = p - 2 * FR_DW;                       // row y - 2: ring 10, 6
    r[6] = __builtin_amdgcn_alignbyte(q[2], q[1], 2); r[10] = __builtin_amdgcn_alignbyte(q[1], q[0], 2);
  }
  {
    const uint32_t* q = p - 3 * FR_DW;                       // row y - 3: ring 9, 8, 7
    const uint32_t l = q[0], m = q[1], rr = q[2];
    r[8] = m; r[7] = __builtin_amdgcn_alignbyte(rr, m, 1); r[9] = __builtin_amdgcn_alignbyte(m, l, 3);
  }
  uint32_t D[16], Bq[16];
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const uint32_t rL = r[k] & Lm;
    D[k] = swar_ge(clH, cl, r[k], rL);                       // centre - (T + 1) >= ring: darker
    Bq[k] = swar_ge_t(r[k], ch, rL + cB);                    // ring >= centre + (T + 1): brighter
  }
  uint32_t d3[16], b3[16];
#pragma unroll
  for (int k = 0; k < 16; k++) {
    d3[k] = BITOP3(D[k], D[(k + 1) & 15], D[(k + 2) & 15], A & B & C);
    b3[k] = BITOP3(Bq[k], Bq[(k + 1) & 15], Bq[(k + 2) & 15], A & B & C);
  }
  uint32_t dany = 0, bany = 0;
#pragma unroll
  for (int k = 0; k < 16; k += 2) {
    const uint32_t d9a = BITOP3(d3[k], d3[(k + 3) & 15], d3[(k + 6) & 15], A & B & C);
    const uint32_t d9b = BITOP3(d3[k + 1], d3[(k + 4) & 15], d3[(k + 7) & 15], A & B & C);
    dany = BITOP3(dany, d9a, d9b, A | B | C);
    const uint32_t b9a = BITOP3(b3[k], b3[(k + 3) & 15], b3[(k + 6) & 15], A & B & C);
    const uint32_t b9b = BITOP3(b3[k + 1], b3[(k + 4) & 15], b3[(k + 7) & 15], A & B & C);
    bany = BITOP3(bany, b9a, b9b, A | B | C);
  }
  const uint32_t Dm = BITOP3(dany, c, t, A & (B | C));       // & (centre >= T + 1): centre - (T + 1) did not wrap
  const uint32_t Bm = BITOP3(bany, c, u, A & ~(B & C));      // & (centre + T + 1 <= 255)
  const uint32_t pass = BITOP3(Dm, Bm, cmask, (A | B) & C);
  return BITOP3(pass, Bm >> 1, cmask >> 1, A | (B & C));     // bit 6 beside a corner's bit 7: the ring is the brighter side
}

// lifted path: only scores >= T are produced.  Phase A: 4-point pre-test at T (any 9-arc holds two adjacent
// compass points), four pixels per 32-bit operation; a quad with at least one passing pixel is queued
// (quad index | pass bits << 16).  Phase B: exact score of the queued pixels, 4 lanes per queued quad.
// FULL16 (reference key-point order, T = the base threshold): phase A is the whole segment test, every passing pixel is a corner
// and is queued on its own with its polarity, and phase B scores one corner per lane on its own side of the ring only.
template <bool FULL16 = false>
__device__ __forceinline__ void fast_lift_scores(FastLds& S, const EvhLevel& L, int x0, int y0, int T) {
  const uint32_t K4 = (uint32_t)(T + 1) * 0x01010101u;
  // tiles whose whole score plane lies inside the testable range need no per-pixel range checks (wave-uniform)
  const bool interior = (y0 - 1 >= 3) && (y0 + FT_H < L.h - 3) && (x0 - 4 >= 3) && (x0 + FT_W + 3 < L.w - 3);
  // a thread takes quads tid, tid+256, tid+512, tid+768 of the 30 x 34 quad grid; the per-quad pass words (bit 7 of
  // byte j = pixel j passes) stay in registers and are queued once after the loop with one LDS atomic per wave
  uint32_t P[4];
  int sr = threadIdx.x / FS_DW, sq = threadIdx.x - sr * FS_DW;
  static_assert((FS_H * FS_DW) % 4 == 0 && FS_H * FS_DW <= 1024, "one 16-byte store per thread clears the score plane");
  if (threadIdx.x < FS_H * FS_DW / 4)                           // phase B overwrites the bytes that reach T
    reinterpret_cast<uint4*>(S.score)[threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
  // two copies of the loop: the interior one (most tiles) is straight-line code, so the LDS reads of its four quads
  // can be issued together instead of each behind its own range test
  auto quads = [&](auto interior_tag) {
    constexpr bool INTERIOR = decltype(interior_tag)::value;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int i = threadIdx.x + 256 * k;
      P[k] = 0;
      if (i < FS_H * FS_DW) {
        uint32_t cmask = 0x80808080u;
        bool rowok = true;
        if constexpr (!INTERIOR) {
          const int y = y0 - 1 + sr, xq = x0 - 4 + sq * 4;
          rowok = y >= 3 && y < L.h - 3;
          cmask = quad_range_mask(xq, 3, L.w - 3);
        }
        if (INTERIOR || (rowok && cmask)) {
          const uint32_t* p = S.raw + mad24((uint32_t)(sr + 3), FR_DW, (uint32_t)sq);    // centre row, dword of x = xq-4
          if constexpr (FULL16) {
            P[k] = corner16_pass4(p, K4, cmask);
          } else {
            const uint32_t Lc = p[0], Mc = p[1], Rc = p[2], Mu = p[1 - 3 * FR_DW], Md = p[1 + 3 * FR_DW];
            P[k] = pretest_pass4(Mc, Md, __builtin_amdgcn_alignbyte(Rc, Mc, 3), Mu, __builtin_amdgcn_alignbyte(Mc, Lc, 1), K4) &
                   cmask;
          }
        }
      }
      sr += 7; sq += 18;                                        // +256 quads = +7 rows +18 quads
      if (sq >= FS_DW) { sq -= FS_DW; sr++; }
    }
  };
  if (interior) quads(std::true_type{}); else quads(std::false_type{});
  const uint8_t* rawb = reinterpret_cast<const uint8_t*>(S.raw);
  uint8_t* scoreb = reinterpret_cast<uint8_t*>(S.score);
  // exact score of the pixel `j` of quad `qi`; writes the score byte when it reaches T
  auto score_pixel = [&](int qi, int j, bool list) {
    const int sr2 = qi / FS_DW, sq2 = qi - sr2 * FS_DW;
    const int pos = sr2 * FQ_PITCH + sq2 * 4 + j;
    const uint8_t* p = rawb + (sr2 + 3) * (FR_DW * 4) + sq2 * 4 + j + 4;
    const int v = p[0];
    uint32_t ring[16];
    fast_ring<FR_DW * 4>(p, ring);
    i16 d[16];
#pragma unroll
    for (int k = 0; k < 16; k++) d[k] = (i16)(v - (int)ring[k]);
    const int sc = fast_score_from_d(d);
    if (sc >= T) {
      scoreb[pos] = (uint8_t)sc;
      if (list) {
        const int k = atomicAdd(&S.scnt, 1);
        if (k < FSC_CAP) S.scored[k] = (uint16_t)pos;
      }
    }
  };
  if constexpr (FULL16) {
    // every passing pixel IS a corner (a fifth of the pixels of a textured frame): one lane per corner.  Queue of 16-bit
    // entries quad << 2 | pixel, bit 15 = the ring is the brighter side (bit 6 of the pass byte), in the words of S.lst
    // (2048 entries); a tile with more corners than that is scored densely.
    uint16_t* pq = reinterpret_cast<uint16_t*>(S.lst);
    constexpr int PQ_CAP = 2 * (FS_H * FS_DW);
    constexpr int PQ_POL = 15;
    static_assert(((FS_H * FS_DW - 1) << 2 | 3) < (1 << PQ_POL), "quad index and pixel stay below the polarity bit of a queue entry");
    const int mine = __popc(P[0] & 0x80808080u) + __popc(P[1] & 0x80808080u) + __popc(P[2] & 0x80808080u) + __popc(P[3] & 0x80808080u);
    int at = mine ? atomicAdd(&S.qcnt, mine) : 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      uint32_t m = P[k] & 0x80808080u;
      while (m) {
        const int b = __ffs(m) - 1;                  // bit 7, 15, 23 or 31
        m &= m - 1;
        const uint32_t pol = (P[k] >> (b - 1)) & 1u;
        if (at < PQ_CAP) pq[at] = (uint16_t)(((threadIdx.x + 256 * k) << 2) | (b >> 3) | (pol << PQ_POL));
        at++;
      }
    }
    __syncthreads();
    const int np = S.qcnt;
    if (np > PQ_CAP) {                               // workgroup-uniform
      fast_dense_scores(S, L, x0, y0);
      return;
    }
    // the segment test has decided both that the pixel is a corner (score >= T: the byte is written unconditionally) and
    // which side its arc is on: fast_score_one_sided
    for (int e = threadIdx.x; e < np; e += 256) {
      const uint32_t ent = pq[e];
      const uint32_t m = (0u - (ent >> PQ_POL)) & 0xFFu;
      const int qi = (ent >> 2) & 0x3FFu, j = ent & 3;
      const int sr2 = qi / FS_DW, sq2 = qi - sr2 * FS_DW;
      const uint8_t* p = rawb + (sr2 + 3) * (FR_DW * 4) + sq2 * 4 + j + 4;
      uint32_t ring[16];
      fast_ring<FR_DW * 4>(p, ring);
      scoreb[sr2 * FQ_PITCH + sq2 * 4 + j] = (uint8_t)fast_score_one_sided(p[0], ring, m);
    }
    return;
  }
  {
    const unsigned long long m0 = __ballot(P[0] != 0), m1 = __ballot(P[1] != 0), m2 = __ballot(P[2] != 0),
                             m3 = __ballot(P[3] != 0);
    const int n0 = __popcll(m0), n1 = __popcll(m1), n2 = __popcll(m2), tot = n0 + n1 + n2 + __popcll(m3);
    if (tot) {                                                  // wave-uniform
      int base = 0;
      if ((threadIdx.x & 63) == 0) base = atomicAdd(&S.qcnt, tot);
      base = __builtin_amdgcn_readfirstlane(base);
      // entry = quad index | bits {16: px0, 24: px1, 17: px2, 25: px3}
#define FQ_PUSH(k, off, m)                                                                                              \
      if (P[k]) S.lst[base + (off) + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)((m) >> 32),                             \
                                                                    __builtin_amdgcn_mbcnt_lo((uint32_t)(m), 0u))] =  \
          (uint32_t)(threadIdx.x + 256 * (k)) | (((P[k] >> 7) | (P[k] >> 22)) << 16)
      FQ_PUSH(0, 0, m0); FQ_PUSH(1, n0, m1); FQ_PUSH(2, n0 + n1, m2); FQ_PUSH(3, n0 + n1 + n2, m3);
#undef FQ_PUSH
    }
  }
  __syncthreads();
  const int nq = S.qcnt;
  // four lanes per queued quad.  (A pixel-granular list -- fewer busy waves -- was measured at +1.0 ms when a few dozen pixels
  // per tile pass: the four lanes of a quad read neighbouring bytes of the same LDS words, scattered pixels conflict on the
  // banks.  With the full segment test a fifth of the pixels pass and the pixel list wins: see FULL16 above.)
  for (int e = threadIdx.x; e < nq * 4; e += 256) {
    const uint32_t ent = S.lst[e >> 2];
    const int j = e & 3;
    if (!((ent >> (16 + 8 * (j & 1) + (j >> 1))) & 1u)) continue;
    score_pixel((int)(ent & 0xFFFu), j, true);
  }
}

// lifted path NMS: only the (few) pixels that reached T are visited
// (run by wave 0 alone: the list holds a few dozen pixels)
__device__ __forceinline__ void fast_nms_scored(FastLds& S, const EvhLevel& L, int x0, int y0) {
  if (!((L.w > 2 * EVH_EDGE) && (L.h > 2 * EVH_EDGE))) return;
  const uint8_t* sc = reinterpret_cast<const uint8_t*>(S.score);
  const int n = min(S.scnt, FSC_CAP);
  for (int i = threadIdx.x; i < n; i += 64) {
    const int pos = S.scored[i];
    const int sr = pos / FQ_PITCH, sx = pos - sr * FQ_PITCH;
    if (sr < 1 || sr > FT_H || sx < 4 || sx >= 4 + FT_W) continue;     // halo pixels belong to neighbouring tiles
    const int x = x0 - 4 + sx, y = y0 - 1 + sr;
    if (x < EVH_EDGE || x >= L.w - EVH_EDGE || y < EVH_EDGE || y >= L.h - EVH_EDGE) continue;
    const uint8_t* c = sc + pos;
    const int s = c[0];
    if (s > c[-1] && s > c[1] && s > c[-FQ_PITCH - 1] && s > c[-FQ_PITCH] && s > c[-FQ_PITCH + 1] &&
        s > c[FQ_PITCH - 1] && s > c[FQ_PITCH] && s > c[FQ_PITCH + 1]) {
      const int slot = atomicAdd(&S.lcnt, 1);
      S.lst[slot] = fast_cand((uint32_t)s, y, x);
    }
  }
}

// 3x3 non-max suppression (strict '>' against all 8 neighbours) + 31-px border filter -> S.lst / S.lcnt
__device__ __forceinline__ void fast_nms_collect(FastLds& S, const EvhLevel& L, int x0, int y0) {
  if (!((L.w > 2 * EVH_EDGE) && (L.h > 2 * EVH_EDGE))) return;
#pragma unroll 1
  for (int i = threadIdx.x; i < (FT_W / 4) * FT_H; i += 256) {
    const int qr = i / (FT_W / 4), qc = i - qr * (FT_W / 4);
    const int y = y0 + qr, xq = x0 + qc * 4;
    const uint32_t* p = S.score + (qr + 1) * FS_DW + (qc + 1);       // this quad, row y
    const uint32_t m = p[0];
    if (m == 0 || y < EVH_EDGE || y >= L.h - EVH_EDGE) continue;
    const uint32_t lft = p[-1], rgt = p[1];
    const uint32_t um = p[-FS_DW], ul = p[-FS_DW - 1], ur = p[-FS_DW + 1];
    const uint32_t dm = p[FS_DW], dl = p[FS_DW - 1], dr = p[FS_DW + 1];
    // 6-byte windows (x-1 .. x+4) of the three rows
    const uint64_t wu = ((uint64_t)ur << 40) | ((uint64_t)um << 8) | (ul >> 24);
    const uint64_t wm = ((uint64_t)rgt << 40) | ((uint64_t)m << 8) | (lft >> 24);
    const uint64_t wd = ((uint64_t)dr << 40) | ((uint64_t)dm << 8) | (dl >> 24);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int s = (int)((wm >> (8 * (j + 1))) & 0xFF);
      const int x = xq + j;
      if (s == 0 || x < EVH_EDGE || x >= L.w - EVH_EDGE) continue;
      const int n0 = (int)((wm >> (8 * j)) & 0xFF), n1 = (int)((wm >> (8 * (j + 2))) & 0xFF);
      const int u0 = (int)((wu >> (8 * j)) & 0xFF), u1 = (int)((wu >> (8 * (j + 1))) & 0xFF), u2 = (int)((wu >> (8 * (j + 2))) & 0xFF);
      const int d0 = (int)((wd >> (8 * j)) & 0xFF), d1 = (int)((wd >> (8 * (j + 1))) & 0xFF), d2 = (int)((wd >> (8 * (j + 2))) & 0xFF);
      if (s > n0 && s > n1 && s > u0 && s > u1 && s > u2 && s > d0 && s > d1 && s > d2) {
        const int slot = atomicAdd(&S.lcnt, 1);
        S.lst[slot] = fast_cand((uint32_t)s, y, x);
      }
    }
  }
}

// The same suppression with the survivors left in ROW-MAJOR order (reference key-point order: FAST hands its corners over
// row by row, and k_select_cv rebuilds a level's row-major list from the tiles' ordered bursts).  Wave w owns tile rows
// 7w .. 7w+6 and walks them two rows (64 quads) a step, so its survivors come out in order from ballots alone -- no
// barrier; they go to the wave's quarter of S.lst (at most one survivor per 2x2 block: <= 256 per wave).  S.wtot receives
// the survivors per wave, S.rowcnt the survivors per tile row (a byte each).
__device__ __forceinline__ void fast_nms_collect_ordered(FastLds& S, const EvhLevel& L, int x0, int y0) {
  const bool live = (L.w > 2 * EVH_EDGE) && (L.h > 2 * EVH_EDGE);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  static_assert(FT_H == 28 && FT_W == 128, "four waves x seven rows of 32 quads");
  uint32_t* mine = S.lst + 256 * wv;
  int running = 0;
  uint32_t rc_lo = 0, rc_hi = 0;        // survivors of this wave's rows 0..3 / 4..6, a byte each (lane 0 keeps them)
#pragma unroll 1
  for (int k = 0; k < 4; k++) {
    const int local = 64 * k + lane;    // quad index inside the wave's 7 x 32 block
    uint32_t v0 = 0, v1 = 0;
    int cnt = 0;
    if (live && local < 7 * 32) {
      const int qr = 7 * wv + (local >> 5), qc = local & 31;
      const int y = y0 + qr, xq = x0 + qc * 4;
      const uint32_t* p = S.score + (qr + 1) * FS_DW + (qc + 1);
      const uint32_t m = p[0];
      if (m != 0 && y >= EVH_EDGE && y < L.h - EVH_EDGE) {
        // byte-parallel 3 x 3 maximum test (round 4; the per-pixel form cost ~130 instructions per quad, a quarter of the
        // kernel): the eight neighbour bytes of the quad's four pixels as eight dwords (two straight, six cut out of two words
        // with v_alignbyte), bit 7 of a byte of swar_ge(n, c) = neighbour >= centre, a survivor = a nonzero centre byte that no
        // neighbour reaches.  Strict maxima in a 3 x 3 window: at most two of four neighbouring pixels survive.
        const uint32_t H = 0x80808080u, Lm = 0x7F7F7F7Fu;
        const uint32_t lft = p[-1], rgt = p[1];
        const uint32_t um = p[-FS_DW], ul = p[-FS_DW - 1], ur = p[-FS_DW + 1];
        const uint32_t dm = p[FS_DW], dl = p[FS_DW - 1], dr = p[FS_DW + 1];
        const uint32_t nl = __builtin_amdgcn_alignbyte(m, lft, 3), nr = __builtin_amdgcn_alignbyte(rgt, m, 1);
        const uint32_t nul = __builtin_amdgcn_alignbyte(um, ul, 3), nur = __builtin_amdgcn_alignbyte(ur, um, 1);
        const uint32_t ndl = __builtin_amdgcn_alignbyte(dm, dl, 3), ndr = __builtin_amdgcn_alignbyte(dr, dm, 1);
        const uint32_t cL = m & Lm;
        const uint32_t g0 = swar_ge(nl | H, nl, m, cL), g1 = swar_ge(nr | H, nr, m, cL), g2 = swar_ge(um | H, um, m, cL);
        const uint32_t g3 = swar_ge(nul | H, nul, m, cL), g4 = swar_ge(nur | H, nur, m, cL), g5 = swar_ge(dm | H, dm, m, cL);
        const uint32_t g6 = swar_ge(ndl | H, ndl, m, cL), g7 = swar_ge(ndr | H, ndr, m, cL);
        const uint32_t ga = BITOP3(g0, g1, g2, A | B | C), gb = BITOP3(g3, g4, g5, A | B | C);
        const uint32_t any_ge = BITOP3(ga, gb, g6 | g7, A | B | C);
        const uint32_t nz = (cL + Lm) | m;                    // bit 7 of a byte: the centre byte is not zero
        uint32_t keep = BITOP3(nz, any_ge, H, A & ~B & C);
        keep &= quad_range_mask(xq, EVH_EDGE, L.w - EVH_EDGE);
        if (keep) {
          const int b0 = __ffs(keep) - 1;                     // bit 7, 15, 23 or 31 of the first survivor
          const int j0 = b0 >> 3;
          v0 = fast_cand((m >> (8 * j0)) & 0xFFu, y, xq + j0);
          cnt = 1;
          const uint32_t rest = keep & (keep - 1u);
          if (rest) {
            const int j1 = (__ffs(rest) - 1) >> 3;
            v1 = fast_cand((m >> (8 * j1)) & 0xFFu, y, xq + j1);
            cnt = 2;
          }
        }
      }
    }
    const unsigned long long m1 = __ballot(cnt >= 1), m2 = __ballot(cnt >= 2);
    const unsigned long long lt = (1ull << lane) - 1ull;
    const int pre = running + __popcll(m1 & lt) + __popcll(m2 & lt);
    if (cnt >= 1) mine[pre] = v0;
    if (cnt >= 2) mine[pre + 1] = v1;
    running += __popcll(m1) + __popcll(m2);
    const uint32_t ra = (uint32_t)(__popcll(m1 & 0xFFFFFFFFull) + __popcll(m2 & 0xFFFFFFFFull));
    const uint32_t rb = (uint32_t)(__popcll(m1 >> 32) + __popcll(m2 >> 32));
    if (k < 2) rc_lo |= (ra << (16 * k)) | (rb << (16 * k + 8));
    else rc_hi |= (ra << (16 * (k - 2))) | (rb << (16 * (k - 2) + 8));
  }
  if (lane == 0) {
    S.wtot[wv] = running;
    // tile row 7w + i -> byte (7w + i) & 3 of word (7w + i) >> 2; the rows of different waves share words: LDS atomics
    for (int i = 0; i < 7; i++) {
      const uint32_t c = i < 4 ? (rc_lo >> (8 * i)) & 0xFFu : (rc_hi >> (8 * (i - 4))) & 0xFFu;
      const int row = 7 * wv + i;
      if (c) atomicOr(&S.rowcnt[row >> 2], c << (8 * (row & 3)));
    }
  }
}

// the candidate list of level L of frame f, and the reservation of n slots at its end (returns the first)
__device__ __forceinline__ uint32_t* fast_cand_list(const FastArgs& A, const EvhLevel& L, int f) {
  return A.cand + (int64_t)f * A.cand_frame_entries + L.cand_off;
}
__device__ __forceinline__ int fast_reserve(const FastArgs& A, int f, int l, int n) {
  return atomicAdd(A.cand_count + f * EVH_NLEVELS + l, n);
}

// ordered bursts: the four waves' quarters of S.lst one after another, then the tile's descriptor for k_select_cv
// (word 0 = offset of the burst in the level's candidate list, words 1..7 = survivors per tile row)
__device__ __forceinline__ void fast_emit_ordered(FastLds& S, const FastArgs& A, const EvhLevel& L, int f, int l, int tile) {
  __syncthreads();
  const int n0 = S.wtot[0], n1 = S.wtot[1], n2 = S.wtot[2], n = n0 + n1 + n2 + S.wtot[3];
  if (n > 0) {                                              // workgroup-uniform
    if (threadIdx.x == 0) S.gbase = fast_reserve(A, f, l, n);
    __syncthreads();
  }
  const int base = n > 0 ? S.gbase : 0;
  if (n > 0) {
    uint32_t* out = fast_cand_list(A, L, f);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int cnt = S.wtot[wv], off = wv == 0 ? 0 : wv == 1 ? n0 : wv == 2 ? n0 + n1 : n0 + n1 + n2;
    for (int i = lane; i < cnt; i += 64)
      if (base + off + i < L.cand_cap) out[base + off + i] = S.lst[256 * wv + i];
  }
  if (threadIdx.x < 8) {
    uint32_t* d = A.tdesc + ((int64_t)f * A.total_tiles + tile) * 8;
    d[threadIdx.x] = threadIdx.x == 0 ? (uint32_t)base : S.rowcnt[threadIdx.x - 1];
  }
}

// survivors -> the level's candidate list; ONE global atomic per workgroup reserves the slots (a returning global
// atomic per wave would serialise on its ~1-2 us latency)
__device__ __forceinline__ void fast_emit(FastLds& S, const FastArgs& A, const EvhLevel& L, int f, int l) {
  __syncthreads();
  const int n = S.lcnt;
  if (n > 0) {
    if (threadIdx.x == 0) S.gbase = fast_reserve(A, f, l, n);
    __syncthreads();
    uint32_t* out = fast_cand_list(A, L, f);
    const int base = S.gbase;
    for (int i = threadIdx.x; i < n; i += 256)
      if (base + i < L.cand_cap) out[base + i] = S.lst[i];
  }
}

// the same by wave 0 alone (the other waves of the workgroup have left): wave-level ordering only, no barrier
__device__ __forceinline__ void fast_emit_wave0(FastLds& S, const FastArgs& A, const EvhLevel& L, int f, int l) {
  WAVE_LDS_SYNC();
  const int n = S.lcnt;
  if (n > 0) {
    int base = 0;
    if (threadIdx.x == 0) base = fast_reserve(A, f, l, n);
    base = __builtin_amdgcn_readfirstlane(base);
    uint32_t* out = fast_cand_list(A, L, f);
    for (int i = threadIdx.x; i < n; i += 64)
      if (base + i < L.cand_cap) out[base + i] = S.lst[i];
  }
}

__device__ __forceinline__ int fast_level_of_tile(const FastArgs& A, int& t) {
  int l = 0;
#pragma unroll
  for (int i = 1; i < EVH_NLEVELS; i++)
    if (t >= A.lv[i].tile_start) l = i;
  t -= A.lv[l].tile_start;
  return l;
}

// origin (x0, y0) of tile t of level L (tiles are numbered row by row)
__device__ __forceinline__ void fast_tile_origin(const EvhLevel& L, int t, int& x0, int& y0) {
  const int ty = t / L.tiles_x, tx = t - ty * L.tiles_x;
  x0 = EVH_FAST_OX + tx * FT_W; y0 = EVH_FAST_OY + ty * FT_H;
}

// K3 dense: every tile of every level at threshold 20
__global__ __launch_bounds__(256) void k_fast(FastArgs A) {
  __shared__ FastLds S;
  const int f = blockIdx.y;
  int t = blockIdx.x;
  const int l = fast_level_of_tile(A, t);
  const EvhLevel L = A.lv[l];
  int x0, y0; fast_tile_origin(L, t, x0, y0);
  fast_stage(S, A.pyr + (int64_t)f * A.pyr_frame_bytes + L.off, L, x0, y0);
  __syncthreads();
  fast_dense_scores(S, L, x0, y0);
  __syncthreads();
  if (A.tdesc) {                                   // reference key-point order (workgroup-uniform)
    fast_nms_collect_ordered(S, L, x0, y0);
    fast_emit_ordered(S, A, L, f, l, (int)blockIdx.x);
    return;
  }
  fast_nms_collect(S, L, x0, y0);
  fast_emit(S, A, L, f, l);
}

// ------------------------------------------------------------------------------------------------------------
// K3, threshold-lifted form.  ORB keeps only the 2*quota best-scoring FAST corners of a level (all ties at the
// cut), typically <1 % of the corners found at threshold 20.  A corner with score >= T is kept by NMS and by that
// selection exactly as before if every pixel with score < T is treated as "no corner": such neighbours cannot
// suppress it and cannot be selected.  So the exact score is only needed for pixels that can reach T.
//   k_fast_sample: threshold 20 on a sparse lattice of tiles (every 27th / 13th / 7th tile of a level), histogram
//                  of the NMS-surviving scores;
//   k_fast_thr:    T per (frame, level) such that ~4x the needed 2*quota corners are expected at or above it;
//   k_fast_main:   all tiles at T (pre-test + queued exact scores; the dense path where T stayed 20);
//   k_fast_verify: a lifted level that delivered fewer than 2*quota corners is reset ...
//   k_fast_redo:   ... and redone at threshold 20.  The result equals the dense kernel's by construction.
__global__ __launch_bounds__(256, 8) void k_fast_sample(FastArgs A) {
  __shared__ FastLds S;
  const int f = blockIdx.y;
  if (A.share_group > 0 && ((f % A.share_group) & 1)) return;   // shares the histogram of frame f - 1
  int s = blockIdx.x, l = 0;
#pragma unroll
  for (int i = 1; i < EVH_NLEVELS; i++)
    if (s >= A.samp_start[i]) l = i;
  s -= A.samp_start[l];
  const int mod = A.samp_mod[l];
  const EvhLevel L = A.lv[l];
  if (mod == 0) return;
  const int t = (f * 5 + l) % mod + s * mod;          // sampled tile index inside the level
  if (t >= L.tiles_x * L.tiles_y) return;
  int x0, y0; fast_tile_origin(L, t, x0, y0);
  const int hint = A.hint_in[l];
  const int Tp = (hint > 36 && hint < 256) ? max(EVH_FAST_THR + 1, (hint * 7) >> 3) : 0;   // 0: dense sample
  fast_stage(S, A.pyr + (int64_t)f * A.pyr_frame_bytes + L.off, L, x0, y0);
  __syncthreads();
  if (Tp) fast_lift_scores(S, L, x0, y0, Tp);          // exact scores >= Tp, zero elsewhere
  else fast_dense_scores(S, L, x0, y0);
  __syncthreads();
  if (Tp && S.scnt <= FSC_CAP) {               // workgroup-uniform: the short list of scored pixels is complete
    if (threadIdx.x < 64) fast_nms_scored(S, L, x0, y0);
  } else {
    fast_nms_collect(S, L, x0, y0);
  }
  __syncthreads();
  const int n = S.lcnt;
  unsigned* h = A.shist + (int64_t)(f * EVH_NLEVELS + l) * 256;
  if (threadIdx.x == 0) h[0] = (unsigned)Tp;            // bin 0 (never a score) carries the floor of this histogram
  // tile histogram in LDS first (the score plane is dead), then one global atomic per non-empty bin
  uint32_t* lh = S.score;
  lh[threadIdx.x] = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += 256) atomicAdd(&lh[cand_score(S.lst[i])], 1u);
  __syncthreads();
  const uint32_t cnt = lh[threadIdx.x];
  if (cnt && threadIdx.x > EVH_FAST_THR) atomicAdd(&h[threadIdx.x], cnt);
}

__global__ void k_fast_thr(FastArgs A, int nframes) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nframes * EVH_NLEVELS) return;
  const int l = i % EVH_NLEVELS;
  const EvhLevel L = A.lv[l];
  const int mod = A.samp_mod[l];
  int T = EVH_FAST_THR;
  if (mod > 0 && L.quota > 0) {
    const int need = max(24, (6 * L.quota + mod - 1) / mod);   // 3x the 2*quota corners the level must deliver (8: +3 % FAST time)
    const int f = i / EVH_NLEVELS;
    const int src = (A.share_group > 0 && ((f % A.share_group) & 1)) ? i - EVH_NLEVELS : i;
    const unsigned* h = A.shist + (int64_t)src * 256;
    const int floor_t = (int)h[0];                       // 0: dense histogram, else exact only from floor_t up
    int acc = 0;
    T = floor_t ? floor_t : EVH_FAST_THR;                // not enough mass above the floor: take all of it (verify decides)
    for (int s = 255; s > max(EVH_FAST_THR, floor_t - 1); s--) {
      acc += (int)h[s];
      if (acc >= need) { T = s; break; }
    }
    if (src == i) atomicAdd(&A.hint_hist[l * 256 + (T > EVH_FAST_THR ? min(T, 255) : 0)], 1u);   // vote for the next call's hint
  }
  A.thr[i] = min(T, 126);   // the byte-parallel pre-test needs T + 1 <= 127; any T in (20, score range] is exact
  if (i == 0) A.redo[0] = 0;                // work list of k_fast_redo: [0] = count, [1..] = frame * 8 + level
}

__global__ __launch_bounds__(256, 8) void k_fast_main(FastArgs A) {
  __shared__ FastLds S;
  const int f = blockIdx.y;      // (the XCD order of the gray / pyramid kernels measured no gain here: VALU-bound)
  int t = blockIdx.x;
  const int l = fast_level_of_tile(A, t);
  const EvhLevel L = A.lv[l];
  int x0, y0; fast_tile_origin(L, t, x0, y0);
  const int T = A.lift_base ? EVH_FAST_THR : A.thr[f * EVH_NLEVELS + l];
  fast_stage(S, A.pyr + (int64_t)f * A.pyr_frame_bytes + L.off, L, x0, y0);
  __syncthreads();
  if (A.lift_base) {
    // reference key-point order: every corner at the base threshold, found by the full segment test, scored exactly, handed
    // over as a row-major burst (fast_nms_collect_ordered walks the score plane, which is complete: zero where no corner is)
    fast_lift_scores<true>(S, L, x0, y0, EVH_FAST_THR);
    __syncthreads();
    fast_nms_collect_ordered(S, L, x0, y0);
    fast_emit_ordered(S, A, L, f, l, (int)blockIdx.x);
    return;
  }
  if (T > EVH_FAST_THR) {
    fast_lift_scores(S, L, x0, y0, T);
    __syncthreads();
    if (S.scnt <= FSC_CAP) {                      // workgroup-uniform.  What is left is a few dozen scored pixels:
      if (threadIdx.x >= 64) return;              // waves 1-3 are done (no barrier follows on this path), wave 0
      fast_nms_scored(S, L, x0, y0);              // runs NMS and the emission on its own
      fast_emit_wave0(S, A, L, f, l);
      return;
    }
    fast_nms_collect(S, L, x0, y0);               // the short list overflowed: the score plane itself is complete
  } else {
    fast_dense_scores(S, L, x0, y0);
    __syncthreads();
    fast_nms_collect(S, L, x0, y0);
  }
  fast_emit(S, A, L, f, l);
}

__global__ void k_fast_verify(FastArgs A, int nframes) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nframes * EVH_NLEVELS) return;
  const int l = i % EVH_NLEVELS;
  if (A.thr[i] > EVH_FAST_THR && A.cand_count[i] < 2 * A.lv[l].quota) {
    A.cand_count[i] = 0;
    A.thr[i] = EVH_FAST_THR;
    A.redo[1 + atomicAdd(&A.redo[0], 1)] = i;
    atomicAdd(&A.hint_hist[l * 256], 1u);               // a vote for 'no hint': the level came up short
  }
}

// next call's hint per level: the lower quartile of this call's votes (robust against a few odd frames; a frame whose
// own threshold lies below 7/8 of it merely takes everything above that floor, and verify/redo stays the safety net)
__global__ void k_fast_hint(FastArgs A) {
  const int l = threadIdx.x;
  if (l >= EVH_NLEVELS) return;
  const unsigned* h = A.hint_hist + l * 256;
  unsigned total = 0;
  for (int s = 0; s < 256; s++) total += h[s];
  int hint = 0;
  if (total) {
    unsigned acc = 0;
    for (int s = 0; s < 256; s++) { acc += h[s]; if (4 * acc >= total) { hint = s; break; } }
  }
  A.hint_out[l] = hint;
}

// dense rescoring of the (frame, level) entries k_fast_verify listed: blockIdx.x = tile of the level, blockIdx.y
// walks the list, so a flagged level is redone by all its tiles in parallel; with an empty list every workgroup leaves
// at once
__global__ __launch_bounds__(256) void k_fast_redo(FastArgs A) {
  __shared__ FastLds S;
  const int count = A.redo[0];
  for (int e = blockIdx.y; e < count; e += gridDim.y) {      // workgroup-uniform bounds
    const int i = A.redo[1 + e];
    const int f = i / EVH_NLEVELS, l = i - f * EVH_NLEVELS;
    const EvhLevel L = A.lv[l];
    const int t = blockIdx.x;
    if (t < L.tiles_x * L.tiles_y) {
      int x0, y0; fast_tile_origin(L, t, x0, y0);
      fast_stage(S, A.pyr + (int64_t)f * A.pyr_frame_bytes + L.off, L, x0, y0);
      __syncthreads();
      fast_dense_scores(S, L, x0, y0);
      __syncthreads();
      fast_nms_collect(S, L, x0, y0);
      fast_emit(S, A, L, f, l);
    }
    __syncthreads();
  }
}
}  // namespace
