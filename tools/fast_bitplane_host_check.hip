// Host check of the bit-plane segment test of evh_detect_fast.h (bp_planes_item, bp_segment32, bp_range_mask: what
// fast_plane_scores runs per lane, and fast_corner_px for the two columns beside the groups) against the definition: a corner has
// nine contiguous ring pixels all below centre - 20 or all above centre + 20, and only a pixel at least 3 from every border of the
// level is tested.  A level is walked tile by tile the way k_fast_main does it: the tile's 36 x 144 bytes staged (zero outside the
// level, garbage in the padding between its width and its stride), 36 x 5 transposition items, 30 x 4 segment items, 60 single
// pixels; corner and polarity masks are compared pixel for pixel over the tile's score window (rows y0 - 1 .. y0 + 28, columns
// x0 - 1 .. x0 + 128).  The host build emulates v_perm, v_alignbit and v_bitop3.  Stand-alone: built for the host (with ASan + UBSan)
// and run by tests/test_fast_bitplane_host.py.
#include "evh_detect_fast.h"
#include <cstdio>
#include <random>
#include <vector>

struct Img {
  int w, h, stride;
  std::vector<uint8_t> px;      // h x stride
  Img(int w_, int h_) : w(w_), h(h_), stride((w_ + 63) / 64 * 64), px((size_t)h_ * ((w_ + 63) / 64 * 64), 0) {}
  uint8_t& at(int x, int y) { return px[(size_t)y * stride + x]; }
};

// 0: no corner, 1: ring darker, 2: ring brighter (from the definition; x, y at least 3 from the borders)
static int corner_def(Img& I, int x, int y) {
  const int c = I.at(x, y);
  bool d[32], b[32];
  for (int k = 0; k < 16; k++) {
    const int r = I.at(x + FAST_RING[k][0], y + FAST_RING[k][1]);
    d[k] = d[k + 16] = r < c - 20;
    b[k] = b[k + 16] = r > c + 20;
  }
  int res = 0;
  for (int k = 0; k < 16; k++) {
    bool ad = true, ab = true;
    for (int i = 0; i < 9; i++) { ad = ad && d[k + i]; ab = ab && b[k + i]; }
    if (ad) res |= 1;
    if (ab) res |= 2;
  }
  return res;
}

static long g_checked = 0, g_dark = 0, g_bright = 0, g_bits[32][3];

// every tile of the level; returns false at the first pixel that differs
static bool check_level(Img& I, const char* what) {
  const int tiles_x = (I.w - EVH_FAST_OX + FT_W - 1) / FT_W + 1, tiles_y = (I.h - EVH_FAST_OY + FT_H - 1) / FT_H + 1;
  std::vector<uint32_t> raw(FR_H * FR_DW), pl(BP_WORDS);
  for (int ty = 0; ty < tiles_y; ty++) for (int tx = 0; tx < tiles_x; tx++) {
    const int x0 = EVH_FAST_OX + FT_W * tx, y0 = EVH_FAST_OY + FT_H * ty;
    uint8_t* rb = reinterpret_cast<uint8_t*>(raw.data());
    for (int r = 0; r < FR_H; r++) for (int c = 0; c < FR_DW * 4; c++) {
      const int x = x0 - 8 + c, y = y0 - 4 + r;
      rb[r * FR_DW * 4 + c] = (x >= 0 && x < I.stride && y >= 0 && y < I.h) ? I.at(x, y) : 0;
    }
    for (auto& v : pl) v = 0xDEADBEEFu;               // the words no item writes (the padding of a row) are never read
    for (int i = 0; i < FR_H * (BP_ROWITEMS + 1); i++) {
      const int r = i / (BP_ROWITEMS + 1), t = i - r * (BP_ROWITEMS + 1);
      bp_planes_item(raw.data() + r * FR_DW, t, pl.data() + r * BP_PITCH);
    }
    // the planes are what they are called: bit i of plane b of a tile group = bit b of its pixel i
    for (int r = 0; r < FR_H; r++) for (int g = 0; g < BP_ROWITEMS; g++) for (int b = 0; b < 8; b++) for (int i = 0; i < 32; i++)
      if (((pl[r * BP_PITCH + b * BP_NG + g + 1] >> i) & 1u) != ((rb[r * FR_DW * 4 + 8 + 32 * g + i] >> b) & 1u)) {
        printf("PLANE %s tile %d,%d row %d group %d plane %d bit %d\n", what, tx, ty, r, g, b, i);
        return false;
      }
    for (int sr = 0; sr < FS_H; sr++) {
      const int y = y0 - 1 + sr;
      const bool rowok = y >= 3 && y < I.h - 3;
      for (int sx = 3; sx <= 4 + FT_W; sx++) {          // score-window columns x0 - 1 .. x0 + FT_W
        const int x = x0 - 4 + sx;
        int got;
        if (sx == 3 || sx == 4 + FT_W) {
          got = 0;
          if (rowok && x >= 3 && x < I.w - 3) {
            const uint32_t c = fast_corner_px(rb + (sr + 3) * (FR_DW * 4) + sx + 4, FR_DW * 4);
            got = (c & 1u) ? ((c & 2u) ? 2 : 1) : 0;
            if (!(c & 1u) && (c & 2u)) { printf("PX polarity without corner\n"); return false; }
          }
        } else {
          const int g = (sx - 4) >> 5, i = (sx - 4) & 31;
          uint32_t cm, pm;
          bp_segment32(pl.data() + (sr + 3) * BP_PITCH + g + 1, cm, pm);
          cm &= rowok ? bp_range_mask(x0 + 32 * g, 3, I.w - 3) : 0u;
          pm &= cm;
          got = ((cm >> i) & 1u) ? (((pm >> i) & 1u) ? 2 : 1) : 0;
          if (got) g_bits[i][got]++;
        }
        const bool testable = rowok && x >= 3 && x < I.w - 3;
        const int want = testable ? corner_def(I, x, y) : 0;
        if (want == 3) { printf("definition: both sides at once?\n"); return false; }
        if (got != want) {
          printf("MISMATCH %s (%d x %d) tile %d,%d x %d y %d (score row %d col %d): got %d want %d\n", what, I.w, I.h, tx, ty, x, y, sr, sx, got, want);
          return false;
        }
        g_checked++; g_dark += want == 1; g_bright += want == 2;
      }
    }
  }
  return true;
}

static void fill_noise(Img& I, std::mt19937& rng, int lo, int hi, int lo2, int hi2) {
  for (int y = 0; y < I.h; y++) for (int x = 0; x < I.stride; x++) {
    const bool second = lo2 >= 0 && (rng() & 1u);
    I.at(x, y) = (uint8_t)(second ? lo2 + rng() % (hi2 - lo2 + 1) : lo + rng() % (hi - lo + 1));
  }
}

int main() {
  std::mt19937 rng(9);
  // 1. uniform noise; levels that end inside a group, levels no wider than one group, levels without a testable pixel
  const int sizes[][2] = {{320, 160}, {97, 131}, {311, 75}, {24 + 128 + 3, 70}, {24 + 128 + 4, 70}, {24 + 32 + 3, 64}, {24 + 32 + 2, 64},
                          {56, 90}, {40, 40}, {33, 47}, {30, 64}, {20, 36}, {7, 7}, {6, 40}, {200, 6}, {24 + 64 + 20, 31 + 28 + 2}};
  for (auto& s : sizes) {
    Img I(s[0], s[1]);
    fill_noise(I, rng, 0, 255, -1, -1);
    if (!check_level(I, "noise")) return 1;
    fill_noise(I, rng, 60, 130, -1, -1);              // low contrast: fewer corners, long arcs of near-threshold differences
    if (!check_level(I, "noise 60..130")) return 1;
    // 2. centres and rings near 0 and near 255: the borrow of centre - 21 and the carry of centre + 21
    fill_noise(I, rng, 0, 41, 214, 255);
    if (!check_level(I, "ends")) return 1;
    fill_noise(I, rng, 0, 20, 235, 255);
    if (!check_level(I, "ends 0..20 / 235..255")) return 1;
  }
  // 3. crafted rings: arcs of exactly 8 and exactly 9 from every ring index (wrapping through 15 -> 0 included), ring values exactly
  // centre +- 20 (no corner) and centre +- 21 (corner), centres through the borrow and carry ranges, centres in the group columns
  // 0, 1, 2, 29, 30, 31 of every group (every dx = +-1 .. +-3 crosses a word boundary) and, with them, in the tile's edge columns
  {
    const int cols[] = {0, 1, 2, 29, 30, 31, 13, 16};
    const int centres[] = {100, 0, 5, 20, 21, 22, 41, 150, 213, 234, 235, 250, 255};
    int cfg = 0;
    for (int pass = 0; pass < 4; pass++) {
      Img I(24 + 2 * 128 + 40, 31 + 28 * 12 + 9);
      for (int y = 0; y < I.h; y++) for (int x = 0; x < I.stride; x++) I.at(x, y) = 0;
      std::vector<int> made;                          // x, y, want of every crafted ring: checked again once the level is complete
      for (int band = 0; 8 * band + 11 < I.h; band++) {
        const int y = 8 * band + 4, col = cols[(band + pass) % 8];
        for (int m = 0; EVH_FAST_OX + 32 * m + col + 4 < I.w; m++, cfg++) {
          const int x = EVH_FAST_OX + 32 * m + col;
          const int start = cfg % 16, len = 8 + (cfg / 16) % 2, side = (cfg / 32) % 2, delta = 20 + (cfg / 64) % 2;
          const int c = centres[(cfg / 128 + cfg) % 13];
          for (int dy = -3; dy <= 3; dy++) for (int dx = -3; dx <= 3; dx++) I.at(x + dx, y + dy) = (uint8_t)c;   // a flat patch
          const int v = side ? c + delta : c - delta;
          for (int i = 0; i < len; i++) {
            const int k = (start + i) & 15;
            I.at(x + FAST_RING[k][0], y + FAST_RING[k][1]) = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
          }
          const int want = (len == 9 && delta == 21 && v >= 0 && v <= 255) ? 1 + side : 0;
          made.insert(made.end(), {x, y, want});
        }
      }
      for (size_t i = 0; i < made.size(); i += 3)
        if (corner_def(I, made[i], made[i + 1]) != made[i + 2]) { printf("crafted ring is not what it is meant to be\n"); return 1; }
      if (!check_level(I, "crafted")) return 1;
    }
    if (cfg < 4 * 128) { printf("too few crafted rings: %d\n", cfg); return 1; }
  }
  // every bit of a word has carried corners of both sides
  for (int i = 0; i < 32; i++)
    if (!g_bits[i][1] || !g_bits[i][2]) { printf("bit %d never carried a corner of side %d\n", i, g_bits[i][1] ? 2 : 1); return 1; }
  printf("bit-plane host check ok: %ld pixels, %ld darker-ring and %ld brighter-ring corners\n", g_checked, g_dark, g_bright);
  return 0;
}
