// Host check of fast_queue_survivor (evh_detect_fast.h: pass 1 of fast_nms_queue_ordered) against the definition: a survivor is a
// corner of the tile proper, at least EVH_EDGE from the border of a level larger than 2 * EVH_EDGE, whose score is strictly greater
// than its eight neighbours'.  Random score planes with ties, shuffled queues with random polarity bits, tiles at nine origins in
// levels of random size.  Stand-alone: built for the host (with ASan + UBSan) and run by tests/test_fast_tail_pass1_host.py.
#include "evh_detect_fast.h"
#include <cstdio>
#include <random>
#include <vector>
#include <algorithm>
int main() {
  std::mt19937 rng(5);
  long checked = 0, surv = 0;
  for (int it = 0; it < 800; it++) {
    std::vector<uint8_t> plane(FS_H * FQ_PITCH, 0);
    const int dens = 1 + rng() % 4, alpha = 1 + rng() % 6;     // ties: few distinct scores
    for (auto& b : plane) if ((int)(rng() % 5) < dens) b = (uint8_t)(it % 7 == 0 ? 20 + rng() % 235 : 20 + rng() % alpha);
    // level geometry: the tile somewhere in a level so that the border rule bites on some sides
    const int tx = rng() % 3, ty = rng() % 3;
    const int x0 = 24 + 128 * tx, y0 = 31 + 28 * ty;
    int w = x0 + (int)(rng() % 200), h = y0 + (int)(rng() % 90);
    if (it % 11 == 0) { w = 40 + rng() % 30; h = 200; }         // not larger than 2 * EVH_EDGE in one direction
    const bool live = w > 2 * EVH_EDGE && h > 2 * EVH_EDGE;
    std::vector<uint32_t> q;
    for (int sr = 0; sr < FS_H; sr++) for (int sx = 0; sx < FQ_PITCH; sx++)
      if (plane[sr * FQ_PITCH + sx]) q.push_back((uint32_t)((((sr * FS_DW + sx / 4) << 2) | (sx & 3)) | ((rng() & 1u) << PQ_POL)));
    std::shuffle(q.begin(), q.end(), rng);
    uint32_t bm[NMS_BM_DW] = {0};
    if (live) for (uint32_t e : q) { int word = -1; uint32_t bit = 0; if (fast_queue_survivor(plane.data(), e, w, h, x0, y0, word, bit)) { if (word < 0 || word >= NMS_BM_DW) { printf("word %d\n", word); return 1; } bm[word] |= bit; } }
    for (int r = 0; r < FT_H; r++) for (int cx = 0; cx < FT_W; cx++) {
      const int sr = r + 1, sx = cx + 4, x = x0 + cx, y = y0 + r;
      const int s = plane[sr * FQ_PITCH + sx];
      bool want = live && s > 0 && x >= 31 && x < w - 31 && y >= 31 && y < h - 31;
      for (int dy = -1; dy <= 1 && want; dy++) for (int dx = -1; dx <= 1; dx++) if ((dx || dy) && plane[(sr + dy) * FQ_PITCH + sx + dx] >= s) want = false;
      const bool got = (bm[4 * r + (cx >> 5)] >> (cx & 31)) & 1u;
      if (got != want) { printf("MISMATCH it %d r %d cx %d got %d want %d\n", it, r, cx, got, want); return 1; }
      checked++; surv += want;
    }
  }
  printf("pass 1 host check ok: %ld pixels, %ld survivors\n", checked, surv);
  return 0;
}
