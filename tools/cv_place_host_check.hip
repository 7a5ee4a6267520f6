// Host check of the row-major placement arithmetic (evh_detect_selcv.h: cvp_tile_total, cvp_corners, cvp_entry,
// cvp_band_row, cvp_place) against the definition: the corners of a level, left by the FAST tiles as row-major
// bursts in any tile order, land in (y, x) order; the band bases and the level total are the plain sums.  Random levels from
// one tile to 32 x 40 tiles, bursts in random tile order, empty tiles, rows and bands, rows at the 64-corner maximum.  The
// program walks a level as k_cv_band_base and k_cv_place do: band totals and their prefix, then band by band the tables of
// the band's own descriptors and every corner of the band's bursts.  Stand-alone: built for the host (with ASan + UBSan) and
// run by tests/test_cv_place_host.py.
#include "evh_detect_selcv.h"
#include <cstdio>
#include <random>
#include <vector>
#include <algorithm>
#include <numeric>

struct Corner { int y, tx, col; uint32_t word; };

int main() {
  std::mt19937 rng(11);
  long levels = 0, corners = 0, bands_empty = 0, rows_full = 0;
  for (int it = 0; it < 120; it++) {
    const int TX = it < 8 ? 1 + it % 2 : it % 9 == 0 ? CVP_MAX_TX : 1 + (int)(rng() % CVP_MAX_TX);
    const int TY = it < 8 ? 1 + it / 4 : it % 13 == 0 ? 40 : 1 + (int)(rng() % 40);
    const int p_tile = rng() % 4, p_row = rng() % 4, p_band = rng() % 3, dens = 1 + rng() % 64;
    // the corners of every tile, row-major inside the tile
    std::vector<std::vector<Corner>> tile(TX * TY);
    std::vector<int> band_sum(TY, 0);
    for (int ty = 0; ty < TY; ty++) {
      const bool band_off = p_band == 0 && rng() % 3 == 0;
      for (int tx = 0; tx < TX; tx++) {
        if (band_off || (p_tile == 0 && rng() % 2)) continue;
        const bool only_last = p_tile == 1 && tx != TX - 1;       // a band whose corners all lie in its last tile
        if (only_last) continue;
        for (int r = 0; r < FT_H; r++) {
          if (p_row == 0 && rng() % 2) continue;
          int cnt = rng() % 16 == 0 ? 64 : (int)(rng() % (dens + 1));
          cnt = std::min(cnt, CVP_NT * CVP_TILE_CHUNKS - (int)tile[ty * TX + tx].size());   // a tile's list holds 1024 corners
          if (cnt == 64) rows_full++;
          std::vector<int> cols(FT_W);
          std::iota(cols.begin(), cols.end(), 0);
          std::shuffle(cols.begin(), cols.end(), rng);
          cols.resize(cnt);
          std::sort(cols.begin(), cols.end());
          for (int col : cols) {
            const int y = EVH_FAST_OY + ty * FT_H + r, x = (EVH_FAST_OX + tx * FT_W + col) & 0xFFF;
            tile[ty * TX + tx].push_back({y, tx, col, ((uint32_t)(20 + rng() % 236) << 24) | ((uint32_t)y << 12) | (uint32_t)x});
          }
        }
        band_sum[ty] += (int)tile[ty * TX + tx].size();
      }
      if (band_sum[ty] == 0) bands_empty++;
    }
    // the level's list: bursts in random tile order, and the descriptors
    std::vector<int> order(TX * TY);
    std::iota(order.begin(), order.end(), 0);
    std::shuffle(order.begin(), order.end(), rng);
    std::vector<uint32_t> cand, desc(8 * TX * TY, 0);
    std::vector<Corner> all;
    for (int t : order) {
      if (tile[t].empty()) continue;                              // an empty tile reserves nothing: offset 0, no corners
      desc[8 * t] = (uint32_t)cand.size();
      for (const Corner& c : tile[t]) {
        const int r = c.y - EVH_FAST_OY - (t / TX) * FT_H;
        desc[8 * t + 1 + (r >> 2)] += 1u << (8 * (r & 3));
        cand.push_back(c.word);
        all.push_back(c);
      }
    }
    const int n = (int)cand.size();
    std::sort(all.begin(), all.end(), [](const Corner& a, const Corner& b) {
      return a.y != b.y ? a.y < b.y : a.tx != b.tx ? a.tx < b.tx : a.col < b.col;
    });
    // band bases and the level total, as k_cv_band_base adds them up
    std::vector<int> base(TY);
    int run = 0;
    for (int ty = 0; ty < TY; ty++) {
      int s = 0;
      for (int tx = 0; tx < TX; tx++) s += cvp_tile_total(&desc[8 * (ty * TX + tx)]);
      if (s != band_sum[ty]) { printf("BAND TOTAL it %d band %d: %d, plain sum %d\n", it, ty, s, band_sum[ty]); return 1; }
      base[ty] = run;
      run += s;
    }
    if (run != n) { printf("LEVEL TOTAL it %d: %d, list %d\n", it, run, n); return 1; }
    // band by band, as k_cv_place
    std::vector<uint32_t> out(n, 0);
    std::vector<char> hit(n, 0);
    for (int ty = 0; ty < TY; ty++) {
      const uint32_t* D = &desc[8 * ty * TX];
      int E[FT_H * CVP_MAX_TX], tile_before[CVP_MAX_TX] = {0}, rows_before = 0;
      for (int r = 0; r < FT_H; r++) {            // the kernel's row loop: the scan over the lanes is the running sum `left`
        int left = 0;
        for (int tx = 0; tx < TX; tx++) {
          const int c = cvp_corners(D + 8 * tx, r);
          E[r * TX + tx] = cvp_entry(rows_before, left, tile_before[tx]);
          left += c;
          tile_before[tx] += c;
        }
        rows_before += left;
      }
      const int bt = rows_before;
      if (bt != band_sum[ty]) { printf("BAND it %d band %d: rows %d want %d\n", it, ty, bt, band_sum[ty]); return 1; }
      for (int tx = 0; tx < TX; tx++) {
        const int off = (int)D[8 * tx], cnt = tile_before[tx];
        if (cnt != (int)tile[ty * TX + tx].size() || cnt != cvp_tile_total(D + 8 * tx)) { printf("TILE it %d band %d tile %d: %d\n", it, ty, tx, cnt); return 1; }
        const int nch = std::min((cnt + CVP_NT - 1) / CVP_NT, CVP_TILE_CHUNKS);
        for (int q = 0; q < nch; q++) for (int lane = 0; lane < CVP_NT; lane++) {      // chunk by chunk, a lane per corner
          const int w = cvp_chunk(tx, q), j = cvp_chunk_first(w) + lane;
          if ((w & 0xFF) != tx) { printf("CHUNK it %d tile %d chunk %d\n", it, tx, q); return 1; }
          if (j >= cnt) continue;
          const int i = off + j;
          if (i < 0 || i >= n) { printf("INDEX it %d band %d tile %d j %d -> %d\n", it, ty, tx, j, i); return 1; }
          const uint32_t c = cand[i];
          const int pos = cvp_place(base[ty], E[cvp_band_row(c, ty) * TX + tx], off, i);
          if (pos < base[ty] || pos >= base[ty] + bt || hit[pos]) { printf("PLACE it %d band %d tile %d j %d -> %d\n", it, ty, tx, j, pos); return 1; }
          hit[pos] = 1;
          out[pos] = c;
        }
      }
    }
    for (int i = 0; i < n; i++)
      if (!hit[i] || out[i] != all[i].word) { printf("ORDER it %d (%d x %d tiles) place %d of %d\n", it, TX, TY, i, n); return 1; }
    levels++; corners += n;
  }
  if (bands_empty == 0 || rows_full == 0) { printf("the cases did not come up: %ld empty bands, %ld full rows\n", bands_empty, rows_full); return 1; }
  printf("cv place host check ok: %ld levels, %ld corners, %ld empty bands, %ld rows of 64\n", levels, corners, bands_empty, rows_full);
  return 0;
}
