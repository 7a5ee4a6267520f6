// evh_detect.hip -- ORB detect + describe for gfx950 (MI355X): gray conversion, 8-level pyramid, FAST-9/16 with
// corner score + 3x3 NMS, per-level selection (FAST score, then Harris), orientation, steered BRIEF.
// Replaces cv2.ORB_create().detectAndCompute (reference: evenvizion/processing/frame_processing.py:59-61).
// Integer stages are exact; float stages use one IEEE operation at a time (-ffp-contract=off).
// One translation unit in stages, includes going one way only: evh_detect_pyr.h (gray, pyramid, XCD order), _fast.h (FAST),
// _select.h (canonical selection), _selcv.h (selection in the reference's order), _describe.h; this file: the launchers.
#include "evh_detect_selcv.h"
#include "evh_detect_describe.h"

// what FastArgs, SelectArgs and DescribeArgs begin with: the level table and the pyramid
template <class Args>
static void detect_common(const evh_ctx* c, Args& A) {
  for (int l = 0; l < EVH_NLEVELS; l++) A.lv[l] = c->g.lv[l];
  A.pyr = c->d_pyr; A.pyr_frame_bytes = c->g.pyr_frame_bytes;
}

// ------------------------------------------------------------------------------------------------------------
int evh_launch_gray_level0(evh_ctx* c, const uint8_t* d_frames, int nframes, int channels, int64_t row_stride,
                           int64_t frame_stride) {
  const EvhLevel& L = c->g.lv[0];
  const EvhLevel& D = c->g.lv[1];
  const int aligned4 = (((uintptr_t)d_frames | (uintptr_t)row_stride | (uintptr_t)frame_stride) & 3) == 0;
  // level 1 is produced by the same launch whenever its scale keeps the footprint of a tile inside the LDS tile
  c->level1_fused = (int64_t)L.w * 100 <= (int64_t)D.w * 121 && (int64_t)L.h * 100 <= (int64_t)D.h * 121 && D.w >= 2 &&
                    D.h >= 2 && row_stride < (1 << 24);
  if (c->level1_fused) {
    const int tiles_x = (D.w + PD_W - 1) / PD_W, tiles_y = (D.h + PD_H - 1) / PD_H;
    const int* t = c->d_tabs + D.tab_off;
    const auto kernel = (channels == 3 && aligned4 && (L.w & 3) == 0) ? k_gray_pyr1<true> : k_gray_pyr1<false>;
    hipLaunchKernelGGL(kernel, xcd_grid(tiles_x * tiles_y, nframes), dim3(256), 0, c->stream, d_frames, channels, row_stride,
                       frame_stride, aligned4, c->d_pyr, c->g.pyr_frame_bytes, L.stride, L.w, L.h, D.off, D.stride, D.w, D.h,
                       tiles_x, tiles_y, magic20(tiles_x), nframes, t, t + D.w, t + 2 * D.w, t + 2 * D.w + D.h);
  } else {
    int quads = ((L.w + 3) / 4) * L.h;
    dim3 grid((quads + 255) / 256, nframes);
    hipLaunchKernelGGL(k_gray_level0, grid, dim3(256), 0, c->stream, d_frames, channels, row_stride, frame_stride,
                       c->d_pyr, c->g.pyr_frame_bytes, L.w, L.h, L.stride, aligned4);
  }
  EVH_HIP(c, hipGetLastError());
  return EVH_SUCCESS;
}

int evh_launch_pyramid(evh_ctx* c, int nframes) {
  for (int l = c->level1_fused ? 2 : 1; l < EVH_NLEVELS; l++) {
    const EvhLevel& S = c->g.lv[l - 1];
    const EvhLevel& D = c->g.lv[l];
    const int* t = c->d_tabs + D.tab_off;   // xofs | xc1 | yofs | yc1 (linear_exact_tab in evh_api.hip)
    // k_pyr_walk stages <= 1.21 x its tile per axis.  ORB's levels shrink by 1.2 (level 1 of a resized frame too), but
    // the rounded sizes of a few small levels shrink by more (400 x 220: level 7, 74 -> 61 rows): those take k_pyr_down
    const bool walk = (int64_t)S.w * 100 <= (int64_t)D.w * 121 && (int64_t)S.h * 100 <= (int64_t)D.h * 121 &&
                      D.w >= 2 && D.h >= 2;
    auto launch = [&](auto kernel, int tiles_x, int tiles_y) {   // the two forms take the same arguments
      hipLaunchKernelGGL(kernel, xcd_grid(tiles_x * tiles_y, nframes), dim3(256), 0, c->stream, c->d_pyr, c->g.pyr_frame_bytes,
                         S.off, S.stride, D.off, D.stride, D.w, D.h, tiles_x, magic20(tiles_x), tiles_x * tiles_y, nframes, t,
                         t + D.w, t + 2 * D.w, t + 2 * D.w + D.h);
    };
    if (walk) launch(k_pyr_walk, (D.w + PW_W - 1) / PW_W, (D.h + PW_H - 1) / PW_H);
    else launch(k_pyr_down, (D.w + PD_W - 1) / PD_W, (D.h + PDN_H - 1) / PDN_H);
    EVH_HIP(c, hipGetLastError());
  }
  return EVH_SUCCESS;
}

int evh_launch_fast(evh_ctx* c, int nframes, int share_group) {
  EVH_HIP(c, hipMemsetAsync(c->d_cand_count, 0, sizeof(int) * EVH_NLEVELS * (size_t)nframes, c->stream));
  FastArgs A;
  detect_common(c, A);
  A.cand = c->d_cand; A.cand_frame_entries = c->g.cand_frame_entries;
  A.cand_count = c->d_cand_count;
  A.thr = c->d_fast_thr; A.shist = c->d_fast_hist; A.redo = c->d_fast_redo;
  A.share_group = share_group > 1 ? share_group : 0;
  A.hint_in = c->fast_hint ? c->d_fast_hint + 8 * c->fast_hint_idx : c->d_fast_hint + 16 + 8 * 256;   // off: all zero
  A.hint_out = c->d_fast_hint + 8 * (c->fast_hint_idx ^ 1);
  A.hint_hist = reinterpret_cast<unsigned*>(c->d_fast_hint + 16);
  c->fast_hint_idx ^= 1;
  int nsamp = 0;
  for (int l = 0; l < EVH_NLEVELS; l++) {
    const int tiles = A.lv[l].tiles_x * A.lv[l].tiles_y;
    A.samp_mod[l] = tiles >= 128 ? 27 : tiles >= 32 ? 13 : tiles >= 14 ? 7 : 0;   // 0: too small to sample, T stays 20
    A.samp_start[l] = nsamp;
    if (A.samp_mod[l]) nsamp += (tiles + A.samp_mod[l] - 1) / A.samp_mod[l];
  }
  const dim3 grid(c->g.total_tiles, nframes);
  A.lift_base = 0;
  A.tdesc = c->order_mode == EVH_ORDER_OPENCV ? c->d_cv_tdesc : nullptr;
  A.total_tiles = c->g.total_tiles;
  // ---- 1. reference order with lifting.  The reference's key-point order is a function of EVERY corner at threshold 20
  // (k_select_cv): the threshold cannot be lifted there, but the exact score is still only needed where the 4-point pre-test
  // at 20 passes.  The full 16-point segment test decides which pixels get an exact score (k_fast_main with lift_base; the
  // 4-point pre-test alone was measured and dropped here: 22.8 ms against 19.8 ms dense on the 720p texture of SURVEY 8d,
  // where it passes most quads).
  if (c->order_mode == EVH_ORDER_OPENCV && c->fast_lift) {
    A.lift_base = 1;
    hipLaunchKernelGGL(k_fast_main, grid, dim3(256), 0, c->stream, A);
    EVH_HIP(c, hipGetLastError());
    return EVH_SUCCESS;
  }
  // ---- 2. dense: evh_set_fast_lift(0) in either order (ordered bursts where A.tdesc is set), or no level large enough to sample
  if (!c->fast_lift || nsamp == 0) {
    hipLaunchKernelGGL(k_fast, grid, dim3(256), 0, c->stream, A);
    EVH_HIP(c, hipGetLastError());
    return EVH_SUCCESS;
  }
  // ---- 3. lifted canonical: sample, threshold, main, verify, hint, redo
  const int nfl = nframes * EVH_NLEVELS;
  EVH_HIP(c, hipMemsetAsync(c->d_fast_hist, 0, sizeof(unsigned) * 256 * (size_t)nfl, c->stream));
  EVH_HIP(c, hipMemsetAsync(A.hint_hist, 0, sizeof(unsigned) * 8 * 256, c->stream));
  hipLaunchKernelGGL(k_fast_sample, dim3(nsamp, nframes), dim3(256), 0, c->stream, A);
  hipLaunchKernelGGL(k_fast_thr, dim3((nfl + 255) / 256), dim3(256), 0, c->stream, A, nframes);
  hipLaunchKernelGGL(k_fast_main, grid, dim3(256), 0, c->stream, A);
  hipLaunchKernelGGL(k_fast_verify, dim3((nfl + 255) / 256), dim3(256), 0, c->stream, A, nframes);
  hipLaunchKernelGGL(k_fast_hint, dim3(1), dim3(64), 0, c->stream, A);
  hipLaunchKernelGGL(k_fast_redo, dim3(A.lv[0].tiles_x * A.lv[0].tiles_y, std::min(nfl, 256)), dim3(256), 0, c->stream, A);
  EVH_HIP(c, hipGetLastError());
  return EVH_SUCCESS;
}

int evh_launch_select(evh_ctx* c, int nframes) {
  SelectArgs A;
  detect_common(c, A);
  A.cand = c->d_cand; A.cand_frame_entries = c->g.cand_frame_entries; A.cand_count = c->d_cand_count;
  A.kp_xy = c->d_kp_xy; A.kp_meta = c->d_kp_meta; A.kp_resp = c->d_kp_resp; A.kp_count = c->d_kp_count;
  A.frame_flags = c->d_frame_flags; A.kcap = c->kcap;
  A.tmp_meta = c->d_tmp_meta; A.tmp_resp = c->d_tmp_resp; A.lvl_count = c->d_lvl_count;
  EVH_HIP(c, hipMemsetAsync(c->d_frame_flags, 0, sizeof(int) * (size_t)nframes, c->stream));
  // LDS capacities: stage 1 keeps 2*q0 + score ties in LDS up to k1cap and spills beyond it (exact either way);
  // stage 2 can hold a whole frame slot (kcap), the only hard bound left
  int q0 = 0;
  for (int l = 0; l < EVH_NLEVELS; l++) q0 = std::max(q0, A.lv[l].quota);
  A.k1cap = std::min(EVH_K1CAP, std::max(1024, (4 * q0 + 63) / 64 * 64));
  A.k2cap = c->kcap;
  const size_t lds = sizeof(uint32_t) * 2 * ((size_t)A.k1cap + A.k2cap);
  A.nframes = nframes;
  if (c->order_mode == EVH_ORDER_OPENCV) {
    SelCvArgs B;
    B.s = A;
    B.seq = c->d_cv_seq; B.seq32 = c->d_cv_seq32; B.lpos = c->d_cv_lpos; B.rpos = c->d_cv_rpos;
    B.band = c->d_cv_band; B.band_frame_entries = c->cv_band_frame_entries;
    B.nbands = 0;
    for (int l = 0; l < EVH_NLEVELS; l++) {
      B.band_start[l] = B.nbands; B.nbands += A.lv[l].tiles_y;
      if (A.lv[l].tiles_x > CVP_MAX_TX || A.lv[l].tiles_y > CVP_MAX_BANDS)
        return evh_fail(c, EVH_ERR_CAPACITY, "evh_launch_select: a level has more FAST tiles per row or per column than the row-major placement takes");
    }
    if (B.nbands + EVH_NLEVELS > c->cv_band_frame_entries) return evh_fail(c, EVH_ERR_CAPACITY, "evh_launch_select: band bases larger than the context's");
    B.heap_cap = 2 * q0 + 2;
    B.tdesc = c->d_cv_tdesc; B.total_tiles = c->g.total_tiles;
    { const char* e = getenv("EVH_CV_PHASE"); B.phase_limit = e ? atoi(e) : 0; }
    // the row-major sequence of every level: band bases (one workgroup per level), then one wave per band of FAST tiles
    hipLaunchKernelGGL(k_cv_band_base, xcd_grid(EVH_NLEVELS, nframes), dim3(256), 0, c->stream, B);
    hipLaunchKernelGGL(k_cv_place, xcd_grid(B.nbands, nframes), dim3(CVP_NT), 0, c->stream, B);
    EVH_HIP(c, hipGetLastError());
    // 256 threads on every level (1024 on the large levels was measured at 10.6 ms against 6.4 ms: a barrier over 16 waves
    // costs more than the partition steps it saves)
    const size_t heap_bytes = sizeof(unsigned long long) * (size_t)B.heap_cap;
    hipLaunchKernelGGL(k_select_cv, xcd_grid(EVH_NLEVELS, nframes), dim3(256), heap_bytes, c->stream, B);
  } else {
    if (lds > 48 * 1024)   // from ~3000 key points on (74.7 KB at 4000): opt in to more dynamic LDS than the default
      EVH_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(k_select), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds));
    hipLaunchKernelGGL(k_select, xcd_grid(EVH_NLEVELS, nframes), dim3(256), lds, c->stream, A);
  }
  EVH_HIP(c, hipGetLastError());
  hipLaunchKernelGGL(k_pack, dim3(nframes), dim3(256), 0, c->stream, A);
  EVH_HIP(c, hipGetLastError());
  return EVH_SUCCESS;
}

int evh_launch_describe(evh_ctx* c, int nframes) {
  DescribeArgs A;
  detect_common(c, A);
  A.kp_xy = c->d_kp_xy; A.kp_meta = c->d_kp_meta; A.kp_count = c->d_kp_count;
  A.kp_angle = c->d_kp_angle; A.desc = c->d_desc; A.kcap = c->kcap;
  hipLaunchKernelGGL(k_describe, dim3((c->kcap + DW_PER_BLOCK - 1) / DW_PER_BLOCK, nframes), dim3(64 * DW_PER_BLOCK), 0,
                     c->stream, A);
  EVH_HIP(c, hipGetLastError());
  return EVH_SUCCESS;
}