// evh_plane.hip -- the products on the fixed plane and the pictures drawn from a batch's results, one translation unit.  This file
// holds the launch plumbing the families share and the extern "C" entries; every family has a header with its kernels, argument
// struct, check() -- every refusal comes before anything is enqueued -- and launch(), included inside the unnamed namespace:
//   evh_plane_sample.h      the run of pixels per thread, the canvas -> frame maps, the sampler, the blends' geometry
//   evh_plane_warp.h        evh_warp_fixed_plane, evh_warp_ray_surface
//   evh_plane_steady.h      evh_steady_frames
//   evh_plane_blend.h       evh_blend_fixed_plane, evh_blend_ray_surface
//   evh_plane_bands.h       evh_seam_labels_*, evh_blend_bands_*
//   evh_plane_align.h       evh_pair_exposure, evh_pair_residual, evh_pair_refine, evh_canvas_refine
//   evh_plane_scene.h       evh_trail_fixed_plane, evh_plate_fixed_plane, evh_rows_moving_filter
//   evh_plane_components.h  evh_mask_components
//   evh_plane_pictures.h    the kernels of evh_heatmap_render and evh_draw_matches (one form each: checks and launch in the entry)
// Every product but the last three also takes decoded 4:2:0 planes.
#include "evh_devmath.h"
#include "evh_frame_checks.h"
#include "evh_internal.h"
#include "evh_pixels.h"
#include <climits>
#include <cmath>
#include <type_traits>

namespace {

#include "evh_plane_sample.h"

// ---- what the entries share: launch plumbing ---------------------------------------------------------------------------------------
// fn(integral_constant<int, CN>, src) with the source as the kernels take it: planes, packed BGR or packed gray
template <class Fn>
void with_source(const EvhFrames& F, Fn fn) {
  if (F.yuv) fn(std::integral_constant<int, 3>{}, yuv420_src(*F.yuv));
  else if (F.channels == 3) fn(std::integral_constant<int, 3>{}, packed_src(F));
  else fn(std::integral_constant<int, 1>{}, packed_src(F));
}
// may the rows at p move as 32-bit words?  The image stride only counts where it is used: between the images of a call.
bool words_ok(const void* p, int64_t row_stride, int64_t img_stride, int64_t nimages) {
  return (((uintptr_t)p | (uintptr_t)row_stride | (nimages > 1 ? (uintptr_t)img_stride : 0)) & 3) == 0;
}
// the runs of WARP_RUN pixels of a w x h picture (the entries have checked w * h <= INT_MAX, so they fit an unsigned)
struct Runs { int per_row; unsigned n; };
Runs runs_of(int w, int h) {
  const int per_row = (w + WARP_RUN - 1) / WARP_RUN;
  return {per_row, (unsigned)per_row * (unsigned)h};
}
// an entry: its refusals, then its launch unless there is nothing to do
template <class Args>
int run(evh_ctx* c, const Args& A) {
  if (!c) return EVH_ERR_INVALID;
  if (int rc = check(c, A)) return rc;
  return A.idle() ? EVH_SUCCESS : launch(c, A);
}

#include "evh_plane_warp.h"
#include "evh_plane_steady.h"
#include "evh_plane_blend.h"
#include "evh_plane_bands.h"
#include "evh_plane_align.h"
#include "evh_plane_scene.h"
#include "evh_plane_components.h"
#include "evh_plane_pictures.h"

}  // namespace

extern "C" {

int evh_warp_fixed_plane(evh_ctx* c, const uint8_t* d_frames, int nframes, int sw, int sh, int channels, int64_t row_stride,
                         int64_t frame_stride, const double* d_M, int inverse_map, int mode, const uint8_t* d_background,
                         uint8_t* d_out, int dw, int dh, int64_t out_row_stride, int64_t out_frame_stride, int ox, int oy) {
  return run(c, WarpArgs{"evh_warp_fixed_plane", packed_frames(d_frames, channels, row_stride, frame_stride), nframes, sw, sh, d_M,
                         inverse_map, mode, d_background, d_out, dw, dh, out_row_stride, out_frame_stride, ox, oy});
}

int evh_warp_fixed_plane_yuv420(evh_ctx* c, const evh_yuv420* src, int nframes, int sw, int sh, const double* d_M,
                                int inverse_map, int mode, const uint8_t* d_background, uint8_t* d_out, int dw, int dh,
                                int64_t out_row_stride, int64_t out_frame_stride, int ox, int oy) {
  return run(c, WarpArgs{"evh_warp_fixed_plane_yuv420", yuv420_frames(src), nframes, sw, sh, d_M, inverse_map, mode, d_background,
                         d_out, dw, dh, out_row_stride, out_frame_stride, ox, oy});
}

int evh_warp_ray_surface(evh_ctx* c, const uint8_t* d_frames, int nframes, int sw, int sh, int channels, int64_t row_stride,
                         int64_t frame_stride, const double* d_A, const double* d_col, const double* d_row, int mode,
                         const uint8_t* d_background, uint8_t* d_out, int dw, int dh, int64_t out_row_stride, int64_t out_frame_stride) {
  return run(c, RayArgs{{"evh_warp_ray_surface", packed_frames(d_frames, channels, row_stride, frame_stride), nframes, sw, sh, d_A,
                         1, mode, d_background, d_out, dw, dh, out_row_stride, out_frame_stride, 0, 0}, d_col, d_row});
}

int evh_warp_ray_surface_yuv420(evh_ctx* c, const evh_yuv420* src, int nframes, int sw, int sh, const double* d_A,
                                const double* d_col, const double* d_row, int mode, const uint8_t* d_background, uint8_t* d_out,
                                int dw, int dh, int64_t out_row_stride, int64_t out_frame_stride) {
  return run(c, RayArgs{{"evh_warp_ray_surface_yuv420", yuv420_frames(src), nframes, sw, sh, d_A, 1, mode, d_background, d_out,
                         dw, dh, out_row_stride, out_frame_stride, 0, 0}, d_col, d_row});
}

int evh_steady_frames(evh_ctx* c, const uint8_t* d_frames, int nframes, int sw, int sh, int channels, int64_t row_stride,
                      int64_t frame_stride, const int32_t* d_tap_frame, const double* d_tap_M, int nout, int ntaps, int feather,
                      const uint8_t* d_background, uint8_t* d_out, int dw, int dh, int64_t out_row_stride, int64_t out_frame_stride,
                      uint8_t* d_tap_of, int64_t tap_of_row_stride, int64_t tap_of_frame_stride, uint32_t* d_counts) {
  return run(c, SteadyArgs{"evh_steady_frames", packed_frames(d_frames, channels, row_stride, frame_stride), nframes, sw, sh, d_tap_frame,
                           d_tap_M, nout, ntaps, feather, d_background, d_out, dw, dh, out_row_stride, out_frame_stride, d_tap_of,
                           tap_of_row_stride, tap_of_frame_stride, d_counts});
}

int evh_steady_frames_yuv420(evh_ctx* c, const evh_yuv420* src, int nframes, int sw, int sh, const int32_t* d_tap_frame,
                             const double* d_tap_M, int nout, int ntaps, int feather, const uint8_t* d_background, uint8_t* d_out,
                             int dw, int dh, int64_t out_row_stride, int64_t out_frame_stride, uint8_t* d_tap_of,
                             int64_t tap_of_row_stride, int64_t tap_of_frame_stride, uint32_t* d_counts) {
  return run(c, SteadyArgs{"evh_steady_frames_yuv420", yuv420_frames(src), nframes, sw, sh, d_tap_frame, d_tap_M, nout, ntaps, feather,
                           d_background, d_out, dw, dh, out_row_stride, out_frame_stride, d_tap_of, tap_of_row_stride,
                           tap_of_frame_stride, d_counts});
}

int evh_blend_fixed_plane(evh_ctx* c, const uint8_t* d_frames, int nframes, int sw, int sh, int channels, int64_t row_stride,
                          int64_t frame_stride, const double* d_M, int inverse_map, int mode, int feather, const uint16_t* d_gain,
                          uint64_t* d_acc, int acc_in, const uint8_t* d_background, uint8_t* d_out, int dw, int dh,
                          int64_t out_row_stride, int ox, int oy) {
  return run(c, BlendArgs{{"evh_blend_fixed_plane", packed_frames(d_frames, channels, row_stride, frame_stride), nframes, sw, sh, d_M,
                           inverse_map, mode, d_background, d_out, dw, dh, out_row_stride, 0, ox, oy},
                          false, nullptr, nullptr, feather, d_gain, d_acc, acc_in});
}

int evh_blend_fixed_plane_yuv420(evh_ctx* c, const evh_yuv420* src, int nframes, int sw, int sh, const double* d_M, int inverse_map,
                                 int mode, int feather, const uint16_t* d_gain, uint64_t* d_acc, int acc_in,
                                 const uint8_t* d_background, uint8_t* d_out, int dw, int dh, int64_t out_row_stride, int ox, int oy) {
  return run(c, BlendArgs{{"evh_blend_fixed_plane_yuv420", yuv420_frames(src), nframes, sw, sh, d_M, inverse_map, mode, d_background,
                           d_out, dw, dh, out_row_stride, 0, ox, oy},
                          false, nullptr, nullptr, feather, d_gain, d_acc, acc_in});
}

int evh_blend_ray_surface(evh_ctx* c, const uint8_t* d_frames, int nframes, int sw, int sh, int channels, int64_t row_stride,
                          int64_t frame_stride, const double* d_A, const double* d_col, const double* d_row, int mode, int feather,
                          const uint16_t* d_gain, uint64_t* d_acc, int acc_in, const uint8_t* d_background, uint8_t* d_out, int dw,
                          int dh, int64_t out_row_stride) {
  return run(c, BlendArgs{{"evh_blend_ray_surface", packed_frames(d_frames, channels, row_stride, frame_stride), nframes, sw, sh, d_A,
                           1, mode, d_background, d_out, dw, dh, out_row_stride, 0, 0, 0},
                          true, d_col, d_row, feather, d_gain, d_acc, acc_in});
}

int evh_blend_ray_surface_yuv420(evh_ctx* c, const evh_yuv420* src, int nframes, int sw, int sh, const double* d_A,
                                 const double* d_col, const double* d_row, int mode, int feather, const uint16_t* d_gain,
                                 uint64_t* d_acc, int acc_in, const uint8_t* d_background, uint8_t* d_out, int dw, int dh,
                                 int64_t out_row_stride) {
  return run(c, BlendArgs{{"evh_blend_ray_surface_yuv420", yuv420_frames(src), nframes, sw, sh, d_A, 1, mode, d_background, d_out, dw,
                           dh, out_row_stride, 0, 0, 0},
                          true, d_col, d_row, feather, d_gain, d_acc, acc_in});
}

int evh_seam_labels_fixed_plane(evh_ctx* c, int nframes, int sw, int sh, const double* d_M, int inverse_map, int feather, int dw, int dh,
                                int ox, int oy, int first_label, uint32_t* d_best, uint16_t* d_label, int state_in) {
  return run(c, LabelArgs{"evh_seam_labels_fixed_plane", nframes, sw, sh, d_M, inverse_map, false, nullptr, nullptr, feather, dw, dh, ox,
                          oy, first_label, d_best, d_label, state_in});
}

int evh_seam_labels_ray_surface(evh_ctx* c, int nframes, int sw, int sh, const double* d_A, const double* d_col, const double* d_row,
                                int feather, int dw, int dh, int first_label, uint32_t* d_best, uint16_t* d_label, int state_in) {
  return run(c, LabelArgs{"evh_seam_labels_ray_surface", nframes, sw, sh, d_A, 1, true, d_col, d_row, feather, dw, dh, 0, 0, first_label,
                          d_best, d_label, state_in});
}

int64_t evh_bands_state_elems(int dw, int dh, int channels, int levels) {
  if (dw < 1 || dh < 1 || (channels != 1 && channels != 3) || levels < 0 || levels > 8) return -1;
  return bands_state_elems(dw, dh, channels, levels);
}

int64_t evh_bands_frame_ws_bytes(int dw, int dh, int channels, int levels) {
  const int64_t elems = evh_bands_state_elems(dw, dh, channels, levels);
  return elems < 0 ? -1 : elems * 4;
}

int evh_blend_bands_fixed_plane(evh_ctx* c, const uint8_t* d_frames, int nframes, int sw, int sh, int channels, int64_t row_stride,
                                int64_t frame_stride, const double* d_M, int inverse_map, int levels, const uint16_t* d_label,
                                int first_label, const uint16_t* d_gain, int64_t* d_state, int state_in, void* d_ws, int64_t ws_bytes,
                                const uint8_t* d_background, uint8_t* d_out, int dw, int dh, int64_t out_row_stride, int ox, int oy) {
  return run(c, BandsArgs{{{"evh_blend_bands_fixed_plane", packed_frames(d_frames, channels, row_stride, frame_stride), nframes, sw, sh,
                            d_M, inverse_map, EVH_BLEND_SEAM, d_background, d_out, dw, dh, out_row_stride, 0, ox, oy},
                           false, nullptr, nullptr, 0, d_gain, reinterpret_cast<uint64_t*>(d_state), state_in},
                          levels, d_label, first_label, d_ws, ws_bytes});
}

int evh_blend_bands_fixed_plane_yuv420(evh_ctx* c, const evh_yuv420* src, int nframes, int sw, int sh, const double* d_M, int inverse_map,
                                       int levels, const uint16_t* d_label, int first_label, const uint16_t* d_gain, int64_t* d_state,
                                       int state_in, void* d_ws, int64_t ws_bytes, const uint8_t* d_background, uint8_t* d_out, int dw,
                                       int dh, int64_t out_row_stride, int ox, int oy) {
  return run(c, BandsArgs{{{"evh_blend_bands_fixed_plane_yuv420", yuv420_frames(src), nframes, sw, sh, d_M, inverse_map, EVH_BLEND_SEAM,
                            d_background, d_out, dw, dh, out_row_stride, 0, ox, oy},
                           false, nullptr, nullptr, 0, d_gain, reinterpret_cast<uint64_t*>(d_state), state_in},
                          levels, d_label, first_label, d_ws, ws_bytes});
}

int evh_blend_bands_ray_surface(evh_ctx* c, const uint8_t* d_frames, int nframes, int sw, int sh, int channels, int64_t row_stride,
                                int64_t frame_stride, const double* d_A, const double* d_col, const double* d_row, int levels,
                                const uint16_t* d_label, int first_label, const uint16_t* d_gain, int64_t* d_state, int state_in,
                                void* d_ws, int64_t ws_bytes, const uint8_t* d_background, uint8_t* d_out, int dw, int dh,
                                int64_t out_row_stride) {
  return run(c, BandsArgs{{{"evh_blend_bands_ray_surface", packed_frames(d_frames, channels, row_stride, frame_stride), nframes, sw, sh,
                            d_A, 1, EVH_BLEND_SEAM, d_background, d_out, dw, dh, out_row_stride, 0, 0, 0},
                           true, d_col, d_row, 0, d_gain, reinterpret_cast<uint64_t*>(d_state), state_in},
                          levels, d_label, first_label, d_ws, ws_bytes});
}

int evh_blend_bands_ray_surface_yuv420(evh_ctx* c, const evh_yuv420* src, int nframes, int sw, int sh, const double* d_A,
                                       const double* d_col, const double* d_row, int levels, const uint16_t* d_label, int first_label,
                                       const uint16_t* d_gain, int64_t* d_state, int state_in, void* d_ws, int64_t ws_bytes,
                                       const uint8_t* d_background, uint8_t* d_out, int dw, int dh, int64_t out_row_stride) {
  return run(c, BandsArgs{{{"evh_blend_bands_ray_surface_yuv420", yuv420_frames(src), nframes, sw, sh, d_A, 1, EVH_BLEND_SEAM,
                            d_background, d_out, dw, dh, out_row_stride, 0, 0, 0},
                           true, d_col, d_row, 0, d_gain, reinterpret_cast<uint64_t*>(d_state), state_in},
                          levels, d_label, first_label, d_ws, ws_bytes});
}

int evh_pair_exposure(evh_ctx* c, const uint8_t* d_frames, int nframes, int w, int h, int channels, int64_t row_stride,
                      int64_t frame_stride, const int32_t* d_pairs, int npairs, const double* d_M, int step, int lo, int hi,
                      uint64_t* d_stats) {
  return run(c, ExposureArgs{"evh_pair_exposure", packed_frames(d_frames, channels, row_stride, frame_stride), nframes, w, h, d_pairs,
                             npairs, d_M, step, lo, hi, d_stats});
}

int evh_pair_exposure_yuv420(evh_ctx* c, const evh_yuv420* src, int nframes, int w, int h, const int32_t* d_pairs, int npairs,
                             const double* d_M, int step, int lo, int hi, uint64_t* d_stats) {
  return run(c, ExposureArgs{"evh_pair_exposure_yuv420", yuv420_frames(src), nframes, w, h, d_pairs, npairs, d_M, step, lo, hi,
                             d_stats});
}

int evh_pair_residual(evh_ctx* c, const uint8_t* d_frames, int npairs, int frame_step, int w, int h, int channels,
                      int64_t row_stride, int64_t frame_stride, const double* d_M, int threshold, uint64_t* d_stats, uint8_t* d_out,
                      int kind, int64_t out_row_stride, int64_t out_frame_stride) {
  return run(c, ResidualArgs{"evh_pair_residual", packed_frames(d_frames, channels, row_stride, frame_stride), npairs, frame_step, w,
                             h, d_M, threshold, d_stats, d_out, kind, out_row_stride, out_frame_stride});
}

int evh_pair_residual_yuv420(evh_ctx* c, const evh_yuv420* src, int npairs, int frame_step, int w, int h, const double* d_M,
                             int threshold, uint64_t* d_stats, uint8_t* d_out, int kind, int64_t out_row_stride,
                             int64_t out_frame_stride) {
  return run(c, ResidualArgs{"evh_pair_residual_yuv420", yuv420_frames(src), npairs, frame_step, w, h, d_M, threshold, d_stats,
                             d_out, kind, out_row_stride, out_frame_stride});
}

int evh_pair_refine(evh_ctx* c, const uint8_t* d_frames, int npairs, int frame_step, int w, int h, int channels, int64_t row_stride,
                    int64_t frame_stride, const double* d_M_in, int iters, int clip, double* d_M_out, uint64_t* d_info,
                    double* d_normal) {
  return run(c, RefineArgs{"evh_pair_refine", packed_frames(d_frames, channels, row_stride, frame_stride), npairs, frame_step, w, h,
                           d_M_in, iters, clip, d_M_out, d_info, d_normal});
}

int evh_pair_refine_yuv420(evh_ctx* c, const evh_yuv420* src, int npairs, int frame_step, int w, int h, const double* d_M_in,
                           int iters, int clip, double* d_M_out, uint64_t* d_info, double* d_normal) {
  return run(c, RefineArgs{"evh_pair_refine_yuv420", yuv420_frames(src), npairs, frame_step, w, h, d_M_in, iters, clip, d_M_out,
                           d_info, d_normal});
}

int evh_canvas_refine(evh_ctx* c, const uint8_t* d_frames, int nframes, int w, int h, int channels, int64_t row_stride,
                      int64_t frame_stride, const uint8_t* d_canvas, int dw, int dh, int64_t canvas_row_stride, const uint8_t* d_count,
                      int64_t count_row_stride, int min_cover, const double* d_M_in, int iters, int clip, double* d_M_out,
                      uint64_t* d_info, double* d_normal) {
  return run(c, CanvasRefineArgs{"evh_canvas_refine", packed_frames(d_frames, channels, row_stride, frame_stride), nframes, w, h,
                                 d_canvas, dw, dh, canvas_row_stride, d_count, count_row_stride, min_cover, d_M_in, iters, clip,
                                 d_M_out, d_info, d_normal});
}

int evh_canvas_refine_yuv420(evh_ctx* c, const evh_yuv420* src, int nframes, int w, int h, const uint8_t* d_canvas, int dw, int dh,
                             int64_t canvas_row_stride, const uint8_t* d_count, int64_t count_row_stride, int min_cover,
                             const double* d_M_in, int iters, int clip, double* d_M_out, uint64_t* d_info, double* d_normal) {
  return run(c, CanvasRefineArgs{"evh_canvas_refine_yuv420", yuv420_frames(src), nframes, w, h, d_canvas, dw, dh, canvas_row_stride,
                                 d_count, count_row_stride, min_cover, d_M_in, iters, clip, d_M_out, d_info, d_normal});
}

int evh_trail_fixed_plane(evh_ctx* c, const uint8_t* d_frames, int nframes, int sw, int sh, int64_t row_stride,
                          int64_t frame_stride, const double* d_M, int inverse_map, const int32_t* d_rect, uint8_t* d_canvas,
                          int64_t canvas_row_stride, uint8_t* d_out, int64_t out_row_stride, int64_t out_frame_stride, int dw,
                          int dh, int ox, int oy) {
  return run(c, TrailArgs{"evh_trail_fixed_plane", packed_frames(d_frames, 3, row_stride, frame_stride), nframes, sw, sh, d_M,
                          inverse_map, d_rect, d_canvas, canvas_row_stride, d_out, out_row_stride, out_frame_stride, dw, dh, ox, oy});
}

int evh_trail_fixed_plane_yuv420(evh_ctx* c, const evh_yuv420* src, int nframes, int sw, int sh, const double* d_M,
                                 int inverse_map, const int32_t* d_rect, uint8_t* d_canvas, int64_t canvas_row_stride,
                                 uint8_t* d_out, int64_t out_row_stride, int64_t out_frame_stride, int dw, int dh, int ox, int oy) {
  return run(c, TrailArgs{"evh_trail_fixed_plane_yuv420", yuv420_frames(src), nframes, sw, sh, d_M, inverse_map, d_rect, d_canvas,
                          canvas_row_stride, d_out, out_row_stride, out_frame_stride, dw, dh, ox, oy});
}

int evh_plate_fixed_plane(evh_ctx* c, const uint8_t* d_frames, int nframes, int sw, int sh, int channels, int64_t row_stride,
                          int64_t frame_stride, const double* d_M, int inverse_map, int min_cover, const uint8_t* d_background,
                          uint8_t* d_plate, int64_t plate_row_stride, uint8_t* d_count, int64_t count_row_stride, uint8_t* d_mask,
                          int threshold, int64_t mask_row_stride, int64_t mask_frame_stride, int dw, int dh, int ox, int oy) {
  return run(c, PlateArgs{"evh_plate_fixed_plane", packed_frames(d_frames, channels, row_stride, frame_stride), nframes, sw, sh, d_M,
                          inverse_map, min_cover, d_background, d_plate, plate_row_stride, d_count, count_row_stride, d_mask,
                          threshold, mask_row_stride, mask_frame_stride, dw, dh, ox, oy});
}

int evh_plate_fixed_plane_yuv420(evh_ctx* c, const evh_yuv420* src, int nframes, int sw, int sh, const double* d_M,
                                 int inverse_map, int min_cover, const uint8_t* d_background, uint8_t* d_plate,
                                 int64_t plate_row_stride, uint8_t* d_count, int64_t count_row_stride, uint8_t* d_mask, int threshold,
                                 int64_t mask_row_stride, int64_t mask_frame_stride, int dw, int dh, int ox, int oy) {
  return run(c, PlateArgs{"evh_plate_fixed_plane_yuv420", yuv420_frames(src), nframes, sw, sh, d_M, inverse_map, min_cover,
                          d_background, d_plate, plate_row_stride, d_count, count_row_stride, d_mask, threshold, mask_row_stride,
                          mask_frame_stride, dw, dh, ox, oy});
}

size_t evh_mask_components_work_bytes(int dw, int dh, int nmasks) { return components_work_bytes(dw, dh, nmasks); }

int evh_mask_components(evh_ctx* c, const uint8_t* d_mask, int nmasks, int dw, int dh, int64_t mask_row_stride, int64_t mask_frame_stride,
                        int connectivity, int open_radius, int min_area, int32_t* d_labels, int64_t label_row_stride,
                        int64_t label_frame_stride, evh_component* d_objects, int max_objects, int32_t* d_nobjects, void* d_work,
                        size_t work_bytes) {
  return run(c, ComponentsArgs{"evh_mask_components", d_mask, nmasks, dw, dh, mask_row_stride, mask_frame_stride, connectivity,
                               open_radius, min_area, d_labels, label_row_stride, label_frame_stride, d_objects, max_objects,
                               d_nobjects, d_work, work_bytes});
}

int evh_rows_moving_filter(evh_ctx* c, const uint8_t* d_frames, int nframes, int sw, int sh, int channels, int64_t row_stride,
                           int64_t frame_stride, const double* d_M, const uint8_t* d_plate, int64_t plate_row_stride,
                           const uint8_t* d_count, int64_t count_row_stride, int dw, int dh, int ox, int oy, int min_cover,
                           int threshold, int radius, int min_hits, double row_sx, double row_sy, const float* d_rows, int row_cap,
                           const int32_t* d_counts, const int32_t* d_status1, int npairs, int frame_step, int min_keep,
                           float* d_out_rows, int32_t* d_out_counts, int32_t* d_moving, uint8_t* d_flags) {
  return run(c, MovingArgs{"evh_rows_moving_filter", packed_frames(d_frames, channels, row_stride, frame_stride), nframes, sw, sh,
                           d_M, d_plate, plate_row_stride, d_count, count_row_stride, dw, dh, ox, oy, min_cover, threshold, radius,
                           min_hits, row_sx, row_sy, d_rows, row_cap, d_counts, d_status1, npairs, frame_step, min_keep, d_out_rows,
                           d_out_counts, d_moving, d_flags});
}

int evh_rows_moving_filter_yuv420(evh_ctx* c, const evh_yuv420* src, int nframes, int sw, int sh, const double* d_M,
                                  const uint8_t* d_plate, int64_t plate_row_stride, const uint8_t* d_count,
                                  int64_t count_row_stride, int dw, int dh, int ox, int oy, int min_cover, int threshold, int radius,
                                  int min_hits, double row_sx, double row_sy, const float* d_rows, int row_cap,
                                  const int32_t* d_counts, const int32_t* d_status1, int npairs, int frame_step, int min_keep,
                                  float* d_out_rows, int32_t* d_out_counts, int32_t* d_moving, uint8_t* d_flags) {
  return run(c, MovingArgs{"evh_rows_moving_filter_yuv420", yuv420_frames(src), nframes, sw, sh, d_M, d_plate, plate_row_stride,
                           d_count, count_row_stride, dw, dh, ox, oy, min_cover, threshold, radius, min_hits, row_sx, row_sy, d_rows,
                           row_cap, d_counts, d_status1, npairs, frame_step, min_keep, d_out_rows, d_out_counts, d_moving, d_flags});
}

// ---- heat-map pictures (processing_visualization.py:336-344): one form, so the checks and the launch sit in the entry ------------
int evh_heatmap_render(evh_ctx* c, const double* d_Hsup, int n, int w, int h, const uint8_t* d_frames, int64_t row_stride,
                       int64_t frame_stride, const uint8_t* d_lut, double heatmap_constant, double alpha, int saturate,
                       uint8_t* d_out, int64_t out_row_stride, int64_t out_frame_stride) {
  if (!c) return EVH_ERR_INVALID;
  const std::string W = "evh_heatmap_render: ";
  if (!d_Hsup || !d_lut || !d_out) return evh_fail(c, EVH_ERR_INVALID, W + "NULL argument");
  if (n < 0 || w < 1 || h < 1) return evh_fail(c, EVH_ERR_INVALID, W + "empty grid or negative n");
  if (!std::isfinite(heatmap_constant) || heatmap_constant <= 0) return evh_fail(c, EVH_ERR_INVALID, W + "heatmap_constant must be finite and positive");
  if (!std::isfinite(alpha) || alpha < 0) return evh_fail(c, EVH_ERR_INVALID, W + "alpha must be finite and not negative");
  if (n > 65535) return evh_fail(c, EVH_ERR_CAPACITY, W + "at most 65535 matrices per call");
  if (int rc = need_area(c, W, "w * h", w, h)) return rc;
  const int64_t row = (int64_t)w * 3;
  if (out_row_stride < row || (d_frames && row_stride < row)) return evh_fail(c, EVH_ERR_INVALID, W + "stride smaller than a row");
  const int64_t picture = (h - 1) * out_row_stride + row, frame = d_frames ? (h - 1) * row_stride + row : 0;
  if (n > 1 && (out_frame_stride < picture || (d_frames && frame_stride < frame)))
    return evh_fail(c, EVH_ERR_INVALID, W + "stride smaller than a frame");
  if (n > 0 && meet({d_frames, frame + (n - 1) * frame_stride, ""}, {d_out, picture + (n - 1) * out_frame_stride, ""}))
    return evh_fail(c, EVH_ERR_INVALID, W + "d_frames overlaps d_out");
  if (n == 0) return EVH_SUCCESS;
  // k_heatmap_render over n frames of w x h
  const Runs R = runs_of(w, h);
  const int vec = (words_ok(d_out, out_row_stride, out_frame_stride, n) ? 1 : 0) |
                  (d_frames && words_ok(d_frames, row_stride, frame_stride, n) ? 2 : 0);
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((R.n + 255) / 256, n), dim3(256), 0, c->stream, d_Hsup, w, d_frames, row_stride, frame_stride,
                       d_lut, heatmap_constant, alpha, saturate, d_out, out_row_stride, out_frame_stride, R.per_row, R.n, vec);
  };
  if (!d_frames || alpha == 0.8) go(k_heatmap_render<false>);      // the integer blend, behind the exact test for its constant
  else go(k_heatmap_render<true>);
  return launched(c);
}

// ---- matching pictures (processing_visualization.py:22-57): one form as well ------------------------------------------------------
int evh_draw_matches(evh_ctx* c, const uint8_t* d_frames, int npairs, int frame_step, int w, int h, int64_t row_stride,
                     int64_t frame_stride, const float* d_rows, int row_cap, const int32_t* d_counts, const int32_t* d_status,
                     int points, uint32_t color_bgr, uint8_t* d_out, int64_t out_row_stride, int64_t out_frame_stride) {
  if (!c) return EVH_ERR_INVALID;
  const std::string W = "evh_draw_matches: ";
  if (!d_frames || !d_rows || !d_counts || !d_out) return evh_fail(c, EVH_ERR_INVALID, W + "NULL argument");
  if (npairs < 0 || w < 1 || h < 1 || row_cap < 1) return evh_fail(c, EVH_ERR_INVALID, W + "empty frame, no row capacity or negative npairs");
  if (frame_step != 1 && frame_step != 2) return evh_fail(c, EVH_ERR_INVALID, W + "frame_step must be 1 or 2");
  if (points != EVH_DRAW_REFERENCE && points != EVH_DRAW_OWN_FRAME) return evh_fail(c, EVH_ERR_INVALID, W + "unknown points value");
  if (color_bgr >> 24) return evh_fail(c, EVH_ERR_INVALID, W + "color_bgr has bits above 24 set");
  if (w > 16383) return evh_fail(c, EVH_ERR_CAPACITY, W + "w above 16383 (a picture's columns are held in 16 bits)");
  const int64_t row = (int64_t)w * 3;
  if (row_stride < row || out_row_stride < 2 * row) return evh_fail(c, EVH_ERR_INVALID, W + "stride smaller than a row");
  const int64_t frame = (h - 1) * row_stride + row, picture = (h - 1) * out_row_stride + 2 * row;
  if ((npairs >= 1 && frame_stride < frame) || (npairs > 1 && out_frame_stride < picture))
    return evh_fail(c, EVH_ERR_INVALID, W + "stride smaller than a frame");
  if (npairs == 0) return EVH_SUCCESS;
  const Span pictures{d_out, picture + (npairs - 1) * out_frame_stride, ""};
  if (meet({d_frames, frame + ((int64_t)(npairs - 1) * frame_step + 1) * frame_stride, ""}, pictures))
    return evh_fail(c, EVH_ERR_INVALID, W + "d_frames overlaps d_out");
  if (meet({d_rows, (int64_t)npairs * row_cap * 4 * (int64_t)sizeof(float), ""}, pictures))
    return evh_fail(c, EVH_ERR_INVALID, W + "d_rows overlaps d_out");
  // k_draw_paste, then k_draw_lines on top (w <= 16383)
  const int runs_per_half = runs_of(w, 1).per_row;
  // the frames' stride always counts: a picture takes two frames
  const bool out_words = words_ok(d_out, out_row_stride, out_frame_stride, npairs);
  const int vec = (out_words ? 1 : 0) | (words_ok(d_frames, row_stride, frame_stride, 2) ? 2 : 0) | (out_words && (w & 3) == 0 ? 4 : 0);
  const dim3 pgrid((2 * runs_per_half + 255) / 256, std::min(h, 65535), std::min(npairs, 65535));
  hipLaunchKernelGGL(k_draw_paste, pgrid, dim3(256), 0, c->stream, d_frames, npairs, frame_step, w, h, row_stride, frame_stride,
                     d_out, out_row_stride, out_frame_stride, runs_per_half, vec);
  EVH_HIP(c, hipGetLastError());
  const dim3 lgrid(std::min(64, (row_cap + 3) / 4), std::min(npairs, 65535));
  hipLaunchKernelGGL(k_draw_lines, lgrid, dim3(256), 0, c->stream, d_rows, row_cap, d_counts, d_status, npairs, points, w, h,
                     color_bgr, d_out, out_row_stride, out_frame_stride);
  return launched(c);
}

}  // extern "C"
