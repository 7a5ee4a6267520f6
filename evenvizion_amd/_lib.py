"""ctypes binding of libevhip.so (include/evhip.h).  Host code stays Python; every kernel is reached through this
thin C-ABI layer.  PyTorch-ROCm is used only to own device memory (tensor.data_ptr()) and for torch.distributed.

There is no CPU fallback: if the HIP library is missing or cannot be loaded this module raises.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# EVHIP_LIBRARY selects another build of the same C ABI (A/B measurements of two kernel variants on one box)
LIB_PATH = os.environ.get("EVHIP_LIBRARY") or os.path.join(_HERE, "libevhip.so")

EVH_SUCCESS = 0
PAIR_OK, PAIR_NO_DESCRIPTORS, PAIR_FEW_MATCHES, PAIR_NO_PROVISIONAL_H, PAIR_LOW_INLIER_RATIO, PAIR_NO_FINAL_H, \
    PAIR_CAPACITY = range(7)
ORDER_CANONICAL, ORDER_OPENCV = 0, 1
SOLVER_EXACT, SOLVER_FAST = 0, 1
MAX_FEATURES = 5984   # EVH_MAX_FEATURES (include/evhip.h): largest max_features a context accepts
MODE_INDEPENDENT_PAIRS, MODE_STREAM = 0, 1
WARP_EACH, WARP_HISTORY, WARP_MOSAIC = 0, 1, 2
WARP_MODES = {"each": WARP_EACH, "history": WARP_HISTORY, "mosaic": WARP_MOSAIC}
PLATE_MAX_FRAMES = 255   # EVH_PLATE_MAX_FRAMES (include/evhip.h): frames one plate_fixed_plane call takes
COMPONENTS_TILE = (32, 16)   # EVH_COMPONENTS_TILE_W, _H (include/evhip.h): the tile of mask_components' first pass
DRAW_REFERENCE, DRAW_OWN_FRAME = 0, 1
DRAW_POINTS = {"reference": DRAW_REFERENCE, "own_frame": DRAW_OWN_FRAME}
RESIDUAL_ABS, RESIDUAL_MASK = 0, 1
RESIDUAL_KINDS = {"abs": RESIDUAL_ABS, "mask": RESIDUAL_MASK}
RES_COVERED, RES_SAD, RES_SSD, RES_SAD0, RES_SSD0, RES_MOVING, RES_NSTATS = range(7)
BLEND_FEATHER, BLEND_SEAM = 0, 1
BLEND_MODES = {"feather": BLEND_FEATHER, "seam": BLEND_SEAM}
EXPO_NSTATS = 7          # EVH_EXPO_NSTATS: (pixels, sum a per channel x3, sum b per channel x3)
REFINE_REFINED, REFINE_UNCHANGED, REFINE_NOTHING_COVERED, REFINE_TOO_FEW, REFINE_DEGENERATE = range(5)
REFINE_INFO = ("status", "evals", "accepted", "covered_in", "ssd_in", "covered_out", "ssd_out", "n_in")
REFINE_NINFO, REFINE_NSUMS, REFINE_MAX_ITERS, REFINE_MAX_SIZE = 8, 45, 64, 4096
TRACK_FLAGS = ("tracked", "bad_point", "no_window", "left_frame", "flat", "high_error", "fb_failed")   # EVH_TRACK_* in order
TRACK_TRACKED, TRACK_NO_ERR = 0, 0xFFFFFFFF
JPEG_444, JPEG_420 = 0, 1   # EVH_JPEG_* (include/evhip.h)
JPEG_SUBSAMPLINGS = {"444": JPEG_444, "420": JPEG_420}
GRAPH_NSUMS, GRAPH_BAD_INDEX, GRAPH_BAD_STATUS = 154, 1, 2   # EVH_GRAPH_* (include/evhip.h)
GRAPH_INFO = ("used", "gated", "behind", "flags")

# every symbol include/evhip.h declares, with its ctypes signature
_vp, _i, _i64, _d = C.c_void_p, C.c_int, C.c_int64, C.c_double
_pi = C.POINTER(C.c_int)
SIGNATURES = {
    "evh_create": (_i, [_i, _i, _i, _i, _i, _vp, C.POINTER(_vp)]),
    "evh_destroy": (None, [_vp]),
    "evh_last_error_string": (C.c_char_p, [_vp]),
    "evh_stream": (_vp, [_vp]),
    "evh_synchronize": (_i, [_vp]),
    "evh_version": (_i, []),
    "evh_set_async_solve": (_i, [_vp, _i]),
    "evh_solve_wait": (_i, [_vp, _vp]),
    "evh_profile_enable": (_i, [_vp, _i]),
    "evh_profile_read": (_i, [_vp, _vp, _vp]),
    "evh_profile_stage_name": (C.c_char_p, [_i]),
    "evh_resize_area_u8": (_i, [_vp, _vp, _i, _i, _i, _i, _i64, _i64, _vp, _i, _i, _i64, _i64]),
    "evh_fixed_plane_field": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "evh_superposition_scan": (_i, [_vp, _vp, _i, _vp]),
    "evh_transform_points": (_i, [_vp, _vp, _i, _vp, _vp, _i, _d, _d, _i, _vp]),
    "evh_orb_detect_batch": (_i, [_vp, _vp, _i, _i, _i, _i, _i64, _i64, _i]),
    "evh_orb_detect_batch_resized": (_i, [_vp, _vp, _i, _i, _i, _i, _i64, _i64, _i, _i, _i]),
    "evh_stream_homography_batch_resized": (_i, [_vp, _vp, _i, _i, _i, _i, _i64, _i64, _i, _i, _i, _d, _i, _d, _i, _vp, _vp, _vp, _vp]),
    "evh_set_fast_lift": (_i, [_vp, _i]),
    "evh_set_solver_mode": (_i, [_vp, _i]),
    "evh_get_solver_mode": (_i, [_vp]),
    "evh_set_keypoint_order": (_i, [_vp, _i]),
    "evh_get_keypoint_order": (_i, [_vp]),
    "evh_set_fast_share": (_i, [_vp, _i]),
    "evh_set_fast_hint": (_i, [_vp, _i]),
    "evh_orb_count": (_i, [_vp, _i]),
    "evh_orb_capacity": (_i, [_vp]),
    "evh_orb_download": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "evh_orb_detect_compute": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "evh_resize_area_u8c3": (_i, [_vp, _vp, _i, _i, _vp, _i, _i]),
    "evh_orb_level_info": (_i, [_vp, _i, _pi, _pi, _pi, C.POINTER(C.c_float)]),
    "evh_orb_download_level": (_i, [_vp, _i, _i, _vp]),
    "evh_orb_download_candidates": (_i, [_vp, _i, _i, _vp, _i]),
    "evh_match_knn2_l2u8": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp]),
    "evh_match_knn2_l2u8x128": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp]),
    "evh_match_knn2_hamming": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp]),
    "evh_ratio_unique_filter": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _d, _i, _vp, _pi, _pi]),
    "evh_find_homography_ransac": (_i, [_vp, _vp, _i, _d, _i, _d, _vp, _vp, _pi, _vp]),
    "evh_find_homography_ransac_fixed": (_i, [_vp, _vp, _i, _d, _i, _d, _vp, _vp, _pi, _vp]),
    "evh_static_filter": (_i, [_vp, _vp, _vp, _i, _vp, _pi]),
    "evh_remove_double_matching": (_i, [_vp, _vp, _i, _vp, _pi]),
    "evh_pair_homography_batch": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i64, _i64, _i, _d, _i, _d, _i, _vp, _vp]),
    "evh_stream_homography_batch": (_i, [_vp, _vp, _i, _i, _i, _i, _i64, _i64, _i, _d, _i, _d, _i, _vp, _vp, _vp, _vp]),
    "evh_multi_stream_homography_batch": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i64, _i64, _i, _d, _i, _d, _i, _vp, _vp, _vp, _vp]),
    "evh_stream_static_batch": (_i, [_vp, _vp, _i, _i, _i, _i, _i64, _i64, _i, _d, _i, _d, _i, _vp, _i, _vp, _vp]),
    "evh_stream_scan": (_i, [_vp, _vp, _i, _vp, _vp, _i, _d, _i, _d, _i, _vp, _vp, _vp, _vp]),
    "evh_pair_from_slots": (_i, [_vp, _i, _i, _vp, _vp, _pi]),
    "evh_match_static_from_slots": (_i, [_vp, _i, _i, _vp, _i, _pi, _pi]),
    "evh_compute_homography": (_i, [_vp, _vp, _i, _vp, _vp, _pi]),
    # N4: SIFT + multi-type pairs
    "evh_sift_enable": (_i, [_vp, _i]),
    "evh_sift_capacity": (_i, [_vp]),
    "evh_sift_detect_batch": (_i, [_vp, _vp, _i, _i, _i, _i, _i64, _i64, _i, _i]),
    "evh_sift_count": (_i, [_vp, _i]),
    "evh_sift_download": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "evh_sift_octave_info": (_i, [_vp, _i, _pi, _pi]),
    "evh_sift_download_gauss": (_i, [_vp, _i, _i, _i, _vp]),
    "evh_surf_enable": (_i, [_vp, _i]),
    "evh_surf_capacity": (_i, [_vp]),
    "evh_surf_detect_batch": (_i, [_vp, _vp, _i, _i, _i, _i, _i64, _i64, _i, _i, _d]),
    "evh_surf_count": (_i, [_vp, _i]),
    "evh_surf_download": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "evh_surf_download_integral": (_i, [_vp, _i, _vp]),
    "evh_match_knn2_l2f32": (_i, [_vp, _vp, _i, _vp, _i, _i, _vp, _vp]),
    "evh_ratio_unique_filter_f32": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _d, _i, _vp, _pi, _pi]),
    "evh_pair_homography_batch_types": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i64, _i64, _i, _i, _i, _vp, _i, _d, _i, _d, _i, _vp, _vp]),
    "evh_stream_homography_batch_types": (_i, [_vp, _vp, _i, _i, _i, _i, _i64, _i64, _i, _i, _i, _vp, _i, _d, _i, _d, _i, _vp, _vp, _vp, _vp]),
    # decoded 4:2:0 planes as the source (the second argument points at a Yuv420)
    "evh_yuv420_to_bgr": (_i, [_vp, _vp, _i, _i, _i, _vp, _i64, _i64]),
    "evh_orb_detect_batch_yuv420": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i]),
    "evh_stream_homography_batch_yuv420": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _d, _i, _d, _i, _vp, _vp, _vp, _vp]),
    "evh_stream_homography_batch_types_yuv420": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _i, _d, _i, _d, _i, _vp, _vp, _vp, _vp]),
    # stabilised output: frames warped into the fixed plane
    "evh_warp_fixed_plane": (_i, [_vp, _vp, _i, _i, _i, _i, _i64, _i64, _vp, _i, _i, _vp, _vp, _i, _i, _i64, _i64, _i, _i]),
    "evh_warp_fixed_plane_yuv420": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _i, _vp, _vp, _i, _i, _i64, _i64, _i, _i]),
    "evh_steady_frames": (_i, [_vp, _vp, _i, _i, _i, _i, _i64, _i64, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _i, _i64, _i64, _vp, _i64,
                               _i64, _vp]),
    "evh_steady_frames_yuv420": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _i, _i64, _i64, _vp, _i64, _i64, _vp]),
    "evh_warp_ray_surface": (_i, [_vp, _vp, _i, _i, _i, _i, _i64, _i64, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i64, _i64]),
    "evh_warp_ray_surface_yuv420": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i64, _i64]),
    # the blended mosaic and the sums its exposure gains are solved from
    "evh_blend_fixed_plane": (_i, [_vp, _vp, _i, _i, _i, _i, _i64, _i64, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _i64, _i, _i]),
    "evh_blend_fixed_plane_yuv420": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _i64, _i, _i]),
    "evh_blend_ray_surface": (_i, [_vp, _vp, _i, _i, _i, _i, _i64, _i64, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _i64]),
    "evh_blend_ray_surface_yuv420": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _i64]),
    # multi-band blending under a label mask, and SEAM's labels from the geometry alone
    "evh_seam_labels_fixed_plane": (_i, [_vp, _i, _i, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _i]),
    "evh_seam_labels_ray_surface": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i]),
    "evh_bands_state_elems": (_i64, [_i, _i, _i, _i]),
    "evh_bands_frame_ws_bytes": (_i64, [_i, _i, _i, _i]),
    "evh_blend_bands_fixed_plane": (_i, [_vp, _vp, _i, _i, _i, _i, _i64, _i64, _vp, _i, _i, _vp, _i, _vp, _vp, _i, _vp, _i64, _vp, _vp, _i,
                                         _i, _i64, _i, _i]),
    "evh_blend_bands_fixed_plane_yuv420": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _i, _vp, _i, _vp, _vp, _i, _vp, _i64, _vp, _vp, _i, _i, _i64,
                                                _i, _i]),
    "evh_blend_bands_ray_surface": (_i, [_vp, _vp, _i, _i, _i, _i, _i64, _i64, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _i64, _vp, _vp,
                                         _i, _i, _i64]),
    "evh_blend_bands_ray_surface_yuv420": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _i64, _vp, _vp, _i, _i,
                                                _i64]),
    "evh_pair_exposure": (_i, [_vp, _vp, _i, _i, _i, _i, _i64, _i64, _vp, _i, _vp, _i, _i, _i, _vp]),
    "evh_pair_exposure_yuv420": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp, _i, _i, _i, _vp]),
    "evh_trail_fixed_plane": (_i, [_vp, _vp, _i, _i, _i, _i64, _i64, _vp, _i, _vp, _vp, _i64, _vp, _i64, _i64, _i, _i, _i, _i]),
    "evh_trail_fixed_plane_yuv420": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _i64, _vp, _i64, _i64, _i, _i, _i, _i]),
    "evh_plate_fixed_plane": (_i, [_vp, _vp, _i, _i, _i, _i, _i64, _i64, _vp, _i, _i, _vp, _vp, _i64, _vp, _i64, _vp, _i, _i64, _i64,
                                   _i, _i, _i, _i]),
    "evh_plate_fixed_plane_yuv420": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _i, _vp, _vp, _i64, _vp, _i64, _vp, _i, _i64, _i64,
                                          _i, _i, _i, _i]),
    # match rows judged against a plate: rows on what moves are dropped, the survivors compacted in order
    "evh_rows_moving_filter": (_i, [_vp, _vp, _i, _i, _i, _i, _i64, _i64, _vp, _vp, _i64, _vp, _i64, _i, _i, _i, _i, _i, _i, _i, _i,
                                    _d, _d, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "evh_rows_moving_filter_yuv420": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _i64, _vp, _i64, _i, _i, _i, _i, _i, _i, _i, _i,
                                           _d, _d, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    # the masks' connected components: labels, and a table of boxes, areas and centre sums
    "evh_mask_components_work_bytes": (C.c_size_t, [_i, _i, _i]),
    "evh_mask_components": (_i, [_vp, _vp, _i, _i, _i, _i64, _i64, _i, _i, _i, _vp, _i64, _i64, _vp, _i, _vp, _vp, C.c_size_t]),
    # heat-map pictures: colour index, table, blend over the frame
    "evh_heatmap_render": (_i, [_vp, _vp, _i, _i, _i, _vp, _i64, _i64, _vp, _d, _d, _i, _vp, _i64, _i64]),
    # matching pictures: the rows a batch handed to its final solve, and the two frames side by side with a line per row
    "evh_batch_static_info": (_i, [_vp, _pi, _pi]),
    "evh_batch_static_rows": (_i, [_vp, _i, _i, _vp, _i, _vp, _vp]),
    "evh_draw_matches": (_i, [_vp, _vp, _i, _i, _i, _i, _i64, _i64, _vp, _i, _vp, _vp, _i, C.c_uint32, _vp, _i64, _i64]),
    # the score of a homography: the motion-compensated residual of a pair
    "evh_pair_residual": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i64, _i64, _vp, _i, _vp, _vp, _i, _i64, _i64]),
    "evh_pair_residual_yuv420": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, _vp, _i, _i64, _i64]),
    "evh_pair_refine": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i64, _i64, _vp, _i, _i, _vp, _vp, _vp]),
    "evh_pair_refine_yuv420": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp]),
    "evh_canvas_refine": (_i, [_vp, _vp, _i, _i, _i, _i, _i64, _i64, _vp, _i, _i, _i64, _vp, _i64, _i, _vp, _i, _i, _vp, _vp, _vp]),
    "evh_canvas_refine_yuv420": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _i, _i64, _vp, _i64, _i, _vp, _i, _i, _vp, _vp, _vp]),
    # points followed between frames, and the points worth following
    "evh_track_points": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i64, _i64, _vp, _vp, _i, _vp, _i, _i, _i, _d, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "evh_track_points_yuv420": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _i, _i, _i, _d, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "evh_track_seeds": (_i, [_vp, _vp, _i, _i, _i, _i, _i64, _i64, _i, _i, _i, _d, _vp, _i, _vp]),
    "evh_track_seeds_yuv420": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _d, _vp, _i, _vp]),
    # pictures encoded on the device: baseline JPEG files (bound and header are host functions without a context)
    "evh_jpeg_bound": (_i64, [_i, _i, _i, _i]),
    "evh_jpeg_header": (_i, [_i, _i, _i, _i, _vp, _vp, _i]),
    "evh_jpeg_encode": (_i, [_vp, _vp, _i, _i, _i, _i64, _i64, _i, _i, _vp, _vp, _i64, _i64, _vp]),
    # global alignment: the normal equations over all superposed matrices, from the match rows of any frame pairs
    "evh_graph_normal": (_i, [_vp, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _d, _d, _vp, _vp]),
    # ragged batches of several streams (h_types, then h_segs: an array of StreamSeg)
    "evh_streams_homography_batch": (_i, [_vp, _vp, _i, _i, _i, _i, _i64, _i64, _i, _i, _i, _vp, _i, _vp, _i, _d, _i, _d, _i, _vp, _vp, _vp, _vp]),
    "evh_streams_homography_batch_yuv420": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _i, _vp, _i, _d, _i, _d, _i, _vp, _vp, _vp, _vp]),
}
FEATURE_ORB, FEATURE_SIFT, FEATURE_SURF = 0, 1, 2
FEATURE_CODES = {"ORB": FEATURE_ORB, "SIFT": FEATURE_SIFT, "SURF": FEATURE_SURF}


class Yuv420(C.Structure):
    """evh_yuv420 (include/evhip.h): three device plane pointers and their strides."""
    _fields_ = [("d_y", _vp), ("d_cb", _vp), ("d_cr", _vp), ("y_stride", _i64), ("c_stride", _i64),
                ("y_frame_stride", _i64), ("c_frame_stride", _i64), ("c_pixel_stride", C.c_int32)]


class StreamSeg(C.Structure):
    """evh_stream_seg (include/evhip.h): one stream's consecutive frames inside a ragged batch."""
    _fields_ = [("first_frame", C.c_int32), ("nframes", C.c_int32), ("start", C.c_int32), ("reserved", C.c_int32)]


def yuv420_size(w, h):
    """Bytes of one packed I420 frame [w*h | cw*ch | cw*ch] and its chroma size (cw, ch)."""
    cw, ch = (int(w) + 1) // 2, (int(h) + 1) // 2
    return int(w) * int(h) + 2 * cw * ch, cw, ch


def yuv420_views(packed, w, h):
    """The (Y [n,h,w], Cb [n,ch,cw], Cr [n,ch,cw]) views of packed I420 frames [n, w*h + 2*cw*ch] (tensor or array)."""
    _, cw, ch = yuv420_size(w, h)
    n = packed.shape[0]
    return (packed[:, :w * h].reshape(n, h, w), packed[:, w * h:w * h + cw * ch].reshape(n, ch, cw),
            packed[:, w * h + cw * ch:w * h + 2 * cw * ch].reshape(n, ch, cw))


class EvhError(RuntimeError):
    pass


def bands_state_elems(dw, dh, channels, levels):
    """int64 words of the band blend's state for a canvas (evh_bands_state_elems; host only, -1 for sizes the entries refuse)."""
    return int(load().evh_bands_state_elems(int(dw), int(dh), int(channels), int(levels)))


def bands_frame_ws_bytes(dw, dh, channels, levels):
    """Workspace bytes one frame's pyramids need (evh_bands_frame_ws_bytes; host only, -1 for sizes the entries refuse).  A
    call holding g frames at once needs g times this, and 8 * bands_state_elems(...) more where it is given no state."""
    return int(load().evh_bands_frame_ws_bytes(int(dw), int(dh), int(channels), int(levels)))


def component_dtype():
    """evh_component (include/evhip.h) as a structured numpy dtype: 40 bytes."""
    import numpy as np
    return np.dtype([("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("area", "<i4"), ("first", "<i4"),
                     ("sx", "<i8"), ("sy", "<i8")])


def mask_components_work_bytes(dw, dh, nmasks):
    """Bytes of scratch mask_components needs (evh_mask_components_work_bytes; host only, 0 for arguments the entry refuses):
    at most 8 * dw * dh * nmasks."""
    args = [int(dw), int(dh), int(nmasks)]
    if any(abs(a) > 0x7fffffff for a in args):
        return 0
    return int(load().evh_mask_components_work_bytes(*args))


def _jpeg_tables(qtabs):
    """Both quantisation tables as a contiguous uint16 [2, 64] array (natural order), as the jpeg entries take them."""
    q = np.ascontiguousarray(np.asarray(qtabs).reshape(2, 64).astype(np.uint16))
    if not np.array_equal(q, np.asarray(qtabs).reshape(2, 64)):
        raise ValueError("qtabs holds values a uint16 cannot")
    return q


def jpeg_bound(w, h, channels, subsampling="420"):
    """The largest file evh_jpeg_encode can write for such a picture (evh_jpeg_bound; host only, -1 for what the entry refuses)."""
    sub = JPEG_SUBSAMPLINGS[subsampling] if isinstance(subsampling, str) else int(subsampling)
    return int(load().evh_jpeg_bound(int(w), int(h), int(channels), sub))


def jpeg_header(w, h, channels, qtabs, subsampling="420"):
    """SOI .. SOS of the files evh_jpeg_encode writes, as bytes (evh_jpeg_header; host only)."""
    sub = JPEG_SUBSAMPLINGS[subsampling] if isinstance(subsampling, str) else int(subsampling)
    q, out = _jpeg_tables(qtabs), np.zeros(1024, np.uint8)
    n = load().evh_jpeg_header(int(w), int(h), int(channels), sub, _hp(q), _hp(out), out.size)
    if n < 0:
        raise EvhError("evh_jpeg_header refuses these arguments (%d)" % n)
    return out[:n].tobytes()


def build(force=False):
    """Compile libevhip.so for gfx950 with hipcc (evenvizion_amd/csrc/Makefile)."""
    if force or not os.path.exists(LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc"), "-s", "-j4"] + (["-B"] if force else []))
    return LIB_PATH


_lib = None


def load():
    """Load libevhip.so and bind every declared symbol.  Raises if the library is missing -- there is no fallback."""
    global _lib
    if _lib is None:
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 and must be loaded FIRST so that
        # libevhip.so binds to that same runtime (two runtimes in one process cannot both see the device).
        import torch  # noqa: F401
        if not os.path.exists(LIB_PATH):
            raise EvhError("libevhip.so not found at %s: build it with `make -C evenvizion_amd/csrc` "
                           "(the HIP library is the only compute backend)" % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)   # AttributeError if an include/evhip.h symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def _hp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _packed(frames, lead=1):
    """frames: contiguous uint8 tensor [*batch, h, w] (gray) or [*batch, h, w, c] with `lead` batch dimensions -> the seven
    arguments of a packed-frame entry: pointer, first batch extent, w, h, channels, row stride, frame stride."""
    h, w = frames.shape[lead:lead + 2]
    cn = 1 if frames.dim() == lead + 2 else frames.shape[lead + 2]
    return (frames.data_ptr(), frames.shape[0], w, h, cn, w * cn, w * h * cn)


def _work_size(resize_to, w, h):
    """The size ORB runs at: resize_to=(w, h), or the frames' own."""
    return (w, h) if resize_to is None else (int(resize_to[0]), int(resize_to[1]))


def _ransac(thr, max_iters, conf, force_max_iters):
    return (float(thr), int(max_iters), float(conf), int(bool(force_max_iters)))


def _tail(ransac, state_in, state_out, out_H, out_status):
    """What every stream entry ends with: the RANSAC parameters, the state in and out, the outputs."""
    return _ransac(*ransac) + (_ptr(state_in), _ptr(state_out), out_H.data_ptr(), out_status.data_ptr())


class Context:
    """One evh_ctx: one device, one HIP stream, device buffers sized at creation (reused across calls)."""

    def __init__(self, device=0, max_w=1280, max_h=720, max_features=500, max_frames=2, stream=None):
        self.lib = load()
        h = C.c_void_p()
        rc = self.lib.evh_create(int(device), int(max_w), int(max_h), int(max_features), int(max_frames),
                                 C.c_void_p(stream) if stream else None, C.byref(h))
        if rc != EVH_SUCCESS:
            raise EvhError("evh_create failed (%d): %s" % (rc, self.lib.evh_last_error_string(None).decode()))
        self.h = h
        self.device = device
        self.max_frames = max_frames
        self.max_features = max_features
        self.max_w, self.max_h = max_w, max_h

    _nothing = None          # a few device bytes for calls that take no frames (see _blend)
    _bands_ws = None         # the workspace of blend_bands_* calls that bring none (see _blend_bands)
    _components_work = None  # the scratch of mask_components calls that bring none: kept, the launches outlive the call

    def close(self):
        if getattr(self, "h", None):
            self.lib.evh_destroy(self.h)
            self.h = None
            self._bands_ws = None
            self._components_work = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _enter(self):
        """Order this context's (non-blocking) stream behind the work already queued on torch's current stream: the
        tensors a call receives may still be being filled there (torch.zeros, copies, a previous op's output)."""
        self.order_after_torch()

    def _check(self, rc):
        if rc < 0:
            raise EvhError("libevhip error %d: %s" % (rc, self.lib.evh_last_error_string(self.h).decode()))
        return rc

    @property
    def stream(self):
        return self.lib.evh_stream(self.h)

    def synchronize(self):
        self._check(self.lib.evh_synchronize(self.h))

    def set_async_solve(self, on=True):
        self._check(self.lib.evh_set_async_solve(self.h, int(bool(on))))

    def solve_wait(self, stream=None):
        """Make `stream` (a hipStream_t handle; None = the context's main stream) wait for the pending solve."""
        self._check(self.lib.evh_solve_wait(self.h, C.c_void_p(stream) if stream else None))

    def profile_enable(self, on=True):
        self._check(self.lib.evh_profile_enable(self.h, int(bool(on))))

    def profile_read(self):
        """-> {stage: (launch_groups, total_ms)} since the last read (synchronises the stream)."""
        ms = np.zeros(9, np.float32); cnt = np.zeros(9, np.int32)
        self._check(self.lib.evh_profile_read(self.h, _hp(ms), _hp(cnt)))
        return {self.lib.evh_profile_stage_name(i).decode(): (int(cnt[i]), float(ms[i])) for i in range(9)}

    # ---- K0 ----
    def resize_area(self, src, dst):
        """src/dst: CUDA uint8 tensors [n,h,w] or [n,h,w,c], contiguous."""
        self._enter()
        n, sh, sw = src.shape[:3]
        cn = 1 if src.dim() == 3 else src.shape[3]
        dh, dw = dst.shape[1:3]
        self._check(self.lib.evh_resize_area_u8(self.h, src.data_ptr(), n, sw, sh, cn, sw * cn, sw * sh * cn,
                                                dst.data_ptr(), dw, dh, dw * cn, dw * dh * cn))

    def resize_area_bgr(self, src, dst):
        """One BGR image: src CUDA uint8 [sh,sw,3] -> dst [dh,dw,3] (imutils.resize / INTER_AREA)."""
        self._enter()
        sh, sw = src.shape[:2]; dh, dw = dst.shape[:2]
        self._check(self.lib.evh_resize_area_u8c3(self.h, src.data_ptr(), sw, sh, dst.data_ptr(), dw, dh))

    def set_fast_lift(self, on=True):
        self._check(self.lib.evh_set_fast_lift(self.h, int(bool(on))))

    def set_solver_mode(self, mode):
        """SOLVER_EXACT (default): LM's 8x8 systems by the operator's Jacobi eigen-solve (H bit-identical to the oracle);
        SOLVER_FAST: by LDL^T (stream pairs ~45 % cheaper; H within ~1e-3 px of the exact mode's, see include/evhip.h)."""
        self._check(self.lib.evh_set_solver_mode(self.h, int(mode)))

    def get_solver_mode(self):
        return int(self.lib.evh_get_solver_mode(self.h))

    def set_keypoint_order(self, mode):
        """ORDER_OPENCV (default): key points leave retainBest in the order (and set) OpenCV 3.4.2 on libstdc++ leaves them --
        the reference's; ORDER_CANONICAL: all ties kept, (level, y, x) order (faster: FAST threshold lifting applies)."""
        self._check(self.lib.evh_set_keypoint_order(self.h, int(mode)))

    def get_keypoint_order(self):
        return int(self.lib.evh_get_keypoint_order(self.h))

    def set_fast_hint(self, on=True):
        self._check(self.lib.evh_set_fast_hint(self.h, int(bool(on))))

    def set_fast_share(self, on=True):
        self._check(self.lib.evh_set_fast_share(self.h, int(bool(on))))

    def fixed_plane_max(self, Hsup, w, h, field=None):
        """Hsup f64[n,3,3] -> f64[n]: max fixed-plane coordinate over the w x h grid of each matrix."""
        Hs = np.ascontiguousarray(Hsup, np.float64).reshape(-1, 9)
        out = np.zeros(len(Hs), np.float64)
        import torch
        if field is not None and not (field.is_cuda and field.dtype == torch.float64 and field.is_contiguous()
                                      and field.numel() == len(Hs) * int(h) * int(w) * 2):
            raise ValueError("fixed_plane_max: field must be a contiguous CUDA float64 tensor of n*h*w*2 elements")
        self._check(self.lib.evh_fixed_plane_field(self.h, _hp(Hs), len(Hs), int(w), int(h),
                                                   field.data_ptr() if field is not None else None, _hp(out)))
        return out

    # ---- N1 ----
    def superposition_scan(self, Hs):
        """Hs f64[n,3,3] per-frame H in frame order -> f64[n,3,3] running superposition (utils.superposition_dict)."""
        Hs = np.ascontiguousarray(Hs, np.float64).reshape(-1, 9)
        out = np.zeros_like(Hs)
        self._check(self.lib.evh_superposition_scan(self.h, _hp(Hs), len(Hs), _hp(out)))
        return out.reshape(-1, 3, 3)

    def transform_points(self, mats, idx, pts, kx=1.0, ky=1.0, decimals=-1):
        """pts f64[n,2], idx i32[n] (row of mats f64[m,3,3] per point) -> f64[n,2] transformed (and rounded) points."""
        mats = np.ascontiguousarray(mats, np.float64).reshape(-1, 9)
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 2)
        idx = np.ascontiguousarray(idx, np.int32).reshape(-1)
        out = np.zeros_like(pts)
        self._check(self.lib.evh_transform_points(self.h, _hp(mats), len(mats), _hp(idx), _hp(pts), len(pts), float(kx),
                                                  float(ky), int(decimals), _hp(out)))
        return out

    # ---- K1..K6 ----
    def orb_detect_batch(self, frames, nfeatures=500, resize_to=None):
        """frames: CUDA uint8 tensor [n,h,w] (gray) or [n,h,w,3] (BGR), contiguous.  resize_to=(w, h): the frames are
        shrunk to that working size inside the ingest kernel (imutils.resize fused into level 0)."""
        self._enter()
        p = _packed(frames)
        if resize_to is not None and tuple(resize_to) != p[2:4]:
            self._check(self.lib.evh_orb_detect_batch_resized(self.h, *p, int(resize_to[0]), int(resize_to[1]), nfeatures))
            return
        self._check(self.lib.evh_orb_detect_batch(self.h, *p, nfeatures))

    def orb_detect_compute(self, frame, nfeatures=500):
        """One frame (CUDA uint8 [h,w] or [h,w,3]) -> (xy f32[n,2], desc u8[n,32], octave i32[n]); the single-frame
        form of cv2.ORB_create().detectAndCompute (frame_processing.py:60-61)."""
        self._enter()
        h, w = frame.shape[:2]
        cn = 1 if frame.dim() == 2 else frame.shape[2]
        cap = self.lib.evh_orb_capacity(self.h)
        xy = np.zeros((cap, 2), np.float32); desc = np.zeros((cap, 32), np.uint8); oc = np.zeros(cap, np.int32)
        n = C.c_int(0)
        self._check(self.lib.evh_orb_detect_compute(self.h, frame.data_ptr(), w, h, cn, nfeatures, _hp(xy), _hp(desc),
                                                    _hp(oc), C.byref(n)))
        return xy[:n.value].copy(), desc[:n.value].copy(), oc[:n.value].copy()

    def orb_download(self, frame):
        cap = self.lib.evh_orb_capacity(self.h)
        xy = np.zeros((cap, 2), np.float32); desc = np.zeros((cap, 32), np.uint8)
        oc = np.zeros(cap, np.int32); lxy = np.zeros((cap, 2), np.int32)
        rs = np.zeros(cap, np.float32); an = np.zeros(cap, np.float32)
        n = self._check(self.lib.evh_orb_download(self.h, frame, _hp(xy), _hp(desc), _hp(oc), _hp(lxy), _hp(rs), _hp(an)))
        return dict(xy=xy[:n].copy(), desc=desc[:n].copy(), octave=oc[:n].copy(), lx=lxy[:n, 0].copy(),
                    ly=lxy[:n, 1].copy(), response=rs[:n].copy(), angle=an[:n].copy())

    def level_info(self, level):
        w = C.c_int(); h = C.c_int(); q = C.c_int(); s = C.c_float()
        self._check(self.lib.evh_orb_level_info(self.h, level, C.byref(w), C.byref(h), C.byref(q), C.byref(s)))
        return w.value, h.value, q.value, s.value

    def download_level(self, frame, level):
        w, h, _, _ = self.level_info(level)
        out = np.zeros((h, w), np.uint8)
        self._check(self.lib.evh_orb_download_level(self.h, frame, level, _hp(out)))
        return out

    def download_candidates(self, frame, level):
        w, h, _, _ = self.level_info(level)
        cap = (w // 2 + 1) * (h // 2 + 1) + 64
        buf = np.zeros(cap, np.uint32)
        n = self._check(self.lib.evh_orb_download_candidates(self.h, frame, level, _hp(buf), cap))
        p = buf[:min(n, cap)]
        return (p & 0xFFF).astype(np.int32), ((p >> 12) & 0xFFF).astype(np.int32), (p >> 24).astype(np.int32)

    # ---- K7 + glue ----
    def knn2(self, q, t, idx, d2, hamming=False):
        self._enter()
        f = self.lib.evh_match_knn2_hamming if hamming else (
            self.lib.evh_match_knn2_l2u8x128 if q.shape[1] == 128 else self.lib.evh_match_knn2_l2u8)
        self._check(f(self.h, q.data_ptr(), q.shape[0], t.data_ptr(), t.shape[0], idx.data_ptr(), d2.data_ptr()))

    def ratio_unique_filter(self, idx, d2, xy_q, xy_t, pts, ratio=0.5, min_matches=4):
        self._enter()
        n = C.c_int(); st = C.c_int()
        self._check(self.lib.evh_ratio_unique_filter(self.h, idx.data_ptr(), d2.data_ptr(), idx.shape[0], xy_t.shape[0],
                                                     xy_q.data_ptr(), xy_t.data_ptr(), float(ratio), int(min_matches),
                                                     pts.data_ptr(), C.byref(n), C.byref(st)))
        return n.value, st.value

    # ---- K8/K9 ----
    def find_homography(self, pts, thr=3.0, max_iters=2000, conf=0.995, force_max_iters=False):
        self._enter()
        n = pts.shape[0]
        H = np.zeros(9, np.float64); mask = np.zeros(max(n, 1), np.uint8); info = np.zeros(3, np.int32)
        found = C.c_int()
        f = self.lib.evh_find_homography_ransac_fixed if force_max_iters else self.lib.evh_find_homography_ransac
        self._check(f(self.h, pts.data_ptr() if n else None, n, float(thr), int(max_iters), float(conf), _hp(H),
                      _hp(mask), C.byref(found), _hp(info)))
        return (H.reshape(3, 3) if found.value else None), mask[:n].copy(), info

    def static_filter(self, H, pts, out):
        self._enter()
        H = np.ascontiguousarray(H, np.float64).reshape(9)
        n = C.c_int()
        self._check(self.lib.evh_static_filter(self.h, _hp(H), pts.data_ptr(), pts.shape[0], out.data_ptr(), C.byref(n)))
        return n.value

    def remove_double_matching(self, pts, out):
        """pts, out: CUDA float32 [n,4] rows (ax, ay, bx, by); -> rows written to out (utils.remove_double_matching)."""
        self._enter()
        n = C.c_int()
        self._check(self.lib.evh_remove_double_matching(self.h, pts.data_ptr() if pts.shape[0] else None, pts.shape[0],
                                                        out.data_ptr() if pts.shape[0] else None, C.byref(n)))
        return n.value

    # ---- fused ----
    def pair_homography_batch(self, frames, npairs, mode, out_H, out_status, nfeatures=500, thr=3.0, max_iters=2000,
                              conf=0.995, force_max_iters=False):
        self._enter()
        p = _packed(frames)
        self._check(self.lib.evh_pair_homography_batch(self.h, p[0], npairs, mode, *p[2:], nfeatures,
                                                       *_ransac(thr, max_iters, conf, force_max_iters), out_H.data_ptr(),
                                                       out_status.data_ptr()))

    def stream_homography_batch(self, frames, out_H, out_status, state_in=None, state_out=None, nfeatures=500, thr=3.0,
                                max_iters=2000, conf=0.995, force_max_iters=False, resize_to=None):
        """frames: CUDA uint8 [n,h,w(,3)], n >= 2 consecutive frames of one stream -> n-1 pairs (stream semantics).
        resize_to=(w, h): full-size frames, the reference's resize_width fused into the ingest kernel."""
        self._enter()
        p = _packed(frames)
        tail = (nfeatures,) + _tail((thr, max_iters, conf, force_max_iters), state_in, state_out, out_H, out_status)
        if resize_to is not None and tuple(resize_to) != p[2:4]:
            self._check(self.lib.evh_stream_homography_batch_resized(self.h, *p, int(resize_to[0]), int(resize_to[1]), *tail))
            return
        self._check(self.lib.evh_stream_homography_batch(self.h, *p, *tail))

    def multi_stream_homography_batch(self, frames, out_H, out_status, state_in=None, state_out=None, nfeatures=500,
                                      thr=3.0, max_iters=2000, conf=0.995, force_max_iters=False):
        """frames: CUDA uint8 [S,F,h,w(,3)] -- S independent streams of F consecutive frames each; out_H f64[S,F-1,9],
        out_status i32[S,F-1]; state_in / state_out f64[S,18] carry {H_sup, H_prev} of every stream between calls."""
        self._enter()
        p = _packed(frames, lead=2)
        self._check(self.lib.evh_multi_stream_homography_batch(
            self.h, p[0], p[1], frames.shape[1], *p[2:], nfeatures,
            *_tail((thr, max_iters, conf, force_max_iters), state_in, state_out, out_H, out_status)))

    def streams_homography_batch(self, frames, segments, out_H, out_status, features=("ORB",), state_in=None, state_out=None,
                                 nfeatures=500, thr=3.0, max_iters=2000, conf=0.995, force_max_iters=False, resize_to=None,
                                 size=None):
        """A ragged batch of several streams (evh_streams_homography_batch[_yuv420]).  frames: CUDA uint8 [n,h,w(,3)], or
        decoded planes (see _yuv420; size=(w, h) for packed I420 frames); segments: a list of (first_frame, nframes, start)
        that tiles the n frames, one stream each, start truthy = the stream begins here and its state_in row is not read.
        out_H f64[n-1,9] / out_status i32[n-1]: pair k of a segment writes row first_frame + k, the row at a segment's last
        frame is left alone.  state_in / state_out f64[len(segments),18] (may be the same tensor; state_in None only when
        every segment starts).  features: a type list as in stream_homography_batch_types, ["ORB"] = the fused ORB path."""
        self._enter()
        segs = (StreamSeg * max(len(segments), 1))(*[StreamSeg(int(a), int(b), int(bool(st)), 0) for a, b, st in segments])
        t = self._types(features)
        if list(t) != [FEATURE_ORB]:
            self._multi_used = True
        tail = (nfeatures, _hp(t), len(t), C.cast(segs, C.c_void_p), len(segments)) + \
            _tail((thr, max_iters, conf, force_max_iters), state_in, state_out, out_H, out_status)
        if isinstance(frames, (tuple, list)) or frames.dim() == 2:
            d, n, w, h = self._yuv420(frames, size, self.device)
            self._check(self.lib.evh_streams_homography_batch_yuv420(self.h, C.byref(d), n, w, h, *_work_size(resize_to, w, h), *tail))
            return
        p = _packed(frames)
        self._check(self.lib.evh_streams_homography_batch(self.h, *p, *_work_size(resize_to, *p[2:4]), *tail))

    # ---- decoded 4:2:0 planes as the source ----
    @staticmethod
    def _yuv420(planes, size, check_device=None):
        """-> (Yuv420, n, w, h).  planes: one uint8 CUDA tensor [n, w*h + 2*cw*ch] of packed I420 frames (size=(w, h)
        required), or (y [n,h,w], cb [n,ch,cw], cr [n,ch,cw]) tensors or VIEWS: rows and frames may be strided, chroma may step
        by 2 bytes per sample -- NV12 is (y, uv[..., 0], uv[..., 1]) of a [n,ch,cw,2] tensor."""
        import torch
        for t in (planes if isinstance(planes, (tuple, list)) else [planes]):
            if t.dtype != torch.uint8:
                raise ValueError("planes must be uint8 tensors")
            if check_device is not None and (not t.is_cuda or t.device.index != check_device):
                raise ValueError("planes must live on the context's device (cuda:%d)" % check_device)
        if not isinstance(planes, (tuple, list)):
            if size is None:
                raise ValueError("packed I420 frames need size=(w, h)")
            w, h = int(size[0]), int(size[1])
            if planes.dim() != 2 or planes.shape[1] != yuv420_size(w, h)[0] or planes.stride(1) != 1:
                raise ValueError("packed I420 frames are [n, w*h + 2*cw*ch] with contiguous rows")
            _, cw, ch = yuv420_size(w, h)
            d = Yuv420(planes.data_ptr(), planes.data_ptr() + w * h, planes.data_ptr() + w * h + cw * ch, w, cw,
                       planes.stride(0), planes.stride(0), 1)
            return d, planes.shape[0], w, h
        y, cb, cr = planes
        n, h, w = y.shape
        cw, ch = (w + 1) // 2, (h + 1) // 2
        if size is not None and (int(size[0]), int(size[1])) != (w, h):
            raise ValueError("size does not match the luma plane")
        if tuple(cb.shape) != (n, ch, cw) or tuple(cr.shape) != (n, ch, cw):
            raise ValueError("chroma planes must be [n, (h+1)//2, (w+1)//2]")
        # a dimension of extent 1 has no meaningful stride: give it the tight one
        ys = [y.stride(0), y.stride(1), y.stride(2) if w > 1 else 1]
        cs = [cb.stride(0), cb.stride(1), cb.stride(2) if cw > 1 else 1]
        if cw == 1 and abs(cb.data_ptr() - cr.data_ptr()) == 1:
            cs[2] = 2                                          # one interleaved chroma pair
        if ys[2] != 1 or (cw > 1 and cr.stride(2) != cs[2]) or (ch > 1 and cr.stride(1) != cs[1]) or \
                (n > 1 and cr.stride(0) != cs[0]):
            raise ValueError("luma samples must be contiguous in a row; Cb and Cr must share their strides")
        d = Yuv420(y.data_ptr(), cb.data_ptr(), cr.data_ptr(), ys[1] if h > 1 else w, cs[1] if ch > 1 else cw * cs[2],
                   ys[0], cs[0], cs[2])
        return d, n, w, h

    def yuv420_to_bgr(self, planes, out, size=None):
        """planes (see _yuv420) -> out: CUDA uint8 [n,h,w,3] (rows / frames may be strided), the BGR bytes
        cv2.VideoCapture.read() returns for the decoded picture (video_processing.py:58,70)."""
        self._enter()
        d, n, w, h = self._yuv420(planes, size, self.device)
        if str(out.dtype) != "torch.uint8" or not out.is_cuda or tuple(out.shape) != (n, h, w, 3) or out.stride(3) != 1 or (w > 1 and out.stride(2) != 3):
            raise ValueError("out must be a CUDA uint8 tensor [n,h,w,3] with packed pixels")
        self._check(self.lib.evh_yuv420_to_bgr(self.h, C.byref(d), n, w, h, out.data_ptr(), out.stride(1) if h > 1 else 3 * w,
                                               out.stride(0)))

    # ---- stabilised output ----
    def _image_rows(self, t, cn, lead, what):
        """A uint8 CUDA tensor or VIEW [*lead dims, h, w] (cn == 1) or [*lead dims, h, w, cn] with packed pixels; rows and
        leading dimensions may be strided.  -> (pointer, w, h, row stride, stride of the first dimension)"""
        import torch
        if t.dtype != torch.uint8 or not t.is_cuda or t.device.index != self.device:
            raise ValueError("%s must be a uint8 tensor on the context's device (cuda:%d)" % (what, self.device))
        if t.dim() != lead + (2 if cn == 1 else 3) or (cn != 1 and t.shape[-1] != cn):
            raise ValueError("%s must be [%sh, w%s]" % (what, "n, " * lead, "" if cn == 1 else ", %d" % cn))
        h, w = t.shape[lead:lead + 2]
        if (cn != 1 and t.stride(lead + 2) != 1) or (w > 1 and t.stride(lead + 1) != cn):
            raise ValueError("%s must have packed pixels" % what)
        return t.data_ptr(), int(w), int(h), (t.stride(lead) if h > 1 else w * cn), t.stride(0)

    def _frame_source(self, frames, size, bgr_only=False, planes=None):
        """The frames of an entry that has a packed and a _yuv420 form: a uint8 CUDA tensor [n,h,w] (gray) or [n,h,w,3] (BGR;
        bgr_only: nothing else), or decoded planes (see _yuv420; planes=None: a tuple or a 2-D tensor is taken for planes).
        -> (planes?, head, n, w, h, cn); head is what follows the context in the call: (description, n, w, h) for planes,
        (pointer, n, w, h, cn, row stride, frame stride) for packed frames, without cn where bgr_only."""
        if planes is None:
            planes = isinstance(frames, (tuple, list)) or frames.dim() == 2
        if planes:
            d, n, w, h = self._yuv420(frames, size, self.device)
            return True, (C.byref(d), n, w, h), n, w, h, 3
        cn = 3 if bgr_only else 1 if frames.dim() == 3 else int(frames.shape[-1])
        fp, w, h, frs, ffs = self._image_rows(frames, cn, 1, "frames")
        n = frames.shape[0]
        return False, (fp, n, w, h) + (() if bgr_only else (cn,)) + (frs, ffs), n, w, h, cn

    def _dev_tensor(self, t, dtype, size, message, *args):
        """ValueError(message % args) unless t is a contiguous CUDA tensor of `dtype` on the context's device with `size`
        elements (an int) or of that shape (a tuple).  The message is only put together when it is needed."""
        if t.dtype != dtype or not t.is_cuda or t.device.index != self.device or not t.is_contiguous() or \
                (t.numel() != size if isinstance(size, int) else tuple(t.shape) != tuple(size)):
            raise ValueError(message % args if args else message)

    def _form(self, name, planes):
        """The entry `name`, or its _yuv420 form for planes."""
        return getattr(self.lib, name + "_yuv420" if planes else name)

    def warp_fixed_plane(self, frames, mats, out, mode, origin, background=None, inverse_map=False, size=None):
        """Frames warped into the fixed plane (evh_warp_fixed_plane[_yuv420], the arithmetic is stated in include/evhip.h).
        frames: CUDA uint8 [n,h,w] (gray) or [n,h,w,3] (BGR), rows and frames may be strided, or decoded planes (see _yuv420;
        size=(w, h) for packed I420 frames; the canvas is then BGR).  mats: CUDA float64, n*9 contiguous elements, frame pixel
        -> plane point (inverse_map=True: plane point -> frame pixel).  mode: "each" / "history" -> out [n,dh,dw(,3)],
        "mosaic" -> out [dh,dw(,3)]; rows (and canvases) may be strided.  origin=(ox, oy): canvas pixel (x, y) is the plane
        point (x + ox, y + oy).  background: [dh,dw(,3)] with out's row stride, or None = zeros; for "mosaic" it may be `out`
        itself (a canvas carried from chunk to chunk).  Does not synchronise."""
        import torch
        self._enter()
        mode = WARP_MODES[mode] if isinstance(mode, str) else int(mode)
        planes, head, n, sw, sh, cn = self._frame_source(frames, size)
        self._dev_tensor(mats, torch.float64, 9 * n, "mats must be a contiguous CUDA float64 tensor of n*9 elements")
        lead = 0 if mode == WARP_MOSAIC else 1
        op, dw, dh, ors, ofs = self._image_rows(out, cn, lead, "out")
        if lead and out.shape[0] != n:
            raise ValueError("out must hold one canvas per frame")
        bp = None
        if background is not None:
            bp, bw, bh, brs, _ = self._image_rows(background, cn, 0, "background")
            if (bw, bh) != (dw, dh) or (dh > 1 and brs != ors):
                raise ValueError("background must be [dh,dw(,3)] with out's row stride")
        tail = (mats.data_ptr(), int(bool(inverse_map)), mode, bp, op, dw, dh, ors, ofs if lead else 0, int(origin[0]), int(origin[1]))
        self._check(self._form("evh_warp_fixed_plane", planes)(self.h, *head, *tail))

    def steady_frames(self, frames, tap_frame, tap_M, out, feather=0, background=None, tap_of=None, counts=None, size=None):
        """The steady view (evh_steady_frames[_yuv420], the arithmetic is stated in include/evhip.h): output picture j from its own
        ordered list of sources.  frames, size: as for warp_fixed_plane.  tap_frame: CUDA int32 [nout,ntaps] contiguous, an index
        into frames per tap, anything outside 0..n-1 = no tap.  tap_M: CUDA float64, nout*ntaps*9 contiguous elements, output
        pixel -> frame pixel.  out: [nout,dh,dw(,3)], rows and pictures may be strided.  feather: in 1/32 pixels.  background:
        [dh,dw(,3)] with out's row stride, or None = zeros.  tap_of: CUDA uint8 [nout,dh,dw] (may be strided) or None; counts: CUDA
        int32 or uint32 [nout,ntaps+1] contiguous, or None.  Does not synchronise."""
        import torch
        self._enter()
        planes, head, n, sw, sh, cn = self._frame_source(frames, size)
        if tap_frame.dim() != 2:
            raise ValueError("tap_frame must be [nout,ntaps]")
        nout, ntaps = (int(v) for v in tap_frame.shape)
        self._dev_tensor(tap_frame, torch.int32, (nout, ntaps), "tap_frame must be a contiguous CUDA int32 tensor [nout,ntaps]")
        self._dev_tensor(tap_M, torch.float64, 9 * nout * ntaps, "tap_M must be a contiguous CUDA float64 tensor of nout*ntaps*9 elements")
        op, dw, dh, ors, ofs = self._image_rows(out, cn, 1, "out")
        if out.shape[0] != nout:
            raise ValueError("out must hold one picture per row of tap_frame")
        bp = None
        if background is not None:
            bp, bw, bh, brs, _ = self._image_rows(background, cn, 0, "background")
            if (bw, bh) != (dw, dh) or (dh > 1 and brs != ors):
                raise ValueError("background must be [dh,dw(,3)] with out's row stride")
        tp, trs, tfs = None, 0, 0
        if tap_of is not None:
            tp, tw, th, trs, tfs = self._image_rows(tap_of, 1, 1, "tap_of")
            if (tap_of.shape[0], tw, th) != (nout, dw, dh):
                raise ValueError("tap_of must be [nout,dh,dw]")
        if counts is not None:
            if counts.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
                raise ValueError("counts must be an int32 or uint32 tensor")
            self._dev_tensor(counts, counts.dtype, (nout, ntaps + 1), "counts must be a contiguous CUDA tensor [nout,ntaps+1]")
        tail = (tap_frame.data_ptr(), tap_M.data_ptr(), nout, ntaps, int(feather), bp, op, dw, dh, ors, ofs, tp, trs, tfs,
                None if counts is None else counts.data_ptr())
        self._check(self._form("evh_steady_frames", planes)(self.h, *head, *tail))

    def warp_ray_surface(self, frames, mats, cols, rows, out, mode, background=None, size=None):
        """Frames warped onto a canvas of viewing rays (evh_warp_ray_surface[_yuv420], the arithmetic is stated in
        include/evhip.h).  frames, out, mode, background, size: as for warp_fixed_plane.  mats: CUDA float64, n*9 contiguous
        elements, ray -> homogeneous frame pixel, used as they are.  cols: CUDA float64 [dw,2], (a, c) per canvas column; rows:
        CUDA float64 [dh], b per canvas row (surface.surface_tables builds them for a cylinder, a sphere or a plane).  Does
        not synchronise."""
        import torch
        self._enter()
        mode = WARP_MODES[mode] if isinstance(mode, str) else int(mode)
        planes, head, n, sw, sh, cn = self._frame_source(frames, size)
        self._dev_tensor(mats, torch.float64, 9 * n, "mats must be a contiguous CUDA float64 tensor of n*9 elements")
        lead = 0 if mode == WARP_MOSAIC else 1
        op, dw, dh, ors, ofs = self._image_rows(out, cn, lead, "out")
        if lead and out.shape[0] != n:
            raise ValueError("out must hold one canvas per frame")
        self._dev_tensor(cols, torch.float64, (dw, 2), "cols must be a contiguous CUDA float64 tensor [dw,2]")
        self._dev_tensor(rows, torch.float64, (dh,), "rows must be a contiguous CUDA float64 tensor [dh]")
        bp = None
        if background is not None:
            bp, bw, bh, brs, _ = self._image_rows(background, cn, 0, "background")
            if (bw, bh) != (dw, dh) or (dh > 1 and brs != ors):
                raise ValueError("background must be [dh,dw(,3)] with out's row stride")
        tail = (mats.data_ptr(), cols.data_ptr(), rows.data_ptr(), mode, bp, op, dw, dh, ors, ofs if lead else 0)
        self._check(self._form("evh_warp_ray_surface", planes)(self.h, *head, *tail))

    # ---- the blended mosaic ----
    def _blend_canvas(self, out, shape, cn, background):
        """The canvas of a blend entry -> (out pointer or None, its row stride, dw, dh, background pointer or None): from out
        [dh,dw(,3)], or from shape=(dh, dw) where out is None; the background counts only beside a picture."""
        op, ors = None, 0
        if out is not None:
            op, dw, dh, ors, _ = self._image_rows(out, cn, 0, "out")
            if shape is not None and (int(shape[0]), int(shape[1])) != (dh, dw):
                raise ValueError("shape does not match out")
        elif shape is None:
            raise ValueError("without out the canvas needs shape=(dh, dw)")
        else:
            dh, dw = int(shape[0]), int(shape[1])
        bp = None
        if background is not None and out is not None:
            bp, bw, bh, brs, _ = self._image_rows(background, cn, 0, "background")
            if (bw, bh) != (dw, dh) or (dh > 1 and brs != ors):
                raise ValueError("background must be [dh,dw(,3)] with out's row stride")
        return op, ors, dw, dh, bp

    def _blend_frames(self, planes, head, n, sw, sh, cn, mats, gains):
        """The matrices and gains of a blend entry checked -> (planes?, head, matrix pointer, gain pointer), with stand-ins
        for a call without frames."""
        import torch
        self._dev_tensor(mats, torch.float64, 9 * n, "mats must be a contiguous CUDA float64 tensor of n*9 elements")
        if gains is not None:
            self._dev_tensor(gains, torch.uint16, (n, 3), "gains must be a contiguous CUDA uint16 tensor [n,3]")
        if n:
            return planes, head, mats.data_ptr(), _ptr(gains)
        # empty tensors have no address to hand over, and the entry reads neither frames nor matrices: packed frames at a few
        # bytes of the context's own
        if self._nothing is None:
            self._nothing = torch.zeros(16, dtype=torch.uint8, device="cuda:%d" % self.device)
        return False, (self._nothing.data_ptr(), 0, sw, sh, cn, sw * cn, sw * sh * cn), self._nothing.data_ptr(), None

    def _blend(self, name, frames, mats, middle, last, shape, mode, feather, gains, acc, acc_in, out, background, size):
        """What blend_fixed_plane and blend_ray_surface share.  middle: the arguments between the matrices and `mode`, last:
        those behind out_row_stride; shape=(dh, dw) or None = out's."""
        import torch
        self._enter()
        mode = BLEND_MODES[mode] if isinstance(mode, str) else int(mode)
        planes, head, n, sw, sh, cn = self._frame_source(frames, size)
        if out is None and acc is None:
            raise ValueError("one of out and acc must be given")
        op, ors, dw, dh, bp = self._blend_canvas(out, shape, cn, background)
        if acc is not None:
            self._dev_tensor(acc, torch.int64, (dh, dw, cn + 1), "acc must be a contiguous CUDA int64 tensor [dh,dw,%d]", cn + 1)
        elif acc_in:
            raise ValueError("acc_in needs acc")
        planes, head, mp, gp = self._blend_frames(planes, head, n, sw, sh, cn, mats, gains)
        tail = (mode, int(feather), gp, _ptr(acc), int(bool(acc_in)), bp, op, dw, dh, ors)
        self._check(self._form(name, planes)(self.h, *head, mp, *middle, *tail, *last))

    def blend_fixed_plane(self, frames, mats, origin, out=None, mode="feather", feather=1024, gains=None, acc=None, acc_in=False,
                          background=None, inverse_map=False, shape=None, size=None):
        """The blended mosaic on the fixed plane (evh_blend_fixed_plane[_yuv420], the arithmetic is stated in include/evhip.h).
        frames, mats, origin, background, inverse_map, size: as for warp_fixed_plane in mode "mosaic"; out: [dh,dw(,3)] or None
        (the call then only advances the state; shape=(dh, dw) says how large the canvas is).  mode "feather" or "seam";
        feather: the feather width in 1/32 pixels, 0..65535; gains: CUDA uint16 [n,3], Q12, or None = 1.0; acc: CUDA int64
        [dh,dw,channels+1] contiguous, the state (the library's u64 values viewed as int64), read when acc_in, written
        always, or None.  Does not synchronise."""
        self._blend("evh_blend_fixed_plane", frames, mats, (int(bool(inverse_map)),), (int(origin[0]), int(origin[1])), shape, mode,
                    feather, gains, acc, acc_in, out, background, size)

    def blend_ray_surface(self, frames, mats, cols, rows, out=None, mode="feather", feather=1024, gains=None, acc=None,
                          acc_in=False, background=None, size=None):
        """The blended mosaic on a canvas of viewing rays (evh_blend_ray_surface[_yuv420]).  frames, mats, cols, rows, size: as
        for warp_ray_surface (the canvas is [len(rows), len(cols)]); everything else as for blend_fixed_plane."""
        import torch
        if cols.dim() != 2 or rows.dim() != 1:
            raise ValueError("cols must be [dw,2] and rows [dh]")
        dw, dh = int(cols.shape[0]), int(rows.shape[0])
        self._dev_tensor(cols, torch.float64, (dw, 2), "cols must be a contiguous CUDA float64 tensor [dw,2]")
        self._dev_tensor(rows, torch.float64, (dh,), "rows must be a contiguous CUDA float64 tensor [dh]")
        self._blend("evh_blend_ray_surface", frames, mats, (cols.data_ptr(), rows.data_ptr()), (), (dh, dw), mode, feather, gains,
                    acc, acc_in, out, background, size)

    # ---- multi-band blending ----
    def _seam_labels(self, name, mats, middle, last, shape, feather, first_label, best, label, state_in, frame_size):
        import torch
        self._enter()
        dh, dw = int(shape[0]), int(shape[1])
        n = int(mats.numel()) // 9
        self._dev_tensor(mats, torch.float64, 9 * n, "mats must be a contiguous CUDA float64 tensor of n*9 elements")
        dev = "cuda:%d" % self.device
        if state_in and (best is None or label is None):
            raise ValueError("state_in needs best and label")
        if best is None:                      # written whole by the entry
            best = torch.empty((dh, dw), dtype=torch.int32, device=dev)
        if label is None:
            label = torch.empty((dh, dw), dtype=torch.uint16, device=dev)
        self._dev_tensor(best, torch.int32, (dh, dw), "best must be a contiguous CUDA int32 tensor [dh,dw]")
        self._dev_tensor(label, torch.uint16, (dh, dw), "label must be a contiguous CUDA uint16 tensor [dh,dw]")
        mp = mats.data_ptr()
        if n == 0:
            if self._nothing is None:
                self._nothing = torch.zeros(16, dtype=torch.uint8, device=dev)
            mp = self._nothing.data_ptr()
        self._check(getattr(self.lib, name)(self.h, n, int(frame_size[0]), int(frame_size[1]), mp, *middle, int(feather), dw, dh, *last,
                                            int(first_label), best.data_ptr(), label.data_ptr(), int(bool(state_in))))
        return best, label

    def seam_labels_fixed_plane(self, mats, frame_size, origin, shape, feather=1024, first_label=0, best=None, label=None,
                                state_in=False, inverse_map=False):
        """SEAM's partition of the canvas from the matrices alone (evh_seam_labels_fixed_plane, stated in include/evhip.h): no
        frame is read.  mats: CUDA float64, n*9 contiguous; frame_size=(sw, sh); shape=(dh, dw); frame k carries label
        first_label + k, 65535 is "nobody".  best: CUDA int32 [dh,dw] (the library's u32), label: CUDA uint16 [dh,dw], read when
        state_in, written always, or None = new tensors.  -> (best, label).  Does not synchronise."""
        return self._seam_labels("evh_seam_labels_fixed_plane", mats, (int(bool(inverse_map)),), (int(origin[0]), int(origin[1])),
                                 shape, feather, first_label, best, label, state_in, frame_size)

    def seam_labels_ray_surface(self, mats, frame_size, cols, rows, feather=1024, first_label=0, best=None, label=None,
                                state_in=False):
        """evh_seam_labels_ray_surface: as seam_labels_fixed_plane on a canvas of viewing rays, [len(rows), len(cols)]."""
        import torch
        if cols.dim() != 2 or rows.dim() != 1:
            raise ValueError("cols must be [dw,2] and rows [dh]")
        dw, dh = int(cols.shape[0]), int(rows.shape[0])
        self._dev_tensor(cols, torch.float64, (dw, 2), "cols must be a contiguous CUDA float64 tensor [dw,2]")
        self._dev_tensor(rows, torch.float64, (dh,), "rows must be a contiguous CUDA float64 tensor [dh]")
        return self._seam_labels("evh_seam_labels_ray_surface", mats, (cols.data_ptr(), rows.data_ptr()), (), (dh, dw), feather,
                                 first_label, best, label, state_in, frame_size)

    def _blend_bands(self, name, frames, mats, middle, last, shape, levels, label, first_label, gains, state, state_in, ws, out,
                     background, size):
        """What blend_bands_fixed_plane and blend_bands_ray_surface share; middle, last, shape: as for _blend."""
        import torch
        self._enter()
        planes, head, n, sw, sh, cn = self._frame_source(frames, size)
        if out is None and state is None:
            raise ValueError("one of out and state must be given")
        op, ors, dw, dh, bp = self._blend_canvas(out, shape, cn, background)
        levels = int(levels)
        elems = bands_state_elems(dw, dh, cn, levels)
        if elems < 0:
            raise ValueError("levels must lie in 0..8")
        if state is not None:
            self._dev_tensor(state, torch.int64, elems, "state must be a contiguous CUDA int64 tensor of %d elements", elems)
        elif state_in:
            raise ValueError("state_in needs state")
        self._dev_tensor(label, torch.uint16, (dh, dw), "label must be a contiguous CUDA uint16 tensor [dh,dw]")
        if ws is None:
            # The context's own workspace, kept from call to call: the launches below are only enqueued, so a tensor dropped on
            # return could be handed out again by torch while they run.  As many frames as the call has, at most 256 MiB, at
            # least one.  Before a larger one replaces it, torch is ordered behind what still uses the old one.
            unit, held = 4 * elems, 0 if state is not None else 8 * elems
            need = held + unit * max(1, min(max(n, 1), (256 << 20) // unit))
            if self._bands_ws is None or self._bands_ws.numel() < need:
                if self._bands_ws is not None:
                    self.order_torch_after()
                self._bands_ws = torch.empty(need, dtype=torch.uint8, device="cuda:%d" % self.device)
            ws = self._bands_ws
        if ws.dtype != torch.uint8 or not ws.is_cuda or not ws.is_contiguous() or ws.dim() != 1:
            raise ValueError("ws must be a contiguous one-dimensional CUDA uint8 tensor")
        planes, head, mp, gp = self._blend_frames(planes, head, n, sw, sh, cn, mats, gains)
        tail = (levels, label.data_ptr(), int(first_label), gp, _ptr(state), int(bool(state_in)), ws.data_ptr(),
                int(ws.numel()), bp, op, dw, dh, ors)
        self._check(self._form(name, planes)(self.h, *head, mp, *middle, *tail, *last))

    def blend_bands_fixed_plane(self, frames, mats, origin, label, levels=5, out=None, first_label=0, gains=None, state=None,
                                state_in=False, ws=None, background=None, inverse_map=False, shape=None, size=None):
        """The multi-band blend on the fixed plane (evh_blend_bands_fixed_plane[_yuv420], stated in include/evhip.h).  frames,
        mats, origin, out, gains, background, inverse_map, shape, size: as for blend_fixed_plane.  label: CUDA uint16 [dh,dw],
        which frame owns a pixel (seam_labels_fixed_plane), frame k of the call being first_label + k.  state: CUDA int64,
        bands_state_elems(dw, dh, channels, levels) contiguous elements, read when state_in, written always, or None.  ws: CUDA
        uint8 workspace (bands_frame_ws_bytes per frame held at once, plus 8 bytes per state element where state is None), or
        None = one the context keeps and grows as needed.  Does not synchronise."""
        self._blend_bands("evh_blend_bands_fixed_plane", frames, mats, (int(bool(inverse_map)),), (int(origin[0]), int(origin[1])),
                          shape, levels, label, first_label, gains, state, state_in, ws, out, background, size)

    def blend_bands_ray_surface(self, frames, mats, cols, rows, label, levels=5, out=None, first_label=0, gains=None, state=None,
                                state_in=False, ws=None, background=None, size=None):
        """The multi-band blend on a canvas of viewing rays (evh_blend_bands_ray_surface[_yuv420]): cols, rows as for
        blend_ray_surface, everything else as for blend_bands_fixed_plane."""
        import torch
        if cols.dim() != 2 or rows.dim() != 1:
            raise ValueError("cols must be [dw,2] and rows [dh]")
        dw, dh = int(cols.shape[0]), int(rows.shape[0])
        self._dev_tensor(cols, torch.float64, (dw, 2), "cols must be a contiguous CUDA float64 tensor [dw,2]")
        self._dev_tensor(rows, torch.float64, (dh,), "rows must be a contiguous CUDA float64 tensor [dh]")
        self._blend_bands("evh_blend_bands_ray_surface", frames, mats, (cols.data_ptr(), rows.data_ptr()), (), (dh, dw), levels, label,
                          first_label, gains, state, state_in, ws, out, background, size)

    # ---- the sums behind exposure gains ----
    def pair_exposure(self, frames, pairs, mats, step=2, lo=8, hi=247, stats=None, size=None):
        """The overlap sums of pairs of frames (evh_pair_exposure[_yuv420], stated in include/evhip.h).  frames: as for
        warp_fixed_plane.  pairs: CUDA int32 [npairs,2] contiguous, (i, j) per pair; an index outside the frames gives seven
        zeros.  mats: CUDA float64, npairs*9 contiguous, pixel of frame i -> pixel of frame j.  stats: CUDA int64 [npairs,7]
        contiguous or None = a new tensor; it is returned: (pixels, sum a per channel, sum b per channel).  Does not
        synchronise."""
        import torch
        self._enter()
        planes, head, n, w, h, cn = self._frame_source(frames, size)
        if pairs.dim() != 2:
            raise ValueError("pairs must be a contiguous CUDA int32 tensor [npairs,2]")
        npairs = int(pairs.shape[0])
        self._dev_tensor(pairs, torch.int32, (npairs, 2), "pairs must be a contiguous CUDA int32 tensor [npairs,2]")
        self._dev_tensor(mats, torch.float64, 9 * npairs, "mats must be a contiguous CUDA float64 tensor of npairs*9 elements")
        if stats is None:
            stats = torch.empty((npairs, EXPO_NSTATS), dtype=torch.int64, device="cuda:%d" % self.device)
        self._dev_tensor(stats, torch.int64, (npairs, EXPO_NSTATS), "stats must be a contiguous CUDA int64 tensor [npairs,%d]", EXPO_NSTATS)
        if npairs == 0:                      # empty tensors have no address to hand over
            return stats
        if n == 0:
            raise ValueError("pairs need frames")
        self._check(self._form("evh_pair_exposure", planes)(self.h, *head, pairs.data_ptr(), npairs, mats.data_ptr(), int(step),
                                                            int(lo), int(hi), stats.data_ptr()))
        return stats

    def trail_fixed_plane(self, frames, mats, canvas, origin, out=None, rects=None, inverse_map=False, size=None):
        """The trail of the stabilised view (evh_trail_fixed_plane[_yuv420], the arithmetic is stated in include/evhip.h): per
        frame the canvas takes the frame, the picture of it goes to out[k] with the white outline of rects[k], and the canvas
        is dimmed.  frames: CUDA uint8 [n,h,w,3] (BGR), rows and frames may be strided, or decoded planes (see _yuv420;
        size=(w, h) for packed I420 frames).  mats: CUDA float64, n*9 contiguous elements, as for warp_fixed_plane.  canvas:
        CUDA uint8 [dh,dw,3], rows may be strided: read, carried through the frames and written back.  out: [n,dh,dw,3], rows
        and pictures may be strided, or None = the canvas only advances.  rects: CUDA int32, n*4 contiguous elements
        (x0, y0, x1, y1) in canvas pixels, or None.  origin=(ox, oy) as for warp_fixed_plane.  Does not synchronise."""
        import torch
        self._enter()
        planes, head, n, sw, sh, _ = self._frame_source(frames, size, bgr_only=True)
        self._dev_tensor(mats, torch.float64, 9 * n, "mats must be a contiguous CUDA float64 tensor of n*9 elements")
        if rects is not None:
            self._dev_tensor(rects, torch.int32, 4 * n, "rects must be a contiguous CUDA int32 tensor of n*4 elements")
        cp, dw, dh, crs, _ = self._image_rows(canvas, 3, 0, "canvas")
        op, ors, ofs = None, 0, 0
        if out is not None:
            op, ow, oh, ors, ofs = self._image_rows(out, 3, 1, "out")
            if (out.shape[0], ow, oh) != (n, dw, dh):
                raise ValueError("out must be [n,dh,dw,3] for a canvas [dh,dw,3]")
        tail = (mats.data_ptr(), int(bool(inverse_map)), _ptr(rects), cp, crs, op, ors, ofs, dw, dh, int(origin[0]), int(origin[1]))
        self._check(self._form("evh_trail_fixed_plane", planes)(self.h, *head, *tail))

    def plate_fixed_plane(self, frames, mats, plate, origin, background=None, count=None, masks=None, threshold=16, min_cover=1,
                          inverse_map=False, size=None):
        """The background plate of frames on the fixed plane (evh_plate_fixed_plane[_yuv420], the contract is stated in
        include/evhip.h): per canvas pixel and channel the lower median of the frames that cover it, where at least min_cover
        (1..255) do; elsewhere the background.  frames, mats, origin, inverse_map, size: as for warp_fixed_plane, at most
        PLATE_MAX_FRAMES frames.  plate: CUDA uint8 [dh,dw] (gray frames) or [dh,dw,3], rows may be strided.  background:
        [dh,dw(,3)] with plate's row stride, or None = zeros.  count: [dh,dw], the number of covering frames, or None.  masks:
        [n,dh,dw], 255 where frame k covers the pixel and its gray differs from the plate's by more than threshold (0..255), or
        None; rows (and masks) may be strided.  Does not synchronise."""
        import torch
        self._enter()
        planes, head, n, sw, sh, cn = self._frame_source(frames, size)
        self._dev_tensor(mats, torch.float64, 9 * n, "mats must be a contiguous CUDA float64 tensor of n*9 elements")
        pp, dw, dh, prs, _ = self._image_rows(plate, cn, 0, "plate")
        bp = None
        if background is not None:
            bp, bw, bh, brs, _ = self._image_rows(background, cn, 0, "background")
            if (bw, bh) != (dw, dh) or (dh > 1 and brs != prs):
                raise ValueError("background must be [dh,dw(,3)] with plate's row stride")
        cp, crs = None, 0
        if count is not None:
            cp, cw, ch, crs, _ = self._image_rows(count, 1, 0, "count")
            if (cw, ch) != (dw, dh):
                raise ValueError("count must be [dh,dw] for a plate [dh,dw(,3)]")
        mp, mrs, mfs = None, 0, 0
        if masks is not None:
            mp, mw, mh, mrs, mfs = self._image_rows(masks, 1, 1, "masks")
            if (masks.shape[0], mw, mh) != (n, dw, dh):
                raise ValueError("masks must be [n,dh,dw] for a plate [dh,dw(,3)]")
        tail = (mats.data_ptr(), int(bool(inverse_map)), int(min_cover), bp, pp, prs, cp, crs, mp, int(threshold), mrs, mfs, dw, dh,
                int(origin[0]), int(origin[1]))
        self._check(self._form("evh_plate_fixed_plane", planes)(self.h, *head, *tail))

    def mask_components(self, masks, labels, connectivity=8, open_radius=0, min_area=1, objects=None, nobjects=None, work=None):
        """The connected components of masks (evh_mask_components, the contract is stated in include/evhip.h).  masks: CUDA
        uint8 [n,dh,dw] as plate_fixed_plane writes them, non-zero = set; rows and masks may be strided.  labels: CUDA int32
        [n,dh,dw], rows and sheets may be strided: 0, or the number 1..K of the pixel's component, numbered by first pixel in
        raster order among the components of at least min_area pixels, after an opening by a (2*open_radius+1)^2 square.
        objects: None, or a contiguous CUDA tensor of n*max_objects*40 bytes (int64 [n,max_objects,5] has the alignment): the
        table of evh_component, read with components_table().  nobjects: CUDA int32 [n] or None (one is made).  work: a
        contiguous CUDA tensor of at least mask_components_work_bytes(dw, dh, n) bytes, or None (the context keeps one).  Returns
        nobjects.  Does not synchronise."""
        import torch
        self._enter()
        mp, dw, dh, mrs, mfs = self._image_rows(masks, 1, 1, "masks")
        n = int(masks.shape[0])
        if labels.dtype != torch.int32 or not labels.is_cuda or labels.device.index != self.device or labels.dim() != 3:
            raise ValueError("labels must be an int32 tensor [n,dh,dw] on the context's device (cuda:%d)" % self.device)
        if tuple(labels.shape) != (n, dh, dw) or (dw > 1 and labels.stride(2) != 1):
            raise ValueError("labels must be [n,dh,dw] for masks [n,dh,dw], with packed rows")
        lrs = labels.stride(1) if dh > 1 else dw
        max_objects = 0
        if objects is not None:
            nbytes = objects.numel() * objects.element_size()
            if not objects.is_cuda or objects.device.index != self.device or not objects.is_contiguous() or \
                    nbytes % (40 * max(n, 1)):
                raise ValueError("objects must be a contiguous CUDA tensor of n*max_objects*40 bytes")
            max_objects = nbytes // (40 * max(n, 1))
        if nobjects is None:
            nobjects = torch.zeros(n, dtype=torch.int32, device=labels.device)
        self._dev_tensor(nobjects, torch.int32, n, "nobjects must be a contiguous CUDA int32 tensor of n elements")
        need = mask_components_work_bytes(dw, dh, n)
        if work is None:
            if self._components_work is None or self._components_work.numel() * 4 < need:
                if self._components_work is not None:
                    self.order_torch_after()         # before a larger one replaces it: torch behind what still uses the old one
                self._components_work = torch.empty(max(need, 4) // 4, dtype=torch.int32, device=labels.device)
            work = self._components_work
        if not work.is_cuda or work.device.index != self.device or not work.is_contiguous():
            raise ValueError("work must be a contiguous CUDA tensor")
        if n == 0:                           # empty tensors have no address to hand over
            return nobjects
        self._check(self.lib.evh_mask_components(self.h, mp, n, dw, dh, mrs, mfs, int(connectivity), int(open_radius), int(min_area),
                                                 labels.data_ptr(), lrs, labels.stride(0),
                                                 objects.data_ptr() if max_objects else None, max_objects, nobjects.data_ptr(),
                                                 work.data_ptr(), work.numel() * work.element_size()))
        return nobjects

    @staticmethod
    def components_table(objects):
        """The table mask_components filled, downloaded: a numpy array [n,max_objects] of component_dtype()."""
        n = objects.shape[0]
        return objects.cpu().contiguous().view(-1).numpy().view("u1").reshape(-1).view(component_dtype()).reshape(n, -1)

    def rows_moving_filter(self, frames, mats, plate, count, origin, rows, counts, status1, out_rows, out_counts, moving=None,
                           flags=None, *, threshold=16, min_cover=1, radius=1, min_hits=1, row_scale=(1.0, 1.0), frame_step=1,
                           min_keep=8, size=None):
        """Match rows judged against a plate (evh_rows_moving_filter[_yuv420], the contract is stated in include/evhip.h): a row
        one of whose points sits, in its frame, on something that differs from the plate is dropped, the others move up in
        order.  frames, mats (frame pixel -> plane point, n*9), origin, size: as for plate_fixed_plane; plate [dh,dw(,3)] and count
        [dh,dw] as plate_fixed_plane wrote them (rows may be strided).  rows f32[npairs,cap,4] as (ax, ay, bx, by) with a on frame
        p*frame_step + 1 and b on frame p*frame_step, counts and status1 i32[npairs]: what batch_static_rows hands out.  out_rows
        like rows, out_counts i32[npairs], moving i32[npairs] or None, flags u8[npairs,cap] or None; all contiguous.  A point is
        moving when at least min_hits of the (2*radius+1)^2 canvas pixels around it (row_scale takes row coordinates to frame
        pixels) differ by more than threshold where count >= min_cover; a pair left with fewer than min_keep rows keeps all of
        them.  Does not synchronise."""
        import torch
        self._enter()
        planes, head, n, sw, sh, cn = self._frame_source(frames, size)
        self._dev_tensor(mats, torch.float64, 9 * n, "mats must be a contiguous CUDA float64 tensor of n*9 elements")
        pp, dw, dh, prs, _ = self._image_rows(plate, cn, 0, "plate")
        cp, cw, ch, crs, _ = self._image_rows(count, 1, 0, "count")
        if (cw, ch) != (dw, dh):
            raise ValueError("count must be [dh,dw] for a plate [dh,dw(,3)]")
        if rows.dim() != 3 or rows.shape[2] != 4 or tuple(out_rows.shape) != tuple(rows.shape):
            raise ValueError("rows and out_rows must be [npairs,cap,4]")
        npairs, cap = int(rows.shape[0]), int(rows.shape[1])
        for t, dt, numel, what in ((rows, torch.float32, npairs * cap * 4, "rows"), (out_rows, torch.float32, npairs * cap * 4, "out_rows"),
                                   (counts, torch.int32, npairs, "counts"), (status1, torch.int32, npairs, "status1"),
                                   (out_counts, torch.int32, npairs, "out_counts"), (moving, torch.int32, npairs, "moving"),
                                   (flags, torch.uint8, npairs * cap, "flags")):
            if t is None and what in ("moving", "flags"):
                continue
            self._dev_tensor(t, dt, numel, "%s must be a contiguous CUDA %s tensor of %d elements", what, dt, numel)
        if npairs == 0:                      # empty tensors have no address to hand over
            return
        tail = (mats.data_ptr(), pp, prs, cp, crs, dw, dh, int(origin[0]), int(origin[1]), int(min_cover), int(threshold),
                int(radius), int(min_hits), float(row_scale[0]), float(row_scale[1]), rows.data_ptr(), cap, counts.data_ptr(),
                status1.data_ptr(), npairs, int(frame_step), int(min_keep), out_rows.data_ptr(), out_counts.data_ptr(),
                _ptr(moving), _ptr(flags))
        self._check(self._form("evh_rows_moving_filter", planes)(self.h, *head, *tail))

    def heatmap_render(self, Hsup, out, lut, frames=None, heatmap_constant=1000.0, alpha=0.8, saturate=False):
        """The heat-map pictures of n superposed matrices (evh_heatmap_render, the arithmetic is stated in include/evhip.h).
        Hsup: CUDA float64, n*9 contiguous elements.  out: CUDA uint8 [n,h,w,3] (BGR), rows and pictures may be strided.
        lut: CUDA uint8 [256,3] contiguous, the colour table in BGR order (heatmap.jet_lut()).  frames: CUDA uint8 [n,h,w,3]
        laid under the colours, or None = black.  Does not synchronise."""
        import torch
        self._enter()
        op, w, h, ors, ofs = self._image_rows(out, 3, 1, "out")
        n = out.shape[0]
        self._dev_tensor(Hsup, torch.float64, 9 * n, "Hsup must be a contiguous CUDA float64 tensor of n*9 elements")
        self._dev_tensor(lut, torch.uint8, (256, 3), "lut must be a contiguous CUDA uint8 tensor [256,3]")
        fp, frs, ffs = None, 0, 0
        if frames is not None:
            fp, fw, fh, frs, ffs = self._image_rows(frames, 3, 1, "frames")
            if (frames.shape[0], fw, fh) != (n, w, h):
                raise ValueError("frames must be [n,h,w,3] like out")
        self._check(self.lib.evh_heatmap_render(self.h, Hsup.data_ptr(), n, w, h, fp, frs, ffs, lut.data_ptr(), float(heatmap_constant),
                                                float(alpha), int(bool(saturate)), op, ors, ofs))

    # ---- matching pictures ----
    def batch_static_info(self):
        """-> (pair slots, rows per pair slot) of the last batch whose static rows are still resident; (0, 0): none."""
        n = C.c_int(); cap = C.c_int()
        self._check(self.lib.evh_batch_static_info(self.h, C.byref(n), C.byref(cap)))
        return n.value, cap.value

    def batch_static_rows(self, first_pair=0, npairs=None, rows=None, counts=None, status=None):
        """The rows that entered the last batch's final solve (evh_batch_static_rows), pair slots first_pair .. + npairs
        (default: to the last) -> (rows f32[npairs,cap,4] as (ax, ay, bx, by) with a = the current frame, counts i32[npairs],
        front status i32[npairs]) CUDA tensors; the three may be handed in (contiguous, cap = batch_static_info()[1]).
        Enqueued on the context's stream: complete after synchronize() or order_torch_after()."""
        import torch
        slots, cap = self.batch_static_info()
        if npairs is None:
            npairs = slots - int(first_pair)
        npairs = int(npairs)
        dev = "cuda:%d" % self.device
        if rows is None:
            rows = torch.empty((max(npairs, 0), cap, 4), dtype=torch.float32, device=dev)
        if counts is None:
            counts = torch.empty(max(npairs, 0), dtype=torch.int32, device=dev)
        if status is None:
            status = torch.empty(max(npairs, 0), dtype=torch.int32, device=dev)
        for t, dt, numel, what in ((rows, torch.float32, npairs * cap * 4, "rows"), (counts, torch.int32, npairs, "counts"),
                                   (status, torch.int32, npairs, "status")):
            if t.dtype != dt or not t.is_cuda or t.device.index != self.device or not t.is_contiguous() or \
                    t.numel() < max(numel, 0):
                raise ValueError("%s must be a contiguous CUDA %s tensor of at least %d elements" % (what, dt, numel))
        self._enter()
        self._check(self.lib.evh_batch_static_rows(self.h, int(first_pair), npairs, rows.data_ptr(), rows.shape[1] if rows.dim() == 3 else cap,
                                                   counts.data_ptr(), status.data_ptr()))
        return rows, counts, status

    def draw_matches(self, frames, rows, counts, out, status=None, frame_step=1, points="reference", color=(0, 255, 0)):
        """The matching pictures (evh_draw_matches, the line rule is stated in include/evhip.h).  frames: uint8 [n,h,w,3] BGR,
        rows and frames may be strided; out: uint8 [npairs,h,2w,3], rows and pictures may be strided: picture p = frame
        p*frame_step | frame p*frame_step + 1 with one line per row r < counts[p] of rows f32[npairs,cap,4] (contiguous);
        status i32[npairs] or None: a picture whose status is not PAIR_OK gets no lines.  points: "reference" (the reference's
        picture: the (ax, ay) end on the left half) or "own_frame"; color: (b, g, r).  Does not synchronise."""
        import torch
        self._enter()
        points = DRAW_POINTS[points] if isinstance(points, str) else int(points)
        fp, w, h, frs, ffs = self._image_rows(frames, 3, 1, "frames")
        op, ow, oh, ors, ofs = self._image_rows(out, 3, 1, "out")
        npairs = out.shape[0]
        if (ow, oh) != (2 * w, h):
            raise ValueError("out must be [npairs,h,2w,3] for frames [n,h,w,3]")
        if npairs and frames.shape[0] < (npairs - 1) * int(frame_step) + 2:
            raise ValueError("frames holds fewer frames than the pictures take")
        if rows.dtype != torch.float32 or not rows.is_cuda or rows.device.index != self.device or rows.dim() != 3 or \
                rows.shape[2] != 4 or rows.shape[0] < npairs or not rows.is_contiguous():
            raise ValueError("rows must be a contiguous CUDA float32 tensor [npairs,cap,4]")
        for t, what in ((counts, "counts"), (status, "status")):
            if t is not None and (t.dtype != torch.int32 or not t.is_cuda or t.device.index != self.device or
                                  not t.is_contiguous() or t.numel() < npairs):
                raise ValueError("%s must be a contiguous CUDA int32 tensor of npairs elements" % what)
        b, g, r = (int(v) for v in color)
        if min(b, g, r) < 0 or max(b, g, r) > 255:
            raise ValueError("color is (b, g, r) with bytes")
        self._check(self.lib.evh_draw_matches(self.h, fp, npairs, int(frame_step), w, h, frs, ffs, rows.data_ptr(), rows.shape[1],
                                              counts.data_ptr(), _ptr(status), points, b | g << 8 | r << 16, op, ors, ofs))

    # ---- pictures encoded on the device ----
    def jpeg_encode(self, pictures, qtabs, subsampling="420", out=None):
        """Baseline JPEG files of pictures that lie on the device (evh_jpeg_encode, the arithmetic is stated in include/evhip.h)
        -> a list of bytes, one file per picture.  pictures: uint8 [n,h,w] gray or [n,h,w,3] BGR, rows and pictures may be
        strided (a view cut out of a larger canvas); qtabs: [2,64] in natural order, each 1..255 (pictures.quant_tables).  The
        files are written into `out` (uint8 [n, cap] on the device; without it a quarter of the raw size per picture); if a
        picture reports more than cap the call is repeated once with the largest length reported.  Synchronises: the lengths
        and the files come to the host."""
        import torch
        sub = JPEG_SUBSAMPLINGS[subsampling] if isinstance(subsampling, str) else int(subsampling)
        cn = 1 if pictures.dim() == 3 else 3
        pp, w, h, prs, pps = self._image_rows(pictures, cn, 1, "pictures")
        n = pictures.shape[0]
        q = _jpeg_tables(qtabs)
        if out is not None:
            self._dev_tensor(out, torch.uint8, out.numel(), "out must be a contiguous CUDA uint8 tensor [n, cap]")
            if out.dim() != 2 or out.shape[0] < n:
                raise ValueError("out must be [n, cap]")
        else:
            out = torch.empty((max(n, 1), max(1024, w * h * cn // 4)), dtype=torch.uint8, device=pictures.device)
        if n == 0:
            return []
        sizes = torch.zeros(max(n, 1), dtype=torch.int64, device=pictures.device)
        for _ in range(2):
            self._enter()
            self._check(self.lib.evh_jpeg_encode(self.h, pp, n, w, h, prs, pps, cn, sub, _hp(q), out.data_ptr(), out.shape[1],
                                                 out.shape[1], sizes.data_ptr()))
            self.order_torch_after()
            lengths = sizes[:n].cpu().numpy()
            if n == 0 or int(lengths.max()) <= out.shape[1]:
                break
            out = torch.empty((n, int(lengths.max())), dtype=torch.uint8, device=pictures.device)
        host = out[:n, :int(lengths.max())].cpu().numpy()       # the files and no more: the slots are far longer than they are
        return [host[p, :int(lengths[p])].tobytes() for p in range(n)]

    # ---- the score of a homography ----
    def _pair_residual(self, planes, frames, mats, stats, out, threshold, kind, frame_step, size):
        import torch
        self._enter()
        kind = RESIDUAL_KINDS[kind] if isinstance(kind, str) else int(kind)
        frame_step = int(frame_step)
        if frame_step not in (1, 2):
            raise ValueError("frame_step must be 1 or 2")
        planes, head, n, w, h, _ = self._frame_source(frames, size, planes=planes)
        npairs = mats.numel() // 9
        self._dev_tensor(mats, torch.float64, 9 * npairs, "mats must be a contiguous CUDA float64 tensor of npairs*9 elements")
        if npairs and n < (npairs - 1) * frame_step + 2:
            raise ValueError("frames holds fewer frames than the pairs take")
        if stats is None:
            stats = torch.empty((npairs, RES_NSTATS), dtype=torch.int64, device="cuda:%d" % self.device)
        self._dev_tensor(stats, torch.int64, (npairs, RES_NSTATS), "stats must be a contiguous CUDA int64 tensor [npairs,%d]", RES_NSTATS)
        op, ors, ofs = None, 0, 0
        if out is not None:
            op, ow, oh, ors, ofs = self._image_rows(out, 1, 1, "out")
            if (out.shape[0], ow, oh) != (npairs, w, h):
                raise ValueError("out must be [npairs,h,w] for frames of h x w")
        if npairs == 0:                      # empty tensors have no address to hand over
            return stats
        tail = (mats.data_ptr(), int(threshold), stats.data_ptr(), op, kind, ors, ofs)
        # the head with (npairs, frame_step) in the place of the frame count
        self._check(self._form("evh_pair_residual", planes)(self.h, head[0], npairs, frame_step, w, h, *head[4:], *tail))
        return stats

    def pair_residual(self, frames, mats, stats=None, out=None, threshold=16, kind="abs", frame_step=1):
        """The motion-compensated residual of pairs of frames (evh_pair_residual, the arithmetic is stated in include/evhip.h).
        frames: CUDA uint8 [n,h,w] (gray) or [n,h,w,3] (BGR), rows and frames may be strided; pair p is (frame p*frame_step,
        frame p*frame_step + 1).  mats: CUDA float64, npairs*9 contiguous elements, pixel of the current frame -> pixel of the
        previous frame.  stats: CUDA int64 [npairs,6] contiguous or None = a new tensor; it is returned: (covered, sad, ssd,
        sad of the unregistered pair, ssd of the unregistered pair, moving) per pair, the library's u64 values viewed as int64
        (all below 2^47).  out: CUDA uint8 [npairs,h,w], rows and pictures may be strided, or None; kind "abs": the
        difference, "mask": 255 where it exceeds threshold.  Does not synchronise."""
        return self._pair_residual(False, frames, mats, stats, out, threshold, kind, frame_step, None)

    def pair_residual_yuv420(self, planes, mats, stats=None, out=None, threshold=16, kind="abs", frame_step=1, size=None):
        """pair_residual on decoded planes (see _yuv420; size=(w, h) for packed I420 frames): every pixel and tap converted as
        yuv420_to_bgr converts it (evh_pair_residual_yuv420)."""
        return self._pair_residual(True, planes, mats, stats, out, threshold, kind, frame_step, size)

    # ---- direct alignment ----
    def _pair_refine(self, planes, frames, mats, iters, clip, out, info, normal, frame_step, size):
        import torch
        self._enter()
        frame_step = int(frame_step)
        if frame_step not in (1, 2):
            raise ValueError("frame_step must be 1 or 2")
        planes, head, n, w, h, _ = self._frame_source(frames, size, planes=planes)
        npairs = mats.numel() // 9
        self._dev_tensor(mats, torch.float64, 9 * npairs, "mats must be a contiguous CUDA float64 tensor of npairs*9 elements")
        if npairs and n < (npairs - 1) * frame_step + 2:
            raise ValueError("frames holds fewer frames than the pairs take")
        dev = "cuda:%d" % self.device
        if out is None:
            out = torch.empty((npairs, 9), dtype=torch.float64, device=dev)
        if info is None:
            info = torch.empty((npairs, REFINE_NINFO), dtype=torch.int64, device=dev)
        self._dev_tensor(out, torch.float64, 9 * npairs, "out must be a contiguous CUDA float64 tensor of npairs*9 elements")
        self._dev_tensor(info, torch.int64, (npairs, REFINE_NINFO), "info must be a contiguous CUDA int64 tensor [npairs,%d]", REFINE_NINFO)
        if normal is not None:
            self._dev_tensor(normal, torch.float64, (npairs, REFINE_NSUMS), "normal must be a contiguous CUDA float64 tensor [npairs,%d]",
                             REFINE_NSUMS)
        if npairs == 0:                      # empty tensors have no address to hand over
            return out, info
        tail = (mats.data_ptr(), int(iters), int(clip), out.data_ptr(), info.data_ptr(), _ptr(normal))
        self._check(self._form("evh_pair_refine", planes)(self.h, head[0], npairs, frame_step, w, h, *head[4:], *tail))
        return out, info

    def pair_refine(self, frames, mats, iters=8, clip=255, out=None, info=None, normal=None, frame_step=1):
        """Direct alignment of pairs of frames (evh_pair_refine, the method is stated in include/evhip.h): each matrix improved
        by damped Gauss-Newton steps on the photometric residual, never made worse.  frames, mats and frame_step as in
        pair_residual.  out: CUDA float64 npairs*9 contiguous (it may be `mats`) or None = a new tensor; info: CUDA int64
        [npairs,8] contiguous (REFINE_INFO names the columns) or None; both are returned.  normal: CUDA float64 [npairs,45] or
        None: the normal sums at `mats`.  Does not synchronise."""
        return self._pair_refine(False, frames, mats, iters, clip, out, info, normal, frame_step, None)

    def pair_refine_yuv420(self, planes, mats, iters=8, clip=255, out=None, info=None, normal=None, frame_step=1, size=None):
        """pair_refine on decoded planes (see _yuv420; size=(w, h) for packed I420 frames): every pixel and tap converted as
        yuv420_to_bgr converts it (evh_pair_refine_yuv420)."""
        return self._pair_refine(True, planes, mats, iters, clip, out, info, normal, frame_step, size)

    # ---- points followed between frames ----
    def _track_points(self, planes, frames, pts, npts, mats, levels, radius, iters, min_eig, fb_max, max_err, rows, counts, flags, err,
                      frame_step, size):
        import torch
        self._enter()
        frame_step = int(frame_step)
        if frame_step not in (1, 2):
            raise ValueError("frame_step must be 1 or 2")
        planes, head, n, w, h, _ = self._frame_source(frames, size, planes=planes)
        if pts.dim() != 3 or pts.shape[2] != 2:
            raise ValueError("pts must be [npairs,pt_cap,2]")
        npairs, pt_cap = int(pts.shape[0]), int(pts.shape[1])
        self._dev_tensor(pts, torch.float32, npairs * pt_cap * 2, "pts must be a contiguous CUDA float32 tensor [npairs,pt_cap,2]")
        self._dev_tensor(npts, torch.int32, npairs, "npts must be a contiguous CUDA int32 tensor of npairs elements")
        if mats is not None:
            self._dev_tensor(mats, torch.float64, 9 * npairs, "mats must be a contiguous CUDA float64 tensor of npairs*9 elements")
        if npairs and n < (npairs - 1) * frame_step + 2:
            raise ValueError("frames holds fewer frames than the pairs take")
        dev = "cuda:%d" % self.device
        if rows is None:
            rows = torch.empty((npairs, pt_cap, 4), dtype=torch.float32, device=dev)
        if counts is None:
            counts = torch.empty(npairs, dtype=torch.int32, device=dev)
        if rows.dim() != 3 or rows.shape[0] != npairs or rows.shape[2] != 4:
            raise ValueError("rows must be [npairs,row_cap,4]")
        row_cap = int(rows.shape[1])
        self._dev_tensor(rows, torch.float32, npairs * row_cap * 4, "rows must be a contiguous CUDA float32 tensor [npairs,row_cap,4]")
        self._dev_tensor(counts, torch.int32, npairs, "counts must be a contiguous CUDA int32 tensor of npairs elements")
        if flags is not None:
            self._dev_tensor(flags, torch.uint8, (npairs, pt_cap), "flags must be a contiguous CUDA uint8 tensor [npairs,pt_cap]")
        if err is not None:
            self._dev_tensor(err, torch.int32, (npairs, pt_cap), "err must be a contiguous CUDA int32 tensor [npairs,pt_cap]")
        if npairs == 0 or pt_cap == 0:       # empty tensors have no address to hand over
            if npairs:
                counts.zero_()
            return rows, counts
        fb = -1 if fb_max is None else int(round(32.0 * float(fb_max)))
        tail = (pts.data_ptr(), npts.data_ptr(), pt_cap, _ptr(mats), int(levels), int(radius), int(iters), float(min_eig), fb,
                -1 if max_err is None else int(max_err), rows.data_ptr(), row_cap, counts.data_ptr(), _ptr(flags), _ptr(err))
        self._check(self._form("evh_track_points", planes)(self.h, head[0], npairs, frame_step, w, h, *head[4:], *tail))
        return rows, counts

    def track_points(self, frames, pts, npts, mats=None, levels=3, radius=7, iters=20, min_eig=0.0, fb_max=None, max_err=None,
                     rows=None, counts=None, flags=None, err=None, frame_step=1):
        """Points of the current frame of every pair followed into its previous frame (evh_track_points, the arithmetic is stated
        in include/evhip.h).  frames and frame_step as in pair_residual.  pts: CUDA float32 [npairs,pt_cap,2], (x, y) on the current
        frame; npts: CUDA int32 [npairs]; mats: CUDA float64 npairs*9, current pixel -> previous pixel, the first guess, or None.
        fb_max: the forward-backward bar in pixels (taken to 1/32 pixel) or None = no backward pass; max_err: 0..255 gray levels of
        mean absolute difference or None.  rows: CUDA float32 [npairs,row_cap >= pt_cap,4] or None = a new tensor, counts: CUDA
        int32 [npairs] or None; both are returned: rows (ax, ay, bx, by) of the kept points in input order, the layout of
        batch_static_rows.  flags: CUDA uint8 [npairs,pt_cap] or None (TRACK_FLAGS names the codes); err: CUDA int32
        [npairs,pt_cap] or None (the library's u32 values; -1 = TRACK_NO_ERR).  Does not synchronise."""
        return self._track_points(False, frames, pts, npts, mats, levels, radius, iters, min_eig, fb_max, max_err, rows, counts, flags,
                                  err, frame_step, None)

    def track_points_yuv420(self, planes, pts, npts, mats=None, levels=3, radius=7, iters=20, min_eig=0.0, fb_max=None, max_err=None,
                            rows=None, counts=None, flags=None, err=None, frame_step=1, size=None):
        """track_points on decoded planes (see _yuv420; size=(w, h) for packed I420 frames): every pixel converted as yuv420_to_bgr
        converts it (evh_track_points_yuv420)."""
        return self._track_points(True, planes, pts, npts, mats, levels, radius, iters, min_eig, fb_max, max_err, rows, counts, flags,
                                  err, frame_step, size)

    def _track_seeds(self, planes, frames, radius, cell, border, min_eig, pts, npts, pt_cap, size):
        import torch
        self._enter()
        planes, head, n, w, h, _ = self._frame_source(frames, size, planes=planes)
        dev = "cuda:%d" % self.device
        if pts is None:
            pts = torch.empty((n, int(pt_cap), 2), dtype=torch.float32, device=dev)
        if npts is None:
            npts = torch.empty(n, dtype=torch.int32, device=dev)
        if pts.dim() != 3 or pts.shape[0] != n or pts.shape[2] != 2:
            raise ValueError("pts must be [n,pt_cap,2]")
        pt_cap = int(pts.shape[1])
        self._dev_tensor(pts, torch.float32, n * pt_cap * 2, "pts must be a contiguous CUDA float32 tensor [n,pt_cap,2]")
        self._dev_tensor(npts, torch.int32, n, "npts must be a contiguous CUDA int32 tensor of n elements")
        if n == 0:                           # empty tensors have no address to hand over
            return pts, npts
        border = int(radius) + 1 if border is None else int(border)
        tail = (int(radius), int(cell), border, float(min_eig), pts.data_ptr(), pt_cap, npts.data_ptr())
        self._check(self._form("evh_track_seeds", planes)(self.h, *head, *tail))
        return pts, npts

    def track_seeds(self, frames, radius=2, cell=16, border=None, min_eig=0.0, pts=None, npts=None, pt_cap=1024):
        """The best-conditioned pixel of every cell of every frame (evh_track_seeds, stated in include/evhip.h).  frames: CUDA uint8
        [n,h,w] or [n,h,w,3], rows and frames may be strided.  border: None = radius + 1.  pts: CUDA float32 [n,pt_cap,2] or None =
        a new tensor of pt_cap slots per frame; npts: CUDA int32 [n] or None; both are returned: the seeds (x, y) in cell raster
        order and their full count (it may exceed pt_cap; only pt_cap are written).  Does not synchronise."""
        return self._track_seeds(False, frames, radius, cell, border, min_eig, pts, npts, pt_cap, None)

    def track_seeds_yuv420(self, planes, radius=2, cell=16, border=None, min_eig=0.0, pts=None, npts=None, pt_cap=1024, size=None):
        """track_seeds on decoded planes (see _yuv420; size=(w, h) for packed I420 frames) (evh_track_seeds_yuv420)."""
        return self._track_seeds(True, planes, radius, cell, border, min_eig, pts, npts, pt_cap, size)

    # ---- direct alignment against the mosaic ----
    def _canvas_refine(self, planes, frames, canvas, mats, count, min_cover, iters, clip, out, info, normal, size):
        import torch
        self._enter()
        planes, head, n, w, h, cn = self._frame_source(frames, size, planes=planes)
        self._dev_tensor(mats, torch.float64, 9 * n, "mats must be a contiguous CUDA float64 tensor of n*9 elements")
        cp, dw, dh, crs, _ = self._image_rows(canvas, cn, 0, "canvas")
        kp, krs = None, 0
        if count is not None:
            kp, kw, kh, krs, _ = self._image_rows(count, 1, 0, "count")
            if (kw, kh) != (dw, dh):
                raise ValueError("count must be [dh,dw] for a canvas [dh,dw(,3)]")
        dev = "cuda:%d" % self.device
        if out is None:
            out = torch.empty((n, 9), dtype=torch.float64, device=dev)
        if info is None:
            info = torch.empty((n, REFINE_NINFO), dtype=torch.int64, device=dev)
        self._dev_tensor(out, torch.float64, 9 * n, "out must be a contiguous CUDA float64 tensor of n*9 elements")
        self._dev_tensor(info, torch.int64, (n, REFINE_NINFO), "info must be a contiguous CUDA int64 tensor [n,%d]", REFINE_NINFO)
        if normal is not None:
            self._dev_tensor(normal, torch.float64, (n, REFINE_NSUMS), "normal must be a contiguous CUDA float64 tensor [n,%d]", REFINE_NSUMS)
        if n == 0:                           # empty tensors have no address to hand over
            return out, info
        tail = (cp, dw, dh, crs, kp, krs, int(min_cover), mats.data_ptr(), int(iters), int(clip), out.data_ptr(), info.data_ptr(),
                _ptr(normal))
        self._check(self._form("evh_canvas_refine", planes)(self.h, *head, *tail))
        return out, info

    def canvas_refine(self, frames, canvas, mats, count=None, min_cover=1, iters=8, clip=255, out=None, info=None, normal=None):
        """Frames aligned against a canvas (evh_canvas_refine, the contract is stated in include/evhip.h): pair_refine with the
        previous frame replaced by `canvas`, CUDA uint8 [dh,dw] (gray frames) or [dh,dw,3], rows may be strided.  frames: as in
        pair_refine, n of them; mats: CUDA float64, n*9 contiguous elements, pixel of frame k -> pixel of the canvas.  count: CUDA
        uint8 [dh,dw], rows may be strided, or None = every canvas pixel is valid; a pixel counts where count >= min_cover
        (1..255).  out, info, normal: as in pair_refine, one row per frame; out and info are returned.  iters=0: the score of
        the frames against the canvas.  Does not synchronise."""
        return self._canvas_refine(False, frames, canvas, mats, count, min_cover, iters, clip, out, info, normal, None)

    def canvas_refine_yuv420(self, planes, canvas, mats, count=None, min_cover=1, iters=8, clip=255, out=None, info=None, normal=None,
                             size=None):
        """canvas_refine on decoded planes (see _yuv420; size=(w, h) for packed I420 frames) against a BGR canvas: every pixel of a
        frame converted as yuv420_to_bgr converts it (evh_canvas_refine_yuv420)."""
        return self._canvas_refine(True, planes, canvas, mats, count, min_cover, iters, clip, out, info, normal, size)

    # ---- global alignment ----
    def graph_normal(self, S, edges, rows, counts, status=None, H_edge=None, inlier_thr=3.0, huber_delta=0.0, sums=None, info=None):
        """The normal equations of the joint problem over all superposed matrices (evh_graph_normal, the arithmetic is stated in
        include/evhip.h).  All CUDA, contiguous: S float64 with nframes*9 elements; edges int32 [nedges,2] = (i, j); rows float32
        [nedges,cap,4] as batch_static_rows lays them out (a in frame i, b in frame j); counts int32 [nedges]; status int32
        [nedges] or None; H_edge float64 with nedges*9 elements (the pair matrices, a onto b: rows beyond inlier_thr are gated) or
        None.  -> (sums float64 [nedges,154], info int32 [nedges,4] = used, gated, behind, flags); the two may be handed in.  Does
        not synchronise."""
        import torch
        nedges = edges.shape[0] if edges.dim() == 2 else -1
        dev = "cuda:%d" % self.device
        if sums is None:
            sums = torch.empty((max(nedges, 0), GRAPH_NSUMS), dtype=torch.float64, device=dev)
        if info is None:
            info = torch.empty((max(nedges, 0), 4), dtype=torch.int32, device=dev)
        if edges.dim() != 2 or edges.shape[1] != 2 or rows.dim() != 3 or rows.shape[2] != 4 or rows.shape[0] < nedges or S.numel() % 9:
            raise ValueError("graph_normal: S holds nframes*9 elements, edges is [nedges,2], rows [nedges,cap,4]")
        for t, dt, numel, what in ((S, torch.float64, 9, "S"), (edges, torch.int32, 2 * nedges, "edges"), (rows, torch.float32, 0, "rows"),
                                   (counts, torch.int32, nedges, "counts"), (status, torch.int32, nedges, "status"),
                                   (H_edge, torch.float64, 9 * nedges, "H_edge"), (sums, torch.float64, GRAPH_NSUMS * nedges, "sums"),
                                   (info, torch.int32, 4 * nedges, "info")):
            if t is not None and (t.dtype != dt or not t.is_cuda or t.device.index != self.device or not t.is_contiguous() or
                                  t.numel() < numel):
                raise ValueError("graph_normal: %s must be a contiguous CUDA %s tensor of at least %d elements" % (what, dt, numel))
        self._enter()
        self._check(self.lib.evh_graph_normal(self.h, S.data_ptr(), S.numel() // 9, edges.data_ptr(), nedges, rows.data_ptr(),
                                              rows.shape[1], counts.data_ptr(), _ptr(status), _ptr(H_edge), float(inlier_thr),
                                              float(huber_delta), sums.data_ptr(), info.data_ptr()))
        return sums, info

    def orb_detect_batch_yuv420(self, planes, size=None, nfeatures=500, resize_to=None):
        """orb_detect_batch on decoded planes (see _yuv420), level 0 straight from them."""
        self._enter()
        d, n, w, h = self._yuv420(planes, size, self.device)
        self._check(self.lib.evh_orb_detect_batch_yuv420(self.h, C.byref(d), n, w, h, *_work_size(resize_to, w, h), nfeatures))

    def stream_homography_batch_yuv420(self, planes, size, out_H, out_status, state_in=None, state_out=None, nfeatures=500,
                                       thr=3.0, max_iters=2000, conf=0.995, force_max_iters=False, resize_to=None):
        """stream_homography_batch on decoded planes (see _yuv420): n >= 2 consecutive frames -> n-1 pairs."""
        self._enter()
        d, n, w, h = self._yuv420(planes, size, self.device)
        self._check(self.lib.evh_stream_homography_batch_yuv420(
            self.h, C.byref(d), n, w, h, *_work_size(resize_to, w, h), nfeatures,
            *_tail((thr, max_iters, conf, force_max_iters), state_in, state_out, out_H, out_status)))

    def stream_homography_batch_types_yuv420(self, planes, size, out_H, out_status, features, state_in=None, state_out=None,
                                             nfeatures=500, thr=3.0, max_iters=2000, conf=0.995, force_max_iters=False,
                                             resize_to=None):
        """stream_homography_batch_types on decoded planes: converted once on the device, then the BGR path."""
        self._enter()
        d, n, w, h = self._yuv420(planes, size, self.device)
        t = self._types(features)
        self._multi_used = True
        self._check(self.lib.evh_stream_homography_batch_types_yuv420(
            self.h, C.byref(d), n, w, h, *_work_size(resize_to, w, h), nfeatures, _hp(t), len(t),
            *_tail((thr, max_iters, conf, force_max_iters), state_in, state_out, out_H, out_status)))

    # ---- N4: SIFT + multi-type pairs ----
    def sift_enable(self, max_sift_features=8192):
        self._check(self.lib.evh_sift_enable(self.h, int(max_sift_features)))

    def sift_detect_batch(self, frames, resize_to=None):
        """frames: CUDA uint8 [n,h,w] or [n,h,w,3]; SIFT_create().detectAndCompute on each (frame_processing.py:62-64)."""
        self._enter()
        p = _packed(frames)
        self._check(self.lib.evh_sift_detect_batch(self.h, *p, *_work_size(resize_to, *p[2:4])))

    def _kp_download(self, det, frame, fields):
        """A frame's SIFT / SURF key points: xy, desc and `fields` (the per-key-point arrays in the C entry's argument order)."""
        cap = getattr(self.lib, "evh_%s_capacity" % det)(self.h)
        out = dict(xy=np.zeros((cap, 2), np.float32), desc=np.zeros((cap, 128), np.float32))
        for k in fields:
            out[k] = np.zeros(cap, np.int32 if k in ("octave", "laplacian") else np.float32)
        n = self._check(getattr(self.lib, "evh_%s_download" % det)(self.h, frame, *[_hp(a) for a in out.values()]))
        return {k: a[:n].copy() for k, a in out.items()}

    def sift_download(self, frame):
        return self._kp_download("sift", frame, ("octave", "size", "angle", "response"))

    def sift_octaves(self):
        out = []
        while True:
            w = C.c_int(); h = C.c_int()
            rc = self.lib.evh_sift_octave_info(self.h, len(out), C.byref(w), C.byref(h))
            if rc != 0:
                break
            out.append((w.value, h.value))
        return out

    def sift_download_gauss(self, frame, octave, layer):
        w, h = self.sift_octaves()[octave]
        out = np.zeros((h, w), np.float32)
        self._check(self.lib.evh_sift_download_gauss(self.h, frame, octave, layer, _hp(out)))
        return out

    def surf_enable(self, max_surf_features=4096):
        self._check(self.lib.evh_surf_enable(self.h, int(max_surf_features)))

    def surf_detect_batch(self, frames, resize_to=None, hessian_threshold=400.0):
        """frames: CUDA uint8 [n,h,w] or [n,h,w,3]; SURF_create(extended=1, hessianThreshold=400).detectAndCompute
        (frame_processing.py:65-67)."""
        self._enter()
        p = _packed(frames)
        dw, dh = _work_size(resize_to, *p[2:4])
        self._surf_shape = (dh, dw)
        self._check(self.lib.evh_surf_detect_batch(self.h, *p, dw, dh, float(hessian_threshold)))

    def surf_download(self, frame):
        return self._kp_download("surf", frame, ("size", "angle", "response", "octave", "laplacian"))

    def surf_download_integral(self, frame):
        h, w = self._surf_shape
        out = np.zeros((h + 1, w + 1), np.int32)
        self._check(self.lib.evh_surf_download_integral(self.h, frame, _hp(out)))
        return out

    def knn2_f32(self, q, t, idx, dist):
        """q, t: CUDA float32 [n,dim] (dim 64 or 128); idx int32 [nq,2], dist float32 [nq,2]."""
        self._enter()
        self._check(self.lib.evh_match_knn2_l2f32(self.h, q.data_ptr(), q.shape[0], t.data_ptr(), t.shape[0], q.shape[1],
                                                  idx.data_ptr(), dist.data_ptr()))

    def ratio_unique_filter_f32(self, idx, dist, xy_q, xy_t, pts, ratio=0.5, min_matches=4):
        self._enter()
        n = C.c_int(); st = C.c_int()
        self._check(self.lib.evh_ratio_unique_filter_f32(self.h, idx.data_ptr(), dist.data_ptr(), idx.shape[0], xy_t.shape[0],
                                                         xy_q.data_ptr(), xy_t.data_ptr(), float(ratio), int(min_matches),
                                                         pts.data_ptr(), C.byref(n), C.byref(st)))
        return n.value, st.value

    @staticmethod
    def _types(features):
        codes = np.ascontiguousarray([FEATURE_CODES[f] if isinstance(f, str) else int(f) for f in features], np.int32)
        return codes

    def pair_homography_batch_types(self, frames, npairs, mode, out_H, out_status, features, nfeatures=500, thr=3.0,
                                    max_iters=2000, conf=0.995, force_max_iters=False, resize_to=None):
        self._enter()
        p = _packed(frames)
        t = self._types(features)
        self._multi_used = True
        self._check(self.lib.evh_pair_homography_batch_types(
            self.h, p[0], npairs, mode, *p[2:], *_work_size(resize_to, *p[2:4]), nfeatures, _hp(t), len(t),
            *_ransac(thr, max_iters, conf, force_max_iters), out_H.data_ptr(), out_status.data_ptr()))

    def stream_homography_batch_types(self, frames, out_H, out_status, features, state_in=None, state_out=None, nfeatures=500,
                                      thr=3.0, max_iters=2000, conf=0.995, force_max_iters=False, resize_to=None):
        """stream_homography_batch with a list of feature types ("SIFT", "ORB", ... in the order the reference's
        FrameProcessing would loop over them, frame_processing.py:91-104)."""
        self._enter()
        p = _packed(frames)
        t = self._types(features)
        self._multi_used = True
        self._check(self.lib.evh_stream_homography_batch_types(
            self.h, *p, *_work_size(resize_to, *p[2:4]), nfeatures, _hp(t), len(t),
            *_tail((thr, max_iters, conf, force_max_iters), state_in, state_out, out_H, out_status)))

    def _torch_stream(self):
        """The context's (non-blocking) HIP stream as a torch stream, for ordering against torch work."""
        import torch
        if getattr(self, "_ext_stream", None) is None:
            self._ext_stream = torch.cuda.ExternalStream(self.stream, device=self.device)
        return self._ext_stream

    def order_after_torch(self):
        """Kernels enqueued by this context from now on wait for the work already on torch's current stream."""
        import torch
        self._torch_stream().wait_stream(torch.cuda.current_stream(self.device))

    def order_torch_after(self):
        """torch's current stream waits for everything this context has enqueued so far (main and solve stream)."""
        import torch
        self.solve_wait()
        torch.cuda.current_stream(self.device).wait_stream(self._torch_stream())

    def stream_static_batch(self, frames, nfeatures=500, thr=3.0, max_iters=2000, conf=0.995, force_max_iters=False):
        """Phase 1 of the two-phase stream path (evh_stream_static_batch): frames CUDA uint8 [n,h,w(,3)] ->
        (rows f32[n-1,cap,4], counts i32[n-1], status1 i32[n-1]) as CUDA tensors.  Asynchronous, but ordered with
        torch's current stream on both sides (inputs produced by torch ops, outputs consumed by torch ops / RCCL)."""
        import torch
        n = frames.shape[0]
        cap = self.lib.evh_orb_capacity(self.h)
        rows = torch.zeros((max(n - 1, 0), cap, 4), dtype=torch.float32, device=frames.device)
        counts = torch.zeros(max(n - 1, 0), dtype=torch.int32, device=frames.device)
        status1 = torch.zeros(max(n - 1, 0), dtype=torch.int32, device=frames.device)
        if n < 2:
            return rows, counts, status1          # an empty block (more ranks than pairs)
        self.order_after_torch()
        self._check(self.lib.evh_stream_static_batch(
            self.h, *_packed(frames), nfeatures, *_ransac(thr, max_iters, conf, force_max_iters), rows.data_ptr(), cap,
            counts.data_ptr(), status1.data_ptr()))
        self.order_torch_after()
        return rows, counts, status1

    def stream_scan(self, rows, counts, status1, state_in=None, state_out=None, thr=3.0, max_iters=2000, conf=0.995,
                    force_max_iters=False):
        """Phase 2 (evh_stream_scan): the sequential compute_homography / matrix_superposition scan over all pairs in
        stream order -> (H f64[npairs,9], status i32[npairs]) CUDA tensors.  Asynchronous, ordered with torch's
        current stream like stream_static_batch."""
        import torch
        npairs, cap = rows.shape[0], rows.shape[1]
        rows = rows.contiguous(); counts = counts.contiguous(); status1 = status1.contiguous()
        H = torch.zeros((npairs, 9), dtype=torch.float64, device=rows.device)
        st = torch.zeros(npairs, dtype=torch.int32, device=rows.device)
        self.order_after_torch()
        self._check(self.lib.evh_stream_scan(
            self.h, rows.data_ptr(), cap, counts.data_ptr(), status1.data_ptr(), npairs,
            *_tail((thr, max_iters, conf, force_max_iters), state_in, state_out, H, st)))
        self.order_torch_after()
        return H, st

    def match_static_from_slots(self, cur_slot, prev_slot):
        cap = self.lib.evh_orb_capacity(self.h)
        pts = np.zeros((cap, 4), np.float32)
        n = C.c_int(); st = C.c_int()
        self._check(self.lib.evh_match_static_from_slots(self.h, cur_slot, prev_slot, _hp(pts), cap, C.byref(n), C.byref(st)))
        return st.value, pts[:n.value].copy()

    def compute_homography(self, pts, Hsup=None):
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
        H = np.zeros(9, np.float64); st = C.c_int()
        hs = None if Hsup is None else np.ascontiguousarray(Hsup, np.float64).reshape(9)
        self._check(self.lib.evh_compute_homography(self.h, _hp(pts), pts.shape[0], _hp(hs), _hp(H), C.byref(st)))
        return st.value, H.reshape(3, 3)

    def pair_from_slots(self, cur_slot, prev_slot, Hsup=None):
        H = np.zeros(9, np.float64); st = C.c_int()
        hs = None if Hsup is None else np.ascontiguousarray(Hsup, np.float64).reshape(9)
        self._check(self.lib.evh_pair_from_slots(self.h, cur_slot, prev_slot, _hp(hs), _hp(H), C.byref(st)))
        return st.value, H.reshape(3, 3)
