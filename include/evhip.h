/*
 * include/evhip.h -- C ABI of libevhip.so: the MI355X (gfx950) implementation of EvenVizion's
 * frame-to-frame homography hot path.
 *
 * The reference (gridl/EvenVizion) has no FFI of its own: its operator boundary is four third-party calls
 * made from Python.  Each entry point below names the reference call site it replaces:
 *
 *   evh_resize_area_u8            imutils.resize(frame, width=)          video_processing.py:62,73
 *   evh_orb_detect_batch          cv2.ORB_create().detectAndCompute      frame_processing.py:59-61
 *   evh_match_knn2_l2u8           DescriptorMatcher("BruteForce").knnMatch(q,t,2)   matching.py:102-108
 *   evh_ratio_unique_filter       lowes_ratio_test + filter_corresponding_points +
 *                                 remove_double_matching                 matching.py:112-119,166-239; utils.py:41-68
 *   evh_superposition_scan        utils.superposition_dict / matrix_superposition   utils.py:118-145,184-211
 *   evh_transform_points          from_original_to_fix / from_fix_to_original       fixed_coordinate_system.py:19-122
 *   evh_find_homography_ransac    cv2.findHomography(a,b,cv2.RANSAC,3.0) matching.py:156-157; utils.py:356-358
 *   evh_static_filter             find_point_displacement + get_largest_group_points   utils.py:258-325
 *   evh_remove_double_matching    utils.remove_double_matching           frame_processing.py:102-104; utils.py:41-68
 *   evh_sift_detect_batch         cv2.xfeatures2d.SIFT_create().detectAndCompute   frame_processing.py:62-64
 *   evh_surf_detect_batch         cv2.xfeatures2d.SURF_create(extended=1, hessianThreshold=400).detectAndCompute   frame_processing.py:65-67
 *   evh_match_knn2_l2f32          knnMatch on float32[N,128] descriptors            matching.py:102-108
 *   evh_*_homography_batch_types  concatenate_all_features_types over a type list   frame_processing.py:91-104
 *   evh_yuv420_to_bgr             the yuv420p -> bgr24 conversion inside cv2.VideoCapture.read()   video_processing.py:58,70
 *   evh_*_yuv420                  capture.read() + imutils.resize + the entry of the same name without the suffix
 *   evh_warp_fixed_plane[_yuv420] stabilize_view / initialize_background: a frame placed on the fixed plane
 *                                 visualization/stabilization.py:129-172, 220-249
 *   evh_warp_ray_surface[_yuv420] no counterpart: the cylindrical coordinate system the reference's known-issues.md names as the way
 *                                 past camera rotations above 90 degrees -- frames placed on a cylinder, a sphere or a plane of rays
 *   evh_steady_frames[_yuv420]    no counterpart (create_video_comparison shows a frame sliding over a canvas): the video itself on a
 *                                 smoothed camera path, every output picture from its frame and, at the borders, its neighbours
 *   evh_blend_fixed_plane[_yuv420], evh_blend_ray_surface[_yuv420] no counterpart: the mosaic with feathered seams (or the frame
 *                                 nearest its centre per pixel) and per-frame exposure gains, on the plane or on a surface
 *   evh_seam_labels_*, evh_blend_bands_*[_yuv420] no counterpart: multi-band blending of that mosaic under a label mask
 *   evh_pair_exposure[_yuv420]    no counterpart: the overlap sums from which those gains are solved
 *   evh_trail_fixed_plane[_yuv420] stabilize_view with decrease_brightness and change_frame_location: earlier frames dimmed,
 *                                 the frame outlined            visualization/stabilization.py:21-97, 129-172
 *   evh_plate_fixed_plane[_yuv420] no counterpart: the "video motion segmentation" the reference's known-issues.md considers --
 *                                 the temporal median of the registered frames (a background plate) and a moving-object mask per frame
 *   evh_rows_moving_filter[_yuv420] no counterpart: match rows whose points differ from that plate are dropped before the final
 *                                 solve (known-issues.md: key points cling to what moves)
 *   evh_mask_components           no counterpart: the connected components of those masks, with box, area and centre sums
 *   evh_heatmap_render            heatmap_frame_processing without part_line: colour index, table, blend
 *                                 visualization/processing_visualization.py:336-344
 *   evh_batch_static_info         the length of the static point lists that reach draw_matches   video_processing.py:69
 *   evh_batch_static_rows         concatenate_all_features_types' two point lists as draw_matches gets them   video_processing.py:69,78-80
 *   evh_draw_matches              draw_matches + imwrite: matching_vis_{i}.png   video_processing.py:78-81,
 *                                 visualization/processing_visualization.py:22-57
 *   evh_pair_residual[_yuv420]    no counterpart: the measure of a matrix the reference's known-issues.md lacks ("Error",
 *                                 "N/A coordinates"): the motion-compensated residual of a pair of frames
 *   evh_pair_refine[_yuv420]      no counterpart: that matrix improved on the pixels of the pair (direct alignment)
 *   evh_canvas_refine[_yuv420]    no counterpart: a frame aligned against the mosaic its predecessors left on the plane, so that
 *                                 revisited ground pulls the chain of pair matrices back into place
 *   evh_track_points[_yuv420], evh_track_seeds[_yuv420] no counterpart: the second source of correspondences the reference's
 *                                 known-issues.md lacks ("H=None": the 4 points can't be found) -- well-conditioned points of a frame
 *                                 followed into the previous one by pyramidal Lucas-Kanade, as (ax, ay, bx, by) rows
 *   evh_graph_normal              no counterpart: the normal equations of ONE least-squares problem over all superposed matrices, from
 *                                 the match rows of any frame pairs, so that a loop's closing error is spread over the whole chain
 *   evh_jpeg_encode, evh_jpeg_header, evh_jpeg_bound   cv2.imwrite of every picture the reference writes: baseline JPEG files of
 *                                 the canvases, encoded where they lie, so that only compressed bytes leave the device
 *                                 visualization/stabilization.py:286
 *   evh_pair_homography_batch     the per-pair body of get_homography_dict video_processing.py:67-105
 *                                 (FrameProcessing.concatenate_all_features_types frame_processing.py:73-108
 *                                  + compute_homography utils.py:328-363 + matrix_superposition utils.py:118-145)
 *
 * Conventions: extern "C", plain pointers and sizes, int return (0 = EVH_SUCCESS, <0 = error; the message is
 * available from evh_last_error_string), never throws.  Pointers named d_* are DEVICE pointers (hipMalloc /
 * torch.Tensor.data_ptr()); pointers named h_* are host pointers.  One context is used from one host thread
 * at a time; multi-GPU = one context (one process) per device.  All work is enqueued on the context's HIP
 * stream; entry points that fill h_* outputs synchronise that stream before returning, the others do not.
 */
#ifndef EVHIP_H
#define EVHIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct evh_ctx evh_ctx;

enum {
  EVH_SUCCESS = 0,
  EVH_ERR_INVALID = -1,   /* bad argument                          */
  EVH_ERR_HIP = -2,       /* a HIP runtime call failed             */
  EVH_ERR_CAPACITY = -3,  /* exceeds the sizes given to evh_create */
  EVH_ERR_UNSUPPORTED = -4
};

/* per-pair status (out_status); mirrors the reference's failure list:
 *  1 matching.py:104-107 descriptors None   2 matching.py:113 fewer than 4 matches
 *  3 matching.py:158 provisional H None     4 utils.py:359 inlier ratio < 0.7     5 utils.py:361 H None
 *  6 an internal fixed-capacity list overflowed for this frame (never silently truncated)             */
enum {
  EVH_PAIR_OK = 0,
  EVH_PAIR_NO_DESCRIPTORS = 1,
  EVH_PAIR_FEW_MATCHES = 2,
  EVH_PAIR_NO_PROVISIONAL_H = 3,
  EVH_PAIR_LOW_INLIER_RATIO = 4,
  EVH_PAIR_NO_FINAL_H = 5,
  EVH_PAIR_CAPACITY = 6
};

enum { EVH_MODE_INDEPENDENT_PAIRS = 0, EVH_MODE_STREAM = 1 };

/* ---- context ------------------------------------------------------------------------------------------------ */
/* stream: a hipStream_t to enqueue on, or NULL to let the context create its own non-blocking stream.          */
/* 64 <= max_w, max_h < 4096; 2 <= max_frames <= 65528 (frames are a grid dimension); else EVH_ERR_INVALID.    */
/* A working frame may be smaller than 64 x 64, down to 2 x 2: a side of 1 leaves pyramid levels 6 and 7 without */
/* pixels, and every entry that detects refuses it with EVH_ERR_UNSUPPORTED.                                    */
int evh_create(int device, int max_w, int max_h, int max_features, int max_frames, void* stream, evh_ctx** out);
void evh_destroy(evh_ctx* ctx);
const char* evh_last_error_string(const evh_ctx* ctx); /* ctx may be NULL: last error of evh_create */
void* evh_stream(const evh_ctx* ctx);                  /* the hipStream_t all kernels are launched on */
int evh_synchronize(evh_ctx* ctx);                     /* waits for the main AND the solve stream */
int evh_version(void);
/* Asynchronous solve (default off): the RANSAC kernels of evh_pair_homography_batch / evh_stream_homography_batch
 * are enqueued on a second, context-owned stream behind an event, so that they overlap the NEXT batch's detect
 * kernels (they are latency-bound and occupy one wave per SIMD).  d_H / d_status are then complete only after
 * evh_synchronize(), or on a stream that has called evh_solve_wait (stream = NULL: the context's main stream). */
int evh_set_async_solve(evh_ctx* ctx, int on);
int evh_solve_wait(evh_ctx* ctx, void* stream);

/* ---- per-stage device timing (measurement aid, used by bench.py) ------------------------------------------- */
/* When enabled, every kernel group launched by the entry points below is bracketed by a pair of hipEvents on
 * the context's stream.  evh_profile_read synchronises the stream, returns for each stage the number of
 * bracketed launches-groups and their summed device time in milliseconds since the last read, and resets.
 * Stage order: gray, pyramid, fast, select, describe, knn2, filter, ransac_static, ransac_final.           */
#define EVH_NSTAGES 9
int evh_profile_enable(evh_ctx* ctx, int on);
int evh_profile_read(evh_ctx* ctx, float* h_total_ms /*[EVH_NSTAGES]*/, int* h_counts /*[EVH_NSTAGES]*/);
const char* evh_profile_stage_name(int stage);

/* ---- K0: imutils.resize -> cv2.resize(INTER_AREA): area sums when shrinking, the operator's bilinear emulation
 * when enlarging (resize_width > frame width), identity = copy ------------------------------------------------- */
/* nimg images of sh x sw x cn uint8 (row stride src_stride bytes, image stride src_img_stride bytes).          */
/* Stream-ordered like every other entry: the result is complete after evh_synchronize() (or on the context's    */
/* stream); a call whose geometry differs from the previous resize or fused ingest drains the stream once.     */
int evh_resize_area_u8(evh_ctx* ctx, const uint8_t* d_src, int nimg, int sw, int sh, int cn, int64_t src_stride,
                       int64_t src_img_stride, uint8_t* d_dst, int dw, int dh, int64_t dst_stride,
                       int64_t dst_img_stride);

/* BGR convenience form of the same call (one image): cn = 3, tight rows.                                        */
int evh_resize_area_u8c3(evh_ctx* ctx, const uint8_t* d_src, int sw, int sh, uint8_t* d_dst, int dw, int dh);

/* ---- N3: fixed-plane coordinate field of the heat-map (processing_visualization.py:407-408,419) ------- */
/* For each of n superposed matrices h_Hsup f64[n,9]: (u,v) = H.(x,y,1) for every pixel of a w x h grid, in the
 * arithmetic of np.apply_along_axis(homography_transformation, 2, template, H) (tx = fma(h0, x, h1*y) + h2, then
 * u = tx / tw), and np.max over the grid of (u,v) -- the per-frame value whose maximum over the video is written to
 * metrics_file.txt.  np.max semantics: a NaN anywhere gives NaN (the positive quiet NaN), an all -inf grid gives
 * -inf.  d_field (device, f64[n,h,w,2], may be NULL) receives the field; h_max f64[n] the maxima.  n <= 65535 and
 * w * h <= INT_MAX, else EVH_ERR_CAPACITY.  Synchronises.                                                     */
int evh_fixed_plane_field(evh_ctx* ctx, const double* h_Hsup, int n, int w, int h, double* d_field, double* h_max);

/* ---- N1: the consumers of dict_with_homography_matrix.json ------------------------------------------------ */
/* utils.superposition_dict (utils.py:184-211): h_H f64[n,9] = the per-frame H in frame order -> h_out f64[n,9] the running
 * superposition: out[0] = H[0], out[i] = np.dot(H[i], out[i-1]) / [2][2] (matrix_superposition, utils.py:139-145; with
 * n = 2 it is one matrix_superposition(H[1], H[0], False)).  Sequential scan on the device.  Synchronises.            */
int evh_superposition_scan(evh_ctx* ctx, const double* h_H, int n, double* h_out);
/* fixed_coordinate_system.from_original_to_fix / from_fix_to_original (fixed_coordinate_system.py:19-69, 72-122) and
 * utils.homography_transformation (utils.py:89-92), batched: point i = (x, y) of h_pts f64[n,2] ->
 * np.around(np.dot(M[h_idx[i]], (kx*x, ky*y, 1))[:2] / [2], decimals) into h_out f64[n,2]; h_M f64[nmat,9] holds the
 * superposed H per frame (or, for the inverse direction, their inverses); decimals < 0: no rounding.  Synchronises. */
int evh_transform_points(evh_ctx* ctx, const double* h_M, int nmat, const int32_t* h_idx, const double* h_pts, int n,
                         double kx, double ky, int decimals, double* h_out);

/* ---- K1..K6: ORB detectAndCompute on a batch of frames ------------------------------------------------------- */
/* channels: 1 (gray) or 3 (BGR, converted like cvtColor(BGR2GRAY)).  Results stay resident in the context
 * (frame slots 0..nframes-1) until the next call.                                                              */
int evh_orb_detect_batch(evh_ctx* ctx, const uint8_t* d_frames, int nframes, int w, int h, int channels,
                         int64_t row_stride, int64_t frame_stride, int nfeatures);
/* FAST threshold lifting (default on): the exact corner score is only evaluated for pixels that can reach the
 * per-(frame, level) score that ORB's retainBest(2*quota) will cut at; keypoints and descriptors are identical
 * either way (a level that comes up short is redone at threshold 20).  With lifting off the candidate lists
 * returned by evh_orb_download_candidates hold every FAST corner at threshold 20.                          */
int evh_set_fast_lift(evh_ctx* ctx, int on);
/* Order (and, with ties at the cut, the set) in which ORB's KeyPointsFilter::retainBest leaves a level's key points --
 * frame_processing.py:59-61 cv2.ORB_create().detectAndCompute; OpenCV 3.4.2 features2d/src/keypoint.cpp:
 *     std::nth_element(begin, begin + n, end, greater-response); amb = kp[n - 1].response;
 *     std::partition(begin + n, end, response >= amb)
 * EVH_ORDER_OPENCV (default): the permutation libstdc++'s introselect / partition leave on the row-major list of a level's
 *   FAST corners -- what the reference's run produces; the order of the matches, and through it the minimal samples RANSAC
 *   draws, follow from it (pinned by the reference's dict_with_homography_matrix.json, tests/test_capture_golden.py).
 *   Needs every corner at threshold 20, so FAST threshold lifting does not apply.
 * EVH_ORDER_CANONICAL: every tie at the cut kept, key points in (level, y, x) order (rounds 1-3); faster (lifting applies),
 *   H agrees with the reference only where RANSAC's consensus does not depend on the draw. */
enum { EVH_ORDER_CANONICAL = 0, EVH_ORDER_OPENCV = 1 };
/* The 8x8 linear systems of findHomography's Levenberg-Marquardt refinement (matching.py:156-157, utils.py:356-358 ->
 * cv::findHomography -> LMSolver -> cv::solve(DECOMP_EIG)).
 * EVH_SOLVER_EXACT (default): the operator's own Jacobi eigen-solve, rotation by rotation in its order -- H bit-identical to the
 *   CPU restatement.
 * EVH_SOLVER_EXACT (default) also means: the operator's bit-exact result on the reference's own video (all 120 recorded matrices).
 * EVH_SOLVER_FAST ("tolerance mode"): after RANSAC -- whose random draw, hypotheses and inlier masks stay exact, so statuses are
 *   identical -- (1) LM's 8x8 systems by LDL^T (a non-positive pivot falls back to the exact path), (2) the sums of the refit and
 *   of the LM evaluations by per-lane partial sums and a tree instead of the operator's point order, (3) the refit itself by the
 *   inhomogeneous least-squares solution with h33 = 1 in the normalised frame (one 8x8 LDL^T; the eigen-solve when a
 *   pivot is not above 1e-10 of its diagonal entry -- h33 ~ 0 there, e.g. a horizon through the centroid -- or |h| >= 1e12) --
 *   it only seeds LM.  A stream pair costs 2.5-3x less (bench.py --config 3: 2.0 k -> 5.8 k pairs/s; the reference's default
 *   detector list at 400x224: 0.85 k -> 1.8 k), but H is no longer OpenCV's to the digit: the systems are graded over 14 orders
 *   of magnitude (raw pixel coordinates), the loop is cut after 10 iterations, and where the data do not determine H the end
 *   points differ -- measured over 140 pairs: frame corners up to 5.3e-4 px, SURVEY 8d's floored-relative h_err up to 2.5e-3
 *   (tests/test_gpu_parity.py::test_fast_solver_mode; bars 5e-3 px / 2e-2).  For callers who need the geometry, not the
 *   operator's digits. */
enum { EVH_SOLVER_EXACT = 0, EVH_SOLVER_FAST = 1 };
int evh_set_solver_mode(evh_ctx* ctx, int mode);
int evh_get_solver_mode(const evh_ctx* ctx);
/* largest max_features evh_create accepts (the matching filter keeps five lists of a frame slot's rows in LDS) */
#define EVH_MAX_FEATURES 5984
int evh_set_keypoint_order(evh_ctx* ctx, int mode);
int evh_get_keypoint_order(const evh_ctx* ctx);
/* The pair / stream entries below additionally let the second frame of a pair -- every other frame of a stream --
 * borrow the sampled score histogram of the frame before it (default on): consecutive video frames look alike, and
 * a threshold that proves too high is redone at 20 like any other, so results never change.  Turn it off for
 * batches of UNRELATED frame pairs, where the borrowed threshold is often wrong and the redo costs more than the
 * sampling it saves.  evh_orb_detect_batch itself always samples every frame.                                */
int evh_set_fast_share(evh_ctx* ctx, int on);
/* A context also carries, per pyramid level, the lower quartile of the lifted thresholds of its previous detect call as
 * a hint for the next call's sampling pass (lifted instead of dense scoring of the sampled tiles; default on, results
 * never change).  Off = every call samples densely, as a context's first call does.                            */
int evh_set_fast_hint(evh_ctx* ctx, int on);
/* number of keypoints of a frame slot, or <0 */
int evh_orb_count(evh_ctx* ctx, int frame);
/* capacity (rows) a caller must provide to evh_orb_download */
/* N2, fused ingest: the same detect on frames of src_w x src_h that the reference would first shrink with
 * imutils.resize(frame, width=w) (video_processing.py:62,73): level 0 is produced straight from the full-size frame
 * (INTER_AREA per channel, rounded to uint8 as the resized image would be, then the gray weights) -- the resized BGR
 * image is never materialised.  (w, h) is the working size: h = int(src_h * (w / float(src_w))); it may
 * also be LARGER than the source (resize_width > frame width: INTER_AREA's bilinear emulation).                       */
int evh_orb_detect_batch_resized(evh_ctx* ctx, const uint8_t* d_frames, int nframes, int src_w, int src_h, int channels,
                                 int64_t row_stride, int64_t frame_stride, int w, int h, int nfeatures);
int evh_orb_capacity(const evh_ctx* ctx);
/* copies one frame's features to HOST arrays (any pointer may be NULL): xy f32[n,2] (level-0 pixels, what
 * the reference keeps from kp.pt), desc u8[n,32], octave i32[n], lxy i32[n,2] (level coordinates),
 * response f32[n], angle f32[n] (degrees).  Returns n. Canonical order: (octave, y, x).                      */
int evh_orb_download(evh_ctx* ctx, int frame, float* h_xy, uint8_t* h_desc, int32_t* h_octave, int32_t* h_lxy,
                     float* h_response, float* h_angle);
/* single-frame convenience form of detectAndCompute (frame_processing.py:60-61): one device frame in (tight
 * rows: row_stride = w * channels), features to HOST arrays sized evh_orb_capacity() rows (any may be NULL),
 * number of key points in *h_count.  Equivalent to evh_orb_detect_batch(nframes = 1) + evh_orb_download(0).   */
int evh_orb_detect_compute(evh_ctx* ctx, const uint8_t* d_frame, int w, int h, int channels, int nfeatures,
                           float* h_xy, uint8_t* h_desc, int32_t* h_octave, int* h_count);
/* test/inspection hooks: pyramid level geometry + contents, FAST candidates (packed score<<24|y<<12|x) */
int evh_orb_level_info(const evh_ctx* ctx, int level, int* w, int* h, int* quota, float* scale);
int evh_orb_download_level(evh_ctx* ctx, int frame, int level, uint8_t* h_pixels /* h*w tight */);
int evh_orb_download_candidates(evh_ctx* ctx, int frame, int level, uint32_t* h_packed, int cap);

/* ---- K7: brute-force 2-NN, L2 over the 32 descriptor bytes (squared distances, exact integers) --------------- */
/* d_idx i32[nq,2] (-1 = missing neighbour), d_d2 u32[nq,2].  Ties -> lowest train index.                      */
int evh_match_knn2_l2u8(evh_ctx* ctx, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int32_t* d_idx,
                        uint32_t* d_d2);
/* the same on 128-byte rows: SIFT's descriptor values (0..255 each, held by the operator as float32; its float sums of
 * squared differences are exact integers).  Squared distances up to 8 323 200: neighbours are compared AFTER sqrt in
 * float32 like the operator does (two different D above 2^22 can round to the same distance and then tie).          */
int evh_match_knn2_l2u8x128(evh_ctx* ctx, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int32_t* d_idx,
                            uint32_t* d_d2);
int evh_match_knn2_hamming(evh_ctx* ctx, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int32_t* d_idx,
                           uint32_t* d_d2);
/* ratio test (d0 < d1*ratio on f32 sqrt distances, evaluated in f64), one-to-one filter, duplicate-coordinate
 * filter.  d_pts f32[nq,4] receives (ax, ay, bx, by) rows; h_count the number of rows; h_status 0 or
 * EVH_PAIR_FEW_MATCHES.  a = query (current frame), b = train (previous frame).                              */
int evh_ratio_unique_filter(evh_ctx* ctx, const int32_t* d_idx, const uint32_t* d_d2, int nq, int nt,
                            const float* d_xy_q, const float* d_xy_t, double ratio, int min_matches, float* d_pts,
                            int* h_count, int* h_status);

/* ---- K8/K9: findHomography(RANSAC) ---------------------------------------------------------------------------- */
/* d_pts f32[n,4] rows (ax, ay, bx, by): H maps a -> b.  h_H f64[9], h_mask u8[n] (may be NULL),
 * h_found 0/1, h_info i32[3] = {ransac iterations, best inlier count, LM iterations} (may be NULL).           */
int evh_find_homography_ransac(evh_ctx* ctx, const float* d_pts, int n, double thr, int max_iters, double conf,
                               double* h_H, uint8_t* h_mask, int* h_found, int* h_info);
/* The same with the iteration bound held fixed: exactly max(max_iters, 1) accepted samples are evaluated (the
 * adaptive bound RANSACUpdateNumIters is not applied).  This is the force_max_iters mode of the fused entries below
 * -- the fixed-iteration workload of BASELINE.json configs[2] -- exposed for one point set.                       */
int evh_find_homography_ransac_fixed(evh_ctx* ctx, const float* d_pts, int n, double thr, int max_iters, double conf,
                                     double* h_H, uint8_t* h_mask, int* h_found, int* h_info);
/* find_point_displacement + get_largest_group_points: rows of the most populated rounded-displacement bin */
int evh_static_filter(evh_ctx* ctx, const double* h_H, const float* d_pts, int n, float* d_out_pts, int* h_count);
/* remove_double_matching (utils.py:41-68) on n rows (ax, ay, bx, by): one row per distinct (ax, ay), in the order of
 * first occurrence, with the (bx, by) of the key's LAST occurrence; +0.0 and -0.0 are the same key and the first
 * occurrence's bits are kept.  This is the merge stage of the *_types entries (frame_processing.py:102-104) run on
 * caller rows.  d_pts, d_out f32[n,4], 16-byte aligned, must not overlap (EVH_ERR_INVALID); h_count the number of rows written; rows of
 * d_out past h_count are left untouched.  n = 0 gives 0 rows; n > 196 605 (three feature types of 65 535 rows each, the
 * largest concatenation of a multi-type pair) is EVH_ERR_CAPACITY.  Synchronises.                                    */
int evh_remove_double_matching(evh_ctx* ctx, const float* d_pts, int n, float* d_out, int* h_count);

/* ---- fused batch entry: frames -> H -------------------------------------------------------------------------------- */
/* mode EVH_MODE_INDEPENDENT_PAIRS: 2*npairs frames laid out (prev0, cur0, prev1, cur1, ...), H_sup = None.
 * mode EVH_MODE_STREAM: npairs+1 consecutive frames, reference stream semantics (running superposition,
 * none_H_processing=True: a failed pair repeats the previous H; a failed FIRST pair gets NaNs + its status).
 * d_H f64[npairs,9] and d_status i32[npairs] are device buffers. Does not synchronise.                        */
int evh_pair_homography_batch(evh_ctx* ctx, const uint8_t* d_frames, int npairs, int mode, int w, int h,
                              int channels, int64_t row_stride, int64_t frame_stride, int nfeatures,
                              double ransac_thr, int ransac_max_iters, double ransac_conf, int force_max_iters,
                              double* d_H, int32_t* d_status);
/* Stream form with explicit carry-over so that a long video can be processed in chunks: nframes consecutive
 * frames -> nframes-1 pairs.  d_state_in: f64[18] = {H_sup(9), H_prev(9)} leaving the previous chunk, or NULL for
 * the first chunk of a stream; d_state_out: f64[18] receives the state after the last pair (may be NULL).
 * Consecutive chunks overlap by one frame.  Does not synchronise.                                              */
int evh_stream_homography_batch(evh_ctx* ctx, const uint8_t* d_frames, int nframes, int w, int h, int channels,
                                int64_t row_stride, int64_t frame_stride, int nfeatures, double ransac_thr,
                                int ransac_max_iters, double ransac_conf, int force_max_iters,
                                const double* d_state_in, double* d_state_out, double* d_H, int32_t* d_status);
/* The stream form on full-size frames with the reference's resize_width fused in (see evh_orb_detect_batch_resized):
 * what get_homography_dict(capture, resize_width=w) runs per chunk.                                               */
int evh_stream_homography_batch_resized(evh_ctx* ctx, const uint8_t* d_frames, int nframes, int src_w, int src_h,
                                        int channels, int64_t row_stride, int64_t frame_stride, int w, int h,
                                        int nfeatures, double ransac_thr, int ransac_max_iters, double ransac_conf,
                                        int force_max_iters, const double* d_state_in, double* d_state_out,
                                        double* d_H, int32_t* d_status);
/* Several independent streams in one batch: d_frames holds nstreams x frames_per_stream frames, stream-major
 * (all frames of stream 0, then stream 1, ...).  Everything up to the static filter runs over all frames / pairs
 * at once; the sequential scans of the streams then run concurrently, one wavefront per stream, each with its own
 * {H_sup, H_prev}: d_state_in / d_state_out f64[nstreams][18] (d_state_in NULL = every stream starts here).
 * d_H f64[nstreams][frames_per_stream-1][9], d_status i32[nstreams][frames_per_stream-1].  Per stream the results
 * are bit-identical to evh_stream_homography_batch on that stream alone.  Does not synchronise.                 */
int evh_multi_stream_homography_batch(evh_ctx* ctx, const uint8_t* d_frames, int nstreams, int frames_per_stream,
                                      int w, int h, int channels, int64_t row_stride, int64_t frame_stride,
                                      int nfeatures, double ransac_thr, int ransac_max_iters, double ransac_conf,
                                      int force_max_iters, const double* d_state_in, double* d_state_out,
                                      double* d_H, int32_t* d_status);
/* Two-phase form of the stream path, for sharding ONE stream over several GPUs with the reference's semantics
 * (video_processing.py:67-105).  Phase 1 is independent per pair and runs wherever the frames are:
 * detect, match, ratio/unique filter, RANSAC #1, static filter (frame_processing.py:91-98, matching.py:131-163) on
 * nframes consecutive frames -> nframes-1 pairs; it leaves per pair the static rows f32[row_cap,4] (ax,ay,bx,by),
 * their count and the phase-1 status (EVH_PAIR_*) in CALLER device buffers; row_cap must equal evh_orb_capacity().
 * Phase 2 is the sequential part (compute_homography with the running superposition, utils.py:328-363, and
 * matrix_superposition, utils.py:118-145): it scans npairs pairs (any number -- rows gathered from all shards) in
 * stream order from d_state_in (f64[18] {H_sup, H_prev} or NULL at the start of the stream) and writes H f64[9] and
 * the final status per pair, plus the state after the last pair.  Running phase 1 on blocks that overlap by one
 * frame and phase 2 once over the concatenated rows gives bit-identical results to evh_stream_homography_batch on
 * the whole stream.  Neither call synchronises.                                                                  */
int evh_stream_static_batch(evh_ctx* ctx, const uint8_t* d_frames, int nframes, int w, int h, int channels,
                            int64_t row_stride, int64_t frame_stride, int nfeatures, double ransac_thr,
                            int ransac_max_iters, double ransac_conf, int force_max_iters, float* d_rows, int row_cap,
                            int32_t* d_counts, int32_t* d_status1);
int evh_stream_scan(evh_ctx* ctx, const float* d_rows, int row_cap, const int32_t* d_counts, const int32_t* d_status1,
                    int npairs, double ransac_thr, int ransac_max_iters, double ransac_conf, int force_max_iters,
                    const double* d_state_in, double* d_state_out, double* d_H, int32_t* d_status);
/* the same per-pair body starting from features already resident in the context (frame slots): used by the
 * Python FrameProcessing/KeyPoints mirror.  cur/prev are frame slots of the last evh_orb_detect_batch.
 * h_Hsup: f64[9] or NULL.  h_H f64[9]; returns the pair status in *h_status.                                 */
int evh_pair_from_slots(evh_ctx* ctx, int cur_slot, int prev_slot, const double* h_Hsup, double* h_H,
                        int* h_status);
/* KeyPoints.match_static_kps on resident slots: static point rows to host, f32[n,4].                          */
int evh_match_static_from_slots(evh_ctx* ctx, int cur_slot, int prev_slot, float* h_pts, int cap, int* h_count,
                                int* h_status);
/* compute_homography (utils.py:328-363) on host point rows f32[n,4] */
int evh_compute_homography(evh_ctx* ctx, const float* h_pts, int n, const double* h_Hsup, double* h_H,
                           int* h_status);

/* ---- N4: SIFT and the reference's multi-type pairs --------------------------------------------------------- */
/* feature types of frame_processing.py:59-67; a list is processed in its own order (reference default: SURF, SIFT, ORB) */
enum { EVH_FEATURE_ORB = 0, EVH_FEATURE_SIFT = 1, EVH_FEATURE_SURF = 2 };
/* Reserves the SIFT buffers of a context: max_sift_features key points per frame slot (SIFT_create() keeps every key
 * point -- 2 500 on a textured 400x224 frame), the float scale space of a group of frames.  Call once, before the entries
 * below.  A frame that delivers more is flagged: its pairs get EVH_PAIR_CAPACITY, evh_sift_count / _download fail.
 * Up to 65 535 per frame in the *_types entries (beyond 7 680 their matching filter works in global memory).         */
int evh_sift_enable(evh_ctx* ctx, int max_sift_features);
int evh_sift_capacity(const evh_ctx* ctx);
/* cv2.xfeatures2d.SIFT_create().detectAndCompute(frame, None) (frame_processing.py:62-64) on a batch of frames of
 * src_w x src_h, working size (w, h) as in evh_orb_detect_batch_resized (equal sizes = no resize).  Results stay
 * resident (frame slots 0..nframes-1).  OpenCV 3.4.2 defaults: 3 layers per octave, contrast 0.04, edge 10, sigma 1.6. */
int evh_sift_detect_batch(evh_ctx* ctx, const uint8_t* d_frames, int nframes, int src_w, int src_h, int channels,
                          int64_t row_stride, int64_t frame_stride, int w, int h);
int evh_sift_count(evh_ctx* ctx, int frame);
/* one frame's key points to HOST arrays (any may be NULL), in the operator's own order (removeDuplicatedSorted: by x,
 * then y, ...): xy f32[n,2], desc f32[n,128] (integer values 0..255 as the operator returns them), octave i32[n] (packed
 * like KeyPoint::octave: octave & 255 | layer << 8 | ...), size, angle (degrees), response.  Returns n.             */
int evh_sift_download(evh_ctx* ctx, int frame, float* h_xy, float* h_desc, int32_t* h_octave, float* h_size,
                      float* h_angle, float* h_response);
/* test / inspection hooks: octave geometry (returns 1 past the last octave) and one Gaussian layer (0..5) of the
 * scale space of a frame of the last detect call (octave 0 = the frame doubled)                                   */
int evh_sift_octave_info(const evh_ctx* ctx, int octave, int* w, int* h);
int evh_sift_download_gauss(evh_ctx* ctx, int frame, int octave, int layer, float* h_pixels /* h*w tight */);
/* SURF: cv2.xfeatures2d.SURF_create(extended=1, hessianThreshold=400).detectAndCompute(frame, None)
 * (frame_processing.py:65-67; OpenCV 3.4.2: 4 octaves x 3 layers, 128-float descriptors, rotation-aware).  Same call
 * shapes as the SIFT entries; hessian_threshold = 400 for the reference.  Key points come in the operator's own order
 * (std::sort by KeypointGreater: response descending); h_laplacian = KeyPoint::class_id (sign of the trace).        */
int evh_surf_enable(evh_ctx* ctx, int max_surf_features);
int evh_surf_capacity(const evh_ctx* ctx);
int evh_surf_detect_batch(evh_ctx* ctx, const uint8_t* d_frames, int nframes, int src_w, int src_h, int channels,
                          int64_t row_stride, int64_t frame_stride, int w, int h, double hessian_threshold);
int evh_surf_count(evh_ctx* ctx, int frame);
int evh_surf_download(evh_ctx* ctx, int frame, float* h_xy, float* h_desc /* f32[n,128] */, float* h_size, float* h_angle,
                      float* h_response, int32_t* h_octave, int32_t* h_laplacian);
/* test hook: the integral image (h+1) x (w+1) of a frame of the last SURF call                                      */
int evh_surf_download_integral(evh_ctx* ctx, int frame, int32_t* h_sum);
/* DescriptorMatcher("BruteForce").knnMatch(q, t, 2) on FLOAT descriptors (matching.py:102-108 with the float32[N,128]
 * rows of SIFT / SURF; dim = 64 or 128): d_idx i32[nq,2] (-1 = missing neighbour), d_dist f32[nq,2] (L2 distances,
 * summed in the operator's order).  Ties -> lowest train index.                                                      */
int evh_match_knn2_l2f32(evh_ctx* ctx, const float* d_q, int nq, const float* d_t, int nt, int dim, int32_t* d_idx,
                         float* d_dist);
/* evh_ratio_unique_filter on the float distances of evh_match_knn2_l2f32                                             */
int evh_ratio_unique_filter_f32(evh_ctx* ctx, const int32_t* d_idx, const float* d_dist, int nq, int nt,
                                const float* d_xy_q, const float* d_xy_t, double ratio, int min_matches, float* d_pts,
                                int* h_count, int* h_status);
/* The fused entries with a LIST of feature types (h_types: EVH_FEATURE_*, ntypes entries, processed in list order), i.e.
 * FrameProcessing(frame, features_type_list).concatenate_all_features_types (frame_processing.py:91-104): per type
 * detect + match + RANSAC #1 + static filter, the static rows of all types concatenated, remove_double_matching again,
 * then compute_homography.  A type that fails (NoMatchesException) fails the pair with its status.  (src_w, src_h) /
 * (w, h) as in evh_stream_homography_batch_resized.  Needs evh_sift_enable / evh_surf_enable (BEFORE the first such call)
 * when the list holds SIFT / SURF.  Do not synchronise.                                                                */
int evh_pair_homography_batch_types(evh_ctx* ctx, const uint8_t* d_frames, int npairs, int mode, int src_w, int src_h,
                                    int channels, int64_t row_stride, int64_t frame_stride, int w, int h, int nfeatures,
                                    const int32_t* h_types, int ntypes, double ransac_thr, int ransac_max_iters,
                                    double ransac_conf, int force_max_iters, double* d_H, int32_t* d_status);
int evh_stream_homography_batch_types(evh_ctx* ctx, const uint8_t* d_frames, int nframes, int src_w, int src_h,
                                      int channels, int64_t row_stride, int64_t frame_stride, int w, int h, int nfeatures,
                                      const int32_t* h_types, int ntypes, double ransac_thr, int ransac_max_iters,
                                      double ransac_conf, int force_max_iters, const double* d_state_in,
                                      double* d_state_out, double* d_H, int32_t* d_status);

/* ---- decoded 4:2:0 planes as the source (video_processing.py:58,70: what capture.read() converts to BGR) ---------------- */
/* One description for every common 8-bit 4:2:0 layout.  Luma is w x h, both chroma planes are ((w+1)/2) x ((h+1)/2) (odd
 * sizes are legal); the chroma sample of luma pixel (x, y) is (x >> 1, y >> 1).  I420 / YV12: c_pixel_stride = 1, three
 * planes.  NV12: c_pixel_stride = 2 and d_cr = d_cb + 1 (NV21: d_cb = d_cr + 1).  All pointers are DEVICE pointers, strides
 * are in bytes.  A packed I420 frame [w*h | cw*ch | cw*ch] is y_stride = w, c_stride = cw, both frame strides =
 * w*h + 2*cw*ch.  Refused with EVH_ERR_INVALID: a NULL plane, c_pixel_stride other than 1 or 2, a stride smaller than
 * the row / frame it steps over.                                                                                        */
typedef struct evh_yuv420 {
  const uint8_t* d_y;
  const uint8_t* d_cb;
  const uint8_t* d_cr;
  int64_t y_stride, c_stride;               /* row strides                                  */
  int64_t y_frame_stride, c_frame_stride;   /* frame strides (ignored when nframes == 1)    */
  int32_t c_pixel_stride;                   /* 1 (planar) or 2 (interleaved chroma)         */
} evh_yuv420;
/* The BGR bytes cv2.VideoCapture.read() hands to video_processing.py:58,70 for a decoded picture: libswscale's unscaled
 * yuv420p -> bgr24 converter as an x86-64 build computes it (EVCAP_BGR_SWSCALE_X86 of include/evcap.h; BT.601 limited
 * range, 13-bit coefficients), per pixel with arithmetic shifts:
 *     Y = (((y << 3) - 128) * 9539) >> 16;  cu = (u << 3) - 1024;  cv = (v << 3) - 1024
 *     B = sat8(Y + ((cu * 16525) >> 16));  G = sat8(Y + ((cu * -3209) >> 16) + ((cv * -6660) >> 16));  R = sat8(Y + ((cv * 13075) >> 16))
 * nframes frames of w x h -> packed BGR at d_bgr (rows of w*3 bytes at row_stride, frames at frame_stride; bytes between
 * rows are not written).  Does not synchronise.
 * Speed, not results, depends on alignment: the converter (and level 0 of evh_*_yuv420 when (w, h) == (src_w, src_h)) moves
 * 16 bytes per load / store when d_y, y_stride, d_bgr and row_stride are multiples of 16 and the chroma side is too --
 * planar: d_cb, d_cr, c_stride multiples of 8; interleaved: the lower of d_cb / d_cr (they must be adjacent bytes) and
 * c_stride multiples of 16 -- together with the frame strides when nframes > 1; anything else takes a bytewise form of the
 * same kernel.  The resizing ingests read single bytes and have no such requirement.                                    */
int evh_yuv420_to_bgr(evh_ctx* ctx, const evh_yuv420* src, int nframes, int w, int h, uint8_t* d_bgr, int64_t row_stride,
                      int64_t frame_stride);
/* evh_orb_detect_batch_resized with the planes as the source, fused: level 0 comes straight from the planes (each source
 * pixel converted as above, then INTER_AREA per channel and the gray weights exactly as for BGR frames); neither the
 * full-size BGR frame nor the resized one exists in memory.  (w, h) == (src_w, src_h): no resize.                        */
int evh_orb_detect_batch_yuv420(evh_ctx* ctx, const evh_yuv420* src, int nframes, int src_w, int src_h, int w, int h,
                                int nfeatures);
/* evh_stream_homography_batch_resized on that ingest: what get_homography_dict runs per chunk of a capture that delivers
 * planes (half the bytes of BGR over the host link).                                                                     */
int evh_stream_homography_batch_yuv420(evh_ctx* ctx, const evh_yuv420* src, int nframes, int src_w, int src_h, int w, int h,
                                       int nfeatures, double ransac_thr, int ransac_max_iters, double ransac_conf,
                                       int force_max_iters, const double* d_state_in, double* d_state_out, double* d_H,
                                       int32_t* d_status);
/* evh_stream_homography_batch_types on planes: the chunk is converted once (evh_yuv420_to_bgr) into a workspace the
 * context owns, then takes the BGR path of every detector in the list.                                                   */
int evh_stream_homography_batch_types_yuv420(evh_ctx* ctx, const evh_yuv420* src, int nframes, int src_w, int src_h, int w,
                                             int h, int nfeatures, const int32_t* h_types, int ntypes, double ransac_thr,
                                             int ransac_max_iters, double ransac_conf, int force_max_iters,
                                             const double* d_state_in, double* d_state_out, double* d_H, int32_t* d_status);

/* ---- stabilised output: frames warped into the fixed plane (stabilization.py:129-172, 220-249) ---------------------------- */
/* What stabilize_view / initialize_background do with a frame and its superposed H -- place it on a canvas of the fixed
 * coordinate system that accumulates the frames -- for nframes frames of sw x sh and their matrices d_M f64[nframes,9] (DEVICE;
 * M maps frame pixels to plane points, as the superposed H does; inverse_map != 0: M maps plane points to frame pixels and is
 * used as it is).  The canvas is dw x dh pixels of the source's channels (the plane form: BGR); canvas pixel (x, y) is the plane
 * point (x + ox, y + oy).  The reference only pastes the frame at int(H.(0,0,1)) (a pure translation: hand in that M, it is
 * reproduced byte for byte); a general M gives the projective warp.
 * Arithmetic, all IEEE float64 with one rounding per operation (no fma):
 *   A = M if inverse_map, else the adjugate of M, each entry one difference of two products (a0 = m4*m8 - m5*m7,
 *   a1 = m2*m7 - m1*m8, a2 = m1*m5 - m2*m4, a3 = m5*m6 - m3*m8, a4 = m0*m8 - m2*m6, a5 = m2*m3 - m0*m5, a6 = m3*m7 - m4*m6,
 *   a7 = m1*m6 - m0*m7, a8 = m0*m4 - m1*m3), not divided by the determinant;
 *   X = (double)(x + ox), Y = (double)(y + oy), the sums formed in int64;
 *   tx = (a0*X + a1*Y) + a2, ty = (a3*X + a4*Y) + a5, tw = (a6*X + a7*Y) + a8;
 *   U = rint(tx / tw * 32), V = rint(ty / tw * 32), halves to even: the source position in 1/32 pixels.
 * Frame k COVERS the pixel iff 0 <= U <= 32*(sw-1) and 0 <= V <= 32*(sh-1), compared in double: a zero, singular, NaN or huge
 * matrix (the stream entries hand out NaN for a failed first pair) and pixels on or beyond the horizon cover nothing and read
 * nothing.  A covered pixel takes, per channel, with sx = U >> 5, fx = U & 31, sy = V >> 5, fy = V & 31,
 *   (p00*(32-fx)*(32-fy) + p01*fx*(32-fy) + p10*(32-fx)*fy + p11*fx*fy + 512) >> 10
 * where a tap of weight 0 is not read (the only way sx + 1 == sw or sy + 1 == sh occurs).  So identity copies the frame and an
 * integer translation is an exact paste.  The five fraction bits are OpenCV's INTER_BITS, but this is NOT
 * cv2.warpPerspective to the byte: that fades the edge taps into its constant border and sums its coordinates block-wise.
 * mode, frames taken in order:
 *   EVH_WARP_EACH     out[k] = frame k over the background;
 *   EVH_WARP_HISTORY  out[k] = frames 0..k over the background, the last covering frame wins (the picture
 *                     create_video_comparison shows for frame k);
 *   EVH_WARP_MOSAIC   one canvas at d_out = all frames over the background (out_frame_stride unused); d_background == d_out
 *                     is allowed in this mode only, so that a canvas is carried from chunk to chunk.
 * d_background: dh rows of dw*channels bytes at out_row_stride, or NULL = zeros.  Every byte of every output row inside
 * dw*channels is written, bytes between rows are not.  Only caller buffers are used: nothing depends on the sizes given to
 * evh_create.  Refused before anything is launched, outputs untouched -- EVH_ERR_INVALID: a NULL pointer, channels not 1 or 3,
 * sw, sh, dw or dh < 1, a stride shorter than its row / frame, an unknown mode, d_background overlapping d_out (except as
 * above); EVH_ERR_CAPACITY: sw or sh >= 2^26, dw*dh > INT_MAX, nframes > 65535.  nframes == 0 succeeds and does nothing.
 * The plane form converts every tap as evh_yuv420_to_bgr does and then interpolates: it equals evh_yuv420_to_bgr followed by
 * the BGR form.  Speed, not results, depends on alignment: d_out, d_background and the output strides multiples of 4 let a
 * thread store its four pixels as words.  Neither entry synchronises.                                                       */
enum { EVH_WARP_EACH = 0, EVH_WARP_HISTORY = 1, EVH_WARP_MOSAIC = 2 };
int evh_warp_fixed_plane(evh_ctx* ctx, const uint8_t* d_frames, int nframes, int sw, int sh, int channels /* 1 | 3 */,
                         int64_t row_stride, int64_t frame_stride, const double* d_M, int inverse_map, int mode,
                         const uint8_t* d_background, uint8_t* d_out, int dw, int dh, int64_t out_row_stride,
                         int64_t out_frame_stride, int ox, int oy);
int evh_warp_fixed_plane_yuv420(evh_ctx* ctx, const evh_yuv420* src, int nframes, int sw, int sh, const double* d_M,
                                int inverse_map, int mode, const uint8_t* d_background, uint8_t* d_out, int dw, int dh,
                                int64_t out_row_stride, int64_t out_frame_stride, int ox, int oy);

/* ---- fixed surfaces: frames warped onto a canvas of viewing rays (cylinder, sphere, plane) ----------------------------------- */
/* evh_warp_fixed_plane's canvas ends at the horizon of a frame's matrix: a camera that turns by 90 degrees runs out of plane.
 * Here canvas pixel (x, y) stands for a viewing ray, not a plane point, and the ray is separable:
 *   ray(x, y) = (a[x], b[y], c[x]),  (a, c) = d_col f64[dw,2] (DEVICE), b = d_row f64[dh] (DEVICE).
 * Rays are projective, so one entry serves every surface the caller tabulates, in double, on the host -- no sin, cos or tan runs
 * on the device:    cylinder  a = sin t, c = cos t, b = v;    sphere (equirectangular)  a = sin t, c = cos t, b = tan p;
 * plane  a = X, c = 1, b = Y.  d_A f64[nframes,9] (DEVICE) maps a ray to homogeneous frame pixels and is used as it is (no
 * adjugate; for a rotating camera A = K . R^T).  Arithmetic, all IEEE float64 with one rounding per operation (no fma), a, c of
 * the pixel's column and b of its row:
 *   tx = (A0*a + A1*b) + A2*c,  ty = (A3*a + A4*b) + A5*c,  tw = (A6*a + A7*b) + A8*c;
 *   U = rint(tx / tw * 32), V = rint(ty / tw * 32), halves to even: the source position in 1/32 pixels.
 * Frame k COVERS the pixel iff tw > 0 and 0 <= U <= 32*(sw-1) and 0 <= V <= 32*(sh-1), all compared in double: NaN fails, so a
 * NaN, zero, infinite or all-negative matrix and a NaN table entry cover nothing and read nothing.  tw > 0 is what a closed
 * surface needs and the plane entry does not have: a ray and its antipode give the same (U, V), and without the sign every
 * frame would appear twice, 180 degrees apart; with it a frame lies on the half of the surface in front of its camera.  A
 * covered pixel takes its bytes exactly as in evh_warp_fixed_plane: sx = U >> 5, fx = U & 31, sy = V >> 5, fy = V & 31,
 *   (p00*(32-fx)*(32-fy) + p01*fx*(32-fy) + p10*(32-fx)*fy + p11*fx*fy + 512) >> 10,  a tap of weight 0 is not read.
 * With the plane's tables and tw > 0 over the canvas the result is evh_warp_fixed_plane's with inverse_map != 0, byte for byte.
 * mode (EVH_WARP_EACH, EVH_WARP_HISTORY, EVH_WARP_MOSAIC), d_background (d_background == d_out for EVH_WARP_MOSAIC only), channels,
 * the plane form, strides, "every byte of every output row inside dw*channels is written, bytes between rows are not", only
 * caller buffers, and the refusals are evh_warp_fixed_plane's -- EVH_ERR_INVALID also for a NULL d_col or d_row; refused before
 * anything is launched, outputs untouched.  The tables are not compared with d_out.  nframes == 0 succeeds and does nothing.
 * Neither entry synchronises.                                                                                                 */
int evh_warp_ray_surface(evh_ctx* ctx, const uint8_t* d_frames, int nframes, int sw, int sh, int channels /* 1 | 3 */,
                         int64_t row_stride, int64_t frame_stride, const double* d_A, const double* d_col, const double* d_row,
                         int mode, const uint8_t* d_background, uint8_t* d_out, int dw, int dh, int64_t out_row_stride,
                         int64_t out_frame_stride);
int evh_warp_ray_surface_yuv420(evh_ctx* ctx, const evh_yuv420* src, int nframes, int sw, int sh, const double* d_A,
                                const double* d_col, const double* d_row, int mode, const uint8_t* d_background, uint8_t* d_out,
                                int dw, int dh, int64_t out_row_stride, int64_t out_frame_stride);

/* ---- the steady view: every output picture from its own ordered list of frames and maps ---------------------------------------- */
/* The products above live on one fixed plane or surface.  A stabilised VIDEO is the input at its own size on a smoother camera
 * path: output picture j is frame k seen through a map of its own, and the wedges that frame leaves uncovered at the borders are
 * filled from its neighbours in time, each through its own map.  So every output picture has its own ordered list of sources:
 *   the frames   nframes frames of sw x sh, gray, BGR or decoded planes, with strides as in evh_warp_fixed_plane;
 *   nout         output pictures of dw x dh pixels of the source's channels (the plane form: BGR);
 *   ntaps        1..16 candidate sources ("taps") per output picture;
 *   d_tap_frame  i32[nout, ntaps] (DEVICE): the tap's frame, an index into the frames of the call;
 *   d_tap_M      f64[nout, ntaps, 9] (DEVICE): the tap's map from output pixel to frame pixel, used as it is (no adjugate, no origin);
 *   feather      F, in 1/32 pixels, 0..8160 (255 pixels);
 *   d_background dh rows of dw*channels bytes at out_row_stride, or NULL = zeros;
 *   d_out        nout pictures at out_frame_stride, dh rows of dw*channels bytes at out_row_stride;
 *   d_tap_of     u8[nout, dh, dw] at tap_of_row_stride / tap_of_frame_stride, or NULL: which tap gave the pixel;
 *   d_counts     u32[nout, ntaps + 1] (DEVICE), or NULL.
 * Arithmetic, all IEEE float64 with one rounding per operation (no fma).  For output picture j, pixel (x, y), tap t with
 * a = d_tap_M[j, t]:  X = (double)x, Y = (double)y, and tx, ty, tw, U, V exactly as evh_warp_fixed_plane forms them with
 * inverse_map != 0:  tx = (a0*X + a1*Y) + a2, ty = (a3*X + a4*Y) + a5, tw = (a6*X + a7*Y) + a8, U = rint(tx / tw * 32),
 * V = rint(ty / tw * 32), halves to even.
 *   1. Tap t is LIVE iff 0 <= d_tap_frame[j, t] < nframes.  Any other value is defined: the tap covers nothing and reads nothing
 *      (its matrix is not looked at either).
 *   2. A live tap COVERS the pixel iff 0 <= U <= 32*(sw-1) and 0 <= V <= 32*(sh-1), compared in double: a NaN, zero or singular
 *      matrix and pixels on or beyond the horizon cover nothing and read nothing.
 *   3. first = the smallest covering t.  None: the pixel takes d_background's bytes, or zeros when that is NULL, and
 *      d_tap_of = 0.  Otherwise the pixel takes v, the bilinear value of frame d_tap_frame[j, first] at (U, V) exactly as in
 *      evh_warp_fixed_plane ((p00*(32-fx)*(32-fy) + ... + 512) >> 10, a tap of weight 0 is not read), and d_tap_of = first + 1.
 *   4. FEATHER, for tap 0 only: when F > 0, first == 0 and d < F, where d = min(U, 32*(sw-1) - U, V, 32*(sh-1) - V) of tap 0 in
 *      int32, its distance to the nearest frame edge in 1/32 pixels.  Let second be the smallest covering t >= 1 and v1 its
 *      bilinear value.  If it exists every channel becomes (v*d + v1*(F - d) + (F >> 1)) / F in unsigned 32-bit integers, the
 *      division rounding down (at most 255 * 8160 + 4080: nothing wraps).  At d = 0 that is v1: the picture is continuous with the
 *      pixel just outside tap 0's frame, which `second` gives as its first tap.  If no second tap covers, the pixel stays v:
 *      nothing is feathered into the background.  d_tap_of stays 1.
 *   5. d_counts[j, 0] = the pixels of picture j no tap covered, d_counts[j, 1 + t] = those first covered by tap t: exact
 *      integers that sum to dw*dh.  The entry zeroes them itself, on its stream, before the launch (d_counts[j, 1] is formed
 *      last, as what the other buckets leave of dw*dh: nearly every pixel of a steady view falls there).
 * What follows: ntaps = 1, d_tap_frame[j] = j, F = 0 is evh_warp_fixed_plane, EVH_WARP_EACH, inverse_map != 0, origin (0, 0), byte
 * for byte; an identity tap copies the frame; taps behind the first covering one matter only inside tap 0's feather band.
 * Every byte of every output row inside dw*channels (d_tap_of: dw) is written, bytes between rows are not.  Only caller buffers are
 * used; on the context's stream, no synchronisation.  The plane form converts every tap as
 * evh_yuv420_to_bgr does and then interpolates: it equals evh_yuv420_to_bgr followed by the BGR form.  Speed, not results,
 * depends on alignment: d_out, d_background and the output strides (d_tap_of and its strides) multiples of 4 let a thread store
 * its four pixels as a word.
 * Refused before anything is launched or zeroed, outputs untouched -- EVH_ERR_INVALID: a NULL source, d_tap_frame, d_tap_M or d_out,
 * channels not 1 or 3, sw, sh, dw or dh < 1, nframes or nout < 0, ntaps outside 1..16, feather outside 0..8160, a stride shorter
 * than its row / frame / picture, d_background, d_tap_of or d_counts overlapping d_out (or one another); EVH_ERR_CAPACITY: sw or
 * sh >= 2^26, dw*dh > INT_MAX, nout > 65535.  nout == 0 succeeds and does nothing.                                              */
int evh_steady_frames(evh_ctx* ctx, const uint8_t* d_frames, int nframes, int sw, int sh, int channels /* 1 | 3 */,
                      int64_t row_stride, int64_t frame_stride, const int32_t* d_tap_frame, const double* d_tap_M, int nout,
                      int ntaps, int feather, const uint8_t* d_background, uint8_t* d_out, int dw, int dh, int64_t out_row_stride,
                      int64_t out_frame_stride, uint8_t* d_tap_of, int64_t tap_of_row_stride, int64_t tap_of_frame_stride,
                      uint32_t* d_counts);
int evh_steady_frames_yuv420(evh_ctx* ctx, const evh_yuv420* src, int nframes, int sw, int sh, const int32_t* d_tap_frame,
                             const double* d_tap_M, int nout, int ntaps, int feather, const uint8_t* d_background, uint8_t* d_out,
                             int dw, int dh, int64_t out_row_stride, int64_t out_frame_stride, uint8_t* d_tap_of,
                             int64_t tap_of_row_stride, int64_t tap_of_frame_stride, uint32_t* d_counts);

/* ---- the blended mosaic: feathered seams and exposure gains, on the plane or on a surface --------------------------------------- */
/* EVH_WARP_MOSAIC gives a canvas pixel to the last frame that covers it: every frame edge stays as a seam, every change of the
 * camera's exposure as a step.  These entries reduce the covering frames otherwise.  The frames, d_M / inverse_map / ox / oy
 * (evh_blend_fixed_plane) or d_A / d_col / d_row (evh_blend_ray_surface), the canvas dw x dh, channels, the strides, the plane
 * forms and d_background are exactly evh_warp_fixed_plane's and evh_warp_ray_surface's, tw > 0 of the ray form included.
 *   mode     EVH_BLEND_FEATHER or EVH_BLEND_SEAM;
 *   feather  F, in 1/32 pixels, 0..65535;
 *   d_gain   u16[nframes][3] (DEVICE), Q12: 4096 is 1.0.  Column c serves channel c, gray uses column 0.  NULL = all 4096.  Any
 *            u16 value is valid;
 *   d_acc    u64[dh][dw][channels + 1] (DEVICE), tight, 8-byte aligned, in and out; may be NULL;
 *   acc_in   non-zero: the state starts from d_acc; zero: from zeros;
 *   d_out    dh rows of dw*channels bytes at out_row_stride; may be NULL: the call then only advances the state.
 * Per canvas pixel the STATE is acc[0 .. cn-1] and acc[cn], unsigned 64-bit.  Frames are taken in order, k = 0 .. nframes-1:
 *   1. Coverage, the position (U, V) and the sample s_c per channel are exactly the warp entry's: positions in 1/32 pixels rounded
 *      half to even, the comparisons in double, the four taps with >> 10, a tap of weight 0 not read; a NaN, singular or
 *      horizon-crossing matrix covers nothing and reads nothing.
 *   2. The WEIGHT of a covering frame, in int32 from the integers U and V: du = min(U, 32*(sw-1) - U), dv = min(V, 32*(sh-1) - V),
 *      d = min(du, dv), w = min(d, F) + 1: the distance to the nearest frame edge, cut at the feather width.  w is never 0, and
 *      F = 0 makes every w equal to 1.
 *   3. With t_c = s_c * g_c (g = d_gain[k]; at most 255 * 65535 < 2^24):
 *      EVH_BLEND_FEATHER  acc[c] += w * t_c, acc[cn] += w;
 *      EVH_BLEND_SEAM     if w > acc[cn]: acc[c] = t_c for every c, acc[cn] = w.  The comparison is strict: among equal weights
 *                         the earliest frame holds, and the first covering frame always takes the pixel.
 *   4. After the last frame the state is stored to d_acc, if given, and if d_out is given, with den = acc[cn]:
 *      den == 0           the pixel takes d_background's bytes, or zeros when that is NULL;
 *      EVH_BLEND_FEATHER  out_c = min(255, (acc[c] + (den << 11)) / (den << 12)), the division rounding down, in u64;
 *      EVH_BLEND_SEAM     out_c = min(255, (acc[c] + 2048) >> 12).
 * BOUNDS, with at most 65535 frames entering one state over all the calls that carry it: w <= 65536 and t_c < 2^24, so acc[c] stays
 * below 2^56, den below 2^32 and den << 12 below 2^44: nothing wraps.  The formulas hold unwrapped for ANY handed-in state with
 * acc[c] < 2^62 and den < 2^44 (a state the entry did not write is the caller's to keep inside these).
 * What follows from the rules: a pixel covered by one frame with gain 4096 holds exactly the warp entry's byte, in both modes and
 * for any F; frames that all show the same value at a pixel blend to that value; d_gain == NULL equals a table of 4096; calls that
 * carry d_acc (acc_in != 0 from the second on) equal one call over all their frames, byte for byte and state for state; the ray
 * form with the plane's tables equals the plane form with inverse_map != 0 wherever tw > 0; the plane forms equal
 * evh_yuv420_to_bgr followed by the BGR forms.
 * Every byte of every output row inside dw*channels is written, bytes between rows are not.  d_background == d_out is allowed (a
 * thread reads only the bytes it writes); d_background is not read when d_out is NULL.  Only caller buffers are used; one launch
 * on the context's stream, no synchronisation.  nframes == 0 succeeds and writes the picture of the incoming state.
 * Refused before anything is launched, outputs untouched -- EVH_ERR_INVALID: everything the warp entries refuse (d_out may be
 * NULL here, its stride then is not looked at), an unknown mode, feather outside 0..65535, d_out and d_acc both NULL, acc_in != 0
 * with d_acc NULL, d_acc not 8-byte aligned, d_acc overlapping any other buffer of the call, d_out overlapping the frames or
 * d_gain, d_background overlapping d_out other than being it; EVH_ERR_CAPACITY: sw or sh >= 2^26, dw*dh > INT_MAX,
 * nframes > 65535.  Speed, not results, depends on alignment: d_acc a multiple of 16 lets a thread move its pixel's state as
 * 128-bit words.                                                                                                                */
enum { EVH_BLEND_FEATHER = 0, EVH_BLEND_SEAM = 1 };
int evh_blend_fixed_plane(evh_ctx* ctx, const uint8_t* d_frames, int nframes, int sw, int sh, int channels /* 1 | 3 */,
                          int64_t row_stride, int64_t frame_stride, const double* d_M, int inverse_map, int mode,
                          int feather /* 0..65535 */, const uint16_t* d_gain /* u16[nframes,3] DEVICE, may be NULL */,
                          uint64_t* d_acc /* u64[dh,dw,channels+1] DEVICE, may be NULL */, int acc_in,
                          const uint8_t* d_background, uint8_t* d_out /* may be NULL */, int dw, int dh, int64_t out_row_stride,
                          int ox, int oy);
int evh_blend_fixed_plane_yuv420(evh_ctx* ctx, const evh_yuv420* src, int nframes, int sw, int sh, const double* d_M,
                                 int inverse_map, int mode, int feather, const uint16_t* d_gain, uint64_t* d_acc, int acc_in,
                                 const uint8_t* d_background, uint8_t* d_out, int dw, int dh, int64_t out_row_stride, int ox,
                                 int oy);
int evh_blend_ray_surface(evh_ctx* ctx, const uint8_t* d_frames, int nframes, int sw, int sh, int channels /* 1 | 3 */,
                          int64_t row_stride, int64_t frame_stride, const double* d_A, const double* d_col, const double* d_row,
                          int mode, int feather, const uint16_t* d_gain, uint64_t* d_acc, int acc_in,
                          const uint8_t* d_background, uint8_t* d_out, int dw, int dh, int64_t out_row_stride);
int evh_blend_ray_surface_yuv420(evh_ctx* ctx, const evh_yuv420* src, int nframes, int sw, int sh, const double* d_A,
                                 const double* d_col, const double* d_row, int mode, int feather, const uint16_t* d_gain,
                                 uint64_t* d_acc, int acc_in, const uint8_t* d_background, uint8_t* d_out, int dw, int dh,
                                 int64_t out_row_stride);

/* ---- multi-band blending of the mosaic: Laplacian pyramids blended under the pyramids of a label mask ----------------------------- */
/* FEATHER smooths exposure steps and every detail on which two frames disagree; SEAM keeps the detail and every step.  The band
 * blend (Burt and Adelson) blends low frequencies over a wide zone and high frequencies over a narrow one, in integers throughout.
 *
 * LABELS.  evh_seam_labels_fixed_plane / evh_seam_labels_ray_surface write SEAM's partition of the canvas from the geometry alone;
 * they read no frame.  nframes, sw, sh, d_M / inverse_map / ox / oy or d_A / d_col / d_row, feather, dw, dh are the blend entries'.
 *   first_label  frame k of the call carries label first_label + k; all labels lie in 0..65534, 65535 means "nobody";
 *   d_best       u32[dh][dw] (DEVICE), tight, in and out: the largest w so far, 0 = nobody;
 *   d_label      u16[dh][dw] (DEVICE), tight, in and out;
 *   state_in     zero: start from best = 0, label = 65535; non-zero: from the two buffers.
 * Frames in order: coverage and w = min(d, F) + 1 are steps 1-2 of the blend entries' contract (tw > 0 of the ray form included);
 * if w > best: best = w, label = first_label + k.  The comparison is strict: the earliest frame holds among equal weights, as in
 * SEAM.  Calls that carry the two buffers equal one call.  One launch, caller buffers only, nframes == 0 writes the start state.
 * Refused before the launch, outputs untouched -- EVH_ERR_INVALID: a NULL argument, d_best not 4-byte or d_label not 2-byte aligned,
 * nframes < 0, an empty frame or canvas, feather outside 0..65535, a label outside 0..65534, d_best or d_label overlapping each
 * other, the matrices or the tables; EVH_ERR_CAPACITY: sw or sh >= 2^26, dw*dh > INT_MAX, nframes > 65535.
 *
 * THE BAND BLEND.  evh_blend_bands_* take the four forms of evh_blend_*: the same frames, geometry, d_gain, d_background, d_out,
 * strides and plane forms, and instead of mode, feather and d_acc:
 *   levels       n in 0..8: the pyramid has levels 0..n.  dw_0 = dw, dw_{l+1} = (dw_l + 1) >> 1, dh alike;
 *   d_label      u16[dh][dw] (DEVICE), tight, read only: which frame owns a pixel;
 *   first_label  frame k of the call is the one d_label calls first_label + k;
 *   d_state      i64 (DEVICE), 8-byte aligned, in and out, may be NULL: per level l an array [dh_l][dw_l][cn + 1], levels 0..n one
 *                after the other; words 0..cn-1 of a pixel hold A_c, word cn holds D.  evh_bands_state_elems gives the word count;
 *   state_in     non-zero: the state starts from d_state; zero: from zeros;
 *   d_ws, ws_bytes  caller workspace (DEVICE), 8-byte aligned.  evh_bands_frame_ws_bytes is what one frame's pyramids need; the
 *                entry takes the frames in groups of as many as fit.  With d_state == NULL the state is kept at the head of d_ws,
 *                which must then hold 8 * evh_bands_state_elems bytes more.  The result does not depend on ws_bytes.
 * Per frame k, in any order (the state is a sum of integers):
 *   1. EXTENDED SAMPLE.  (U, V) is the warp entry's position, the same operations in the same order.  It is VALID if neither is NaN
 *      (ray form: and tw > 0).  U' = min(max(U, 0), 32*(sw-1)) in double, V' alike; the taps and the >> 10 at (U', V') are the warp
 *      entry's: the frame continued past its border by its edge pixels, no tap leaves the frame.  An invalid position gives
 *      s_c = 0.  G0_c(p) = s_c * g_c (below 2^24) at EVERY canvas pixel p: a frame's border is no step inside its own pyramid.
 *   2. MASK.  W0(p) = 65536 if d_label[p] == first_label + k, else 0.
 *   3. REDUCE.  K = (1,4,6,4,1) in both directions, indices clamped to the level:
 *      G{l+1}(x,y) = (sum_ij K_i K_j Gl(2x+i-2, 2y+j-2) + 128) >> 8 (the sum fits u32); W{l+1} the same with + 255: it rounds up,
 *      a weight with any support stays positive, and a full mask stays 65536 at every level.
 *   4. EXPAND E(G{l+1}) to the size of level l.  Along an axis, with j = i >> 1 and clamped indices: even i gives
 *      g[j-1] + 6 g[j] + g[j+1], odd i gives 4 g[j] + 4 g[j+1].  Rows, then columns, then (. + 32) >> 6 once (>> rounds down, also
 *      below zero).  Ll = Gl - E(G{l+1}) for l < n, Ln = Gn.
 *   5. ACCUMULATE.  Al_c += Wl * Ll_c, Dl += Wl, in i64.
 * The PICTURE, written when d_out is given, is a function of the state alone.  With ql_c = floor((2 A + D) / (2 D)) where D > 0,
 * else 0: Rn = qn, Rl = ql + E(R{l+1}) top-down; out_c = clamp((R0_c + 2048) >> 12, 0, 255) where D0 > 0; elsewhere the pixel takes
 * d_background's bytes, or zeros.  nframes == 0 writes the picture of the incoming state.
 * BOUNDS.  The labels partition the canvas, so over all frames sum_k W_k^l <= 65536 + (frames whose masks reach the pixel);
 * |L| < 2^25, so |A| < 2^42 + small for any number of frames; |q| < 2^26, |R| < 9 * 2^26.  The formulas hold unwrapped for ANY
 * handed-in state with 0 <= D < 2^25 and |A_c| <= 2^26 * D (a state the entry did not write is the caller's to keep inside these).
 * What follows from the rules:
 *   (a) if every covered pixel is labelled with the one frame that entered, the picture holds min(255, (s*g + 2048) >> 12) at every
 *       labelled pixel, at any `levels`: the warp entry's byte for gain 4096 (the round-up of W makes this hold to the border);
 *   (b) levels = 0 with labels from evh_seam_labels_* equals evh_blend_* in mode SEAM with the same feather and gains, byte for byte;
 *   (c) frames that show one constant value s*g everywhere give R0 exactly equal to it, for any labels that give every pixel to
 *       one of them (a level with D = 0 somewhere has q = 0 there, and an expansion beside such a hole mixes that 0 in);
 *   (d) calls that carry d_state equal one call, state word for state word; so do any frame order and any ws_bytes;
 *   (e) the plane forms equal evh_yuv420_to_bgr followed by the BGR forms; the ray form with the plane's tables equals the plane
 *       form with inverse_map != 0 wherever tw > 0 holds on the whole canvas.
 * Only caller buffers are used; the launches go to the context's stream, no synchronisation.  d_background == d_out is allowed.
 * Refused before anything is launched, outputs untouched -- everything evh_blend_* refuses (with d_state for d_acc), and
 * EVH_ERR_INVALID: levels outside 0..8, d_label NULL or not 2-byte aligned, a label outside 0..65534, d_out and d_state both NULL,
 * state_in with d_state NULL, d_ws NULL or not 8-byte aligned, ws_bytes below one frame's pyramids (plus the state where d_state
 * is NULL), d_ws overlapping any other buffer, d_state or d_out overlapping d_label.
 * The sizing helpers run on the host alone and touch no device; they return -1 for sizes the entries refuse.  What to allocate
 * for d_ws: g * evh_bands_frame_ws_bytes(...) for groups of g >= 1 frames, plus 8 * evh_bands_state_elems(...) when d_state is NULL. */
int evh_seam_labels_fixed_plane(evh_ctx* ctx, int nframes, int sw, int sh, const double* d_M, int inverse_map,
                                int feather /* 0..65535 */, int dw, int dh, int ox, int oy, int first_label,
                                uint32_t* d_best /* u32[dh,dw] DEVICE */, uint16_t* d_label /* u16[dh,dw] DEVICE */, int state_in);
int evh_seam_labels_ray_surface(evh_ctx* ctx, int nframes, int sw, int sh, const double* d_A, const double* d_col,
                                const double* d_row, int feather, int dw, int dh, int first_label, uint32_t* d_best,
                                uint16_t* d_label, int state_in);
int64_t evh_bands_state_elems(int dw, int dh, int channels, int levels);
int64_t evh_bands_frame_ws_bytes(int dw, int dh, int channels, int levels);
int evh_blend_bands_fixed_plane(evh_ctx* ctx, const uint8_t* d_frames, int nframes, int sw, int sh, int channels /* 1 | 3 */,
                                int64_t row_stride, int64_t frame_stride, const double* d_M, int inverse_map, int levels /* 0..8 */,
                                const uint16_t* d_label, int first_label, const uint16_t* d_gain /* may be NULL */,
                                int64_t* d_state /* may be NULL */, int state_in, void* d_ws, int64_t ws_bytes,
                                const uint8_t* d_background, uint8_t* d_out /* may be NULL */, int dw, int dh,
                                int64_t out_row_stride, int ox, int oy);
int evh_blend_bands_fixed_plane_yuv420(evh_ctx* ctx, const evh_yuv420* src, int nframes, int sw, int sh, const double* d_M,
                                       int inverse_map, int levels, const uint16_t* d_label, int first_label,
                                       const uint16_t* d_gain, int64_t* d_state, int state_in, void* d_ws, int64_t ws_bytes,
                                       const uint8_t* d_background, uint8_t* d_out, int dw, int dh, int64_t out_row_stride, int ox,
                                       int oy);
int evh_blend_bands_ray_surface(evh_ctx* ctx, const uint8_t* d_frames, int nframes, int sw, int sh, int channels /* 1 | 3 */,
                                int64_t row_stride, int64_t frame_stride, const double* d_A, const double* d_col,
                                const double* d_row, int levels, const uint16_t* d_label, int first_label, const uint16_t* d_gain,
                                int64_t* d_state, int state_in, void* d_ws, int64_t ws_bytes, const uint8_t* d_background,
                                uint8_t* d_out, int dw, int dh, int64_t out_row_stride);
int evh_blend_bands_ray_surface_yuv420(evh_ctx* ctx, const evh_yuv420* src, int nframes, int sw, int sh, const double* d_A,
                                       const double* d_col, const double* d_row, int levels, const uint16_t* d_label,
                                       int first_label, const uint16_t* d_gain, int64_t* d_state, int state_in, void* d_ws,
                                       int64_t ws_bytes, const uint8_t* d_background, uint8_t* d_out, int dw, int dh,
                                       int64_t out_row_stride);

/* ---- the sums behind exposure gains: two frames of a batch compared where one maps onto the other -------------------------------- */
/* What a gain solve needs (Brown and Lowe's gain compensation: per overlapping pair the number of pixels and the mean of either
 * frame over them), for arbitrary pairs of the nframes frames of w x h at d_frames; evh_pair_residual is tied to neighbours, gray
 * and differences.  d_pairs i32[npairs,2] (DEVICE): pair p = (i, j).  d_M f64[npairs,9] (DEVICE): d_M[p] maps pixels of frame i to
 * pixels of frame j and is used as it is.  Over the pixels (x, y) of frame i with x % step == 0 and y % step == 0:
 *   a = the pixel's bytes; b = the sample of frame j at d_M[p] . (x, y), coverage and sample exactly evh_warp_fixed_plane's with
 *   A = d_M[p], sw = w, sh = h (as in evh_pair_residual);
 *   the pixel COUNTS iff it is covered and every channel of a and of b lies in [lo, hi] -- clipped pixels bias a gain;
 *   d_stats[p][0] += 1, [1 + c] += a_c, [4 + c] += b_c; gray uses [1] and [4], the others stay 0.
 * d_stats u64[npairs,EVH_EXPO_NSTATS] (DEVICE): the entry zeroes it itself, stream-ordered.  A pair with an index outside
 * 0 .. nframes-1 reads nothing and has seven zeros: the indices live on the device, so the kernel checks them.  i == j is allowed.
 * The sums are exact integers (below 2^39) and do not depend on the order of addition.  Only caller buffers are used; one memset
 * and one launch on the context's stream, no synchronisation.  Refused before anything is launched, outputs untouched --
 * EVH_ERR_INVALID: NULL d_frames (a NULL plane), d_pairs, d_M or d_stats, channels not 1 or 3, w or h < 1, nframes or npairs < 0,
 * step outside 1..64, lo or hi outside 0..255 or lo > hi, a stride shorter than its row / frame, d_stats overlapping the frames,
 * d_pairs or d_M; EVH_ERR_CAPACITY: w or h >= 2^26, w*h > INT_MAX, npairs > 65535, nframes > 65535.  npairs == 0 succeeds and
 * does nothing.  The plane form converts every pixel and tap as evh_yuv420_to_bgr does.                                         */
enum { EVH_EXPO_NSTATS = 7 };
int evh_pair_exposure(evh_ctx* ctx, const uint8_t* d_frames, int nframes, int w, int h, int channels /* 1 | 3 */,
                      int64_t row_stride, int64_t frame_stride, const int32_t* d_pairs /* i32[npairs,2] DEVICE */, int npairs,
                      const double* d_M /* f64[npairs,9] DEVICE */, int step /* 1..64 */, int lo, int hi /* 0..255, lo <= hi */,
                      uint64_t* d_stats /* u64[npairs,7] DEVICE */);
int evh_pair_exposure_yuv420(evh_ctx* ctx, const evh_yuv420* src, int nframes, int w, int h, const int32_t* d_pairs, int npairs,
                             const double* d_M, int step, int lo, int hi, uint64_t* d_stats);

/* ---- the trail: earlier frames fade out behind the current one (stabilization.py:21-97, 129-172) -------------------------- */
/* What stabilize_view does to its canvas per frame -- paste, white outline on a copy, both through 8-bit BGR -> HSV -> BGR with
 * V lowered by 2 -- for nframes BGR frames of sw x sh and their matrices d_M f64[nframes,9] (DEVICE), over a BGR canvas of
 * dw x dh at d_canvas (rows of 3*dw bytes at canvas_row_stride), which is read, carried through the frames and written back:
 * hand the same canvas to the next call and the trail goes on.  Only BGR is supported.  Frames are taken in order,
 * k = 0 .. nframes-1; a canvas pixel carries its value c, starting from d_canvas:
 *   1. Paste.  If frame k covers the pixel, c becomes the sampled value; coverage and sampling are exactly
 *      evh_warp_fixed_plane's (d_M, inverse_map, ox, oy as there).  A NaN, singular or horizon-crossing matrix covers nothing;
 *      the dimming still goes on.
 *   2. Picture.  q = c.  If d_rect i32[nframes,4] (DEVICE; may be NULL) is given and the pixel lies on the outline of rectangle
 *      k = (x0, y0, x1, y1) in canvas pixels, q becomes (255, 255, 255).  The outline is x0 <= x <= x1 && y0 <= y <= y1 &&
 *      (x == x0 || x == x1 || y == y0 || y == y1); x1 < x0 or y1 < y0: no rectangle for this frame; parts outside the canvas
 *      do not exist.  These are the pixels of the four cv2.line calls of change_frame_location (axis-aligned, both ends
 *      inclusive).  If d_out is given (it may be NULL: the call then only advances the canvas), out[k] = show(q), picture k at
 *      d_out + k*out_frame_stride, rows of 3*dw bytes at out_row_stride.
 *   3. Carry.  c = keep(c): the pasted value, not the one with the outline (the reference draws the outline on a copy).
 * After the last frame c is stored to d_canvas.
 * Colour arithmetic.  Tables, built on the host in double: S[0] = H[0] = 0 and for i = 1..255 S[i] = rint(1044480.0 / i)
 * (255 << 12), H[i] = rint(737280.0 / (6.0 * i)) (180 << 12), halves to even.
 *   to_hsv(b, g, r), int32: v = max, m = min, d = v - m; s = (d*S[v] + 2048) >> 12; t = g - b if v == r, else b - r + 2d if
 *     v == g, else r - g + 4d; h = (t*H[d] + 2048) >> 12 with an arithmetic shift (a floor); h += 180 if h < 0.  h is in [0, 179].
 *   from_hsv(h, s, v), IEEE float32, one rounding per operation, no fma: hf = (float)h * C6 with C6 the float32 0x3D088889
 *     (6.f/180.f); while hf >= 6: hf -= 6.f; k = floor(hf), f = hf - k; sf = (float)s * K, vf = (float)v * K with K the float32
 *     0x3B808081 (1.f/255.f).  If s == 0: b = g = r = vf.  Otherwise tab = {vf, vf*(1 - sf), vf*(1 - sf*f),
 *     vf*(1 - sf*(1 - f))} and (b, g, r) = tab[.] by sector k: 0: {1,3,0}  1: {1,0,2}  2: {3,0,1}  3: {0,2,1}  4: {0,1,3}
 *     5: {2,1,0}.  Each output byte is clamp(rint(x * 255.f), 0, 255), halves to even.
 *   keep(p) = from_hsv(h, s, max(v - 2, 0)) with (h, s, v) = to_hsv(p): np.where((v - 2) >= 254, 0, v - 2) on uint8.
 *   show(p) = from_hsv(h, s, v - 2) if v >= 2, else from_hsv(222, 12, 31): the reference stores [222, 12.35, 31.76] into a
 *     uint8 array, which truncates; the result is the constant BGR (30, 31, 30).
 * The two conversions are OpenCV 3.4.2's scalar 8-bit BGR2HSV and HSV2BGR restated from its source; no OpenCV binary or source
 * was at hand to compare with, so byte identity with cv2.cvtColor is NOT claimed -- the claim is the arithmetic above.
 * Every byte of every picture and canvas row inside 3*dw is written, bytes between rows are not; a thread reads only the canvas
 * bytes it later writes.  Only caller buffers are used: nothing depends on the sizes given to evh_create.  Refused before
 * anything is launched, outputs untouched -- EVH_ERR_INVALID: d_M, d_canvas or the frames NULL, nframes < 0, sw, sh, dw or
 * dh < 1, a stride shorter than its row / frame (frame strides count when nframes > 1, the picture strides when d_out is
 * given), d_out overlapping d_canvas or the frames, d_canvas overlapping the frames; EVH_ERR_CAPACITY: sw or sh >= 2^26,
 * dw*dh > INT_MAX, nframes > 65535.  nframes == 0 succeeds and does nothing.  The plane form converts every tap as
 * evh_yuv420_to_bgr does: it equals evh_yuv420_to_bgr followed by the BGR form.  Speed, not results, depends on alignment:
 * d_out and its strides multiples of 4 let a thread store its four pixels as words, d_canvas and canvas_row_stride alike.
 * Neither entry synchronises.                                                                                              */
int evh_trail_fixed_plane(evh_ctx* ctx, const uint8_t* d_frames, int nframes, int sw, int sh, int64_t row_stride,
                          int64_t frame_stride, const double* d_M, int inverse_map, const int32_t* d_rect /* may be NULL */,
                          uint8_t* d_canvas /* in and out */, int64_t canvas_row_stride, uint8_t* d_out /* may be NULL */,
                          int64_t out_row_stride, int64_t out_frame_stride, int dw, int dh, int ox, int oy);
int evh_trail_fixed_plane_yuv420(evh_ctx* ctx, const evh_yuv420* src, int nframes, int sw, int sh, const double* d_M,
                                 int inverse_map, const int32_t* d_rect /* may be NULL */, uint8_t* d_canvas /* in and out */,
                                 int64_t canvas_row_stride, uint8_t* d_out /* may be NULL */, int64_t out_row_stride,
                                 int64_t out_frame_stride, int dw, int dh, int ox, int oy);

/* ---- the background plate: the scene without its moving objects, and the moving objects --------------------------------------- */
/* The per-pixel temporal median of nframes frames of sw x sh registered on the fixed plane -- the scene without whatever crosses
 * it (a background plate) -- and, by differencing each frame against that plate, a moving-object mask per frame in fixed-plane
 * coordinates: the "video motion segmentation" the reference's known-issues.md asks for.  The frames (BGR or gray), their
 * matrices d_M f64[nframes,9] (DEVICE), inverse_map, the canvas of dw x dh pixels and its origin (ox, oy) are
 * evh_warp_fixed_plane's.  Per canvas pixel (x, y), the plane point (x + ox, y + oy):
 *   1. Samples.  For k = 0 .. nframes-1, whether frame k covers the pixel and the sampled value s_k[c] per channel are exactly
 *      evh_warp_fixed_plane's: the adjugate or inverse_map, U and V in 1/32 pixels rounded half to even, the comparison in double
 *      (a NaN, zero, singular, huge or horizon-crossing matrix covers nothing and reads nothing), the four taps with >> 10, a tap
 *      of weight 0 not read.  C is the set of covering frames, n = |C|.
 *   2. Plate.  If n >= min_cover (1..255), channel c of the plate is the element of 0-based rank (n - 1) >> 1 of the samples
 *      {s_k[c] : k in C} sorted ascending: the lower median, per channel independently, so the three channels may come from
 *      different frames; the value always occurred, nothing is averaged or rounded.  Otherwise the pixel takes d_background's
 *      bytes (dh rows of dw*channels bytes at plate_row_stride), or zeros when d_background is NULL.
 *   3. Count.  If d_count is given (it may be NULL), d_count[y][x] = n as a byte, rows of dw bytes at count_row_stride, whatever
 *      min_cover is.
 *   4. Masks.  If d_mask is given (it may be NULL), mask k is gray, dh rows of dw bytes at mask_row_stride, at
 *      d_mask + k*mask_frame_stride.  Its pixel is 255 iff k is in C and n >= min_cover and |gray(s_k) - gray(plate)| > threshold
 *      (0..255), else 0, with gray(b, g, r) = (b*1868 + g*9617 + r*4899 + 8192) >> 14 as in evh_pair_residual; with
 *      channels == 1 the byte is the gray value.
 * Every byte of every plate row inside dw*channels is written, count and mask rows inside dw; bytes between rows are not.  Only
 * caller buffers are used (the kernel keeps a pixel's samples in LDS, 256 bytes per frame and workgroup, which is where
 * EVH_PLATE_MAX_FRAMES comes from): nothing depends on the sizes given to evh_create.  One launch on the context's stream; neither
 * entry synchronises.  Refused before anything is launched, outputs untouched -- EVH_ERR_INVALID: a NULL d_frames (a NULL plane),
 * d_M or d_plate, channels not 1 or 3, sw, sh, dw or dh < 1, nframes < 0, min_cover outside 1..255, threshold outside 0..255 when
 * d_mask is given, a stride shorter than its row / frame (frame strides count when nframes > 1, the count and mask strides when
 * those outputs are given), any output overlapping another output, the frames or d_background; EVH_ERR_CAPACITY:
 * nframes > EVH_PLATE_MAX_FRAMES, sw or sh >= 2^26, dw*dh > INT_MAX.  nframes == 0 succeeds: every pixel takes the background, the
 * count is 0, no mask is written.  The plane form (BGR plate) converts every tap as evh_yuv420_to_bgr does: it equals
 * evh_yuv420_to_bgr followed by the BGR form.                                                                               */
enum { EVH_PLATE_MAX_FRAMES = 255 };
int evh_plate_fixed_plane(evh_ctx* ctx, const uint8_t* d_frames, int nframes, int sw, int sh, int channels /* 1 | 3 */,
                          int64_t row_stride, int64_t frame_stride, const double* d_M, int inverse_map,
                          int min_cover /* 1..255 */, const uint8_t* d_background /* may be NULL */,
                          uint8_t* d_plate, int64_t plate_row_stride,
                          uint8_t* d_count /* may be NULL */, int64_t count_row_stride,
                          uint8_t* d_mask /* may be NULL */, int threshold /* 0..255 */, int64_t mask_row_stride,
                          int64_t mask_frame_stride, int dw, int dh, int ox, int oy);
int evh_plate_fixed_plane_yuv420(evh_ctx* ctx, const evh_yuv420* src, int nframes, int sw, int sh, const double* d_M,
                                 int inverse_map, int min_cover, const uint8_t* d_background, uint8_t* d_plate,
                                 int64_t plate_row_stride, uint8_t* d_count, int64_t count_row_stride, uint8_t* d_mask,
                                 int threshold, int64_t mask_row_stride, int64_t mask_frame_stride,
                                 int dw, int dh, int ox, int oy);
/* Match rows judged against a plate: the rows of a batch (evh_batch_static_rows) whose points sit on something that differs from
 * the plate are dropped before the final solve, so that the homography follows the camera and not what moves -- the step between
 * evh_plate_fixed_plane and evh_stream_scan.  It judges ANY frame against a given plate (the masks above exist only for the plate's
 * own frames) and reads only the canvas pixels around each key point.  The frames, d_M f64[nframes,9] (DEVICE; frame pixels ->
 * plane, the inverse_map == 0 form only), the canvas of dw x dh pixels and its origin (ox, oy) are evh_plate_fixed_plane's; d_plate
 * has the frames' channels (the plane form: BGR), d_count one byte per pixel.  d_rows f32[npairs][row_cap][4] holds rows
 * (ax, ay, bx, by), a on the current and b on the previous frame; pair p has its previous frame at index fp = p*frame_step and its
 * current frame at fc = fp + 1, as in evh_draw_matches and evh_pair_residual; nframes must reach the last index used.  All
 * arithmetic is IEEE float64 with one rounding per operation (no fma).
 *   1. Rows of a pair.  n = min(max(d_counts[p], 0), row_cap).  If d_status1[p] != EVH_PAIR_OK or n == 0: d_out_counts[p] =
 *      d_counts[p], d_moving[p] = 0, and no row and no flag of the pair is written.
 *   2. An end point's place.  End point (x, y) lies in frame f (fc for a, fp for b): px = (double)x * row_sx, py = (double)y * row_sy;
 *      with m = d_M[f]: tx = (m0*px + m1*py) + m2, ty = (m3*px + m4*py) + m5, tw = (m6*px + m7*py) + m8; cx = rint(tx / tw),
 *      cy = rint(ty / tw), halves to even.  Unless |cx| <= 2^30 and |cy| <= 2^30, compared in double (NaN fails), the end point is
 *      not moving.
 *   3. Window and hits.  The window pixels are (X, Y) = (cx - ox + i, cy - oy + j) for |i|, |j| <= radius (0..7), formed in int64.
 *      A window pixel is a HIT iff 0 <= X < dw and 0 <= Y < dh, and d_count[Y][X] >= min_cover (1..255), and frame f covers (X, Y)
 *      exactly as evh_warp_fixed_plane defines coverage (the adjugate of m, U and V in 1/32 pixels), and
 *      |gray(s_f) - gray(plate[Y][X])| > threshold (0..255), s_f being that entry's four-tap sample and gray the integer gray of
 *      evh_pair_residual; with channels == 1 the byte is the gray value.  A hit is precisely the byte evh_plate_fixed_plane would have
 *      written into frame f's mask, had f been one of the plate's frames.  The end point is moving iff hits >= min_hits
 *      (1..(2*radius+1)^2).
 *   4. A row is moving iff a is moving in fc or b is moving in fp; moving = the number of such rows among the n.  If d_flags is
 *      given (u8[npairs][row_cap]; it may be NULL), row i < n gets (a moving) | (b moving) << 1; flags past n are untouched.
 *   5. Output.  If n - moving >= min_keep (>= 0): the rows that are not moving go to the head of pair p's block of d_out_rows
 *      f32[npairs][row_cap][4] in their original order, each copied as 16 bytes (bit patterns: -0.0 and NaN payloads survive), and
 *      d_out_counts[p] = n - moving.  Otherwise all n rows are copied unfiltered and d_out_counts[p] = n: a filter must never starve
 *      a pair that had a solution.  d_moving[p] = moving in both cases (d_moving may be NULL).  Rows past the out count are untouched.
 * Only caller buffers are used; one launch on the context's stream (one workgroup per pair; the survivors are compacted by a prefix
 * scan, so their order is stable), neither entry synchronises, and the record of the last batch is left alone.  Refused before
 * anything is launched, outputs untouched -- EVH_ERR_INVALID: a NULL source (a NULL plane), d_M, d_plate, d_count, d_rows, d_counts,
 * d_status1, d_out_rows or d_out_counts, channels not 1 or 3, sw, sh, dw, dh or row_cap < 1, nframes or npairs < 0, frame_step not 1
 * or 2, nframes < (npairs - 1)*frame_step + 2 when npairs >= 1, min_cover outside 1..255, threshold outside 0..255, radius outside
 * 0..7, min_hits outside 1..(2*radius+1)^2, min_keep < 0, row_sx or row_sy not finite or <= 0, a stride shorter than its row / frame
 * (frame strides count when nframes > 1), d_rows or d_out_rows not 16-byte aligned, any output overlapping any input or another
 * output; EVH_ERR_CAPACITY: npairs > 65535, sw or sh >= 2^26, dw*dh > INT_MAX.  npairs == 0 succeeds and does nothing.  The plane
 * form converts every tap as evh_yuv420_to_bgr does: it equals evh_yuv420_to_bgr followed by the BGR form.                       */
int evh_rows_moving_filter(evh_ctx* ctx, const uint8_t* d_frames, int nframes, int sw, int sh, int channels /* 1 | 3 */,
                           int64_t row_stride, int64_t frame_stride, const double* d_M /* f64[nframes,9] DEVICE */,
                           const uint8_t* d_plate, int64_t plate_row_stride, const uint8_t* d_count, int64_t count_row_stride,
                           int dw, int dh, int ox, int oy, int min_cover /* 1..255 */, int threshold /* 0..255 */,
                           int radius /* 0..7 */, int min_hits /* 1..(2r+1)^2 */, double row_sx, double row_sy,
                           const float* d_rows, int row_cap, const int32_t* d_counts, const int32_t* d_status1, int npairs,
                           int frame_step /* 1 | 2 */, int min_keep /* >= 0 */, float* d_out_rows, int32_t* d_out_counts,
                           int32_t* d_moving /* may be NULL */, uint8_t* d_flags /* may be NULL */);
int evh_rows_moving_filter_yuv420(evh_ctx* ctx, const evh_yuv420* src, int nframes, int sw, int sh, const double* d_M,
                                  const uint8_t* d_plate, int64_t plate_row_stride, const uint8_t* d_count,
                                  int64_t count_row_stride, int dw, int dh, int ox, int oy, int min_cover, int threshold, int radius,
                                  int min_hits, double row_sx, double row_sy, const float* d_rows, int row_cap,
                                  const int32_t* d_counts, const int32_t* d_status1, int npairs, int frame_step, int min_keep,
                                  float* d_out_rows, int32_t* d_out_counts, int32_t* d_moving, uint8_t* d_flags);
/* The masks turned into objects: connected-component labelling of nmasks masks of dw x dh bytes, with each object's box, area and
 * centre sums in a compact table, so that only a few kilobytes leave the device.  Mask m is dh rows of dw bytes at
 * mask_row_stride, at d_mask + m*mask_frame_stride: exactly what evh_plate_fixed_plane writes into d_mask.  For each mask m,
 * independently:
 *   1. Foreground.  A pixel is set iff its byte is non-zero.
 *   2. Opening, when open_radius = r > 0 (0..3).  E[y][x] is set iff every (x+i, y+j) with |i|, |j| <= r lies inside the canvas
 *      and is set; O[y][x] is set iff some (x+i, y+j) with |i|, |j| <= r lies inside the canvas and has E set.  Outside the canvas
 *      counts as background.  With r = 0, O is the foreground itself.
 *   3. Components of O under connectivity 4 (the pixels left, right, above and below) or 8 (the diagonals too).  A component's
 *      area is its number of pixels, its `first` the raster index y*dw + x of its first pixel in raster order.  A component is KEPT
 *      iff area >= min_area (>= 1).  Kept components are numbered 1..K in ascending order of `first`.
 *   4. Labels.  d_labels[m][y][x] (i32, rows of dw elements at label_row_stride ELEMENTS, sheet m at m*label_frame_stride
 *      elements) is the number of the pixel's component if that component is kept, else 0.  Every element inside dw of every row
 *      is written; elements between rows are not.
 *   5. Objects.  d_nobjects[m] = K, whatever max_objects is.  d_objects[m*max_objects + k-1] holds component k for
 *      k <= min(K, max_objects): its inclusive box x0 <= x <= x1, y0 <= y <= y1 in canvas pixels, area, first, and sx, sy, the sums
 *      of x and of y over its pixels (the centre is sx/area, sy/area).  Entries past that are untouched.  max_objects never
 *      changes a label.
 * The result is a pure function of the mask: every sum is an integer, nothing depends on the order in which workgroups arrive.
 * Only caller buffers are used.  d_work is scratch of at least evh_mask_components_work_bytes(dw, dh, nmasks) bytes, 4-byte
 * aligned: one i32 of area and one of scanned ordinal per pixel (8*dw*dh bytes per mask) for as many masks as are labelled at
 * once -- all of them up to 256 MiB, beyond that the entry loops over groups of masks, and a larger buffer means larger groups.
 * d_labels serves as the parent array while the call runs.  The call is a fixed sequence of launches on the context's stream
 * (eight per group of masks, six when the canvas is one tile; each kernel ends on its own: every link of the union-find points to a smaller raster index, and no
 * workgroup waits for another); it does not synchronise and leaves the record of the last batch alone.  Refused before anything
 * is launched, outputs untouched -- EVH_ERR_INVALID: a NULL d_mask, d_labels, d_nobjects or d_work, d_objects NULL while
 * max_objects > 0, connectivity not 4 or 8, open_radius outside 0..3, min_area < 1, max_objects < 0, dw or dh < 1, nmasks < 0, a
 * stride shorter than its row / frame (frame strides count when nmasks > 1), d_labels, d_nobjects or d_work not 4-byte aligned,
 * d_objects not 8-byte aligned, work_bytes too small, any output or the work buffer overlapping the mask or another output;
 * EVH_ERR_CAPACITY: dw*dh > INT_MAX, nmasks > 65535.  nmasks == 0 succeeds and does nothing.  The tile of the first pass is
 * EVH_COMPONENTS_TILE_W x EVH_COMPONENTS_TILE_H pixels; results do not depend on it.                                         */
enum { EVH_COMPONENTS_TILE_W = 32, EVH_COMPONENTS_TILE_H = 16 };
typedef struct evh_component {        /* 40 bytes, 8-byte aligned */
  int32_t x0, y0, x1, y1;             /* bounding box in canvas pixels, inclusive */
  int32_t area;                       /* pixels */
  int32_t first;                      /* y*dw + x of the first pixel in raster order */
  int64_t sx, sy;                     /* sum of x, sum of y over the pixels: centre = sx/area, sy/area */
} evh_component;
/* host only; 0 for arguments the entry would refuse (and for nmasks == 0); at most 8*dw*dh*nmasks bytes */
size_t evh_mask_components_work_bytes(int dw, int dh, int nmasks);
int evh_mask_components(evh_ctx* ctx, const uint8_t* d_mask, int nmasks, int dw, int dh, int64_t mask_row_stride,
                        int64_t mask_frame_stride, int connectivity /* 4 | 8 */, int open_radius /* 0..3 */,
                        int min_area /* >= 1 */, int32_t* d_labels, int64_t label_row_stride /* in elements */,
                        int64_t label_frame_stride, evh_component* d_objects /* may be NULL iff max_objects == 0 */,
                        int max_objects /* >= 0 */, int32_t* d_nobjects /* i32[nmasks] */, void* d_work, size_t work_bytes);

/* ---- heat-map pictures: the colouring of heatmap_frame_processing (processing_visualization.py:336-344) ------------------------ */
/* What heatmap_frame_processing does with the field of evh_fixed_plane_field and the resized frame, without part_line's grid,
 * arrows and text: for each of n superposed matrices d_Hsup f64[n,9] (DEVICE) a BGR picture of w x h, frame k into
 * d_out + k*out_frame_stride, rows of 3*w bytes at out_row_stride.  d_frames: n BGR frames of w x h (rows at row_stride, frames
 * at frame_stride), or NULL = black frames.  d_lut u8[256,3] (DEVICE) is the colour table in BGR order, what
 * cv2.applyColorMap(np.arange(256, dtype=np.uint8), cv2.COLORMAP_JET) returns for the reference's pictures.
 * Field and colour index of pixel (x, y), all IEEE float64 with one rounding per operation:
 *   tx = fma(h0, x, h1*y) + h2, ty and tw alike (the order of evh_fixed_plane_field); u = tx / tw, v = ty / tw;
 *   s = u*u + v*v (each product rounded, then the sum; no fma); r = sqrt(s); t = 255 * (r / heatmap_constant) (a true division,
 *   then the product);
 *   i = (int64)trunc(t) & 255 when t is finite and 0 <= t < 2^31, else i = 0;
 *   with saturate != 0: i = 255 for t >= 255 and for t = +inf, i = 0 for NaN.
 * The wrap (saturate == 0) is what np.uint8(255 * heatmap) gives on the reference's platform for every value whose cast is
 * defined.  For NaN, +inf and t >= 2^31 the C cast is undefined and numpy versions differ: index 0 there is this library's
 * choice, not the reference's.
 * Blend, per channel ch: c = d_lut[3*i + ch], p = the frame's byte (0 without frames), o = rint((double)c * alpha + (double)p)
 * (the product rounded, then the sum; halves to even) clamped to [0, 255]: heatmap * hif + image followed by the conversion
 * cv2.imwrite applies to float64 pixels (cvRound, saturating); hif = alpha = 0.8 in the reference.
 * Every byte of every output row inside 3*w is written, bytes between rows are not.  Only caller buffers are used: nothing
 * depends on the sizes given to evh_create.  Refused before anything is launched, outputs untouched -- EVH_ERR_INVALID: a NULL
 * d_Hsup, d_lut or d_out, w or h < 1, n < 0, a stride shorter than its row / frame (frame strides count when n > 1),
 * heatmap_constant not finite or <= 0, alpha not finite or < 0, d_frames overlapping d_out; EVH_ERR_CAPACITY: n > 65535,
 * w*h > INT_MAX (the limits of evh_fixed_plane_field).  n == 0 succeeds and does nothing.  Speed, not results, depends on
 * alignment: d_out and the output strides multiples of 4 let a thread store its four pixels as words (d_frames and its
 * strides: load them so).  Does not synchronise.                                                                              */
int evh_heatmap_render(evh_ctx* ctx, const double* d_Hsup, int n, int w, int h, const uint8_t* d_frames, int64_t row_stride,
                       int64_t frame_stride, const uint8_t* d_lut, double heatmap_constant, double alpha, int saturate,
                       uint8_t* d_out, int64_t out_row_stride, int64_t out_frame_stride);

/* ---- matching pictures: draw_matches (processing_visualization.py:22-57) as video_processing.py:78-81 calls it -------------------- */
/* The rows a batch handed to compute_homography, read back out of the context.  A context records its LAST BATCH: which pair
 * buffers it used (the fused ORB path or the multi-type path, after accumulate and merge) and how many pair slots it had (pair
 * slot p as in the entry that ran: (frame 2p + 1, frame 2p) for independent pairs, else (frame p + 1, frame p); the slots
 * between two streams of a multi-stream / ragged batch are computed and belong to no stream).  The record is set by every
 * batch entry -- evh_pair_homography_batch[_types], evh_stream_homography_batch[_resized|_types|_yuv420|_types_yuv420],
 * evh_multi_stream_homography_batch, evh_streams_homography_batch[_yuv420] -- and by evh_stream_static_batch, when they return
 * EVH_SUCCESS.  It is cleared by every other entry that writes those pair buffers: evh_match_static_from_slots,
 * evh_pair_from_slots, evh_compute_homography, evh_stream_scan; a batch entry that returns an error may leave it cleared.
 * (The detect entries, the matchers and filters on caller buffers, evh_find_homography_ransac* and evh_static_filter use other
 * buffers and leave it alone.)
 * evh_batch_static_info: the pair slots and the row capacity (rows per pair slot) of that batch; 0, 0 when there is none.   */
int evh_batch_static_info(const evh_ctx* ctx, int* npairs, int* row_cap);
/* Pair slots first_pair .. first_pair + npairs - 1 of that batch into caller DEVICE buffers: d_rows f32[npairs][row_cap][4], rows
 * (ax, ay, bx, by) with a = the current frame and b = the previous frame as evh_stream_static_batch lays them out, rows past a
 * pair's count hold whatever the buffers held; d_counts i32[npairs]; d_status1 i32[npairs] the FRONT status (EVH_PAIR_* of
 * detect, match and static filter -- what evh_stream_static_batch calls the phase-1 status -- not the final one: a pair whose
 * front status is EVH_PAIR_OK entered compute_homography with these rows, whatever came of it).  Three contiguous device-to-device
 * copies on the context's stream, ordered behind an asynchronous solve by a stream wait; never synchronises the host, nothing is
 * ever truncated.  Refused with EVH_ERR_INVALID before anything is enqueued, outputs untouched: a NULL pointer, first_pair < 0,
 * npairs < 1, first_pair + npairs beyond the batch's pair slots, no resident batch, row_cap other than the reported capacity. */
int evh_batch_static_rows(evh_ctx* ctx, int first_pair, int npairs, float* d_rows, int row_cap, int32_t* d_counts,
                          int32_t* d_status1);
/* The matching pictures.  Picture p (into d_out + p*out_frame_stride, rows at out_row_stride) is BGR, h rows of 2*w pixels: the
 * left half is frame p*frame_step of d_frames (BGR, w x h, rows at row_stride, frames at frame_stride) -- the PREVIOUS frame --
 * the right half frame p*frame_step + 1, the CURRENT frame; frame_step is 1 for streams and ragged batches and 2 for
 * independent pairs.  On top, one line of colour color_bgr = b | g << 8 | r << 16 (the reference draws (0, 255, 0) = 0x00ff00) per
 * row r < min(d_counts[p], row_cap) of d_rows f32[npairs][row_cap][4] (a count above row_cap is taken as row_cap, a negative one as
 * 0: nothing is read past a pair's rows); with d_status given (it may be NULL) a picture whose d_status[p] != EVH_PAIR_OK gets no
 * lines and is the two frames only.
 * Ends of the line of row (ax, ay, bx, by), trunc toward zero as Python's int():
 *   points == EVH_DRAW_REFERENCE (0): (trunc(ax), trunc(ay)) and (trunc(bx) + w, trunc(by)).  With the rows of a batch (a = the
 *     current frame) the current frame's points land on the previous frame's half and vice versa: that is what
 *     video_processing.py:69-80 draws, because concatenate_all_features_types returns self's (the newer frame's) points first
 *     and draw_matches puts its first point list on its first image.  The quirk is kept as the default.
 *   points == EVH_DRAW_OWN_FRAME (1): (trunc(bx), trunc(by)) and (trunc(ax) + w, trunc(ay)): each point on its own frame.
 * A row with a coordinate that is not finite, or whose truncated value lies outside [-32768, 32767], is skipped (the reference
 * would raise there: this library's choice).
 * The line is the 8-connected walk of OpenCV 3.4.2's LineIterator with leftToRight, which cv2.line(..., thickness=1) uses, from
 * pt1 (first end above) to pt2:
 *   1. (dx, dy) = pt2 - pt1.  If dx < 0 the ends are swapped and (dx, dy) negated; with dx == 0 the walk starts at pt1.
 *   2. sy = sign(dy), dy = |dy|.  If dy > dx the major axis is y, stepped by sy, and the minor axis is x, stepped by +1;
 *      otherwise the major axis is x, stepped by +1, and the minor axis is y, stepped by sy.
 *   3. With D the major and d the minor extent: err = D - 2d, and D + 1 pixels are emitted, the first at the start.
 *   4. After each pixel: if err < 0 the minor axis steps and err += 2D; then, always, the major axis steps and err -= 2d.
 * Equivalently pixel k = 0..D has the minor offset (2*d*k + D - 1) div (2*D) for D > 0, which is how the kernel shares a line
 * among lanes.  (0,0) -> (5,2) and (5,2) -> (0,0) both give (0,0) (1,0) (2,1) (3,1) (4,2) (5,2).
 * Pixels outside [0, 2w) x [0, h) are not written.  cv2.line clips the segment to the image first, which can shift interior
 * pixels of a line that leaves it, so equality with cv2.line is claimed only for lines inside the picture (key points never
 * leave their frame) -- and that claim rests on the rule above as restated from OpenCV's source: no OpenCV binary was at hand
 * to compare pictures with.
 * Two launches on the context's stream, the frames first and the lines on top; all lines of a call share one colour, so
 * lines that cross or coincide need no order.  Every byte of every output row inside 6*w is written, bytes between rows are
 * not.  Only caller buffers are used: nothing depends on the sizes given to evh_create.  Refused before anything is launched,
 * outputs untouched -- EVH_ERR_INVALID: a NULL d_frames, d_rows, d_counts or d_out, w, h or row_cap < 1, npairs < 0, frame_step
 * not 1 or 2, an unknown points value, bits above 24 set in color_bgr, a stride shorter than its row / frame (row strides
 * always; frame_stride when npairs >= 1, out_frame_stride when npairs > 1), d_out overlapping d_frames or d_rows;
 * EVH_ERR_CAPACITY: w > 16383.  npairs == 0 succeeds and does nothing.  Speed, not results, depends on alignment: the paste moves
 * 4 pixels as three words where the pointers, strides and w allow it.  Does not synchronise.                                  */
enum { EVH_DRAW_REFERENCE = 0, EVH_DRAW_OWN_FRAME = 1 };
int evh_draw_matches(evh_ctx* ctx, const uint8_t* d_frames, int npairs, int frame_step, int w, int h, int64_t row_stride,
                     int64_t frame_stride, const float* d_rows, int row_cap, const int32_t* d_counts,
                     const int32_t* d_status /* may be NULL */, int points, uint32_t color_bgr, uint8_t* d_out,
                     int64_t out_row_stride, int64_t out_frame_stride);

/* ---- the score of a homography: the motion-compensated residual of a pair of frames ---------------------------------------------- */
/* How well a matrix registers two consecutive frames: the previous frame is sampled where the matrix sends each pixel of the current
 * frame, the two are differenced in gray, and the differences are summed per pair -- the sums behind the PSNR / ITF figures of the
 * stabilisation literature -- with, optionally, the difference picture or its thresholded mask (the moving objects the reference's
 * known-issues.md names as the cause of bad matrices).  No warped frame is stored.
 * d_frames: frames of w x h with `channels` bytes per pixel (BGR or gray), rows at row_stride, frames at frame_stride.  Pair p has
 * the PREVIOUS frame p*frame_step and the CURRENT frame p*frame_step + 1, as in evh_draw_matches (frame_step 1 for streams, 2 for
 * independent pairs): (npairs - 1)*frame_step + 2 frames are read.  d_M f64[npairs,9] (DEVICE): d_M[p] maps pixels of the current
 * frame to pixels of the previous frame and is used as it is, the inverse_map != 0 form of evh_warp_fixed_plane.
 * Per pixel (x, y) of the current frame, in this order:
 *   1. X = (double)x, Y = (double)y; tx, ty, tw, U, V, coverage and, for a covered pixel, the sampled value of the previous frame per
 *      channel are exactly evh_warp_fixed_plane's with A = d_M[p], sw = w, sh = h: positions in 1/32 pixels, the comparison in
 *      double, the four taps with >> 10, a tap of weight 0 not read.
 *   2. gray(b, g, r) = (b*1868 + g*9617 + r*4899 + 8192) >> 14 (the weights of the ingest); with 3 channels the sample is
 *      interpolated per channel first and converted afterwards; with channels == 1 the byte is the gray value.
 *   3. g_cur = gray of the current frame's pixel, g_reg = gray of the sample, g_prev = gray of the previous frame's pixel at the same
 *      (x, y); d = |g_cur - g_reg|, d0 = |g_cur - g_prev|.
 * d_stats u64[npairs,EVH_RES_NSTATS] (DEVICE), over the COVERED pixels of pair p only, exact unsigned integers:
 *   [EVH_RES_COVERED] += 1; [EVH_RES_SAD] += d; [EVH_RES_SSD] += d*d; [EVH_RES_SAD0] += d0; [EVH_RES_SSD0] += d0*d0;
 *   [EVH_RES_MOVING] += (d > threshold).
 * The entry zeroes d_stats itself, stream-ordered, whatever it held.  Every value stays below 2^47 (w*h <= INT_MAX times 255^2).  A
 * NaN, zero, singular or horizon-crossing matrix covers nothing or only part, exactly as in evh_warp_fixed_plane; a pair without a
 * covered pixel has six zeros.  The sums are integers, so they do not depend on the order in which the device adds them.
 * d_out (may be NULL): pair p's picture at d_out + p*out_frame_stride, gray, h rows of w bytes at out_row_stride.  A covered pixel
 * holds d (EVH_RESIDUAL_ABS) or 255 if d > threshold, else 0 (EVH_RESIDUAL_MASK); an uncovered pixel holds 0 in both kinds.  Every
 * byte of every row inside w is written, bytes between rows are not.
 * Only caller buffers are used: nothing depends on the sizes given to evh_create.  Refused before anything is launched, outputs
 * untouched -- EVH_ERR_INVALID: NULL d_frames (a NULL plane), d_M or d_stats, channels not 1 or 3, frame_step not 1 or 2, w or h < 1,
 * npairs < 0, threshold outside 0..255, an unknown kind, a stride shorter than its row / frame (the frames' always: a pair takes two
 * frames; the pictures' when d_out is given, out_frame_stride when npairs > 1), d_out overlapping the frames or d_stats;
 * EVH_ERR_CAPACITY: w or h >= 2^26, w*h > INT_MAX, npairs > 65535.  npairs == 0 succeeds and does nothing.  The plane form converts
 * every tap and every pixel as evh_yuv420_to_bgr does: it equals evh_yuv420_to_bgr followed by the BGR form.  Speed, not results,
 * depends on alignment: d_frames and its strides multiples of 4 let a thread load its four pixels as words, d_out and its strides
 * store them so.  One memset and one launch on the context's stream; neither entry synchronises.                                */
enum { EVH_RESIDUAL_ABS = 0, EVH_RESIDUAL_MASK = 1 };
enum { EVH_RES_COVERED = 0, EVH_RES_SAD, EVH_RES_SSD, EVH_RES_SAD0, EVH_RES_SSD0, EVH_RES_MOVING, EVH_RES_NSTATS };  /* 6 */
int evh_pair_residual(evh_ctx* ctx, const uint8_t* d_frames, int npairs, int frame_step /* 1 | 2 */, int w, int h,
                      int channels /* 1 | 3 */, int64_t row_stride, int64_t frame_stride,
                      const double* d_M /* f64[npairs,9] DEVICE */, int threshold /* 0..255 */,
                      uint64_t* d_stats /* u64[npairs,6] DEVICE */,
                      uint8_t* d_out /* may be NULL */, int kind, int64_t out_row_stride, int64_t out_frame_stride);
int evh_pair_residual_yuv420(evh_ctx* ctx, const evh_yuv420* src, int npairs, int frame_step, int w, int h,
                             const double* d_M, int threshold, uint64_t* d_stats,
                             uint8_t* d_out, int kind, int64_t out_row_stride, int64_t out_frame_stride);

/* ---- direct alignment: a pair's matrix refined on the pixels ---------------------------------------------------------------------- */
/* evh_pair_residual judges a matrix; this entry improves it: inverse-compositional Gauss-Newton with Levenberg damping on the
 * photometric residual, starting from d_M_in.  Frames, npairs, frame_step, w, h, channels and strides are evh_pair_residual's;
 * d_M_in f64[npairs,9] (DEVICE) maps pixels of the current frame to pixels of the previous frame.  tests/refine_checks.py restates
 * all of the following in numpy and is the definition where this text is unclear.
 * COST of a matrix M: (covered, ssd) = evh_pair_residual's [EVH_RES_COVERED] and [EVH_RES_SSD] for M -- the same coverage, byte
 *   samples and gray weights, exact integers.  A is BETTER than B iff ssd_A * covered_B < ssd_B * covered_A, compared exactly (the
 *   products reach 2^78: 128 bits).
 * NORMAL EQUATIONS at M, over the pixels (x, y) that are covered, interior (1 <= x <= w-2, 1 <= y <= h-2) and have |r| <= clip:
 *   r = g_cur - g_reg (signed), gx = g_cur(x+1, y) - g_cur(x-1, y), gy = g_cur(x, y+1) - g_cur(x, y-1) (gray values of the current
 *   frame), X = 2x - (w-1), Y = 2y - (h-1), s = gx*X + gy*Y, J = (gx*X, gx*Y, gx, gy*X, gy*Y, gy, -X*s, -Y*s): exact integers
 *   below 2^53 for w, h <= 4096.  Each entry is converted to double; each product J_i*J_j (i <= j) and J_i*r is ONE rounded double
 *   multiplication, accumulated in double.  The EVH_REFINE_NSUMS = 45 sums: [0..35] the upper triangle of J'J row by row ((0,0),
 *   (0,1) .. (0,7), (1,1) .. (7,7)), [36..43] J'r, [44] the number of pixels n.  The order of summation is fixed by the launch
 *   geometry (which depends on w and h only): a fixed assignment of pixels to threads, a fixed tree inside a workgroup, the
 *   workgroups' partial sums added in index order.  No floating-point atomics: the same call twice gives the same bytes.
 * STEP from the sums (A = J'J, b = J'r) and the damping lambda: d_i = sqrt(A_ii), Ah = A_ij / (d_i d_j) + lambda * I,
 *   bh = b_i / d_i, Ah y = bh solved by an 8x8 LDL' in double, Delta_i = -4 y_i / d_i (4: doubled coordinates and doubled
 *   differences).  P = I + [[D0, D1, D2], [D3, D4, D5], [D6, D7, 0]], C = [[2, 0, -(w-1)], [0, 2, -(h-1)], [0, 0, 1]],
 *   Q = C^-1 P C (C^-1 = [[.5, 0, (w-1)/2], [0, .5, (h-1)/2], [0, 0, 1]], the two products left to right), M_try = M * adj(Q)
 *   divided by its [2][2] (adj: the adjugate as evh_warp_fixed_plane forms it; the determinant goes with the normalisation).
 * LOOP: lambda = 1e-3; the first evaluation is at M_in; evaluation k = 1 .. iters is at M_try and is ACCEPTED iff
 *   covered_try > 0, 10 * covered_try >= 9 * covered_in and it is better than the current matrix: then M, its cost and its sums
 *   become the trial's and lambda = max(lambda / 10, 1e-9); else lambda = 10 * lambda.  A pair STOPS, and later launches skip
 *   it, when M_in covers nothing (a NaN, zero, singular-with-tw-0 or otherwise non-finite matrix covers nothing), when n < 64 at
 *   the current matrix, when a d_i is 0, when Delta or M_try is not finite.
 * d_M_out f64[npairs,9]: the last accepted matrix; without an accepted step the nine input doubles byte for byte, NaNs
 *   included.  d_M_out may BE d_M_in (any other overlap is refused).
 * d_info u64[npairs,EVH_REFINE_NINFO]: [EVH_REFINE_STATUS] EVH_REFINE_REFINED when a step was accepted, else the reason the pair
 *   stopped (NOTHING_COVERED, TOO_FEW: n < 64, DEGENERATE: a zero d_i or a non-finite step), else EVH_REFINE_UNCHANGED;
 *   [EVALS] evaluations made, [ACCEPTED] steps accepted, [COVERED_IN], [SSD_IN] the cost of M_in, [COVERED_OUT], [SSD_OUT] the cost of
 *   d_M_out, [N_IN] n at M_in.
 * d_normal f64[npairs,45] (may be NULL): the sums at M_in (zeros for a pair that covers nothing).
 * Launches: iters + 1 evaluations (grid.y = pair, a fixed number of workgroups per pair striding over the runs of 4 pixels), each
 * followed by one launch of the solving kernel, which adds the partial sums, judges the trial and forms the next one; the last one
 * only judges and writes the results.  All on the context's stream, no host synchronisation (a first call, or one that needs a
 * larger workspace than any before, allocates: the workspace belongs to the context and grows on demand).
 * Refused before anything is launched, outputs untouched -- EVH_ERR_INVALID: NULL frames (a NULL plane), d_M_in, d_M_out or d_info,
 * channels not 1 or 3, frame_step not 1 or 2, w or h < 1, npairs < 0, iters outside 0..64, clip outside 0..255, a frame stride
 * shorter than its row / frame, an output overlapping the frames, another output or (other than d_M_out == d_M_in) d_M_in;
 * EVH_ERR_CAPACITY: w or h > 4096, npairs > 65535.  npairs == 0 succeeds and does nothing.  The plane form converts every pixel and
 * tap as evh_yuv420_to_bgr does: it equals evh_yuv420_to_bgr followed by the BGR form.                                           */
enum { EVH_REFINE_REFINED = 0, EVH_REFINE_UNCHANGED, EVH_REFINE_NOTHING_COVERED, EVH_REFINE_TOO_FEW, EVH_REFINE_DEGENERATE };
enum { EVH_REFINE_STATUS = 0, EVH_REFINE_EVALS, EVH_REFINE_ACCEPTED, EVH_REFINE_COVERED_IN, EVH_REFINE_SSD_IN,
       EVH_REFINE_COVERED_OUT, EVH_REFINE_SSD_OUT, EVH_REFINE_N_IN, EVH_REFINE_NINFO };  /* 8 */
enum { EVH_REFINE_NSUMS = 45, EVH_REFINE_MIN_PIXELS = 64, EVH_REFINE_MAX_ITERS = 64, EVH_REFINE_MAX_SIZE = 4096 };
int evh_pair_refine(evh_ctx* ctx, const uint8_t* d_frames, int npairs, int frame_step /* 1 | 2 */, int w, int h,
                    int channels /* 1 | 3 */, int64_t row_stride, int64_t frame_stride,
                    const double* d_M_in /* f64[npairs,9] DEVICE */, int iters /* 0..64 */, int clip /* 0..255 */,
                    double* d_M_out /* f64[npairs,9] DEVICE */, uint64_t* d_info /* u64[npairs,8] DEVICE */,
                    double* d_normal /* f64[npairs,45] DEVICE, may be NULL */);
int evh_pair_refine_yuv420(evh_ctx* ctx, const evh_yuv420* src, int npairs, int frame_step, int w, int h,
                           const double* d_M_in, int iters, int clip, double* d_M_out, uint64_t* d_info, double* d_normal);

/* ---- direct alignment against the mosaic: a frame's matrix refined on a canvas with holes ----------------------------------------- */
/* evh_pair_refine with the previous frame replaced by a canvas: frame k of nframes frames (w x h, packed or planes exactly as for
 * evh_pair_refine) is aligned against d_canvas, dh rows of dw * channels bytes at canvas_row_stride -- the frames' channel count;
 * the plane form takes a BGR canvas -- which need not be valid everywhere.  d_count (may be NULL = every pixel valid): one byte per
 * canvas pixel, rows of dw at count_row_stride, as evh_plate_fixed_plane writes it; min_cover in 1..255 has evh_rows_moving_filter's
 * meaning: a canvas pixel counts where d_count >= min_cover.  d_M_in f64[nframes,9] (DEVICE) maps pixels of frame k to pixels of the
 * canvas (the caller folds the canvas origin in).  tests/canvas_checks.py restates the following in numpy.
 * SAMPLE for pixel (x, y) of frame k: the position, the coverage test, the taps and the rounding of evh_warp_fixed_plane with
 *   A = d_M_in[k], inverse_map != 0, sw = dw, sh = dh and the canvas as the source.  A tap of weight 0 is not read.
 * VALID: every tap of non-zero weight has d_count >= min_cover at its pixel; a count under a tap of weight 0 is not consulted.
 * COVERED = the warp's coverage AND valid.
 * COST, NORMAL EQUATIONS, STEP, LOOP, d_M_out, d_info, d_normal: evh_pair_refine's text with "the previous frame" read as "the
 *   canvas" and "covered" as above: r = g_frame - g_canvas_sample, the gradients and the doubled centred coordinates are the frame's
 *   (its w, h).  iters == 0 makes the entry the score of a frame against the canvas.
 * The launch geometry -- the assignment of runs to threads, the tree, the order of workgroups -- is evh_pair_refine's for the same w, h,
 *   and the solving kernel is the same: with the canvas = the previous frame (dw = w, dh = h) and d_count NULL or valid everywhere,
 *   d_M_out, d_info and d_normal equal evh_pair_refine's for that pair byte for byte.
 * Launches: iters + 1 evaluations (grid.y = frame), each followed by evh_pair_refine's solving kernel, on the same context workspace;
 *   no host synchronisation.
 * Refused before anything is launched, outputs untouched -- EVH_ERR_INVALID: NULL frames (a NULL plane), d_canvas, d_M_in, d_M_out or
 * d_info, channels not 1 or 3, w, h, dw or dh < 1, nframes < 0, iters outside 0..64, clip outside 0..255, min_cover outside 1..255
 * (looked at only when d_count is given), a stride shorter than its row / frame (the frame stride when nframes > 1), an output
 * overlapping the frames, the canvas, d_count, another output or (other than d_M_out == d_M_in) d_M_in; EVH_ERR_CAPACITY: w or
 * h > 4096, dw or dh >= 2^26, dw*dh > INT_MAX, nframes > 65535.  nframes == 0 succeeds and does nothing.  The plane form converts every
 * pixel of a frame as evh_yuv420_to_bgr does: it equals evh_yuv420_to_bgr followed by the BGR form.                              */
int evh_canvas_refine(evh_ctx* ctx, const uint8_t* d_frames, int nframes, int w, int h, int channels /* 1 | 3 */, int64_t row_stride,
                      int64_t frame_stride, const uint8_t* d_canvas, int dw, int dh, int64_t canvas_row_stride,
                      const uint8_t* d_count /* may be NULL */, int64_t count_row_stride, int min_cover /* 1..255 */,
                      const double* d_M_in /* f64[nframes,9] DEVICE */, int iters /* 0..64 */, int clip /* 0..255 */,
                      double* d_M_out /* f64[nframes,9] DEVICE */, uint64_t* d_info /* u64[nframes,8] DEVICE */,
                      double* d_normal /* f64[nframes,45] DEVICE, may be NULL */);
int evh_canvas_refine_yuv420(evh_ctx* ctx, const evh_yuv420* src, int nframes, int w, int h, const uint8_t* d_canvas, int dw, int dh,
                             int64_t canvas_row_stride, const uint8_t* d_count, int64_t count_row_stride, int min_cover,
                             const double* d_M_in, int iters, int clip, double* d_M_out, uint64_t* d_info, double* d_normal);

/* ---- points followed between frames: sparse pyramidal Lucas-Kanade in integers ------------------------------------------------------ */
/* Where descriptors find nothing to match -- defocus, blur, fog, low contrast: gradients but no corners -- points of the current
 * frame are followed into the previous one on the pixels.  Frames, npairs, frame_step, w, h, channels and strides are
 * evh_pair_residual's: pair p has the previous frame p*frame_step and the current frame p*frame_step + 1.  d_pts f32[npairs][pt_cap][2]
 * holds points (x, y) of the CURRENT frame, d_npts i32[npairs] how many (above pt_cap: pt_cap, negative: 0); d_M f64[npairs,9] (may be
 * NULL = identity) maps pixels of the current frame to pixels of the previous one and is only the first guess.  The result is a PURE
 * FUNCTION of the inputs -- integer sums, one rounded double operation at a time in the 2x2 solve, no atomics -- and
 * tests/track_checks.py restates all of the following in numpy, for equality; it is the definition where this text is unclear.
 * GRAY: (b*1868 + g*9617 + r*4899 + 8192) >> 14, with one channel the byte.  LEVEL l (l < levels) is level l-1 reduced by 2x2 means,
 *   (a + b + c + d + 2) >> 2, of size (w_{l-1} >> 1, h_{l-1} >> 1): an odd last column or row is dropped.  A level with a side < 2 does
 *   not exist, nor do the levels above it.
 * POSITIONS are integers in 1/32 pixel.  A0 = (rint(32 x), rint(32 y)) in double, halves to even; the point is EVH_TRACK_BAD_POINT
 *   unless 0 <= A0 <= (32 (w-1), 32 (h-1)) (NaN and +-inf fail).  B0 = evh_warp_fixed_plane's (U, V) for A = d_M[p], inverse_map != 0,
 *   at (X, Y) = A0 / 32; B0 = A0 without d_M, or when |U| or |V| is not <= EVH_TRACK_GUESS_MAX (a NaN, zero or huge matrix).
 *   One level down: P_l = (P_{l-1} - 16) >> 1, arithmetic shift (the centre of a 2x2 mean lies at +0.5); one level up: P_{l-1} =
 *   2 P_l + 16.  A_l always comes from A0; B is taken down to the top level once and then carried up.
 * SAMPLE S(img, X, Y) = p00 (32-fx)(32-fy) + p01 fx (32-fy) + p10 (32-fx) fy + p11 fx fy with x = X >> 5, fx = X & 31 (rows alike):
 *   evh_warp_fixed_plane's bilinear sum before its shift.  A tap of weight 0 is not read.  It is defined iff 0 <= X <= 32 (w_l - 1) and
 *   0 <= Y <= 32 (h_l - 1).
 * A LEVEL, radius r, n = (2r+1)^2 window offsets (i, j): T(i, j) = S(cur_l, A_l + 32 (i, j)) for |i|, |j| <= r + 1; gx = T(i+1, j) -
 *   T(i-1, j), gy = T(i, j+1) - T(i, j-1); Gxx, Gxy, Gyy = the sums of gx gx, gx gy, gy gy over the window, exact integers below 2^48,
 *   converted to double; det = Gxx Gyy - Gxy Gxy.  Then, k = 0, 1, ...: d = S(prev_l, B_l + 32 (i, j)) - T(i, j), err = sum |d|,
 *   bx = sum d gx, by = sum d gy (exact integers, converted); after `iters` steps the level ends; else dx = (Gyy bx - Gxy by) / det,
 *   dy = (Gxx by - Gxy bx) / det, step = (rint(-64 dx), rint(-64 dy)), each component clamped to +-32 r (64: the differences are doubled,
 *   positions are 1/32 pixel); a step (0, 0) ends the level, any other is added to B_l.
 * FAILURES.  A level fails when the template (|i|, |j| <= r + 1 around A_l) is not defined everywhere, when det is not > 0, or when
 *   the search window (|i|, |j| <= r around B_l) is not defined at some k.  Above level 0 such a level is skipped: B_l stays what it was
 *   when the level began.  At level 0 the point is dropped: EVH_TRACK_NO_WINDOW, EVH_TRACK_FLAT or EVH_TRACK_LEFT_FRAME, in this order
 *   of the checks; EVH_TRACK_FLAT also when lambda = ((Gxx + Gyy) - sqrt((Gxx - Gyy)^2 + 4 Gxy^2)) * 0.5 < (min_eig * n) * 2^22 --
 *   min_eig is the smaller eigenvalue of the mean structure tensor, in gray levels squared per pixel squared.
 * d_err: err at the final B of level 0.  max_err >= 0: a point with err > max_err * n * 1024 is dropped (EVH_TRACK_HIGH_ERROR).
 * FORWARD-BACKWARD (fb_max32 >= 0): the same procedure with the frames exchanged -- the template around the found B in the previous
 *   frame, the search in the current frame starting at A0, giving A'.  The point is dropped (EVH_TRACK_FB_FAILED) when the backward pass
 *   fails at level 0 or max(|A'x - A0x|, |A'y - A0y|) > fb_max32.
 * OUTPUTS.  d_out_rows f32[npairs][row_cap][4]: a kept point's row (A0x/32, A0y/32, Bx/32, By/32) = (ax, ay, bx, by) -- a on the current
 *   frame, b on the previous one, the layout of evh_batch_static_rows; exact in float32 --, compacted IN INPUT ORDER; rows past the
 *   count are untouched.  d_out_counts i32[npairs].  d_flags u8[npairs][pt_cap] (may be NULL): the code of every point below the count;
 *   d_err u32[npairs][pt_cap] (may be NULL): its err, EVH_TRACK_NO_ERR for a point that failed before level 0 was solved.  Entries of points
 *   at or past the count are untouched.  row_cap >= pt_cap.
 * Launches: the gray pyramids of every frame of the call (level 0 fused with the ingest, planes converted as evh_yuv420_to_bgr does),
 * one wave per point with levels, iterations and the backward pass inside the kernel, one workgroup per pair for the compaction;
 * all on the context's stream, no host synchronisation (the workspace belongs to the context and grows on demand).
 * Refused before anything is launched, outputs untouched -- EVH_ERR_INVALID: NULL frames (a NULL plane), d_pts, d_npts, d_out_rows or
 * d_out_counts, channels not 1 or 3, frame_step not 1 or 2, w or h < 1, npairs < 0, pt_cap < 1, row_cap < pt_cap, levels outside 1..4,
 * radius outside 1..10, iters outside 1..64, min_eig negative or not finite, max_err outside -1..255, a frame stride shorter than its
 * row / frame, an output overlapping another output, the frames, d_pts, d_npts or d_M; EVH_ERR_CAPACITY: w or h > 4096, npairs > 65535,
 * pt_cap > 65535.  npairs == 0 succeeds and does nothing.                                                                          */
enum { EVH_TRACK_TRACKED = 0, EVH_TRACK_BAD_POINT, EVH_TRACK_NO_WINDOW, EVH_TRACK_LEFT_FRAME, EVH_TRACK_FLAT, EVH_TRACK_HIGH_ERROR,
       EVH_TRACK_FB_FAILED, EVH_TRACK_NFLAGS };  /* 7 */
enum { EVH_TRACK_MAX_LEVELS = 4, EVH_TRACK_MAX_RADIUS = 10, EVH_TRACK_MAX_ITERS = 64, EVH_TRACK_MAX_SIZE = 4096,
       EVH_TRACK_GUESS_MAX = 1 << 24 };
#define EVH_TRACK_NO_ERR 0xFFFFFFFFu
int evh_track_points(evh_ctx* ctx, const uint8_t* d_frames, int npairs, int frame_step /* 1 | 2 */, int w, int h,
                     int channels /* 1 | 3 */, int64_t row_stride, int64_t frame_stride,
                     const float* d_pts /* f32[npairs,pt_cap,2] DEVICE */, const int32_t* d_npts /* i32[npairs] DEVICE */, int pt_cap,
                     const double* d_M /* f64[npairs,9] DEVICE, may be NULL */, int levels /* 1..4 */, int radius /* 1..10 */,
                     int iters /* 1..64 */, double min_eig, int fb_max32 /* < 0: off */, int max_err /* -1 | 0..255 */,
                     float* d_out_rows /* f32[npairs,row_cap,4] DEVICE */, int row_cap, int32_t* d_out_counts /* i32[npairs] DEVICE */,
                     uint8_t* d_flags /* u8[npairs,pt_cap] DEVICE, may be NULL */, uint32_t* d_err /* u32[npairs,pt_cap] DEVICE, may be NULL */);
int evh_track_points_yuv420(evh_ctx* ctx, const evh_yuv420* src, int npairs, int frame_step, int w, int h, const float* d_pts,
                            const int32_t* d_npts, int pt_cap, const double* d_M, int levels, int radius, int iters, double min_eig,
                            int fb_max32, int max_err, float* d_out_rows, int row_cap, int32_t* d_out_counts, uint8_t* d_flags,
                            uint32_t* d_err);

/* Points worth following on frames where FAST finds none.  Per frame of nframes frames (packed or planes as above), on the gray values
 * of level 0: gx = g(x+1, y) - g(x-1, y), gy = g(x, y+1) - g(x, y-1); Gxx, Gxy, Gyy summed over the (2 radius + 1)^2 window around a
 * pixel (exact integers), lambda from them as above.  The rectangle [border, w-1-border] x [border, h-1-border] is tiled from its
 * top-left corner by cells of cell x cell pixels (partial cells at the right and at the bottom count).  Per cell the pixel of largest
 * lambda is taken, ties to the smallest (y, x); it is a seed iff lambda >= (min_eig * n) * 4, n = (2 radius + 1)^2 -- min_eig in
 * evh_track_points's unit.  d_pts f32[nframes][pt_cap][2] receives the seeds (x, y) in cell raster order, d_npts i32[nframes] their
 * full count, also where it exceeds pt_cap (only pt_cap are written; slots past the seeds are untouched).  A border above
 * (w - 1) / 2 or (h - 1) / 2, up to INT_MAX, leaves an empty rectangle, which gives 0 seeds.  tests/track_checks.py restates it, for equality.  Two launches (cells, compaction) on the context's stream, no host
 * synchronisation.  Refused before anything is launched, outputs untouched -- EVH_ERR_INVALID: NULL frames (a NULL plane), d_pts or
 * d_npts, channels not 1 or 3, w or h < 1, nframes < 0, pt_cap < 1, radius outside 1..3, cell outside 8..64, border < radius + 1,
 * min_eig negative or not finite, a frame stride shorter than its row / frame (the frame stride when nframes > 1), an output
 * overlapping the other or the frames; EVH_ERR_CAPACITY: w or h > 4096, nframes > 65535, pt_cap > 65535.  nframes == 0 succeeds and
 * does nothing.                                                                                                                    */
int evh_track_seeds(evh_ctx* ctx, const uint8_t* d_frames, int nframes, int w, int h, int channels /* 1 | 3 */, int64_t row_stride,
                    int64_t frame_stride, int radius /* 1..3 */, int cell /* 8..64 */, int border /* >= radius + 1 */, double min_eig,
                    float* d_pts /* f32[nframes,pt_cap,2] DEVICE */, int pt_cap, int32_t* d_npts /* i32[nframes] DEVICE */);
int evh_track_seeds_yuv420(evh_ctx* ctx, const evh_yuv420* src, int nframes, int w, int h, int radius, int cell, int border,
                           double min_eig, float* d_pts, int pt_cap, int32_t* d_npts);

/* ---- pictures encoded on the device: baseline JPEG -------------------------------------------------------------------------
 * evh_jpeg_encode writes, for each of n pictures (gray, or BGR as every canvas here is), a complete baseline JFIF file to
 * d_out + p * out_stride; only the compressed bytes have to cross the host link.  Every step is stated in integers, so a file is
 * a PURE FUNCTION of the pixels, the two tables and the layout; tests/jpeg_checks.py restates all of it in numpy, for equality
 * of the bytes, and is the definition where this text is unclear.
 * FILE: SOI | APP0 (JFIF 1.01, no units, 1:1, no thumbnail) | DQT table 0 (8-bit, zig-zag order) | with three channels DQT
 *   table 1 | SOF0 (8 bits, h, w; component ids 1 2 3; Y samples 1x1, with EVH_JPEG_420 2x2; Y uses table 0, Cb Cr table 1) |
 *   DHT DC 0 | DHT AC 0 | DHT DC 1 | DHT AC 1 -- the four tables of T.81 Annex K.3, always, each a segment of its own | DRI |
 *   SOS (Y: tables 0/0, Cb Cr: 1/1; 0, 63, 0) | the scan | EOI.  That head is 550 bytes with one channel, 629 with three.
 * COLOUR (three channels): Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) +
 *   32767) >> 16, Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16 (arithmetic shifts; the rows sum to 65536, 0, 0, so
 *   every value lies in 0..255 unclamped).  One channel: Y is the byte.
 * GEOMETRY: an MCU is 8 x 8 pixels, with EVH_JPEG_420 16 x 16 (blocks Y0 Y1 / Y2 Y3, then Cb, Cr); otherwise its blocks are Y
 *   [, Cb, Cr].  A pixel past the right or bottom edge is the last pixel of its row / column.  A 4:2:0 chroma sample is
 *   (a + b + c + d + 2) >> 2 of the 2 x 2 converted values, taken after that padding.  Every sample s has 128 subtracted.
 * TRANSFORM: T[u][x] = rint(8192 * c(u) / 2 * cos((2 x + 1) u pi / 16)), c(0) = 1 / sqrt 2, c(u > 0) = 1; the rows are
 *   u = 0:  2896  2896  2896  2896  2896  2896  2896  2896      u = 4:  2896 -2896 -2896  2896  2896 -2896 -2896  2896
 *   u = 1:  4017  3406  2276   799  -799 -2276 -3406 -4017      u = 5:  2276 -4017   799  3406 -3406  -799  4017 -2276
 *   u = 2:  3784  1567 -1567 -3784 -3784 -1567  1567  3784      u = 6:  1567 -3784  3784 -1567 -1567  3784 -3784  1567
 *   u = 3:  3406  -799 -4017 -2276  2276  4017   799 -3406      u = 7:   799 -2276  3406 -4017  4017 -3406  2276  -799
 *   Rows first: A[y][u] = (sum_x T[u][x] s[y][x] + 128) >> 8 (five fraction bits stay); then columns:
 *   F[v][u] = (sum_y T[v][y] A[y][u] + (1 << 17)) >> 18.  Both sums fit 32 bits (|A| <= 11585, second sum below 2^29); F lies within
 *   1 of the float64 orthonormal DCT-II (measured: tests/test_jpeg_host.py).
 * QUANTISATION: q = sign(F) * ((|F| + (Q >> 1)) / Q), Q = qtab[0][8 v + u] for Y, qtab[1][8 v + u] for Cb and Cr.
 * SCAN: baseline Huffman with the Annex K.3 tables; the coefficients of a block in zig-zag order; DC as the difference to the
 *   previous block of the same component, category = bit length of |d|, a negative d sent as d - 1 in that many bits; AC as
 *   (run, size) with ZRL (0xF0) for each 16 zeros of a run and EOB (0x00) unless coefficient 63 is non-zero.  The restart interval is
 *   ONE MCU ROW, always: DRI = ceil(w / mcu_w).  Each interval is padded to a byte with 1-bits, the DC prediction starts at 0
 *   in each, RSTm with m = row mod 8 stands between intervals (none after the last), and a 0xFF data byte is followed by 0x00.
 *   An MCU row's bytes are thus a function of its own pixels.
 * BOUND: a block has at most 20 bits of DC (a 9-bit code, 11 bits) and 63 * 26 of AC (a 16-bit code, 10 bits) = 1658 bits
 *   (an 8-bit sample cannot reach an AC magnitude of 1024: sum |basis| * 128 <= 1024 is not met with equality by samples in
 *   -128..127).  A row of B blocks has at most ceil(1658 B / 8) bytes before stuffing, at most twice that after, and 2 of a
 *   marker: evh_jpeg_bound = head + rows * (2 * ceil(1658 B / 8) + 2) + 2, or -1 for arguments evh_jpeg_encode refuses.
 * evh_jpeg_header writes the head (SOI..SOS) to `out` and returns its length, or EVH_ERR_INVALID for the arguments
 * evh_jpeg_encode refuses, a NULL pointer, or cap below that length (nothing is written then).  Both are host functions and need
 * no context.
 * evh_jpeg_encode: d_pictures u8, picture p at d_pictures + p * picture_stride, its rows row_stride bytes apart, pixels packed
 * (B, G, R with three channels); qtab is a HOST array u16[2][64] in natural (row-major) order, every entry in 1..255 (both tables
 * are checked, also with one channel).  d_out_bytes[p] receives the file's length, ALSO where it exceeds out_cap: then the first
 * out_cap bytes of the file are written, nothing at or past d_out + p * out_stride + out_cap, and the other pictures are not
 * affected.  Bytes of a slot past the file's end are untouched.  The context keeps a workspace that grows on demand (128 bytes of
 * coefficients and 8 of lengths per block, the rows' bit buffers at the bound above); six launches and one clearing of the bit
 * buffers on the context's stream, no host synchronisation.  Refused before anything is launched, outputs untouched --
 * EVH_ERR_INVALID: a NULL context, d_pictures, qtab, d_out or d_out_bytes, n < 0, w or h outside 1..65535, channels not 1 or 3,
 * a subsampling other than the two or EVH_JPEG_420 with one channel, a table entry outside 1..255, row_stride < w * channels,
 * out_cap < 0, out_stride < out_cap.  n == 0 succeeds and does nothing.                                                      */
enum { EVH_JPEG_444 = 0, EVH_JPEG_420 = 1 };
int64_t evh_jpeg_bound(int w, int h, int channels, int subsampling);
int evh_jpeg_header(int w, int h, int channels, int subsampling, const uint16_t* qtab /* HOST u16[2][64] */, uint8_t* out, int cap);
int evh_jpeg_encode(evh_ctx* ctx, const uint8_t* d_pictures, int n, int w, int h, int64_t row_stride, int64_t picture_stride,
                    int channels /* 1 gray | 3 BGR */, int subsampling /* EVH_JPEG_444 | EVH_JPEG_420 */,
                    const uint16_t* qtab /* HOST u16[2][64], natural order, each 1..255 */, uint8_t* d_out /* DEVICE */,
                    int64_t out_stride, int64_t out_cap, int64_t* d_out_bytes /* i64[n] DEVICE */);

/* ---- ragged batches of several streams: many videos or cameras in one call ----------------------------------------------- */
/* One stream's share of a batch: nframes consecutive frames starting at frame first_frame of the batch's one frame buffer.  */
typedef struct evh_stream_seg {
  int32_t first_frame;  /* index of the segment's first frame in the batch                          */
  int32_t nframes;      /* >= 2 consecutive frames -> nframes - 1 pairs                             */
  int32_t start;        /* non-zero: the stream starts in this call; its d_state_in row is not read */
  int32_t reserved;     /* 0 */
} evh_stream_seg;
/* evh_multi_stream_homography_batch for streams of unequal length that start and end in different calls, with the ingests and
 * the feature type lists of the single-stream entries: what get_homography_dicts (several captures at once) runs per round.
 * d_frames holds total_frames frames of src_w x src_h, working size (w, h) as in evh_stream_homography_batch_resized (equal
 * sizes = no resize); h_segs cuts them into nstreams segments that tile [0, total_frames) in ascending order (anything else,
 * a segment of fewer than 2 frames, or reserved != 0: EVH_ERR_INVALID; total_frames > max_frames: EVH_ERR_CAPACITY).  Pair
 * slot p is (frame p + 1, frame p) as in the stream entries; pair k of a segment writes d_H[first_frame + k] and
 * d_status[first_frame + k] (d_H f64[total_frames - 1][9], d_status i32[total_frames - 1]); the row at a segment's last frame
 * belongs to no stream and is never written.  d_state_in / d_state_out f64[nstreams][18] carry {H_sup, H_prev} of stream s in
 * row s and may be the same buffer; a segment with start != 0 does not read its row, and d_state_in may be NULL only when every
 * segment starts here (else EVH_ERR_INVALID).  h_types as in evh_stream_homography_batch_types: a list of exactly
 * {EVH_FEATURE_ORB} takes the fused ORB path (with asynchronous solve when enabled), any other list the multi-type path; a
 * bad list, a type named twice, SIFT / SURF without their _enable are refused with the codes of that entry.  Every refusal
 * comes before the first launch: the outputs are untouched.  Everything up to the static filter runs over all frames and pair
 * slots at once; the sequential scans then run concurrently, one workgroup per stream, a shorter stream leaving early (with
 * force_max_iters the per-pair launches run up to the longest stream).  Per stream the results are bit-identical to that stream
 * alone through evh_stream_homography_batch[_resized|_types] in the same chunks.  Does not synchronise.                        */
int evh_streams_homography_batch(evh_ctx* ctx, const uint8_t* d_frames, int total_frames, int src_w, int src_h, int channels,
                                 int64_t row_stride, int64_t frame_stride, int w, int h, int nfeatures, const int32_t* h_types,
                                 int ntypes, const evh_stream_seg* h_segs, int nstreams, double ransac_thr, int ransac_max_iters,
                                 double ransac_conf, int force_max_iters, const double* d_state_in, double* d_state_out,
                                 double* d_H, int32_t* d_status);
/* The same on decoded 4:2:0 planes (total_frames frames behind one evh_yuv420): the {ORB} list takes level 0 straight from the
 * planes as evh_stream_homography_batch_yuv420 does, any other list converts the batch once as
 * evh_stream_homography_batch_types_yuv420 does.  Bit-identical to the BGR form on the frames the planes convert to.          */
int evh_streams_homography_batch_yuv420(evh_ctx* ctx, const evh_yuv420* src, int total_frames, int src_w, int src_h, int w, int h,
                                        int nfeatures, const int32_t* h_types, int ntypes, const evh_stream_seg* h_segs,
                                        int nstreams, double ransac_thr, int ransac_max_iters, double ransac_conf,
                                        int force_max_iters, const double* d_state_in, double* d_state_out, double* d_H,
                                        int32_t* d_status);

/* ---- global alignment: the normal equations of one joint least-squares problem over all superposed matrices --------------------- */
/* Every coordinate the library hands out goes through S_k, a product of k pair matrices.  This entry turns the match rows of
 * ARBITRARY frame pairs ("edges": consecutive frames and frames that see the same ground again) into the normal equations of one
 * problem over all S_k; the solve is the host's (evenvizion_amd/graph.py).  tests/graph_checks.py restates all of the following in
 * numpy float64 and is the definition where this text is unclear.  All buffers are DEVICE buffers.
 * d_S f64[nframes][9]: S_k takes pixels of frame k to the plane.  d_edges i32[nedges][2] = (i, j).  d_rows f32[nedges][row_cap][4]:
 * rows (ax, ay, bx, by) in the layout of evh_batch_static_rows, a = the point in frame i (the CURRENT frame of a pair slot),
 * b = the point in frame j (the PREVIOUS frame).  Edge e reads rows r < n = min(max(d_counts[e], 0), row_cap): a count above
 * row_cap is taken as row_cap, a negative one as 0, as in evh_draw_matches.  d_status (may be NULL): i32[nedges].  d_H_edge (may be
 * NULL): f64[nedges][9], the matrix of the pair, which maps a onto b -- the direction of compute_homography(pts_a, pts_b), whose
 * residual is H.a - b (evh_compute_homography, evh_pair_homography_batch: what EVH_MODE_INDEPENDENT_PAIRS returns for the slot
 * (frame j, frame i) = (prev, cur)).
 * Per row, IEEE float64 with one rounding per operation (the library is built with -ffp-contract=off), after ax, ay, bx, by have
 * been converted to double:
 *   1. Plane points.  (tx, ty, tw) = (fma(s0, ax, s1*ay) + s2, fma(s3, ax, s4*ay) + s5, fma(s6, ax, s7*ay) + s8) with s = S_i, and
 *      (sx, sy, sw) alike from S_j and (bx, by): the order of evh_transform_points, so U, V below equal its output bit for bit.
 *   2. Validity.  If tw or sw is not finite or is <= 0 the row is skipped and counted in `behind`.
 *   3. Gate, only with d_H_edge: (hx, hy, hw) from H_e and (ax, ay) as in 1; gx = hx / hw - bx, gy = hy / hw - by; the row is used
 *      iff gx*gx + gy*gy <= inlier_thr*inlier_thr (both products rounded, then the sum), otherwise it is counted in `gated` (a NaN
 *      compares false: gated).  No validity rule applies to hw.
 *   4. U = tx / tw, V = ty / tw (P_i); X = sx / sw, Y = sy / sw (P_j).  Residual ru = U - X, rv = V - Y, in plane units.
 *   5. Weight.  q = ru*ru + rv*rv.  With huber_delta <= 0, or q <= d*d (d = huber_delta): w = 1, rho = q.  Else s = sqrt(q),
 *      w = d / s, rho = (2*d)*s - d*d.
 * Steps 1 to 5 fix used, gated, behind and the atoms U, V, X, Y, ru, rv, q, w, rho of every used row bit for bit.
 * The unknown of frame k is a correction D_k = I + Delta_k composed on the left, S'_k = D_k . S_k, Delta_k = (d0 d1 d2; d3 d4 d5;
 * d6 d7 0).  At Delta = 0 the derivatives of a plane point P = (U, V) are Ju(P) = (U, V, 1, 0, 0, 0, -U*U, -U*V) and
 * Jv(P) = (0, 0, 0, U, V, 1, -U*V, -V*V); J_i = J(P_i), J_j = -J(P_j).
 * d_sums f64[nedges][EVH_GRAPH_NSUMS], over the used rows of the edge:
 *   [0..35]    the upper triangle, row-major, of A_ii = sum w (Ju_i^T Ju_i + Jv_i^T Jv_i)
 *   [36..71]   the same of A_jj
 *   [72..135]  A_ij = sum w (Ju_i^T Ju_j + Jv_i^T Jv_j), the full 8 x 8 block, row = parameter of frame i
 *   [136..143] g_i = sum w (Ju_i ru + Jv_i rv)        [144..151] g_j
 *   [152]      sum rho                                  [153] sum q
 * Every entry is, up to one sign, a sum of TERMS, a term being w (for the gradients w*ru or w*rv) times a product of up to four of
 * U, V, X, Y: one term per row for most entries, two (the u and the v part) for rows and columns 6 and 7 among themselves and for
 * g[6], g[7]; entries that are structurally zero hold +0.0.  The device forms a term with at most four roundings and adds the
 * terms in an order fixed by the row index alone (row r belongs to lane r mod 256; lanes, then the four waves, are added in a fixed
 * tree; no atomics), so an edge's sums are a pure function of that edge's rows, counts, matrices and the two parameters, wherever
 * the edge sits in the list; each lies within (n + 8) * 2^-53 * sum |term| of the exact sum of the exact terms, n = used.  With
 * huber_delta <= 0, [152] and [153] are the same bytes.
 * d_info i32[nedges][4] = {used, gated, behind, flags}.  flags: EVH_GRAPH_BAD_INDEX: i or j outside [0, nframes), or i == j;
 * EVH_GRAPH_BAD_STATUS: d_status given and d_status[e] != EVH_PAIR_OK.  A flagged edge reads no row and no matrix, has all 154
 * sums +0.0 and the three counters 0.  An edge without a used row has +0.0 everywhere too.
 * One launch of nedges workgroups on the context's stream; does not synchronise; only caller buffers are used.  Refused with
 * EVH_ERR_INVALID before anything is enqueued, outputs untouched: a NULL d_S, d_edges, d_rows, d_counts, d_sums or d_info; nframes,
 * nedges or row_cap < 1; nedges > 4 194 304 (2^22 workgroups of 256 threads: a grid of 2^30 threads); a NaN inlier_thr or
 * huber_delta; d_H_edge given with inlier_thr < 0; d_rows not 16-byte aligned (a row is loaded as one vector) or another buffer not
 * aligned to its element.                                                                                                        */
enum { EVH_GRAPH_NSUMS = 154 };
enum { EVH_GRAPH_BAD_INDEX = 1, EVH_GRAPH_BAD_STATUS = 2 };
int evh_graph_normal(evh_ctx* ctx, const double* d_S /* f64[nframes][9] */, int nframes,
                     const int32_t* d_edges /* i32[nedges][2] = (i, j) */, int nedges,
                     const float* d_rows /* f32[nedges][row_cap][4] */, int row_cap, const int32_t* d_counts,
                     const int32_t* d_status /* may be NULL */, const double* d_H_edge /* f64[nedges][9], may be NULL */,
                     double inlier_thr, double huber_delta,
                     double* d_sums /* f64[nedges][EVH_GRAPH_NSUMS] */, int32_t* d_info /* i32[nedges][4] */);

#ifdef __cplusplus
}
#endif
#endif
