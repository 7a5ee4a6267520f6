// evh_internal.h -- shared declarations of libevhip.so (host context + kernel launch prototypes).
// Product code: nothing here (or in any file of this directory) includes or links oracle/.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../../include/evhip.h"

#define EVH_NLEVELS 8
#define EVH_EDGE 31          // ORB edgeThreshold
#define EVH_FAST_THR 20      // ORB fastThreshold
#define EVH_FAST_OX 24       // origin of the FAST tile grid (multiple of 8: the staging loads are 8-byte aligned)
#define EVH_FAST_OY 31
#define EVH_K1CAP 4096       // stage-1 (FAST-score) survivors per level held in LDS
#define EVH_K2CAP 1280       // stage-2 (Harris) survivors per level held in LDS
#define EVH_SEG_TURNS 4      // segment tables of the ragged stream entries in rotation (evh_ctx::d_segs)

struct EvhLevel {
  int w, h, stride;     // stride in bytes (64-byte aligned)
  int quota;            // nfeaturesPerLevel
  float scale;          // layerScale
  int64_t off;          // byte offset inside one frame's pyramid
  int64_t cand_off;     // entry offset inside one frame's candidate buffer
  int cand_cap;
  int tile_start;       // first FAST tile index of this level
  int tiles_x, tiles_y;
  int tab_off;          // offset (ints) of the resize tables of this level inside d_tabs
  int kp_base, kp_cap;  // this level's segment inside a frame's keypoint staging arrays
};

struct EvhGeom {
  int w, h, nfeatures;
  EvhLevel lv[EVH_NLEVELS];
  int64_t pyr_frame_bytes;
  int64_t cand_frame_entries;
  int total_tiles;
};

// N4: SIFT scale-space geometry of one frame size (octave 0 = the frame doubled, 6 Gaussian layers per octave)
#define EVH_SIFT_MAXOCT 13
struct EvhSiftGeom {
  int w, h, noct;
  int ow[EVH_SIFT_MAXOCT], oh[EVH_SIFT_MAXOCT], os[EVH_SIFT_MAXOCT];   // octave width / height / row stride (floats)
  int64_t ooff[EVH_SIFT_MAXOCT];                                       // float offset of an octave's layer 0 inside a frame
  int64_t frame_floats, tmp_floats;
};

// N4: a float detector's (SIFT, SURF) per-frame key-point lists.  A record is 8 floats: x, y, size, angle, response,
// octave bits, (SURF) laplacian bits, 0.  EvhKpDev is the part the kernels are handed.
struct EvhKpDev {
  float* raw = nullptr; int* nraw = nullptr;    // [F][cap][8] key points as detected, [F] how many (may exceed cap)
  float* srt = nullptr;                         // [F][cap][8] in the operator's order
  float* kp = nullptr;                          // [F][cap][8] final records
  float* xy = nullptr;                          // [F][cap][2]
  uint8_t* desc = nullptr;                      // [F][cap] descriptor rows (SIFT: 128 uint8 VALUES 0..255, SURF: 128 float)
  int* count = nullptr; int* flags = nullptr;   // [F] final records; bit0: a buffer of this frame overflowed
  int cap = 0;                                  // records per frame slot (0: the detector is not enabled)
};
struct EvhKpList : EvhKpDev {
  int desc_row_bytes = 0;
  int group = 0;                                // frames whose working buffers (scale space / integral + Hessian) are resident at once
  int frames_resident = 0;                      // frames of the last launch
};

// the frames an entry was handed: packed rows of `channels` bytes per pixel, or (yuv) decoded 4:2:0 planes
struct EvhFrames {
  const uint8_t* packed = nullptr; int channels = 0; int64_t row_stride = 0, frame_stride = 0;
  const evh_yuv420* yuv = nullptr;
  bool planes = false;       // the entry takes planes (yuv may still be NULL: refused with the plane description)
};
inline EvhFrames packed_frames(const uint8_t* d, int channels, int64_t row_stride, int64_t frame_stride) {
  EvhFrames F; F.packed = d; F.channels = channels; F.row_stride = row_stride; F.frame_stride = frame_stride; return F;
}
inline EvhFrames yuv420_frames(const evh_yuv420* src) { EvhFrames F; F.channels = 3; F.yuv = src; F.planes = true; return F; }

// per-pair working buffers of the matching / RANSAC stages (max_pairs = max_frames, row stride `cap` rows per pair)
struct EvhPairBufs {
  int cap = 0;
  int32_t* knn_idx = nullptr;     // [max_pairs][cap][2]
  uint32_t* knn_d2 = nullptr;     // [max_pairs][cap][2]
  float* pts = nullptr;           // [max_pairs][cap][4] matched rows
  float* pts2 = nullptr;          // [max_pairs][cap][4] static rows
  float* crow = nullptr;          // [max_pairs][cap][4] compacted inlier rows
  int* npts = nullptr; int* npts2 = nullptr; int* pstatus = nullptr;   // [max_pairs]
  double* H1 = nullptr;           // [max_pairs][9]
  uint8_t* mask = nullptr;        // [max_pairs][cap]
  double* lm = nullptr;           // [max_pairs][cap][4] LM per-point temporaries
  int* info = nullptr;            // [max_pairs][8]
};

// the 64-double staging area of the single-problem entries (d_small): what each entry keeps where
struct EvhSmall {
  union {                                              // +0: result matrix | ratio filter: row count, status
    double H[16]; int count_status[2];
    struct { int nacc, accstatus, nout, status; } merge;   // evh_remove_double_matching: the one "pair" of k_merge_dup / k_merge
  };
  union {                                              // +16 doubles
    double Hsup[16];                                   // superposition entering a one-pair final solve
    struct { int found, pad_, info[3]; };              // evh_find_homography_ransac*: found flag, +17 doubles: info
    int count;                                         // evh_static_filter: rows kept
  };
  union { int out_status; double tail_[32]; };         // +32 doubles: status of a one-pair final solve
};
static_assert(sizeof(EvhSmall) == 64 * sizeof(double) && offsetof(EvhSmall, Hsup) == 16 * sizeof(double) &&
              offsetof(EvhSmall, info) == 17 * sizeof(double) && offsetof(EvhSmall, out_status) == 32 * sizeof(double),
              "EvhSmall keeps the byte offsets of the 64-double staging area");

struct evh_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  // asynchronous solve: the RANSAC kernels of a batch run on a second stream so that they overlap the next
  // batch's detect kernels (they occupy one wave per SIMD and are latency-bound)
  hipStream_t solve_stream = nullptr;
  hipEvent_t ev_match_done = nullptr, ev_solve_done = nullptr;
  bool async_solve = false, solve_pending = false;
  int max_w = 0, max_h = 0, max_features = 0, max_frames = 0;
  int kcap = 0;  // keypoint rows per frame slot
  EvhGeom g{};
  bool geom_valid = false;
  bool level1_fused = false;   // set by evh_launch_gray_level0: level 1 was produced together with level 0
  int nframes_resident = 0;
  // device buffers
  uint8_t* d_pyr = nullptr;       // [max_frames][pyr_frame_bytes]
  uint32_t* d_cand = nullptr;     // [max_frames][cand_frame_entries]
  int* d_cand_count = nullptr;    // [max_frames][8]
  int* d_tabs = nullptr;          // resize tables for levels 1..7
  int* h_tabs = nullptr;          // pinned staging of the same (configure() uploads stream-ordered, no host sync)
  hipEvent_t ev_tabs = nullptr;   // the last upload out of h_tabs
  float* d_kp_xy = nullptr;       // [max_frames][kcap][2]
  uint32_t* d_kp_meta = nullptr;  // [max_frames][kcap]  level<<24 | y<<12 | x
  float* d_kp_resp = nullptr;     // [max_frames][kcap]
  float* d_kp_angle = nullptr;    // [max_frames][kcap]
  uint8_t* d_desc = nullptr;      // [max_frames][kcap][32]
  int* d_kp_count = nullptr;      // [max_frames]
  int* d_frame_flags = nullptr;   // [max_frames] bit0: capacity overflow
  uint32_t* d_tmp_meta = nullptr; // [max_frames][8][kcap] per-level segments before packing
  float* d_tmp_resp = nullptr;    // [max_frames][8][kcap]
  int* d_lvl_count = nullptr;     // [max_frames][8]
  int* d_fast_thr = nullptr;      // [max_frames][8] lifted FAST threshold
  unsigned* d_fast_hist = nullptr;// [max_frames][8][256] sampled score histogram
  int* d_fast_hint = nullptr;     // [2][8] per-level threshold hint (ping-pong between detect calls) + [8][256] votes + [8] zeros
  int fast_hint_idx = 0;
  double* d_lane_v = nullptr;     // fixed-iteration RANSAC: per-lane eigenvector matrices [max_frames][4][81][64] (lazy)
  int* d_merge_ws = nullptr; size_t merge_ws_bytes = 0;     // k_merge_dup -> k_merge
  int* d_filter_ws = nullptr; size_t filter_ws_bytes = 0;   // k_filter<true>: work arrays of key-point budgets beyond the LDS form
  char* d_scan_ws = nullptr;      // fixed-iteration stream scan: state, sample table and hypothesis results (evh_ransac.hip, lazy)
  size_t scan_ws_bytes = 0;
  int* d_area_tab = nullptr; size_t area_tab_bytes = 0;     // INTER_AREA tables of the last (sw, sh, dw, dh): fused ingest and stand-alone resize alike
  int area_geom[4] = {0, 0, 0, 0}; int area_nx = 0, area_ny = 0;   // {sw, sh, dw, dh} of the tables held, zeros: none
  // segment tables of evh_streams_homography_batch: EVH_SEG_TURNS tables of max_frames / 2 segments each, taken in turn, in
  // pinned staging (h_segs, one event per turn: the host must not overwrite a table whose upload is still queued) and on the
  // device (d_segs, same turns for simplicity: the device side is ordered by the stream anyway -- an upload is enqueued
  // behind the filter of its call, which has waited for the previous call's solve)
  evh_stream_seg* d_segs = nullptr; evh_stream_seg* h_segs = nullptr;
  hipEvent_t ev_segs[EVH_SEG_TURNS] = {};
  unsigned seg_turn = 0;
  uint8_t* d_yuv_bgr = nullptr; size_t yuv_bgr_bytes = 0;   // BGR frames of evh_stream_homography_batch_types_yuv420's chunk
  char* d_refine_ws = nullptr; size_t refine_ws_bytes = 0;  // evh_pair_refine: per-pair state, then the workgroups' partial sums
  char* d_track_ws = nullptr; size_t track_ws_bytes = 0;    // evh_track_points: the gray pyramids, then a record per point; evh_track_seeds: a word per cell
  char* d_jpeg_ws = nullptr; size_t jpeg_ws_bytes = 0;      // evh_jpeg_encode: tables and head, coefficients, code lengths, the rows' bit buffers
  bool trail_tab_ready = false;   // evh_trail_fixed_plane's colour tables are on the device (uploaded by its first launch)
  int* d_fast_redo = nullptr;     // [1 + max_frames*8] redo work list (count first)
  // key-point order of the reference (EVH_ORDER_OPENCV): work arrays of k_select_cv
  int order_mode = 1;             // EVH_ORDER_OPENCV
  int solver_mode = 0;            // EVH_SOLVER_EXACT
  unsigned long long* d_cv_seq = nullptr;   // [max_frames][cand_frame_entries] key << 32 | candidate, row-major then permuted
  uint32_t* d_cv_seq32 = nullptr; // [max_frames][cand_frame_entries] the first retainBest works on the candidates themselves
  uint32_t* d_cv_lpos = nullptr;  // [max_frames][cand_frame_entries] stopper positions of the partition passes
  uint32_t* d_cv_rpos = nullptr;
  int* d_cv_band = nullptr;       // [max_frames][cv_band_frame_entries] corners before each band of FAST tiles, then the level totals (evh_detect_selcv.h)
  uint32_t* d_cv_tdesc = nullptr; // [max_frames][total_tiles][8] FAST tile burst descriptors
  int cv_band_frame_entries = 0;
  bool fast_lift = true;
  bool fast_share = true;         // evh_set_fast_share
  bool fast_hint = true;          // evh_set_fast_hint
  EvhPairBufs orb;                // pair buffers of the ORB path, orb.cap = kcap
  EvhSmall* d_small = nullptr;    // small staging area for single-problem entries (H, counts)
  char* d_scratch = nullptr;      // growable scratch of the host-pointer entries (N1 / N3): no hipMalloc per call
  size_t scratch_bytes = 0;
  // ---- N4: SIFT (allocated by evh_sift_enable) ----
  EvhKpList sift;                 // the key-point lists; records: x, y, size, angle, response, octave bits
  int sift_cand_cap = 0;
  EvhSiftGeom sg{}; bool sift_geom_valid = false;
  int64_t sift_pyr_frame_floats = 0, sift_tmp_frame_floats = 0;
  float* d_sift_pyr = nullptr;    // [group][frame_floats] Gaussian scale space
  float* d_sift_tmp = nullptr;    // [group][octave-0 layer] row-pass temporary
  uint32_t* d_sift_cand = nullptr; int* d_sift_ncand = nullptr;   // extrema: octave<<28 | layer<<26 | r<<13 | c
  // ---- N4: SURF (allocated by evh_surf_enable) ----
  EvhKpList surf;                 // the key-point lists; records: ... octave bits, laplacian bits
  int surf_tab_w = 0, surf_tab_h = 0;
  int64_t surf_sum_frame_ints = 0, surf_det_frame_floats = 0;
  char* d_surf_tabs = nullptr;    // SurfTabs: layer boxes, orientation / descriptor weights
  int* d_surf_sum = nullptr;      // [group] integral images, (h+1) x (w+1)
  float* d_surf_det = nullptr; float* d_surf_trace = nullptr;   // [group] the 20 Hessian layers
  // multi-type pairs (frame_processing.py:91-104): per-type match / static rows, their concatenation, the merged rows
  EvhPairBufs mt;                 // stride mt.cap = kcap + sift.cap + surf.cap
  // the last batch whose static rows (pts2, npts2, pstatus) are still resident: which of orb / mt it used and its pair
  // slots (evh_batch_static_info / _rows); NULL, 0: none.  Set and cleared in evh_batch.hip, by the entries evhip.h names.
  const EvhPairBufs* static_bufs = nullptr; int static_pairs = 0;
  float* d_acc = nullptr; int* d_nacc = nullptr; int* d_accstatus = nullptr;
  std::vector<void**> owned;      // the pointer members above that hold a live hipMalloc (dalloc / grow): what evh_destroy frees
  size_t bytes_allocated = 0;
  std::string err;
  // per-stage timing (evh_profile_*)
  bool profiling = false;
  struct ProfSpan { int stage; hipEvent_t a, b; };
  std::vector<ProfSpan> prof_spans;       // recorded since the last read
  std::vector<hipEvent_t> prof_pool;      // recycled events
};

enum { EVH_ST_GRAY = 0, EVH_ST_PYRAMID, EVH_ST_FAST, EVH_ST_SELECT, EVH_ST_DESCRIBE, EVH_ST_KNN, EVH_ST_FILTER,
       EVH_ST_RANSAC_STATIC, EVH_ST_RANSAC_FINAL };
// RAII bracket: records an event pair around the launches issued while it is alive (no-op unless profiling)
struct EvhProfScope {
  evh_ctx* c; int idx; hipStream_t st;
  EvhProfScope(evh_ctx* ctx, int stage, hipStream_t on = nullptr);
  ~EvhProfScope();
};

int evh_fail(evh_ctx* ctx, int code, const std::string& msg);
#define EVH_HIP(ctx, call)                                                                              \
  do {                                                                                                  \
    hipError_t e_ = (call);                                                                             \
    if (e_ != hipSuccess)                                                                               \
      return evh_fail(ctx, EVH_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));              \
  } while (0)

// ---- device memory of a context: every allocation goes into `p`, a pointer member of *c, and is recorded there ----
template <class T>
int evh_dev_alloc(evh_ctx* c, T** p, size_t bytes) {
  EVH_HIP(c, hipMalloc(reinterpret_cast<void**>(p), bytes));
  c->owned.push_back(reinterpret_cast<void**>(p));
  return EVH_SUCCESS;
}
// fixed-size buffers (counted in bytes_allocated)
template <class T>
int dalloc(evh_ctx* c, T** p, size_t n) {
  int rc = evh_dev_alloc(c, p, n * sizeof(T));
  if (rc == EVH_SUCCESS) c->bytes_allocated += n * sizeof(T);
  return rc;
}
// frees the allocations recorded at position `first` and later (all of them: evh_destroy; the tail: a failed enable)
inline void dfree_from(evh_ctx* c, size_t first) {
  for (size_t i = first; i < c->owned.size(); i++) { (void)hipFree(*c->owned[i]); *c->owned[i] = nullptr; }
  c->owned.resize(std::min(first, c->owned.size()));
}
template <class T>
void dfree(evh_ctx* c, T** p) {
  auto it = std::find(c->owned.begin(), c->owned.end(), reinterpret_cast<void**>(p));
  if (it == c->owned.end()) return;
  (void)hipFree(*p); *p = nullptr;
  c->owned.erase(it);
}
// the lists of a float detector (inside the caller's release-on-failure bracket): max_features records per frame slot,
// descriptor rows of desc_row_bytes; `who` names the entry in the message
inline int alloc_kp_list(evh_ctx* c, EvhKpList& L, const char* who, int max_features, int desc_row_bytes) {
  if (max_features < 64 || max_features > 65536) return evh_fail(c, EVH_ERR_INVALID, std::string(who) + ": capacity out of range (64..65536)");
  const size_t F = (size_t)c->max_frames, cap = (size_t)((max_features + 63) & ~63);
  int rc;
  if ((rc = dalloc(c, &L.raw, F * cap * 8)) || (rc = dalloc(c, &L.nraw, F)) || (rc = dalloc(c, &L.srt, F * cap * 8)) ||
      (rc = dalloc(c, &L.kp, F * cap * 8)) || (rc = dalloc(c, &L.xy, F * cap * 2)) ||
      (rc = dalloc(c, &L.desc, F * cap * desc_row_bytes)) || (rc = dalloc(c, &L.count, F)) || (rc = dalloc(c, &L.flags, F)))
    return rc;
  EVH_HIP(c, hipMemsetAsync(L.count, 0, F * sizeof(int), c->stream));
  EVH_HIP(c, hipMemsetAsync(L.flags, 0, F * sizeof(int), c->stream));
  L.cap = (int)cap; L.desc_row_bytes = desc_row_bytes;
  return EVH_SUCCESS;
}
// frames per group of a float detector: what fits the memory budget, at most what one launch takes (its grid bound), and at
// most EVH_DETECT_GROUP=n where set (tests: several groups at small frames; read at enable time)
inline int kp_group_size(size_t fits, int launch_limit) {
  size_t group = std::max<size_t>(1, std::min<size_t>(fits, (size_t)launch_limit));
  if (const char* e = getenv("EVH_DETECT_GROUP")) if (atoi(e) > 0) group = std::min<size_t>(group, (size_t)atoi(e));
  return (int)group;
}
// grow-on-demand workspace: kernels already enqueued may still use the old one, so the stream drains before it is freed
template <class T>
int grow(evh_ctx* c, T** p, size_t* bytes, size_t need) {
  if (need <= *bytes) return EVH_SUCCESS;
  if (*p) { EVH_HIP(c, hipStreamSynchronize(c->stream)); dfree(c, p); *bytes = 0; }
  int rc = evh_dev_alloc(c, p, need);
  if (rc == EVH_SUCCESS) *bytes = need;
  return rc;
}

// ---- host stages shared by evh_api.hip (which defines them) and evh_batch.hip ----
// one set of per-pair buffers with `cap` rows per pair (the ORB path: kcap; the multi-type path: every type's rows)
int evh_alloc_pair_bufs(evh_ctx* c, EvhPairBufs& B, int cap);
// the argument checks of every entry that takes planes: nothing is launched on a description that fails them
int evh_check_yuv420(evh_ctx* c, const char* who, const evh_yuv420* s, int nframes, int w, int h);
// level 0 (gray) of every frame: (sw, sh) = size of the frames handed over, (w, h) = working size; different sizes = fused
// ingest (N2).  The one place where the frame description of a detect / pair / stream entry is checked and the geometry set.
int evh_ingest_level0(evh_ctx* c, const char* who, const EvhFrames& F, int nframes, int sw, int sh, int w, int h, int nfeatures);
// ORB K2..K6 on the frames whose level 0 is resident; FAST thresholds shared inside groups of share_group frames (0: none)
int evh_orb_stages(evh_ctx* c, int nframes, int share_group);
// entry points that reuse the pair buffers on the main stream first order themselves behind a pending async solve
int evh_join_solve(evh_ctx* c);
// fixed-iteration mode keeps the per-lane eigenvector matrices of its hypotheses in a global scratch, allocated on first use
int evh_ensure_lane_scratch(evh_ctx* c);
// one feature type's per-frame results, as the matching stages and the downloads read them
struct EvhFeatView {
  const int* counts; const int* flags; const float* xy;
  const void* desc; int desc_bytes; bool f32;    // uint8 rows of desc_bytes values, or (f32) rows of 128 floats
  int cap;                                       // rows per frame slot
};
EvhFeatView evh_feat_view(const evh_ctx* c, int type);

// ---- kernel launchers (each enqueues on ctx->stream) ----
int evh_launch_gray_level0(evh_ctx* c, const uint8_t* d_frames, int nframes, int channels, int64_t row_stride,
                           int64_t frame_stride);
int evh_launch_ingest_level0(evh_ctx* c, const EvhFrames& src, int nimg, int sw, int sh, int dw, int dh);
int evh_launch_yuv420_to_bgr(evh_ctx* c, const evh_yuv420& src, int nimg, int w, int h, uint8_t* d_dst, int64_t dst_stride,
                             int64_t dst_img_stride);
int evh_launch_pyramid(evh_ctx* c, int nframes);
int evh_launch_fast(evh_ctx* c, int nframes, int share_group);
int evh_launch_select(evh_ctx* c, int nframes);
int evh_launch_describe(evh_ctx* c, int nframes);
int evh_launch_superposition_scan(evh_ctx* c, const double* d_H, int n, double* d_out);
int evh_launch_transform_points(evh_ctx* c, const double* d_M, const int* d_idx, const double* d_pts, int n, double kx,
                                double ky, int decimals, double* d_out);
int evh_launch_fixed_plane(evh_ctx* c, const double* d_H, int n, int w, int h, double* d_field, unsigned long long* d_max);
// N4: SIFT (evh_sift.hip)
int evh_sift_allocate(evh_ctx* c, int max_sift_features);
int evh_launch_sift(evh_ctx* c, int nframes, int w, int h);
// N4: SURF (evh_surf.hip)
int evh_surf_allocate(evh_ctx* c, int max_surf_features);
int evh_launch_surf(evh_ctx* c, int nframes, int w, int h, float hessian_threshold);
int evh_launch_resize_area(evh_ctx* c, const uint8_t* d_src, int nimg, int sw, int sh, int cn, int64_t src_stride,
                           int64_t src_img_stride, uint8_t* d_dst, int dw, int dh, int64_t dst_stride,
                           int64_t dst_img_stride);
