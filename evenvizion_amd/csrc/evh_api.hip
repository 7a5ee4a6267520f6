// evh_api.hip -- host side of libevhip.so: context, geometry, settings, and the single-problem entry points of include/evhip.h
// (the pair / stream / ragged batch entries are evh_batch.hip).
#include "evh_internal.h"
#include "evh_match.h"
#include "evh_ransac.h"
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

static std::string g_create_error;

int evh_fail(evh_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg; else g_create_error = msg;
  return code;
}

static hipEvent_t prof_event(evh_ctx* c) {
  hipEvent_t e = nullptr;
  if (!c->prof_pool.empty()) { e = c->prof_pool.back(); c->prof_pool.pop_back(); return e; }
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}
EvhProfScope::EvhProfScope(evh_ctx* ctx, int stage, hipStream_t on) : c(ctx), idx(-1), st(on) {
  if (!c || !c->profiling) return;
  if (!st) st = c->stream;
  evh_ctx::ProfSpan s{stage, prof_event(c), prof_event(c)};
  if (!s.a || !s.b) return;
  (void)hipEventRecord(s.a, st);
  c->prof_spans.push_back(s);
  idx = (int)c->prof_spans.size() - 1;
}
EvhProfScope::~EvhProfScope() {
  if (idx >= 0) (void)hipEventRecord(c->prof_spans[idx].b, st);
}

namespace {

inline int align_up(int v, int a) { return (v + a - 1) / a * a; }
inline int64_t align_up64(int64_t v, int64_t a) { return (v + a - 1) / a * a; }
inline int round_f(float v) { return (int)lrintf(v); }

// ORB_create() defaults: 8 levels, scale factor 1.2f (held as double), per-level size = cvRound(size / scale),
// per-level quota from the geometric series (orb.cpp); see SURVEY Appendix A.1.
void compute_geometry(int w, int h, int nfeatures, EvhGeom& g) {
  g.w = w; g.h = h; g.nfeatures = nfeatures;
  const double scaleFactor = (double)1.2f;
  int64_t off = 0, coff = 0;
  int tiles = 0, tab = 0;
  for (int l = 0; l < EVH_NLEVELS; l++) {
    EvhLevel& L = g.lv[l];
    L.scale = (float)std::pow(scaleFactor, (double)l);
    L.w = round_f((float)w / L.scale);
    L.h = round_f((float)h / L.scale);
    L.stride = align_up(L.w, 64);
    L.off = off;
    // two rows at the least: the pyramid kernels stage the row below a tap's (weight 0 under a source of one row)
    off += align_up64((int64_t)L.stride * std::max(L.h, 2), 256);
    L.cand_cap = (L.w / 2 + 1) * (L.h / 2 + 1) + 64;  // NMS admits at most one corner per 2x2 block
    L.cand_off = coff;
    coff += L.cand_cap;
    // k_fast tiles (128 x 28) cover only what can be emitted: ORB drops corners within 31 px of the border
    // (runByImageBorder), so the tile grid starts at (EVH_FAST_OX, EVH_FAST_OY) = (24, 31) and ends at w-32 / h-32;
    // the one ring of neighbours NMS needs comes from the tiles' halo
    L.tiles_x = std::max(1, (L.w - 31 - EVH_FAST_OX + 127) / 128); L.tiles_y = std::max(1, (L.h - 31 - EVH_FAST_OY + 27) / 28);
    L.tile_start = tiles;
    tiles += L.tiles_x * L.tiles_y;
    L.tab_off = tab;
    if (l > 0) tab += 2 * L.w + 2 * L.h;
  }
  g.pyr_frame_bytes = off;
  g.cand_frame_entries = coff;
  g.total_tiles = tiles;
  const float factor = (float)(1.0 / scaleFactor);
  float ndes = nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)EVH_NLEVELS));
  int sum = 0;
  for (int l = 0; l < EVH_NLEVELS - 1; l++) {
    g.lv[l].quota = round_f(ndes);
    sum += g.lv[l].quota;
    ndes *= factor;
  }
  g.lv[EVH_NLEVELS - 1].quota = std::max(nfeatures - sum, 0);
  int kb = 0;
  for (int l = 0; l < EVH_NLEVELS; l++) {   // room for ties at the Harris cut: quota + 25 % + 16 per level
    g.lv[l].kp_base = kb;
    g.lv[l].kp_cap = g.lv[l].quota + g.lv[l].quota / 4 + 16;
    kb += g.lv[l].kp_cap;
  }
}

// INTER_LINEAR_EXACT coefficient tables for one axis: offset of the left/top tap and the 8.8 weight of the
// right/bottom tap; samples that fall off either end are encoded as a full weight on the edge sample.
void linear_exact_tab(int ssize, int dsize, int* ofs, int* c1) {
  const double inv_scale = (double)dsize / ssize;
  const double scale = 1.0 / inv_scale;
  for (int v = 0; v < dsize; v++) {
    const double fval = scale * ((double)v + 0.5) - 0.5;
    int ival = (int)std::floor(fval);
    if (ival >= 0 && ssize > 1) {
      if (ival < ssize - 1) {
        ofs[v] = ival;
        c1[v] = (int)std::lrint((fval - (double)ival) * 256.0);
      } else { ofs[v] = ssize - 2; c1[v] = 256; }
    } else { ofs[v] = 0; c1[v] = 0; }
  }
}

int kcap_for(int nfeatures) { return align_up(nfeatures + nfeatures / 4 + 8 * 17 + 64, 64); }

int configure(evh_ctx* c, int w, int h, int nfeatures) {
  if (c->geom_valid && c->g.w == w && c->g.h == h && c->g.nfeatures == nfeatures) return EVH_SUCCESS;
  if (w > c->max_w || h > c->max_h || w * (int64_t)h > (int64_t)c->max_w * c->max_h)
    return evh_fail(c, EVH_ERR_CAPACITY, "frame larger than the size given to evh_create");
  if (nfeatures > c->max_features || nfeatures < 1)
    return evh_fail(c, EVH_ERR_CAPACITY, "nfeatures outside [1, max_features]");
  if (w >= 4096 || h >= 4096) return evh_fail(c, EVH_ERR_UNSUPPORTED, "frames must be smaller than 4096 in each dimension");
  EvhGeom g;
  compute_geometry(w, h, nfeatures, g);
  // a side of 1 rounds to 0 from level 6 on (1 / 2.99): a level without pixels is a launch with an empty grid
  if (g.lv[EVH_NLEVELS - 1].w < 1 || g.lv[EVH_NLEVELS - 1].h < 1)
    return evh_fail(c, EVH_ERR_UNSUPPORTED, "frames must be at least 2 pixels in each dimension: a pyramid level would be empty");
  EvhGeom gmax;
  compute_geometry(c->max_w, c->max_h, c->max_features, gmax);
  if (g.pyr_frame_bytes > gmax.pyr_frame_bytes || g.cand_frame_entries > gmax.cand_frame_entries)
    return evh_fail(c, EVH_ERR_CAPACITY, "geometry exceeds the buffers sized by evh_create");
  std::vector<int> tabs;
  for (int l = 1; l < EVH_NLEVELS; l++) {
    const EvhLevel& S = g.lv[l - 1];
    const EvhLevel& D = g.lv[l];
    size_t base = tabs.size();
    tabs.resize(base + 2 * D.w + 2 * D.h);
    linear_exact_tab(S.w, D.w, &tabs[base], &tabs[base + D.w]);
    linear_exact_tab(S.h, D.h, &tabs[base + 2 * D.w], &tabs[base + 2 * D.w + D.h]);
  }
  // stream-ordered upload through pinned staging: kernels already enqueued keep the old tables, later ones see the new
  EVH_HIP(c, hipEventSynchronize(c->ev_tabs));                       // the previous upload has left h_tabs
  std::memcpy(c->h_tabs, tabs.data(), tabs.size() * sizeof(int));
  EVH_HIP(c, hipMemcpyAsync(c->d_tabs, c->h_tabs, tabs.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  EVH_HIP(c, hipEventRecord(c->ev_tabs, c->stream));
  c->g = g;
  c->geom_valid = true;
  return EVH_SUCCESS;
}

// context-owned scratch of the host-pointer entries (evh_transform_points, evh_superposition_scan,
// evh_fixed_plane_field): grown on demand, reused across calls (those entries synchronise before returning)
int ensure_scratch(evh_ctx* c, size_t bytes) {
  if (bytes <= c->scratch_bytes) return EVH_SUCCESS;
  return grow(c, &c->d_scratch, &c->scratch_bytes, std::max(bytes, (size_t)1 << 16));
}

// the detect-only entries: unrelated frames, no FAST threshold sharing
int detect_batch(evh_ctx* c, const EvhFrames& F, int nframes, int sw, int sh, int w, int h, int nfeatures) {
  int rc = evh_ingest_level0(c, "evh_orb_detect_batch", F, nframes, sw, sh, w, h, nfeatures);
  if (rc) return rc;
  return evh_orb_stages(c, nframes, 0);
}

// a frame slot's key-point count and flags word of one feature type, in one synchronisation
int frame_count(evh_ctx* c, const EvhFeatView& V, int frame, int* flags) {
  int n = 0;
  EVH_HIP(c, hipMemcpyAsync(&n, V.counts + frame, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  EVH_HIP(c, hipMemcpyAsync(flags, V.flags + frame, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  EVH_HIP(c, hipStreamSynchronize(c->stream));
  return n;
}

// the 8-float key-point records of SIFT and SURF: x, y, size, angle, response, octave bits, (SURF) laplacian bits
void unpack_records(const std::vector<float>& rec, int n, float* h_xy, float* h_size, float* h_angle, float* h_response,
                    int32_t* h_octave, int32_t* h_laplacian) {
  for (int i = 0; i < n; i++) {
    const float* r = &rec[(size_t)i * 8];
    if (h_xy) { h_xy[2 * i] = r[0]; h_xy[2 * i + 1] = r[1]; }
    if (h_size) h_size[i] = r[2];
    if (h_angle) h_angle[i] = r[3];
    if (h_response) h_response[i] = r[4];
    if (h_octave) memcpy(&h_octave[i], &r[5], 4);
    if (h_laplacian) memcpy(&h_laplacian[i], &r[6], 4);
  }
}

// ---- what SIFT and SURF share on their key-point lists (EvhKpList) ----
// level 0 of a float detector's batch, then its launch
template <class Launch>
int kp_detect_batch(evh_ctx* c, const char* who, const uint8_t* d_frames, int nframes, int src_w, int src_h, int channels,
                    int64_t row_stride, int64_t frame_stride, int w, int h, Launch launch) {
  int rc = evh_join_solve(c);
  if (rc) return rc;
  const int nf = c->geom_valid ? c->g.nfeatures : std::min(500, c->max_features);
  if ((rc = evh_ingest_level0(c, who, packed_frames(d_frames, channels, row_stride, frame_stride), nframes, src_w, src_h, w, h, nf)))
    return rc;
  c->nframes_resident = 0;            // level 0 was rewritten: the ORB results of an earlier call no longer match it
  return launch();
}

// key points of a resident frame; a flagged frame is an error (`overflow`)
int kp_count(evh_ctx* c, int type, const char* name, const char* overflow, int frame) {
  if (!c || frame < 0 || frame >= (type == EVH_FEATURE_SIFT ? c->sift : c->surf).frames_resident)
    return evh_fail(c, EVH_ERR_INVALID, std::string("bad ") + name + " frame slot");
  int fl = 0;
  const int n = frame_count(c, evh_feat_view(c, type), frame, &fl);
  if (n < 0) return n;
  if (fl) return evh_fail(c, EVH_ERR_CAPACITY, overflow);
  return n;
}

// the n records of a frame unpacked into the caller's arrays, its n descriptor rows as they are stored (h_desc_rows may be NULL)
int kp_download(evh_ctx* c, const EvhKpList& L, int frame, int n, void* h_desc_rows, float* h_xy, float* h_size, float* h_angle,
                float* h_response, int32_t* h_octave, int32_t* h_laplacian) {
  const size_t o = (size_t)frame * L.cap;
  std::vector<float> rec((size_t)n * 8);
  EVH_HIP(c, hipMemcpyAsync(rec.data(), L.kp + o * 8, sizeof(float) * 8 * n, hipMemcpyDeviceToHost, c->stream));
  if (h_desc_rows)
    EVH_HIP(c, hipMemcpyAsync(h_desc_rows, L.desc + o * L.desc_row_bytes, (size_t)n * L.desc_row_bytes, hipMemcpyDeviceToHost, c->stream));
  EVH_HIP(c, hipStreamSynchronize(c->stream));
  unpack_records(rec, n, h_xy, h_size, h_angle, h_response, h_octave, h_laplacian);
  return EVH_SUCCESS;
}

// evh_ratio_unique_filter / _f32: d2 holds integer squared distances, or (is_dist) the float32 bits of distances
int ratio_filter(evh_ctx* c, const char* who, const int32_t* d_idx, const uint32_t* d_d2, int is_dist, int nq, int nt,
                 const float* d_xy_q, const float* d_xy_t, double ratio, int min_matches, float* d_pts, int* h_count, int* h_status) {
  if (!c || !d_idx || !d_d2 || !d_xy_q || !d_xy_t || !d_pts || !h_count || !h_status || nq < 0 || nt < 0)
    return evh_fail(c, EVH_ERR_INVALID, std::string(who) + ": bad argument");
  const int kc = std::max(std::max(nq, nt), 1);
  if (kc > 65535) return evh_fail(c, EVH_ERR_CAPACITY, std::string(who) + ": too many rows");
  if (((uintptr_t)d_pts) & 15) return evh_fail(c, EVH_ERR_INVALID, "d_pts must be 16-byte aligned");
  int* d_cnt = c->d_small->count_status;
  EvhFilterArgs F{};
  F.idx = d_idx; F.d2 = d_d2; F.d2_is_dist = is_dist; F.knn_stride = nq; F.xy_q = d_xy_q; F.xy_t = d_xy_t; F.xy_slot_floats = 0;
  F.nq_fixed = nq; F.nt_fixed = nt; F.ratio = ratio; F.min_matches = min_matches;
  F.pts = d_pts; F.pts_stride = nq; F.npts = d_cnt; F.status = d_cnt + 1; F.kcap = kc;
  int rc = evh_launch_filter(c, F, 1);
  if (rc) return rc;
  int host[2];
  EVH_HIP(c, hipMemcpyAsync(host, d_cnt, 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  EVH_HIP(c, hipStreamSynchronize(c->stream));
  *h_count = host[0]; *h_status = host[1];
  return EVH_SUCCESS;
}

}  // namespace

// ---- host stages shared with evh_batch.hip (declared in evh_internal.h) ----
// one set of per-pair buffers with `cap` rows per pair (the ORB path: kcap; the multi-type path: every type's rows)
int evh_alloc_pair_bufs(evh_ctx* c, EvhPairBufs& B, int cap) {
  const size_t P = (size_t)c->max_frames, K = (size_t)cap;
  int rc;
#define A_(call) if ((rc = (call)) != EVH_SUCCESS) return rc
  A_(dalloc(c, &B.knn_idx, P * K * 2));
  A_(dalloc(c, &B.knn_d2, P * K * 2));
  A_(dalloc(c, &B.pts, P * K * 4));
  A_(dalloc(c, &B.pts2, P * K * 4));
  A_(dalloc(c, &B.crow, P * K * 4));
  A_(dalloc(c, &B.npts, P));
  A_(dalloc(c, &B.npts2, P));
  A_(dalloc(c, &B.pstatus, P));
  A_(dalloc(c, &B.H1, P * 9));
  A_(dalloc(c, &B.mask, P * K));
  A_(dalloc(c, &B.lm, P * K * 4));
  A_(dalloc(c, &B.info, P * 8));
#undef A_
  B.cap = cap;
  return EVH_SUCCESS;
}

// fixed-iteration mode keeps the per-lane eigenvector matrices of its hypotheses in a global scratch (one block per
// workgroup = per pair slot); allocated on first use
int evh_ensure_lane_scratch(evh_ctx* c) {
  if (c->d_lane_v) return EVH_SUCCESS;
  return dalloc(c, &c->d_lane_v, (size_t)c->max_frames * EVH_LANE_V_DOUBLES);
}

EvhFeatView evh_feat_view(const evh_ctx* c, int type) {
  if (type == EVH_FEATURE_SIFT || type == EVH_FEATURE_SURF) {
    const EvhKpList& L = type == EVH_FEATURE_SIFT ? c->sift : c->surf;
    const bool f32 = type == EVH_FEATURE_SURF;
    return {L.count, L.flags, L.xy, L.desc, f32 ? 0 : L.desc_row_bytes, f32, L.cap};
  }
  return {c->d_kp_count, c->d_frame_flags, c->d_kp_xy, c->d_desc, 32, false, c->kcap};
}

// entry points that reuse the pair buffers on the main stream first order themselves behind a pending async solve
int evh_join_solve(evh_ctx* c) {
  if (c->solve_pending) EVH_HIP(c, hipStreamWaitEvent(c->stream, c->ev_solve_done, 0));
  return EVH_SUCCESS;
}

// the argument checks of every entry that takes planes: nothing is launched on a description that fails them
int evh_check_yuv420(evh_ctx* c, const char* who, const evh_yuv420* s, int nframes, int w, int h) {
  const std::string W = std::string(who) + ": ";
  if (!c) return EVH_ERR_INVALID;
  if (!s || !s->d_y || !s->d_cb || !s->d_cr) return evh_fail(c, EVH_ERR_INVALID, W + "NULL plane");
  if (w < 1 || h < 1) return evh_fail(c, EVH_ERR_INVALID, W + "empty source frame");
  if (nframes < 1 || nframes > 65535) return evh_fail(c, EVH_ERR_CAPACITY, W + "between 1 and 65535 frames per call");
  if (s->c_pixel_stride != 1 && s->c_pixel_stride != 2) return evh_fail(c, EVH_ERR_INVALID, W + "chroma pixel stride must be 1 or 2");
  const int64_t cw = (w + 1) / 2, ch = (h + 1) / 2, crow = (cw - 1) * s->c_pixel_stride + 1;
  if (s->y_stride < w) return evh_fail(c, EVH_ERR_INVALID, W + "luma row stride smaller than the width");
  if (s->c_stride < crow) return evh_fail(c, EVH_ERR_INVALID, W + "chroma row stride smaller than a chroma row");
  if (nframes > 1 && (s->y_frame_stride < (h - 1) * s->y_stride + w || s->c_frame_stride < (ch - 1) * s->c_stride + crow))
    return evh_fail(c, EVH_ERR_INVALID, W + "frame stride smaller than a plane");
  return EVH_SUCCESS;
}

// level 0 (gray) of every frame: (sw, sh) = size of the frames handed over, (w, h) = working size.  Different sizes =
// fused ingest (N2).  Shared by every feature type of a call.  The one place where the frames of a detect / pair / stream
// entry are checked.
int evh_ingest_level0(evh_ctx* c, const char* who, const EvhFrames& F, int nframes, int sw, int sh, int w, int h, int nfeatures) {
  if (!c) return EVH_ERR_INVALID;
  if (F.yuv) {
    if (int rc = evh_check_yuv420(c, who, F.yuv, nframes, sw, sh)) return rc;
  } else {
    if (!F.packed) return evh_fail(c, EVH_ERR_INVALID, std::string(who) + ": NULL argument");
    if (F.channels != 1 && F.channels != 3) return evh_fail(c, EVH_ERR_INVALID, "channels must be 1 or 3");
    if (F.row_stride < (int64_t)sw * F.channels) return evh_fail(c, EVH_ERR_INVALID, "row_stride smaller than a row");
    if (sw < 1 || sh < 1) return evh_fail(c, EVH_ERR_INVALID, "empty source frame");
  }
  if (nframes < 1 || nframes > c->max_frames) return evh_fail(c, EVH_ERR_CAPACITY, "nframes exceeds max_frames");
  if (nframes > 65535 || h > 65535) return evh_fail(c, EVH_ERR_CAPACITY, "too many frames / rows for one launch");
  int rc = configure(c, w, h, nfeatures);
  if (rc) return rc;
  EvhProfScope ps(c, EVH_ST_GRAY);
  if (!F.yuv && sw == w && sh == h)
    return evh_launch_gray_level0(c, F.packed, nframes, F.channels, F.row_stride, F.frame_stride);
  return evh_launch_ingest_level0(c, F, nframes, sw, sh, w, h);
}

// ORB K2..K6 on the frames whose level 0 is resident
int evh_orb_stages(evh_ctx* c, int nframes, int share_group) {
  int rc;
  { EvhProfScope ps(c, EVH_ST_PYRAMID); rc = evh_launch_pyramid(c, nframes); }
  if (rc) return rc;
  { EvhProfScope ps(c, EVH_ST_FAST); rc = evh_launch_fast(c, nframes, share_group); }
  if (rc) return rc;
  { EvhProfScope ps(c, EVH_ST_SELECT); rc = evh_launch_select(c, nframes); }
  if (rc) return rc;
  { EvhProfScope ps(c, EVH_ST_DESCRIBE); rc = evh_launch_describe(c, nframes); }
  if (rc) return rc;
  c->nframes_resident = nframes;
  return EVH_SUCCESS;
}

extern "C" {

int evh_version(void) { return 100; }

const char* evh_last_error_string(const evh_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int evh_create(int device, int max_w, int max_h, int max_features, int max_frames, void* stream, evh_ctx** out) {
  if (!out) return evh_fail(nullptr, EVH_ERR_INVALID, "evh_create: out is NULL");
  *out = nullptr;
  // frames are a grid dimension of every per-frame kernel (rounded up to a multiple of 8 by the XCD-ordered ones)
  if (max_w < 64 || max_h < 64 || max_w >= 4096 || max_h >= 4096 || max_features < 1 || max_frames < 2 || max_frames > 65528)
    return evh_fail(nullptr, EVH_ERR_INVALID, "evh_create: sizes out of range (64 <= w,h < 4096, 2 <= frames <= 65528)");
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return evh_fail(nullptr, EVH_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
  evh_ctx* c = new evh_ctx();
  c->device = device; c->max_w = max_w; c->max_h = max_h; c->max_features = max_features; c->max_frames = max_frames;
  c->kcap = kcap_for(max_features);
  // k_filter keeps five int lists of kcap entries in LDS; k_select 8 * (EVH_K1CAP + kcap) bytes of dynamic LDS next to
  // ~5 KB of static arrays (both opt in to more than the default 64 KB at launch)
  if ((size_t)c->kcap * 5 * sizeof(int) > 150 * 1024 || 8 * ((size_t)EVH_K1CAP + c->kcap) + 8 * 1024 > 160 * 1024) {
    delete c;
    return evh_fail(nullptr, EVH_ERR_CAPACITY, "evh_create: max_features too large for the LDS lists of the matching filter / key-point selection (<= EVH_MAX_FEATURES = 5984)");
  }
  int rc = EVH_SUCCESS;
  auto fail = [&](int code) { g_create_error = c->err; evh_destroy(c); return code; };
  if (stream) { c->stream = (hipStream_t)stream; c->own_stream = false; }
  else {
    e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { c->err = std::string("hipStreamCreate: ") + hipGetErrorString(e); return fail(EVH_ERR_HIP); }
    c->own_stream = true;
  }
  EvhGeom gmax;
  compute_geometry(max_w, max_h, max_features, gmax);
  const size_t F = (size_t)max_frames, K = (size_t)c->kcap;
  int tabn = 0;
  for (int l = 1; l < EVH_NLEVELS; l++) tabn += 2 * gmax.lv[l].w + 2 * gmax.lv[l].h;
#define A_(call) if ((rc = (call)) != EVH_SUCCESS) return fail(rc)
  A_(dalloc(c, &c->d_pyr, F * (size_t)gmax.pyr_frame_bytes + 256));
  A_(dalloc(c, &c->d_cand, F * (size_t)gmax.cand_frame_entries));
  A_(dalloc(c, &c->d_cand_count, F * EVH_NLEVELS));
  A_(dalloc(c, &c->d_tabs, (size_t)tabn + 64));
  if (hipHostMalloc(reinterpret_cast<void**>(&c->h_tabs), ((size_t)tabn + 64) * sizeof(int), hipHostMallocDefault) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_tabs, hipEventDisableTiming) != hipSuccess) {
    c->err = "evh_create: pinned table staging (hipHostMalloc) or its event could not be created";
    return fail(EVH_ERR_HIP);
  }
  A_(dalloc(c, &c->d_kp_xy, F * K * 2));
  A_(dalloc(c, &c->d_kp_meta, F * K));
  A_(dalloc(c, &c->d_kp_resp, F * K));
  A_(dalloc(c, &c->d_kp_angle, F * K));
  A_(dalloc(c, &c->d_desc, F * K * 32));
  A_(dalloc(c, &c->d_kp_count, F));
  A_(dalloc(c, &c->d_frame_flags, F));
  A_(dalloc(c, &c->d_tmp_meta, F * EVH_NLEVELS * K));   // one frame-slot-sized segment per level
  A_(dalloc(c, &c->d_tmp_resp, F * EVH_NLEVELS * K));
  A_(dalloc(c, &c->d_lvl_count, F * EVH_NLEVELS));
  A_(dalloc(c, &c->d_fast_thr, F * EVH_NLEVELS));
  A_(dalloc(c, &c->d_fast_hist, F * EVH_NLEVELS * 256));
  A_(dalloc(c, &c->d_fast_redo, F * EVH_NLEVELS + 1));
  c->cv_band_frame_entries = EVH_NLEVELS;   // a base per band of FAST tiles (tiles_y grows with the frame's height), then the level totals
  for (int l = 0; l < EVH_NLEVELS; l++) c->cv_band_frame_entries += gmax.lv[l].tiles_y;
  A_(dalloc(c, &c->d_cv_seq, F * (size_t)gmax.cand_frame_entries));
  A_(dalloc(c, &c->d_cv_seq32, F * (size_t)gmax.cand_frame_entries));
  A_(dalloc(c, &c->d_cv_lpos, F * (size_t)gmax.cand_frame_entries));
  A_(dalloc(c, &c->d_cv_rpos, F * (size_t)gmax.cand_frame_entries));
  A_(dalloc(c, &c->d_cv_band, F * (size_t)c->cv_band_frame_entries));
  A_(dalloc(c, &c->d_cv_tdesc, F * 8 * (size_t)gmax.total_tiles + 64));
  A_(dalloc(c, &c->d_fast_hint, 16 + 8 * 256 + 8));
  if (hipMemset(c->d_fast_hint, 0, sizeof(int) * (16 + 8 * 256 + 8)) != hipSuccess) {
    c->err = "hipMemset(d_fast_hint) failed";
    return fail(EVH_ERR_HIP);
  }
  A_(evh_alloc_pair_bufs(c, c->orb, c->kcap));
  A_(dalloc(c, &c->d_small, 1));
#undef A_
  e = hipMemset(c->d_kp_count, 0, F * sizeof(int));
  if (e == hipSuccess) e = hipMemset(c->d_frame_flags, 0, F * sizeof(int));
  if (e != hipSuccess) { c->err = std::string("hipMemset: ") + hipGetErrorString(e); return fail(EVH_ERR_HIP); }
  *out = c;
  return EVH_SUCCESS;
}

void evh_destroy(evh_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  dfree_from(c, 0);
  for (auto& s : c->prof_spans) { (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b); }
  for (auto e : c->prof_pool) (void)hipEventDestroy(e);
  if (c->solve_stream) { (void)hipStreamSynchronize(c->solve_stream); (void)hipStreamDestroy(c->solve_stream); }
  if (c->h_tabs) (void)hipHostFree(c->h_tabs);
  if (c->h_segs) (void)hipHostFree(c->h_segs);
  for (auto e : c->ev_segs) if (e) (void)hipEventDestroy(e);
  if (c->ev_tabs) (void)hipEventDestroy(c->ev_tabs);
  if (c->ev_match_done) (void)hipEventDestroy(c->ev_match_done);
  if (c->ev_solve_done) (void)hipEventDestroy(c->ev_solve_done);
  if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

int evh_set_fast_lift(evh_ctx* c, int on) {
  if (!c) return EVH_ERR_INVALID;
  c->fast_lift = on != 0;
  return EVH_SUCCESS;
}

int evh_set_solver_mode(evh_ctx* c, int mode) {
  if (!c || (mode != EVH_SOLVER_EXACT && mode != EVH_SOLVER_FAST)) return EVH_ERR_INVALID;
  c->solver_mode = mode;
  return EVH_SUCCESS;
}

int evh_get_solver_mode(const evh_ctx* c) { return c ? c->solver_mode : EVH_ERR_INVALID; }

int evh_set_keypoint_order(evh_ctx* c, int mode) {
  if (!c || (mode != EVH_ORDER_CANONICAL && mode != EVH_ORDER_OPENCV)) return EVH_ERR_INVALID;
  c->order_mode = mode;
  return EVH_SUCCESS;
}

int evh_get_keypoint_order(const evh_ctx* c) { return c ? c->order_mode : EVH_ERR_INVALID; }

int evh_set_fast_hint(evh_ctx* c, int on) {
  if (!c) return EVH_ERR_INVALID;
  c->fast_hint = on != 0;
  return EVH_SUCCESS;
}

int evh_set_fast_share(evh_ctx* c, int on) {
  if (!c) return EVH_ERR_INVALID;
  c->fast_share = on != 0;
  return EVH_SUCCESS;
}

int evh_profile_enable(evh_ctx* c, int on) {
  if (!c) return EVH_ERR_INVALID;
  c->profiling = on != 0;
  return EVH_SUCCESS;
}

const char* evh_profile_stage_name(int stage) {
  static const char* names[EVH_NSTAGES] = {"gray", "pyramid", "fast", "select", "describe", "knn2", "filter",
                                           "ransac_static", "ransac_final"};
  return stage >= 0 && stage < EVH_NSTAGES ? names[stage] : "";
}

int evh_profile_read(evh_ctx* c, float* h_total_ms, int* h_counts) {
  if (!c || !h_total_ms || !h_counts) return evh_fail(c, EVH_ERR_INVALID, "evh_profile_read: bad argument");
  EVH_HIP(c, hipStreamSynchronize(c->stream));
  if (c->solve_stream) EVH_HIP(c, hipStreamSynchronize(c->solve_stream));
  for (int i = 0; i < EVH_NSTAGES; i++) { h_total_ms[i] = 0.f; h_counts[i] = 0; }
  for (auto& s : c->prof_spans) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) { h_total_ms[s.stage] += ms; h_counts[s.stage]++; }
    c->prof_pool.push_back(s.a); c->prof_pool.push_back(s.b);
  }
  c->prof_spans.clear();
  return EVH_SUCCESS;
}

void* evh_stream(const evh_ctx* c) { return c ? (void*)c->stream : nullptr; }

int evh_synchronize(evh_ctx* c) {
  if (!c) return EVH_ERR_INVALID;
  EVH_HIP(c, hipStreamSynchronize(c->stream));
  if (c->solve_stream) EVH_HIP(c, hipStreamSynchronize(c->solve_stream));
  c->solve_pending = false;
  return EVH_SUCCESS;
}

int evh_set_async_solve(evh_ctx* c, int on) {
  if (!c) return EVH_ERR_INVALID;
  if (on && !c->solve_stream) {
    EVH_HIP(c, hipStreamCreateWithFlags(&c->solve_stream, hipStreamNonBlocking));
    EVH_HIP(c, hipEventCreateWithFlags(&c->ev_match_done, hipEventDisableTiming));
    EVH_HIP(c, hipEventCreateWithFlags(&c->ev_solve_done, hipEventDisableTiming));
  }
  if (!on && c->solve_stream) { EVH_HIP(c, hipStreamSynchronize(c->solve_stream)); c->solve_pending = false; }
  c->async_solve = on != 0;
  return EVH_SUCCESS;
}

int evh_solve_wait(evh_ctx* c, void* stream) {
  if (!c) return EVH_ERR_INVALID;
  if (c->solve_pending) EVH_HIP(c, hipStreamWaitEvent(stream ? (hipStream_t)stream : c->stream, c->ev_solve_done, 0));
  return EVH_SUCCESS;
}

int evh_resize_area_u8(evh_ctx* c, const uint8_t* d_src, int nimg, int sw, int sh, int cn, int64_t src_stride,
                       int64_t src_img_stride, uint8_t* d_dst, int dw, int dh, int64_t dst_stride,
                       int64_t dst_img_stride) {
  if (!c || !d_src || !d_dst || nimg < 1 || sw < 1 || sh < 1 || dw < 1 || dh < 1 || (cn != 1 && cn != 3))
    return evh_fail(c, EVH_ERR_INVALID, "evh_resize_area_u8: bad argument");
  if (nimg > 65535 || dh > 65535) return evh_fail(c, EVH_ERR_CAPACITY, "evh_resize_area_u8: too many images/rows");
  return evh_launch_resize_area(c, d_src, nimg, sw, sh, cn, src_stride, src_img_stride, d_dst, dw, dh, dst_stride,
                                dst_img_stride);
}

int evh_resize_area_u8c3(evh_ctx* c, const uint8_t* d_src, int sw, int sh, uint8_t* d_dst, int dw, int dh) {
  return evh_resize_area_u8(c, d_src, 1, sw, sh, 3, (int64_t)sw * 3, (int64_t)sw * sh * 3, d_dst, dw, dh, (int64_t)dw * 3,
                            (int64_t)dw * dh * 3);
}

int evh_fixed_plane_field(evh_ctx* c, const double* h_Hsup, int n, int w, int h, double* d_field, double* h_max) {
  if (!c || !h_Hsup || !h_max || n < 1 || w < 1 || h < 1) return evh_fail(c, EVH_ERR_INVALID, "evh_fixed_plane_field: bad argument");
  if (n > 65535) return evh_fail(c, EVH_ERR_CAPACITY, "evh_fixed_plane_field: at most 65535 matrices per call");
  if ((int64_t)w * h > INT_MAX) return evh_fail(c, EVH_ERR_CAPACITY, "evh_fixed_plane_field: w * h above INT_MAX");
  { int sr = ensure_scratch(c, (sizeof(double) * 9 + sizeof(unsigned long long)) * (size_t)n); if (sr) return sr; }
  double* d_H = reinterpret_cast<double*>(c->d_scratch);
  unsigned long long* d_max = reinterpret_cast<unsigned long long*>(c->d_scratch + sizeof(double) * 9 * (size_t)n);
  std::vector<unsigned long long> keys(n);
  int rc = EVH_SUCCESS;
  hipError_t e = hipMemcpyAsync(d_H, h_Hsup, sizeof(double) * 9 * (size_t)n, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) rc = evh_launch_fixed_plane(c, d_H, n, w, h, d_field, d_max);
  if (e == hipSuccess && rc == EVH_SUCCESS)
    e = hipMemcpyAsync(keys.data(), d_max, sizeof(unsigned long long) * (size_t)n, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return evh_fail(c, EVH_ERR_HIP, std::string("evh_fixed_plane_field: ") + hipGetErrorString(e));
  if (rc) return rc;
  for (int i = 0; i < n; i++) {
    unsigned long long b = keys[i];
    b = (b >> 63) ? (b & 0x7FFFFFFFFFFFFFFFull) : ~b;
    memcpy(&h_max[i], &b, sizeof(double));
  }
  return EVH_SUCCESS;
}

int evh_superposition_scan(evh_ctx* c, const double* h_H, int n, double* h_out) {
  if (!c || !h_H || !h_out || n < 1) return evh_fail(c, EVH_ERR_INVALID, "evh_superposition_scan: bad argument");
  const size_t bytes = sizeof(double) * 9 * (size_t)n;
  { int sr = ensure_scratch(c, 2 * bytes); if (sr) return sr; }
  double* d = reinterpret_cast<double*>(c->d_scratch);
  int rc = EVH_SUCCESS;
  hipError_t e = hipMemcpyAsync(d, h_H, bytes, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) rc = evh_launch_superposition_scan(c, d, n, d + 9 * (size_t)n);
  if (e == hipSuccess && rc == EVH_SUCCESS) e = hipMemcpyAsync(h_out, d + 9 * (size_t)n, bytes, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return evh_fail(c, EVH_ERR_HIP, std::string("evh_superposition_scan: ") + hipGetErrorString(e));
  return rc;
}

int evh_transform_points(evh_ctx* c, const double* h_M, int nmat, const int32_t* h_idx, const double* h_pts, int n, double kx,
                         double ky, int decimals, double* h_out) {
  if (!c || !h_M || !h_idx || !h_pts || !h_out || nmat < 1 || n < 0 || decimals > 15)
    return evh_fail(c, EVH_ERR_INVALID, "evh_transform_points: bad argument");
  if (n == 0) return EVH_SUCCESS;
  for (int i = 0; i < n; i++)
    if (h_idx[i] < 0 || h_idx[i] >= nmat) return evh_fail(c, EVH_ERR_INVALID, "evh_transform_points: matrix index out of range");
  const size_t bm = sizeof(double) * 9 * (size_t)nmat, bp = sizeof(double) * 2 * (size_t)n, bi = sizeof(int32_t) * (size_t)n;
  { int sr = ensure_scratch(c, bm + 2 * bp + bi); if (sr) return sr; }
  char* d = c->d_scratch;
  double* d_M = reinterpret_cast<double*>(d);
  double* d_pts = reinterpret_cast<double*>(d + bm);
  double* d_out = reinterpret_cast<double*>(d + bm + bp);
  int* d_idx = reinterpret_cast<int*>(d + bm + 2 * bp);
  int rc = EVH_SUCCESS;
  hipError_t e = hipMemcpyAsync(d_M, h_M, bm, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_pts, h_pts, bp, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_idx, h_idx, bi, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) rc = evh_launch_transform_points(c, d_M, d_idx, d_pts, n, kx, ky, decimals, d_out);
  if (e == hipSuccess && rc == EVH_SUCCESS) e = hipMemcpyAsync(h_out, d_out, bp, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return evh_fail(c, EVH_ERR_HIP, std::string("evh_transform_points: ") + hipGetErrorString(e));
  return rc;
}

int evh_orb_detect_batch(evh_ctx* c, const uint8_t* d_frames, int nframes, int w, int h, int channels,
                         int64_t row_stride, int64_t frame_stride, int nfeatures) {
  return detect_batch(c, packed_frames(d_frames, channels, row_stride, frame_stride), nframes, w, h, w, h, nfeatures);
}

int evh_orb_detect_batch_resized(evh_ctx* c, const uint8_t* d_frames, int nframes, int src_w, int src_h, int channels,
                                 int64_t row_stride, int64_t frame_stride, int w, int h, int nfeatures) {
  return detect_batch(c, packed_frames(d_frames, channels, row_stride, frame_stride), nframes, src_w, src_h, w, h, nfeatures);
}

int evh_orb_capacity(const evh_ctx* c) { return c ? c->kcap : EVH_ERR_INVALID; }

int evh_orb_count(evh_ctx* c, int frame) {
  if (!c || frame < 0 || frame >= c->nframes_resident) return evh_fail(c, EVH_ERR_INVALID, "bad frame slot");
  int fl = 0;
  const int n = frame_count(c, evh_feat_view(c, EVH_FEATURE_ORB), frame, &fl);
  if (n < 0) return n;
  if (fl & 2) return evh_fail(c, EVH_ERR_CAPACITY, "key-point selection: nth_element's depth limit was reached for this frame (heap-select fall-back)");
  if (fl) return evh_fail(c, EVH_ERR_CAPACITY, "a fixed-capacity keypoint list overflowed for this frame");
  return n;
}

int evh_orb_download(evh_ctx* c, int frame, float* h_xy, uint8_t* h_desc, int32_t* h_octave, int32_t* h_lxy,
                     float* h_response, float* h_angle) {
  int n = evh_orb_count(c, frame);
  if (n <= 0) return n;
  const size_t o = (size_t)frame * c->kcap;
  std::vector<uint32_t> meta;
  if (h_xy) EVH_HIP(c, hipMemcpyAsync(h_xy, c->d_kp_xy + 2 * o, sizeof(float) * 2 * n, hipMemcpyDeviceToHost, c->stream));
  if (h_desc) EVH_HIP(c, hipMemcpyAsync(h_desc, c->d_desc + 32 * o, 32 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  if (h_response) EVH_HIP(c, hipMemcpyAsync(h_response, c->d_kp_resp + o, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
  if (h_angle) EVH_HIP(c, hipMemcpyAsync(h_angle, c->d_kp_angle + o, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
  if (h_octave || h_lxy) {
    meta.resize(n);
    EVH_HIP(c, hipMemcpyAsync(meta.data(), c->d_kp_meta + o, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, c->stream));
  }
  EVH_HIP(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < n && !meta.empty(); i++) {
    if (h_octave) h_octave[i] = (int32_t)(meta[i] >> 24);
    if (h_lxy) { h_lxy[2 * i] = (int32_t)(meta[i] & 0xFFFu); h_lxy[2 * i + 1] = (int32_t)((meta[i] >> 12) & 0xFFFu); }
  }
  return n;
}

int evh_orb_detect_compute(evh_ctx* c, const uint8_t* d_frame, int w, int h, int channels, int nfeatures, float* h_xy,
                           uint8_t* h_desc, int32_t* h_octave, int* h_count) {
  if (!c) return EVH_ERR_INVALID;
  int rc = evh_orb_detect_batch(c, d_frame, 1, w, h, channels, (int64_t)w * channels, (int64_t)w * h * channels, nfeatures);
  if (rc != EVH_SUCCESS) return rc;
  const int n = evh_orb_download(c, 0, h_xy, h_desc, h_octave, nullptr, nullptr, nullptr);
  if (n < 0) return n;
  if (h_count) *h_count = n;
  return EVH_SUCCESS;
}

int evh_orb_level_info(const evh_ctx* c, int level, int* w, int* h, int* quota, float* scale) {
  if (!c || !c->geom_valid || level < 0 || level >= EVH_NLEVELS) return EVH_ERR_INVALID;
  const EvhLevel& L = c->g.lv[level];
  if (w) *w = L.w; if (h) *h = L.h; if (quota) *quota = L.quota; if (scale) *scale = L.scale;
  return EVH_SUCCESS;
}

int evh_orb_download_level(evh_ctx* c, int frame, int level, uint8_t* h_pixels) {
  if (!c || !c->geom_valid || level < 0 || level >= EVH_NLEVELS || frame < 0 || frame >= c->nframes_resident || !h_pixels)
    return evh_fail(c, EVH_ERR_INVALID, "evh_orb_download_level: bad argument");
  const EvhLevel& L = c->g.lv[level];
  EVH_HIP(c, hipMemcpy2DAsync(h_pixels, L.w, c->d_pyr + (size_t)frame * c->g.pyr_frame_bytes + L.off, L.stride, L.w, L.h,
                              hipMemcpyDeviceToHost, c->stream));
  EVH_HIP(c, hipStreamSynchronize(c->stream));
  return EVH_SUCCESS;
}

int evh_orb_download_candidates(evh_ctx* c, int frame, int level, uint32_t* h_packed, int cap) {
  if (!c || !c->geom_valid || level < 0 || level >= EVH_NLEVELS || frame < 0 || frame >= c->nframes_resident)
    return evh_fail(c, EVH_ERR_INVALID, "evh_orb_download_candidates: bad argument");
  const EvhLevel& L = c->g.lv[level];
  int n = 0;
  EVH_HIP(c, hipMemcpyAsync(&n, c->d_cand_count + frame * EVH_NLEVELS + level, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  EVH_HIP(c, hipStreamSynchronize(c->stream));
  int m = std::min(std::min(n, cap), L.cand_cap);
  if (m > 0 && h_packed) {
    EVH_HIP(c, hipMemcpyAsync(h_packed, c->d_cand + (size_t)frame * c->g.cand_frame_entries + L.cand_off,
                              sizeof(uint32_t) * m, hipMemcpyDeviceToHost, c->stream));
    EVH_HIP(c, hipStreamSynchronize(c->stream));
  }
  return n;
}

static int knn_generic(evh_ctx* c, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int32_t* d_idx, uint32_t* d_d2,
                       int hamming, int desc_bytes = 32) {
  if (!c || !d_idx || !d_d2 || nq < 0 || nt < 0) return evh_fail(c, EVH_ERR_INVALID, "evh_match_knn2: bad argument");
  if (nq == 0) return EVH_SUCCESS;
  if (((uintptr_t)d_q | (uintptr_t)d_t) & 15) return evh_fail(c, EVH_ERR_INVALID, "descriptor buffers must be 16-byte aligned");
  EvhKnnArgs K{};
  K.q = d_q; K.t = d_t; K.slot_bytes = 0; K.nq_fixed = nq; K.nt_fixed = nt;
  K.idx = d_idx; K.d2 = d_d2; K.out_stride = nq; K.hamming = hamming; K.desc_bytes = desc_bytes;
  return evh_launch_knn2(c, K, 1);
}

int evh_match_knn2_l2u8(evh_ctx* c, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int32_t* d_idx, uint32_t* d_d2) {
  return knn_generic(c, d_q, nq, d_t, nt, d_idx, d_d2, 0);
}
int evh_match_knn2_l2u8x128(evh_ctx* c, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int32_t* d_idx, uint32_t* d_d2) {
  return knn_generic(c, d_q, nq, d_t, nt, d_idx, d_d2, 0, 128);
}
int evh_match_knn2_hamming(evh_ctx* c, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int32_t* d_idx,
                           uint32_t* d_d2) {
  return knn_generic(c, d_q, nq, d_t, nt, d_idx, d_d2, 1);
}

int evh_ratio_unique_filter(evh_ctx* c, const int32_t* d_idx, const uint32_t* d_d2, int nq, int nt, const float* d_xy_q,
                            const float* d_xy_t, double ratio, int min_matches, float* d_pts, int* h_count, int* h_status) {
  return ratio_filter(c, "evh_ratio_unique_filter", d_idx, d_d2, 0, nq, nt, d_xy_q, d_xy_t, ratio, min_matches, d_pts, h_count,
                      h_status);
}

static int find_homography_entry(evh_ctx* c, const float* d_pts, int n, double thr, int max_iters, double conf, int force_max,
                                 double* h_H, uint8_t* h_mask, int* h_found, int* h_info) {
  if (!c || (!d_pts && n > 0) || n < 0 || !h_H || !h_found) return evh_fail(c, EVH_ERR_INVALID, "evh_find_homography_ransac: bad argument");
  if (n > c->kcap * c->max_frames) return evh_fail(c, EVH_ERR_CAPACITY, "evh_find_homography_ransac: too many rows");
  if (((uintptr_t)d_pts) & 15) return evh_fail(c, EVH_ERR_INVALID, "d_pts must be 16-byte aligned");
  { int jr = evh_join_solve(c); if (jr) return jr; }
  // scratch: the per-pair buffers viewed as one big problem
  EvhRansacArgs R{};
  R.fast_solver = c->solver_mode;
  R.pts = const_cast<float*>(d_pts); R.n_fixed = n; R.thr = thr; R.max_iters = max_iters; R.conf = conf; R.force_max = force_max;
  if (force_max) { int lr = evh_ensure_lane_scratch(c); if (lr) return lr; R.lane_v = c->d_lane_v; }
  EvhSmall* S = c->d_small;
  R.mask = c->orb.mask; R.crow = c->orb.crow; R.lm = c->orb.lm;
  R.H = S->H; R.found = &S->found; R.info = S->info;
  int rc = evh_launch_find_homography(c, R);
  if (rc) return rc;
  double Hh[9]; int found = 0, info[3] = {0, 0, 0};
  EVH_HIP(c, hipMemcpyAsync(Hh, S->H, sizeof(Hh), hipMemcpyDeviceToHost, c->stream));
  EVH_HIP(c, hipMemcpyAsync(&found, &S->found, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  EVH_HIP(c, hipMemcpyAsync(info, S->info, sizeof(info), hipMemcpyDeviceToHost, c->stream));
  if (h_mask && n > 0) EVH_HIP(c, hipMemcpyAsync(h_mask, c->orb.mask, (size_t)n, hipMemcpyDeviceToHost, c->stream));
  EVH_HIP(c, hipStreamSynchronize(c->stream));
  memcpy(h_H, Hh, sizeof(Hh));
  *h_found = found;
  if (h_info) memcpy(h_info, info, sizeof(info));
  return EVH_SUCCESS;
}

int evh_find_homography_ransac(evh_ctx* c, const float* d_pts, int n, double thr, int max_iters, double conf, double* h_H,
                               uint8_t* h_mask, int* h_found, int* h_info) {
  return find_homography_entry(c, d_pts, n, thr, max_iters, conf, 0, h_H, h_mask, h_found, h_info);
}
int evh_find_homography_ransac_fixed(evh_ctx* c, const float* d_pts, int n, double thr, int max_iters, double conf,
                                     double* h_H, uint8_t* h_mask, int* h_found, int* h_info) {
  return find_homography_entry(c, d_pts, n, thr, max_iters, conf, 1, h_H, h_mask, h_found, h_info);
}

int evh_static_filter(evh_ctx* c, const double* h_H, const float* d_pts, int n, float* d_out_pts, int* h_count) {
  if (!c || !h_H || (!d_pts && n > 0) || !d_out_pts || !h_count || n < 0) return evh_fail(c, EVH_ERR_INVALID, "evh_static_filter: bad argument");
  if (n > c->kcap * c->max_frames) return evh_fail(c, EVH_ERR_CAPACITY, "evh_static_filter: too many rows");
  if ((((uintptr_t)d_pts) | ((uintptr_t)d_out_pts)) & 15) return evh_fail(c, EVH_ERR_INVALID, "row buffers must be 16-byte aligned");
  { int jr = evh_join_solve(c); if (jr) return jr; }
  EvhSmall* S = c->d_small;
  EVH_HIP(c, hipMemcpyAsync(S->H, h_H, 9 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  int* d_cnt = &S->count;
  int rc = evh_launch_static_filter(c, S->H, d_pts, n, reinterpret_cast<int*>(c->orb.lm), d_out_pts, d_cnt);
  if (rc) return rc;
  EVH_HIP(c, hipMemcpyAsync(h_count, d_cnt, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  EVH_HIP(c, hipStreamSynchronize(c->stream));
  return EVH_SUCCESS;
}

// the multi-type entries' merge stage on caller rows: one "pair" whose concatenation is the n rows themselves
int evh_remove_double_matching(evh_ctx* c, const float* d_pts, int n, float* d_out, int* h_count) {
  if (!c || (!d_pts && n > 0) || (!d_out && n > 0) || !h_count || n < 0)
    return evh_fail(c, EVH_ERR_INVALID, "evh_remove_double_matching: bad argument");
  // the largest concatenation a multi-type pair can hold: three feature types of up to 65 535 rows each
  if (n > 3 * 65535) return evh_fail(c, EVH_ERR_CAPACITY, "evh_remove_double_matching: too many rows");
  if ((((uintptr_t)d_pts) | ((uintptr_t)d_out)) & 15) return evh_fail(c, EVH_ERR_INVALID, "row buffers must be 16-byte aligned");
  if (n == 0) { *h_count = 0; return EVH_SUCCESS; }
  const uintptr_t lo = (uintptr_t)d_pts, lo2 = (uintptr_t)d_out, len = sizeof(float) * 4 * (size_t)n;
  if (lo < lo2 + len && lo2 < lo + len)                 // k_merge reads a key's last row while other rows are being written
    return evh_fail(c, EVH_ERR_INVALID, "evh_remove_double_matching: d_pts and d_out overlap");
  { int jr = evh_join_solve(c); if (jr) return jr; }        // d_small is the staging area of a one-pair solve still in flight
  EvhSmall* S = c->d_small;
  const int head[2] = {n, 0};                           // nacc, accstatus
  EVH_HIP(c, hipMemcpyAsync(&S->merge.nacc, head, sizeof(head), hipMemcpyHostToDevice, c->stream));
  EvhMergeArgs M{};
  M.acc = d_pts; M.nacc = &S->merge.nacc; M.accstatus = &S->merge.accstatus; M.acc_stride = n;
  M.out = d_out; M.nout = &S->merge.nout; M.status = &S->merge.status; M.out_stride = n;
  int rc = evh_launch_merge(c, M, 1);
  if (rc) return rc;
  EVH_HIP(c, hipMemcpyAsync(h_count, &S->merge.nout, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  EVH_HIP(c, hipStreamSynchronize(c->stream));
  return EVH_SUCCESS;
}

// ---- N4: SIFT ------------------------------------------------------------------------------------------------------------------
int evh_sift_enable(evh_ctx* c, int max_sift_features) {
  if (!c) return EVH_ERR_INVALID;
  return evh_sift_allocate(c, max_sift_features);
}

int evh_sift_capacity(const evh_ctx* c) { return c ? c->sift.cap : EVH_ERR_INVALID; }

int evh_sift_detect_batch(evh_ctx* c, const uint8_t* d_frames, int nframes, int src_w, int src_h, int channels,
                          int64_t row_stride, int64_t frame_stride, int w, int h) {
  if (!c) return EVH_ERR_INVALID;
  if (!c->sift.cap) return evh_fail(c, EVH_ERR_INVALID, "evh_sift_detect_batch: call evh_sift_enable first");
  return kp_detect_batch(c, "evh_sift_detect_batch", d_frames, nframes, src_w, src_h, channels, row_stride, frame_stride, w, h,
                         [&] { return evh_launch_sift(c, nframes, w, h); });
}

int evh_sift_count(evh_ctx* c, int frame) {
  return kp_count(c, EVH_FEATURE_SIFT, "SIFT", "more SIFT key points (or scale-space extrema) than evh_sift_enable reserved for a frame", frame);
}

int evh_sift_download(evh_ctx* c, int frame, float* h_xy, float* h_desc, int32_t* h_octave, float* h_size, float* h_angle,
                      float* h_response) {
  const int n = evh_sift_count(c, frame);
  if (n <= 0) return n;
  std::vector<uint8_t> d8(h_desc ? (size_t)n * 128 : 0);
  if (int rc = kp_download(c, c->sift, frame, n, h_desc ? d8.data() : nullptr, h_xy, h_size, h_angle, h_response, h_octave, nullptr)) return rc;
  for (size_t i = 0; i < d8.size(); i++) h_desc[i] = (float)d8[i];
  return n;
}

int evh_sift_octave_info(const evh_ctx* c, int octave, int* w, int* h) {
  if (!c || !c->sift_geom_valid || octave < 0) return EVH_ERR_INVALID;
  if (octave >= c->sg.noct) return 1;
  if (w) *w = c->sg.ow[octave]; if (h) *h = c->sg.oh[octave];
  return EVH_SUCCESS;
}

int evh_sift_download_gauss(evh_ctx* c, int frame, int octave, int layer, float* h_pixels) {
  if (!c || !c->sift_geom_valid || !h_pixels || octave < 0 || octave >= c->sg.noct || layer < 0 || layer > 5 || frame < 0)
    return evh_fail(c, EVH_ERR_INVALID, "evh_sift_download_gauss: bad argument");
  // only the LAST group's scale space is resident
  const int g0 = ((c->sift.frames_resident - 1) / c->sift.group) * c->sift.group;
  if (frame < g0 || frame >= c->sift.frames_resident) return evh_fail(c, EVH_ERR_INVALID, "evh_sift_download_gauss: that frame's scale space is no longer resident");
  const EvhSiftGeom& g = c->sg;
  const float* src = c->d_sift_pyr + (int64_t)(frame - g0) * c->sift_pyr_frame_floats + g.ooff[octave] + (int64_t)layer * g.os[octave] * g.oh[octave];
  EVH_HIP(c, hipMemcpy2DAsync(h_pixels, sizeof(float) * g.ow[octave], src, sizeof(float) * g.os[octave], sizeof(float) * g.ow[octave],
                              g.oh[octave], hipMemcpyDeviceToHost, c->stream));
  EVH_HIP(c, hipStreamSynchronize(c->stream));
  return EVH_SUCCESS;
}

int evh_match_knn2_l2f32(evh_ctx* c, const float* d_q, int nq, const float* d_t, int nt, int dim, int32_t* d_idx, float* d_dist) {
  if (!c || !d_idx || !d_dist || nq < 0 || nt < 0) return evh_fail(c, EVH_ERR_INVALID, "evh_match_knn2_l2f32: bad argument");
  if (nq == 0) return EVH_SUCCESS;
  if (((uintptr_t)d_q | (uintptr_t)d_t) & 15) return evh_fail(c, EVH_ERR_INVALID, "descriptor buffers must be 16-byte aligned");
  EvhKnnF32Args A{d_q, d_t, nq, nt, dim, d_idx, d_dist};
  return evh_launch_knn2_f32(c, A);
}

int evh_ratio_unique_filter_f32(evh_ctx* c, const int32_t* d_idx, const float* d_dist, int nq, int nt, const float* d_xy_q,
                                const float* d_xy_t, double ratio, int min_matches, float* d_pts, int* h_count, int* h_status) {
  return ratio_filter(c, "evh_ratio_unique_filter_f32", d_idx, reinterpret_cast<const uint32_t*>(d_dist), 1, nq, nt, d_xy_q, d_xy_t,
                      ratio, min_matches, d_pts, h_count, h_status);
}

// ---- decoded 4:2:0 planes as the source (video_processing.py:58,70) ----------------------------------------------------------
int evh_yuv420_to_bgr(evh_ctx* c, const evh_yuv420* src, int nframes, int w, int h, uint8_t* d_bgr, int64_t row_stride,
                      int64_t frame_stride) {
  if (int rc = evh_check_yuv420(c, "evh_yuv420_to_bgr", src, nframes, w, h)) return rc;
  if (!d_bgr) return evh_fail(c, EVH_ERR_INVALID, "evh_yuv420_to_bgr: d_bgr is NULL");
  if (row_stride < (int64_t)w * 3 || (nframes > 1 && frame_stride < (h - 1) * row_stride + (int64_t)w * 3))
    return evh_fail(c, EVH_ERR_INVALID, "evh_yuv420_to_bgr: output stride smaller than a row / frame");
  return evh_launch_yuv420_to_bgr(c, *src, nframes, w, h, d_bgr, row_stride, frame_stride);
}

int evh_orb_detect_batch_yuv420(evh_ctx* c, const evh_yuv420* src, int nframes, int src_w, int src_h, int w, int h,
                                int nfeatures) {
  return detect_batch(c, yuv420_frames(src), nframes, src_w, src_h, w, h, nfeatures);
}

// ---- N4: SURF --------------------------------------------------------------------------------------------------------------------
int evh_surf_enable(evh_ctx* c, int max_surf_features) {
  if (!c) return EVH_ERR_INVALID;
  return evh_surf_allocate(c, max_surf_features);
}
int evh_surf_capacity(const evh_ctx* c) { return c ? c->surf.cap : EVH_ERR_INVALID; }

int evh_surf_detect_batch(evh_ctx* c, const uint8_t* d_frames, int nframes, int src_w, int src_h, int channels,
                          int64_t row_stride, int64_t frame_stride, int w, int h, double hessian_threshold) {
  if (!c) return EVH_ERR_INVALID;
  if (!c->surf.cap) return evh_fail(c, EVH_ERR_INVALID, "evh_surf_detect_batch: call evh_surf_enable first");
  if (!(hessian_threshold >= 0)) return evh_fail(c, EVH_ERR_INVALID, "evh_surf_detect_batch: hessian_threshold must be >= 0");
  return kp_detect_batch(c, "evh_surf_detect_batch", d_frames, nframes, src_w, src_h, channels, row_stride, frame_stride, w, h,
                         [&] { return evh_launch_surf(c, nframes, w, h, (float)hessian_threshold); });
}

int evh_surf_count(evh_ctx* c, int frame) {
  return kp_count(c, EVH_FEATURE_SURF, "SURF", "more SURF key points than evh_surf_enable reserved for a frame", frame);
}

int evh_surf_download(evh_ctx* c, int frame, float* h_xy, float* h_desc, float* h_size, float* h_angle, float* h_response,
                      int32_t* h_octave, int32_t* h_laplacian) {
  const int n = evh_surf_count(c, frame);
  if (n <= 0) return n;
  if (int rc = kp_download(c, c->surf, frame, n, h_desc, h_xy, h_size, h_angle, h_response, h_octave, h_laplacian)) return rc;
  return n;
}

int evh_surf_download_integral(evh_ctx* c, int frame, int32_t* h_sum) {
  if (!c || !h_sum || !c->surf_tab_w || frame < 0) return evh_fail(c, EVH_ERR_INVALID, "evh_surf_download_integral: bad argument");
  const int g0 = ((c->surf.frames_resident - 1) / c->surf.group) * c->surf.group;
  if (frame < g0 || frame >= c->surf.frames_resident) return evh_fail(c, EVH_ERR_INVALID, "evh_surf_download_integral: that frame's integral image is no longer resident");
  const int w = c->surf_tab_w, h = c->surf_tab_h, st = (w + 1 + 15) & ~15;
  EVH_HIP(c, hipMemcpy2DAsync(h_sum, sizeof(int) * (w + 1), c->d_surf_sum + (int64_t)(frame - g0) * c->surf_sum_frame_ints, sizeof(int) * st,
                              sizeof(int) * (w + 1), h + 1, hipMemcpyDeviceToHost, c->stream));
  EVH_HIP(c, hipStreamSynchronize(c->stream));
  return EVH_SUCCESS;
}

}  // extern "C"
