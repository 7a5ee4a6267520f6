// evh_batch.hip -- host only: what a batch entry asks for (EvhBatch), the one pipeline that runs it (run_batch), and the pair /
// stream / ragged entry points of include/evhip.h, each of which fills the struct and calls it.  No kernel lives here.
#include "evh_internal.h"
#include "evh_match.h"
#include "evh_ransac.h"
#include <cstring>

namespace {

struct EvhRansacParams { double thr; int max_iters; double conf; int force_max; };
const EvhRansacParams kReferenceRansac{3.0, 2000, 0.995, 0};    // constants.py:22 THRESHOLD_FOR_FIND_HOMOGRAPHY, cv2's defaults
// the stream state {H_sup, H_prev} entering a solve (NULL: first pair of the stream) and leaving it (may be NULL), its results
struct EvhSolveIO { const double* state_in; double* state_out; double* H; int32_t* status; };

// the launchers report a lane scratch that could not be allocated (force_max without lane_v)
EvhRansacArgs ransac_args(evh_ctx* c, const EvhPairBufs& B, const EvhRansacParams& P) {
  EvhRansacArgs R{};
  R.fast_solver = c->solver_mode;
  if (P.force_max && evh_ensure_lane_scratch(c) == EVH_SUCCESS) R.lane_v = c->d_lane_v;
  R.pts = B.pts; R.pts2 = B.pts2; R.row_stride = B.cap; R.npts = B.npts; R.npts2 = B.npts2;
  R.status = B.pstatus; R.thr = P.thr; R.max_iters = P.max_iters; R.conf = P.conf; R.force_max = P.force_max;
  R.mask = B.mask; R.crow = B.crow; R.lm = B.lm; R.H1 = B.H1; R.info = B.info;
  return R;
}
EvhRansacArgs solve_args(evh_ctx* c, const EvhPairBufs& B, const EvhRansacParams& P, const EvhSolveIO& io) {
  EvhRansacArgs R = ransac_args(c, B, P);
  R.H = io.H; R.out_status = io.status; R.state_out = io.state_out;
  if (io.state_in) { R.Hsup0 = io.state_in; R.Hprev0 = io.state_in + 9; }
  return R;
}

// K7 + glue on resident slots for `npairs` pairs of one feature type, into the pair buffers B.  filter_kcap selects the
// LDS or the global-scratch form of k_filter and sizes its work arrays.  join_solve_at_filter: the filter overwrites the
// matched-row buffers the previous batch's (asynchronous) solve may still be reading, so it waits for that solve -- as
// late as possible, K7 of this batch overlaps it.  Pair p = (slot q0 + p * step, slot t0 + p * step)
int match_pairs(evh_ctx* c, const EvhFeatView& V, const EvhPairBufs& B, int filter_kcap, bool join_solve_at_filter, int npairs,
                int q0, int t0, int step) {
  int rc;
  if (V.f32) {            // real-valued float rows: the float matcher, distances carried as float bits
    EvhKnnF32Args K{};
    K.q = static_cast<const float*>(V.desc); K.t = K.q; K.dim = 128; K.n_arr = V.counts; K.slot_floats = (int64_t)V.cap * 128;
    K.q_slot0 = q0; K.q_slot_step = step; K.t_slot0 = t0; K.t_slot_step = step;
    K.idx = B.knn_idx; K.dist = reinterpret_cast<float*>(B.knn_d2); K.out_stride = B.cap;
    { EvhProfScope ps(c, EVH_ST_KNN); rc = evh_launch_knn2_f32(c, K, npairs); }
  } else {
    EvhKnnArgs K{};
    K.q = static_cast<const uint8_t*>(V.desc); K.t = K.q; K.slot_bytes = (int64_t)V.cap * V.desc_bytes; K.desc_bytes = V.desc_bytes;
    K.nq_arr = V.counts; K.nt_arr = V.counts;
    K.q_slot0 = q0; K.q_slot_step = step; K.t_slot0 = t0; K.t_slot_step = step;
    K.idx = B.knn_idx; K.d2 = B.knn_d2; K.out_stride = B.cap; K.hamming = 0;
    { EvhProfScope ps(c, EVH_ST_KNN); rc = evh_launch_knn2(c, K, npairs); }
  }
  if (rc) return rc;
  EvhFilterArgs F{};
  F.idx = B.knn_idx; F.d2 = B.knn_d2; F.knn_stride = B.cap; F.d2_is_dist = V.f32 ? 1 : 0;
  F.xy_q = V.xy; F.xy_t = V.xy; F.xy_slot_floats = (int64_t)V.cap * 2;
  F.nq_arr = V.counts; F.nt_arr = V.counts; F.flags_arr = V.flags;
  F.q_slot0 = q0; F.q_slot_step = step; F.t_slot0 = t0; F.t_slot_step = step;
  F.ratio = 0.5; F.min_matches = 4;  // constants.py:25,28 (LOWES_RATIO, MINIMUM_MATCHING_POINTS)
  F.pts = B.pts; F.pts_stride = B.cap; F.npts = B.npts; F.status = B.pstatus; F.kcap = filter_kcap;
  if (join_solve_at_filter && c->solve_pending) EVH_HIP(c, hipStreamWaitEvent(c->stream, c->ev_solve_done, 0));
  EvhProfScope ps(c, EVH_ST_FILTER);
  return evh_launch_filter(c, F, npairs);
}
int match_orb_pairs(evh_ctx* c, int npairs, int q0, int t0, int step) {      // orders itself behind a pending async solve
  return match_pairs(c, evh_feat_view(c, EVH_FEATURE_ORB), c->orb, c->kcap, true, npairs, q0, t0, step);
}

int final_solve(evh_ctx* c, const EvhRansacArgs& R, const EvhSolveLayout& L) {
  EvhProfScope ps(c, EVH_ST_RANSAC_FINAL, c->stream);
  return evh_launch_ransac_final(c, R, L);
}

// RANSAC #1 + static filter over `npairs` pair slots, then compute_homography as L lays it out, on the solve stream when
// asynchronous solve is enabled
int solve_pairs(evh_ctx* c, const EvhRansacArgs& R, int npairs, const EvhSolveLayout& L) {
  hipStream_t main = c->stream;
  const bool async = c->async_solve && c->solve_stream;
  if (async) {
    EVH_HIP(c, hipEventRecord(c->ev_match_done, main));
    EVH_HIP(c, hipStreamWaitEvent(c->solve_stream, c->ev_match_done, 0));
    c->stream = c->solve_stream;          // the launchers enqueue on c->stream
  }
  int rc;
  { EvhProfScope ps(c, EVH_ST_RANSAC_STATIC, c->stream); rc = evh_launch_ransac_static(c, R, npairs); }
  if (!rc) rc = final_solve(c, R, L);
  if (async) {
    hipError_t e = hipEventRecord(c->ev_solve_done, c->solve_stream);
    c->stream = main;
    c->solve_pending = true;
    if (e != hipSuccess) return evh_fail(c, EVH_ERR_HIP, std::string("hipEventRecord: ") + hipGetErrorString(e));
  }
  return rc;
}

// ---- multi-type pairs (frame_processing.py:91-104) ---------------------------------------------------------------------------
int ensure_multitype(evh_ctx* c) {
  if (c->mt.cap) return EVH_SUCCESS;
  const int each = std::max(c->kcap, std::max(c->sift.cap, c->surf.cap)), cap = c->kcap + c->sift.cap + c->surf.cap;
  if (each > 65536)
    return evh_fail(c, EVH_ERR_CAPACITY, "multi-type pairs: at most 65536 key points per frame and type");
  const size_t P = (size_t)c->max_frames, K = (size_t)cap, first = c->owned.size();
  int rc = evh_alloc_pair_bufs(c, c->mt, cap);
  if (!rc) rc = dalloc(c, &c->d_acc, P * K * 4);
  if (!rc) rc = dalloc(c, &c->d_nacc, P);
  if (!rc) rc = dalloc(c, &c->d_accstatus, P);
  if (rc) { dfree_from(c, first); c->mt.cap = 0; }     // a partial allocation is released: a later call starts afresh
  return rc;
}

// the type list of an entry that takes one: every name known, none twice, SIFT / SURF enabled; -> which detectors it names
struct EvhWanted { bool orb = false, sift = false, surf = false; };
int check_types(evh_ctx* c, const char* who, const int* types, int ntypes, EvhWanted& want) {
  const std::string W = std::string(who) + ": ";
  if (!types || ntypes < 1 || ntypes > 8) return evh_fail(c, EVH_ERR_INVALID, W + "bad feature type list");
  for (int i = 0; i < ntypes; i++) {
    // the concatenation buffer holds one segment per detector (kcap + sift.cap + surf.cap rows): a type named twice would
    // overflow it, so it is refused (the reference would simply match the same key points twice and deduplicate them)
    bool* seen = types[i] == EVH_FEATURE_ORB ? &want.orb : types[i] == EVH_FEATURE_SIFT ? &want.sift :
                 types[i] == EVH_FEATURE_SURF ? &want.surf : nullptr;
    if (!seen) return evh_fail(c, EVH_ERR_INVALID, W + "unknown feature type");
    if (*seen) return evh_fail(c, EVH_ERR_INVALID, W + "a feature type appears twice in the list");
    *seen = true;
  }
  if (want.sift && !c->sift.cap) return evh_fail(c, EVH_ERR_INVALID, W + "SIFT in the list needs evh_sift_enable");
  if (want.surf && !c->surf.cap) return evh_fail(c, EVH_ERR_INVALID, W + "SURF in the list needs evh_surf_enable");
  if (c->mt.cap && c->mt.cap < c->kcap + c->sift.cap + c->surf.cap)
    return evh_fail(c, EVH_ERR_INVALID, W + "enable SIFT and SURF before the first multi-type call");
  return EVH_SUCCESS;
}

// the device copy of a ragged batch's segment table, uploaded stream-ordered through pinned staging.  The turns are for the
// HOST side: a call waits only for the upload EVH_SEG_TURNS calls back to have left its staging table, never for the device
// to drain (the device tables are ordered by the stream: the upload sits behind this call's filter, which has joined the
// previous call's solve)
int upload_segs(evh_ctx* c, const evh_stream_seg* h_segs, int nstreams, const evh_stream_seg** d_out) {
  const size_t per = (size_t)c->max_frames / 2;
  if (!c->d_segs) {
    int rc = dalloc(c, &c->d_segs, per * EVH_SEG_TURNS);
    if (rc) return rc;
    if (hipHostMalloc(reinterpret_cast<void**>(&c->h_segs), per * EVH_SEG_TURNS * sizeof(evh_stream_seg), hipHostMallocDefault) != hipSuccess) {
      c->h_segs = nullptr;
      dfree(c, &c->d_segs);
      return evh_fail(c, EVH_ERR_HIP, "segment table: pinned staging (hipHostMalloc) could not be allocated");
    }
  }
  // (a call that fails below has used up its turn without recording an event: harmless, the turn's next user finds no
  // event, or an older one that has long completed.  A table holds max_frames / 2 segments: check_batch has refused
  // segments of fewer than 2 frames and batches of more than max_frames frames, so nstreams cannot exceed that)
  const unsigned t = c->seg_turn++ % EVH_SEG_TURNS;
  if (!c->ev_segs[t]) EVH_HIP(c, hipEventCreateWithFlags(&c->ev_segs[t], hipEventDisableTiming));
  else EVH_HIP(c, hipEventSynchronize(c->ev_segs[t]));              // the upload that used this turn last has left the staging
  std::memcpy(c->h_segs + t * per, h_segs, sizeof(evh_stream_seg) * (size_t)nstreams);
  EVH_HIP(c, hipMemcpyAsync(c->d_segs + t * per, c->h_segs + t * per, sizeof(evh_stream_seg) * (size_t)nstreams, hipMemcpyHostToDevice, c->stream));
  EVH_HIP(c, hipEventRecord(c->ev_segs[t], c->stream));
  *d_out = c->d_segs + t * per;
  return EVH_SUCCESS;
}

// ---- what a batch entry asks for -----------------------------------------------------------------------------------------------
// How the frames pair up.  Pair slot p is (frame 2p + 1, frame 2p) for independent pairs, else (frame p + 1, frame p): a slot
// that straddles two streams is computed and never read.
enum { EVH_PAIRS_INDEPENDENT, EVH_PAIRS_UNIFORM, EVH_PAIRS_RAGGED, EVH_PAIRS_UNKNOWN };
struct EvhPairing {
  int kind;                        // EVH_PAIRS_UNKNOWN: the caller's mode value named none of them
  int64_t n;                       // INDEPENDENT: pairs; UNIFORM: frames of EACH stream; RAGGED: frames of the whole batch
  int nstreams;                    // UNIFORM, RAGGED
  const evh_stream_seg* h_segs;    // RAGGED: the nstreams segments that tile the n frames (host)
};
EvhPairing pairing_of_mode(int mode, int npairs) {          // the mode argument of the evh_pair_* entries
  if (mode == EVH_MODE_INDEPENDENT_PAIRS) return {EVH_PAIRS_INDEPENDENT, npairs, 0, nullptr};
  if (mode == EVH_MODE_STREAM) return {EVH_PAIRS_UNIFORM, (int64_t)npairs + 1, 1, nullptr};
  return {EVH_PAIRS_UNKNOWN, npairs, 0, nullptr};
}
EvhPairing one_stream(int nframes) { return {EVH_PAIRS_UNIFORM, nframes, 1, nullptr}; }

// Which detectors.  FUSED_ORB: no list, the fused ORB path (asynchronous solve when enabled).  MULTI: the list goes through the
// multi-type path (c->mt, accumulate, merge, no asynchronous solve), {ORB} too.  MULTI_UNLESS_ORB: the same, but a list of
// exactly {ORB} takes the fused path (the ragged entries).
enum { EVH_LIST_FUSED_ORB, EVH_LIST_MULTI, EVH_LIST_MULTI_UNLESS_ORB };
struct EvhTypeList { int use; const int32_t* types; int ntypes; };
const EvhTypeList kFusedOrb{EVH_LIST_FUSED_ORB, nullptr, 0};

struct EvhBatch {
  const char* who;                 // the entry that was called: every message begins with it
  EvhFrames frames; int sw, sh, w, h, nfeatures;          // (sw, sh): the frames as handed over, (w, h): the size ORB runs at
  EvhPairing pairing;
  EvhTypeList list;
  EvhRansacParams ransac;
  EvhSolveIO io;
};
// what check_batch derives from the pairing
struct EvhBatchShape {
  int nframes, npairs, step;       // frames, pair slots, frames from one pair slot to the next
  int share_group;                 // FAST thresholds are shared inside groups of this many consecutive frames (0: not at all)
  int max_pairs;                   // RAGGED: pairs of the longest stream
};

// The checks every batch entry makes before anything else, in the order every entry made them: NULL frames and minimum
// counts, the mode, max_frames, the segment table.  (The outputs are the caller's to check first, the type list and the
// frame description follow: run_batch.)
int check_batch(evh_ctx* c, const EvhBatch& B, EvhBatchShape& S) {
  const std::string W = std::string(B.who) + ": ";
  const EvhPairing& P = B.pairing;
  const bool streams = P.kind == EVH_PAIRS_UNIFORM || P.kind == EVH_PAIRS_RAGGED;
  if ((!B.frames.planes && !B.frames.packed) || (streams ? P.nstreams < 1 || P.n < 2 : P.n < 1) ||
      (P.kind == EVH_PAIRS_RAGGED && !P.h_segs))
    return evh_fail(c, EVH_ERR_INVALID, W + "bad argument");
  if (P.kind == EVH_PAIRS_UNKNOWN) return evh_fail(c, EVH_ERR_INVALID, W + "unknown mode");
  const int64_t nframes = P.kind == EVH_PAIRS_INDEPENDENT ? 2 * P.n : P.kind == EVH_PAIRS_UNIFORM ? P.nstreams * P.n : P.n;
  if (nframes > c->max_frames) return evh_fail(c, EVH_ERR_CAPACITY, W + "batch needs more frame slots than max_frames");
  S.nframes = (int)nframes;
  S.npairs = streams ? S.nframes - 1 : (int)P.n;
  S.step = streams ? 1 : 2;
  // shared by the two frames of a pair, by the frames of a stream, or by the frames 2k, 2k + 1 of a ragged batch across segment
  // borders too: a borrowed threshold that proves too high is redone, so sharing is exact per frame
  S.share_group = !c->fast_share ? 0 : P.kind == EVH_PAIRS_INDEPENDENT ? 2 : P.kind == EVH_PAIRS_UNIFORM ? (int)P.n : S.nframes;
  S.max_pairs = 0;
  if (P.kind != EVH_PAIRS_RAGGED) return EVH_SUCCESS;
  int next = 0;
  for (int s = 0; s < P.nstreams; s++) {
    const evh_stream_seg& g = P.h_segs[s];
    if (g.nframes < 2) return evh_fail(c, EVH_ERR_INVALID, W + "a segment needs at least 2 frames");
    if (g.first_frame != next || g.nframes > S.nframes - next)
      return evh_fail(c, EVH_ERR_INVALID, W + "the segments must tile [0, total_frames) in ascending order");
    if (g.reserved != 0) return evh_fail(c, EVH_ERR_INVALID, W + "evh_stream_seg.reserved must be 0");
    if (!g.start && !B.io.state_in) return evh_fail(c, EVH_ERR_INVALID, W + "a segment with start == 0 needs d_state_in");
    next += g.nframes;
    S.max_pairs = std::max(S.max_pairs, g.nframes - 1);
  }
  if (next != S.nframes) return evh_fail(c, EVH_ERR_INVALID, W + "the segments must tile [0, total_frames) in ascending order");
  return EVH_SUCCESS;
}

// the fused ORB front: detect every frame, match every pair slot into c->orb
int detect_match_orb(evh_ctx* c, const EvhBatch& B, const EvhBatchShape& S) {
  int rc = evh_ingest_level0(c, B.who, B.frames, S.nframes, B.sw, B.sh, B.w, B.h, B.nfeatures);
  if (!rc) rc = evh_orb_stages(c, S.nframes, S.share_group);
  if (!rc) rc = match_orb_pairs(c, S.npairs, 1, 0, S.step);
  return rc;
}

// the multi-type front, in list order (the reference's default list is SURF, SIFT, ORB): per type detect, match, RANSAC #1,
// static filter; concatenate; remove_double_matching -> the merged static rows in c->mt
int detect_match_types(evh_ctx* c, const EvhBatch& B, const EvhBatchShape& S, const EvhWanted& want) {
  int rc = ensure_multitype(c);
  if (rc) return rc;
  if ((rc = evh_join_solve(c))) return rc;
  EvhFrames P = B.frames;
  if (P.yuv) {      // SIFT and SURF read BGR through the shared front end: the chunk is converted once, then takes that path
    const int64_t row = (int64_t)B.sw * 3, frame = row * B.sh;
    if ((rc = evh_check_yuv420(c, B.who, P.yuv, S.nframes, B.sw, B.sh))) return rc;
    if ((rc = grow(c, &c->d_yuv_bgr, &c->yuv_bgr_bytes, (size_t)frame * S.nframes))) return rc;
    if ((rc = evh_launch_yuv420_to_bgr(c, *P.yuv, S.nframes, B.sw, B.sh, c->d_yuv_bgr, row, frame))) return rc;
    P = packed_frames(c->d_yuv_bgr, 3, row, frame);
  }
  if ((rc = evh_ingest_level0(c, B.who, P, S.nframes, B.sw, B.sh, B.w, B.h, B.nfeatures))) return rc;
  if (want.sift && (rc = evh_launch_sift(c, S.nframes, B.w, B.h))) return rc;       // reads level 0 before ORB's kernels run on it
  if (want.surf && (rc = evh_launch_surf(c, S.nframes, B.w, B.h, 400.f))) return rc; // SURF_create(extended=1, hessianThreshold=400)
  if (want.orb && (rc = evh_orb_stages(c, S.nframes, S.share_group))) return rc;
  const EvhRansacArgs R = ransac_args(c, c->mt, B.ransac);
  const int each = std::max(c->kcap, std::max(c->sift.cap, c->surf.cap));   // one filter form for every type of the list
  for (int i = 0; i < B.list.ntypes; i++) {
    // the solve was joined once, above: this path has no asynchronous solve of its own to overlap
    if ((rc = match_pairs(c, evh_feat_view(c, B.list.types[i]), c->mt, each, false, S.npairs, 1, 0, S.step))) return rc;
    { EvhProfScope ps(c, EVH_ST_RANSAC_STATIC); rc = evh_launch_ransac_static(c, R, S.npairs); }
    if (rc) return rc;
    EvhAccArgs A{};
    A.rows = c->mt.pts2; A.nrows = c->mt.npts2; A.status = c->mt.pstatus; A.row_stride = c->mt.cap;
    A.acc = c->d_acc; A.nacc = c->d_nacc; A.accstatus = c->d_accstatus; A.acc_stride = c->mt.cap; A.first = i == 0;
    if ((rc = evh_launch_accumulate(c, A, S.npairs))) return rc;
  }
  EvhMergeArgs M{};
  M.acc = c->d_acc; M.nacc = c->d_nacc; M.accstatus = c->d_accstatus; M.acc_stride = c->mt.cap;
  M.out = c->mt.pts2; M.nout = c->mt.npts2; M.status = c->mt.pstatus; M.out_stride = c->mt.cap;
  return evh_launch_merge(c, M, S.npairs);
}

// the context's record of the last batch whose static rows are resident (evh_batch_static_info / _rows): every entry that
// writes pts2 / npts2 / pstatus of c->orb or c->mt forgets it first, a batch that ran through sets it
void forget_static(evh_ctx* c) { c->static_bufs = nullptr; c->static_pairs = 0; }
void record_static(evh_ctx* c, const EvhPairBufs& B, int npairs) { c->static_bufs = &B; c->static_pairs = npairs; }

// frames -> H per pair slot.  Every refusal comes before the first launch and before anything is written (one exception as
// before: a list entry on planes converts them before the geometry is set).
int run_batch(evh_ctx* c, const EvhBatch& B) {
  if (!c) return EVH_ERR_INVALID;
  if (!B.io.H || !B.io.status) return evh_fail(c, EVH_ERR_INVALID, std::string(B.who) + ": bad argument");
  EvhBatchShape S;
  int rc = check_batch(c, B, S);
  if (rc) return rc;
  EvhWanted want;
  bool multi = B.list.use != EVH_LIST_FUSED_ORB;
  if (multi && (rc = check_types(c, B.who, B.list.types, B.list.ntypes, want))) return rc;
  if (B.list.use == EVH_LIST_MULTI_UNLESS_ORB && B.list.ntypes == 1 && want.orb) multi = false;
  forget_static(c);
  if ((rc = multi ? detect_match_types(c, B, S, want) : detect_match_orb(c, B, S))) return rc;
  const EvhPairing& P = B.pairing;
  const evh_stream_seg* d_segs = nullptr;
  if (P.kind == EVH_PAIRS_RAGGED && (rc = upload_segs(c, P.h_segs, P.nstreams, &d_segs))) return rc;
  const EvhSolveLayout L = P.kind == EVH_PAIRS_INDEPENDENT ? EvhSolveLayout::pairs(S.npairs) :
                           P.kind == EVH_PAIRS_UNIFORM ? EvhSolveLayout::streams((int)P.n - 1, P.nstreams, (int)P.n) :
                                                         EvhSolveLayout::ragged(S.npairs, P.nstreams, d_segs, S.max_pairs);
  const EvhRansacArgs R = solve_args(c, multi ? c->mt : c->orb, B.ransac, B.io);
  rc = multi ? final_solve(c, R, L) : solve_pairs(c, R, S.npairs, L);       // (the multi-type front has done RANSAC #1 per type)
  if (!rc) record_static(c, multi ? c->mt : c->orb, S.npairs);              // the final solve only reads the static rows
  return rc;
}

// final solve of pair slot 0 of the ORB buffers (its static rows are resident), optionally behind the superposition
// h_Hsup; H and status to the host
int final_solve_one(evh_ctx* c, const double* h_Hsup, double* h_H, int* h_status) {
  EvhSmall* S = c->d_small;
  EvhRansacArgs R = solve_args(c, c->orb, kReferenceRansac, {nullptr, nullptr, S->H, &S->out_status});
  if (h_Hsup) {
    EVH_HIP(c, hipMemcpyAsync(S->Hsup, h_Hsup, 9 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    R.Hsup0 = S->Hsup;
  }
  // the stream kernel with one pair applies the optional pre-transform; Hprev0 = Hsup0 only marks "not first"
  R.Hprev0 = R.Hsup0;
  int rc = evh_launch_ransac_final(c, R, h_Hsup ? EvhSolveLayout::streams(1, 1, 1) : EvhSolveLayout::pairs(1));
  if (rc) return rc;
  EVH_HIP(c, hipStreamSynchronize(c->stream));
  EVH_HIP(c, hipMemcpy(h_H, S->H, 9 * sizeof(double), hipMemcpyDeviceToHost));
  EVH_HIP(c, hipMemcpy(h_status, &S->out_status, sizeof(int), hipMemcpyDeviceToHost));
  return EVH_SUCCESS;
}

}  // namespace

extern "C" {

int evh_pair_homography_batch(evh_ctx* c, const uint8_t* d_frames, int npairs, int mode, int w, int h, int channels,
                              int64_t row_stride, int64_t frame_stride, int nfeatures, double ransac_thr,
                              int ransac_max_iters, double ransac_conf, int force_max_iters, double* d_H, int32_t* d_status) {
  return run_batch(c, {"evh_pair_homography_batch", packed_frames(d_frames, channels, row_stride, frame_stride), w, h, w, h,
                       nfeatures, pairing_of_mode(mode, npairs), kFusedOrb,
                       {ransac_thr, ransac_max_iters, ransac_conf, force_max_iters}, {nullptr, nullptr, d_H, d_status}});
}

int evh_stream_homography_batch(evh_ctx* c, const uint8_t* d_frames, int nframes, int w, int h, int channels,
                                int64_t row_stride, int64_t frame_stride, int nfeatures, double ransac_thr,
                                int ransac_max_iters, double ransac_conf, int force_max_iters, const double* d_state_in,
                                double* d_state_out, double* d_H, int32_t* d_status) {
  return run_batch(c, {"evh_stream_homography_batch", packed_frames(d_frames, channels, row_stride, frame_stride), w, h, w, h,
                       nfeatures, one_stream(nframes), kFusedOrb,
                       {ransac_thr, ransac_max_iters, ransac_conf, force_max_iters}, {d_state_in, d_state_out, d_H, d_status}});
}

int evh_stream_homography_batch_resized(evh_ctx* c, const uint8_t* d_frames, int nframes, int src_w, int src_h, int channels,
                                        int64_t row_stride, int64_t frame_stride, int w, int h, int nfeatures,
                                        double ransac_thr, int ransac_max_iters, double ransac_conf, int force_max_iters,
                                        const double* d_state_in, double* d_state_out, double* d_H, int32_t* d_status) {
  return run_batch(c, {"evh_stream_homography_batch_resized", packed_frames(d_frames, channels, row_stride, frame_stride),
                       src_w, src_h, w, h, nfeatures, one_stream(nframes), kFusedOrb,
                       {ransac_thr, ransac_max_iters, ransac_conf, force_max_iters}, {d_state_in, d_state_out, d_H, d_status}});
}

int evh_multi_stream_homography_batch(evh_ctx* c, const uint8_t* d_frames, int nstreams, int frames_per_stream, int w,
                                      int h, int channels, int64_t row_stride, int64_t frame_stride, int nfeatures,
                                      double ransac_thr, int ransac_max_iters, double ransac_conf, int force_max_iters,
                                      const double* d_state_in, double* d_state_out, double* d_H, int32_t* d_status) {
  return run_batch(c, {"evh_multi_stream_homography_batch", packed_frames(d_frames, channels, row_stride, frame_stride), w, h,
                       w, h, nfeatures, {EVH_PAIRS_UNIFORM, frames_per_stream, nstreams, nullptr}, kFusedOrb,
                       {ransac_thr, ransac_max_iters, ransac_conf, force_max_iters}, {d_state_in, d_state_out, d_H, d_status}});
}

int evh_pair_homography_batch_types(evh_ctx* c, const uint8_t* d_frames, int npairs, int mode, int src_w, int src_h,
                                    int channels, int64_t row_stride, int64_t frame_stride, int w, int h, int nfeatures,
                                    const int32_t* h_types, int ntypes, double ransac_thr, int ransac_max_iters,
                                    double ransac_conf, int force_max_iters, double* d_H, int32_t* d_status) {
  return run_batch(c, {"evh_pair_homography_batch_types", packed_frames(d_frames, channels, row_stride, frame_stride),
                       src_w, src_h, w, h, nfeatures, pairing_of_mode(mode, npairs), {EVH_LIST_MULTI, h_types, ntypes},
                       {ransac_thr, ransac_max_iters, ransac_conf, force_max_iters}, {nullptr, nullptr, d_H, d_status}});
}

int evh_stream_homography_batch_types(evh_ctx* c, const uint8_t* d_frames, int nframes, int src_w, int src_h, int channels,
                                      int64_t row_stride, int64_t frame_stride, int w, int h, int nfeatures,
                                      const int32_t* h_types, int ntypes, double ransac_thr, int ransac_max_iters,
                                      double ransac_conf, int force_max_iters, const double* d_state_in, double* d_state_out,
                                      double* d_H, int32_t* d_status) {
  return run_batch(c, {"evh_stream_homography_batch_types", packed_frames(d_frames, channels, row_stride, frame_stride),
                       src_w, src_h, w, h, nfeatures, one_stream(nframes), {EVH_LIST_MULTI, h_types, ntypes},
                       {ransac_thr, ransac_max_iters, ransac_conf, force_max_iters}, {d_state_in, d_state_out, d_H, d_status}});
}

// ---- decoded 4:2:0 planes as the source (video_processing.py:58,70) ----------------------------------------------------------
int evh_stream_homography_batch_yuv420(evh_ctx* c, const evh_yuv420* src, int nframes, int src_w, int src_h, int w, int h,
                                       int nfeatures, double ransac_thr, int ransac_max_iters, double ransac_conf,
                                       int force_max_iters, const double* d_state_in, double* d_state_out, double* d_H,
                                       int32_t* d_status) {
  return run_batch(c, {"evh_stream_homography_batch_yuv420", yuv420_frames(src), src_w, src_h, w, h, nfeatures,
                       one_stream(nframes), kFusedOrb, {ransac_thr, ransac_max_iters, ransac_conf, force_max_iters},
                       {d_state_in, d_state_out, d_H, d_status}});
}

int evh_stream_homography_batch_types_yuv420(evh_ctx* c, const evh_yuv420* src, int nframes, int src_w, int src_h, int w,
                                             int h, int nfeatures, const int32_t* h_types, int ntypes, double ransac_thr,
                                             int ransac_max_iters, double ransac_conf, int force_max_iters,
                                             const double* d_state_in, double* d_state_out, double* d_H, int32_t* d_status) {
  return run_batch(c, {"evh_stream_homography_batch_types_yuv420", yuv420_frames(src), src_w, src_h, w, h, nfeatures,
                       one_stream(nframes), {EVH_LIST_MULTI, h_types, ntypes},
                       {ransac_thr, ransac_max_iters, ransac_conf, force_max_iters}, {d_state_in, d_state_out, d_H, d_status}});
}

// ---- ragged batches of several streams: total_frames frames cut into nstreams segments of consecutive frames, one stream each.
// Everything up to the static filter runs over all frames / pair slots at once; the scans run one workgroup per stream off
// the segment table -------------------------------------------------------------------------------------------------------------
int evh_streams_homography_batch(evh_ctx* c, const uint8_t* d_frames, int total_frames, int src_w, int src_h, int channels,
                                 int64_t row_stride, int64_t frame_stride, int w, int h, int nfeatures, const int32_t* h_types,
                                 int ntypes, const evh_stream_seg* h_segs, int nstreams, double ransac_thr, int ransac_max_iters,
                                 double ransac_conf, int force_max_iters, const double* d_state_in, double* d_state_out,
                                 double* d_H, int32_t* d_status) {
  return run_batch(c, {"evh_streams_homography_batch", packed_frames(d_frames, channels, row_stride, frame_stride), src_w, src_h,
                       w, h, nfeatures, {EVH_PAIRS_RAGGED, total_frames, nstreams, h_segs},
                       {EVH_LIST_MULTI_UNLESS_ORB, h_types, ntypes},
                       {ransac_thr, ransac_max_iters, ransac_conf, force_max_iters}, {d_state_in, d_state_out, d_H, d_status}});
}

int evh_streams_homography_batch_yuv420(evh_ctx* c, const evh_yuv420* src, int total_frames, int src_w, int src_h, int w, int h,
                                        int nfeatures, const int32_t* h_types, int ntypes, const evh_stream_seg* h_segs,
                                        int nstreams, double ransac_thr, int ransac_max_iters, double ransac_conf,
                                        int force_max_iters, const double* d_state_in, double* d_state_out, double* d_H,
                                        int32_t* d_status) {
  // this entry alone refuses a NULL src with the other NULL arguments, ahead of max_frames; the planes themselves are checked
  // with the frame description, like those of the other plane entries
  if (c && !src) return evh_fail(c, EVH_ERR_INVALID, "evh_streams_homography_batch_yuv420: bad argument");
  return run_batch(c, {"evh_streams_homography_batch_yuv420", yuv420_frames(src), src_w, src_h, w, h, nfeatures,
                       {EVH_PAIRS_RAGGED, total_frames, nstreams, h_segs}, {EVH_LIST_MULTI_UNLESS_ORB, h_types, ntypes},
                       {ransac_thr, ransac_max_iters, ransac_conf, force_max_iters}, {d_state_in, d_state_out, d_H, d_status}});
}

// ---- the stream path in two phases, and single pairs on resident frame slots: the same stages, called one by one ------------
int evh_stream_static_batch(evh_ctx* c, const uint8_t* d_frames, int nframes, int w, int h, int channels,
                            int64_t row_stride, int64_t frame_stride, int nfeatures, double ransac_thr,
                            int ransac_max_iters, double ransac_conf, int force_max_iters, float* d_rows, int row_cap,
                            int32_t* d_counts, int32_t* d_status1) {
  if (!c) return EVH_ERR_INVALID;
  if (!d_rows || !d_counts || !d_status1) return evh_fail(c, EVH_ERR_INVALID, "evh_stream_static_batch: bad argument");
  const EvhBatch B{"evh_stream_static_batch", packed_frames(d_frames, channels, row_stride, frame_stride), w, h, w, h, nfeatures,
                   one_stream(nframes), kFusedOrb, {ransac_thr, ransac_max_iters, ransac_conf, force_max_iters}, {}};
  EvhBatchShape S;
  int rc = check_batch(c, B, S);
  if (rc) return rc;
  if (row_cap != c->kcap) return evh_fail(c, EVH_ERR_INVALID, "evh_stream_static_batch: row_cap must equal evh_orb_capacity()");
  forget_static(c);
  if ((rc = detect_match_orb(c, B, S))) return rc;
  { EvhProfScope ps(c, EVH_ST_RANSAC_STATIC); rc = evh_launch_ransac_static(c, ransac_args(c, c->orb, B.ransac), S.npairs); }
  if (rc) return rc;
  EVH_HIP(c, hipMemcpyAsync(d_rows, c->orb.pts2, sizeof(float) * 4 * (size_t)c->kcap * S.npairs, hipMemcpyDeviceToDevice, c->stream));
  EVH_HIP(c, hipMemcpyAsync(d_counts, c->orb.npts2, sizeof(int) * (size_t)S.npairs, hipMemcpyDeviceToDevice, c->stream));
  EVH_HIP(c, hipMemcpyAsync(d_status1, c->orb.pstatus, sizeof(int) * (size_t)S.npairs, hipMemcpyDeviceToDevice, c->stream));
  record_static(c, c->orb, S.npairs);
  return EVH_SUCCESS;
}

int evh_batch_static_info(const evh_ctx* c, int* npairs, int* row_cap) {
  if (!c || !npairs || !row_cap) return EVH_ERR_INVALID;
  *npairs = c->static_bufs ? c->static_pairs : 0;
  *row_cap = c->static_bufs ? c->static_bufs->cap : 0;
  return EVH_SUCCESS;
}

int evh_batch_static_rows(evh_ctx* c, int first_pair, int npairs, float* d_rows, int row_cap, int32_t* d_counts,
                          int32_t* d_status1) {
  if (!c) return EVH_ERR_INVALID;
  const std::string W = "evh_batch_static_rows: ";
  if (!d_rows || !d_counts || !d_status1) return evh_fail(c, EVH_ERR_INVALID, W + "NULL argument");
  const EvhPairBufs* B = c->static_bufs;
  if (!B) return evh_fail(c, EVH_ERR_INVALID, W + "no batch whose static rows are still resident");
  if (first_pair < 0 || npairs < 1 || npairs > c->static_pairs - first_pair)
    return evh_fail(c, EVH_ERR_INVALID, W + "pair range outside the batch's pair slots");
  if (row_cap != B->cap) return evh_fail(c, EVH_ERR_INVALID, W + "row_cap must equal the capacity evh_batch_static_info reports");
  { int jr = evh_join_solve(c); if (jr) return jr; }           // RANSAC #1 and the static filter may run on the solve stream
  const size_t p0 = (size_t)first_pair, n = (size_t)npairs;
  EVH_HIP(c, hipMemcpyAsync(d_rows, B->pts2 + p0 * B->cap * 4, sizeof(float) * 4 * (size_t)B->cap * n, hipMemcpyDeviceToDevice, c->stream));
  EVH_HIP(c, hipMemcpyAsync(d_counts, B->npts2 + p0, sizeof(int) * n, hipMemcpyDeviceToDevice, c->stream));
  EVH_HIP(c, hipMemcpyAsync(d_status1, B->pstatus + p0, sizeof(int) * n, hipMemcpyDeviceToDevice, c->stream));
  return EVH_SUCCESS;
}

int evh_stream_scan(evh_ctx* c, const float* d_rows, int row_cap, const int32_t* d_counts, const int32_t* d_status1,
                    int npairs, double ransac_thr, int ransac_max_iters, double ransac_conf, int force_max_iters,
                    const double* d_state_in, double* d_state_out, double* d_H, int32_t* d_status) {
  if (!c || !d_rows || !d_counts || !d_status1 || !d_H || !d_status || npairs < 1)
    return evh_fail(c, EVH_ERR_INVALID, "evh_stream_scan: bad argument");
  if (row_cap < 1 || row_cap > c->kcap) return evh_fail(c, EVH_ERR_CAPACITY, "row_cap larger than evh_orb_capacity()");
  if (((uintptr_t)d_rows) & 15) return evh_fail(c, EVH_ERR_INVALID, "d_rows must be 16-byte aligned");
  { int jr = evh_join_solve(c); if (jr) return jr; }                  // the scan uses slot 0 of the pair scratch
  forget_static(c);
  EvhRansacArgs R = solve_args(c, c->orb, {ransac_thr, ransac_max_iters, ransac_conf, force_max_iters},
                               {d_state_in, d_state_out, d_H, d_status});
  R.pts2 = const_cast<float*>(d_rows); R.npts2 = const_cast<int*>(d_counts); R.status = const_cast<int*>(d_status1);
  R.row_stride = row_cap; R.info = nullptr;
  return final_solve(c, R, EvhSolveLayout::streams(npairs, 1, npairs));
}

int evh_match_static_from_slots(evh_ctx* c, int cur_slot, int prev_slot, float* h_pts, int cap, int* h_count, int* h_status) {
  if (!c || !h_count || !h_status || cur_slot < 0 || prev_slot < 0 || cur_slot >= c->nframes_resident ||
      prev_slot >= c->nframes_resident)
    return evh_fail(c, EVH_ERR_INVALID, "evh_match_static_from_slots: bad argument");
  { int jr = evh_join_solve(c); if (jr) return jr; }
  forget_static(c);
  int rc = match_orb_pairs(c, 1, cur_slot, prev_slot, 0);
  if (rc) return rc;
  if ((rc = evh_launch_ransac_static(c, ransac_args(c, c->orb, kReferenceRansac), 1))) return rc;
  int st = 0, n = 0;
  EVH_HIP(c, hipMemcpyAsync(&st, c->orb.pstatus, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  EVH_HIP(c, hipMemcpyAsync(&n, c->orb.npts2, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  EVH_HIP(c, hipStreamSynchronize(c->stream));
  *h_status = st; *h_count = n;
  if (st == EVH_PAIR_OK && n > 0 && h_pts) {
    if (n > cap) return evh_fail(c, EVH_ERR_CAPACITY, "h_pts too small");
    EVH_HIP(c, hipMemcpy(h_pts, c->orb.pts2, sizeof(float) * 4 * (size_t)n, hipMemcpyDeviceToHost));
  }
  return EVH_SUCCESS;
}

int evh_compute_homography(evh_ctx* c, const float* h_pts, int n, const double* h_Hsup, double* h_H, int* h_status) {
  if (!c || (!h_pts && n > 0) || !h_H || !h_status || n < 0) return evh_fail(c, EVH_ERR_INVALID, "evh_compute_homography: bad argument");
  if (n > c->kcap) return evh_fail(c, EVH_ERR_CAPACITY, "evh_compute_homography: too many rows");
  { int jr = evh_join_solve(c); if (jr) return jr; }
  forget_static(c);
  const int zero = 0;
  EVH_HIP(c, hipMemcpyAsync(c->orb.pts2, h_pts, sizeof(float) * 4 * (size_t)n, hipMemcpyHostToDevice, c->stream));
  EVH_HIP(c, hipMemcpyAsync(c->orb.npts2, &n, sizeof(int), hipMemcpyHostToDevice, c->stream));
  EVH_HIP(c, hipMemcpyAsync(c->orb.pstatus, &zero, sizeof(int), hipMemcpyHostToDevice, c->stream));
  return final_solve_one(c, h_Hsup, h_H, h_status);
}

int evh_pair_from_slots(evh_ctx* c, int cur_slot, int prev_slot, const double* h_Hsup, double* h_H, int* h_status) {
  if (!c || !h_H || !h_status) return evh_fail(c, EVH_ERR_INVALID, "evh_pair_from_slots: bad argument");
  int n = 0, st = 0;
  int rc = evh_match_static_from_slots(c, cur_slot, prev_slot, nullptr, 0, &n, &st);
  if (rc) return rc;
  if (st != EVH_PAIR_OK) { *h_status = st; memset(h_H, 0, 9 * sizeof(double)); return EVH_SUCCESS; }
  return final_solve_one(c, h_Hsup, h_H, h_status);   // the static rows are already resident in pair slot 0
}

}  // extern "C"
