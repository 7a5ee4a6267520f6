"""How good is each homography?  The motion-compensated residual of every pair of consecutive frames, computed on the GPU.

The library returns one matrix per frame; the reference's known-issues.md names a poorly obtained homography as its open problem
("Error": it distorts every recalculated coordinate; "N/A coordinates": matches clinging to moving objects cause it, and the
authors "consider applying video motion segmentation").  The stabilisation literature measures exactly this: warp frame k-1 onto
frame k through the estimated motion, difference the two, report the PSNR and its mean over the video (the inter-frame
transformation fidelity, ITF); the same difference, thresholded, is the moving-object mask.

`pair_maps` forms the matrix that registers a pair, `registration_report` the per-pair figures and the two means,
`residual_frames` the difference pictures or masks.  The sampling, differencing and summing is one fused operator,
evh_pair_residual (include/evhip.h states its arithmetic): no warped frame is ever stored.

`refine_pair_maps` improves each pair's matrix on the pixels (evh_pair_refine); `anchor_superposition` aligns every frame against
the mosaic of the frames before it (evh_canvas_refine), which is what keeps a long chain of pair matrices from drifting.
"""
import math

import numpy as np

from . import runtime
from .frames import DeviceLadder, FrameReader, check_ingest, entry_matrix

STAT_NAMES = ("covered", "sad", "ssd", "sad_unregistered", "ssd_unregistered", "moving")


def _pair_map(S_prev, S_cur):
    nan = np.full((3, 3), np.nan)
    if not (np.isfinite(S_prev).all() and np.isfinite(S_cur).all()):
        return nan
    with np.errstate(all="ignore"):
        if np.linalg.det(S_prev) == 0 or np.linalg.det(S_cur) == 0:
            return nan
        try:
            M = np.linalg.solve(S_prev, S_cur)
        except np.linalg.LinAlgError:
            return nan
    return M if np.isfinite(M).all() else nan


def pair_maps(superposition_homography_dict):
    """{frame_no: superposed S} -> {frame_no: f64[3,3] M_k}, M_k = S_{k-1}^-1 . S_k, for every entry but the first, taking
    consecutive entries in the dictionary's order; float64 on the host, np.linalg.solve(S_{k-1}, S_k).  NaN where either
    matrix is None, not finite or singular (such a pair then covers nothing and scores nothing).

    M_k takes pixels of frame k to pixels of frame k-1, which is what evh_pair_residual samples through.  It is NOT the
    per-frame H_k of dict_with_homography_matrix.json: the reference composes S_k = H_k . S_{k-1} (normalised by [2][2]) and
    S_k takes frame k's pixels to the fixed plane, so the pixel-to-pixel map of a pair is S_{k-1}^-1 . S_k.  On the reference's
    test_video.mp4 with its recorded dictionary (frames subsampled to 400x224), the registered sum of squared differences lies
    below the unregistered one on 120 of 120 pairs with M_k, on 56 of 120 with H_k itself and on 2 of 120 with H_k^-1."""
    entries = [(k, entry_matrix(v)) for k, v in superposition_homography_dict.items() if k != "resize_info"]
    return {k1: _pair_map(S0, S1) for (_, S0), (k1, S1) in zip(entries, entries[1:])}


def psnr(covered, ssd):
    """10 log10(255^2 covered / ssd): inf for ssd == 0, None for a pair without a covered pixel."""
    if covered <= 0:
        return None
    if ssd == 0:
        return math.inf
    return 10.0 * math.log10(65025.0 * covered / ssd)


def report_from_stats(stats_by_frame):
    """{frame_no: (covered, sad, ssd, sad0, ssd0, moving)} (evh_pair_residual's six sums) -> the report registration_report
    returns.  worst: the frame numbers in ascending order of psnr - psnr_unregistered, pairs without a covered pixel (no
    score at all) first; a pair whose two PSNRs are both inf counts as a gain of 0; equal gains keep the dictionary's order."""
    frames, finite, finite0, order = {}, [], [], []
    for pos, (no, s) in enumerate(stats_by_frame.items()):
        s = [int(v) for v in s]
        e = dict(zip(STAT_NAMES, s))
        e["psnr"], e["psnr_unregistered"] = psnr(s[0], s[2]), psnr(s[0], s[4])
        frames[no] = e
        if e["psnr"] is None:
            gain = -math.inf
        else:
            if math.isfinite(e["psnr"]):
                finite.append(e["psnr"])
            if math.isfinite(e["psnr_unregistered"]):
                finite0.append(e["psnr_unregistered"])
            both_inf = math.isinf(e["psnr"]) and math.isinf(e["psnr_unregistered"])
            gain = 0.0 if both_inf else e["psnr"] - e["psnr_unregistered"]
        order.append((gain, pos, no))
    mean = lambda v: float(np.mean(v)) if v else None
    return {"frames": frames, "itf": mean(finite), "itf_unregistered": mean(finite0), "worst": [no for _, _, no in sorted(order)]}


def _arguments(superposition_homography_dict, resize_info, threshold, chunk_frames, ingest, kind):
    """The refusals of both drivers, before the capture is opened or the device touched -> (entries, maps, w, h, threshold, chunk)"""
    from ._lib import RESIDUAL_KINDS
    check_ingest(ingest)
    if kind not in RESIDUAL_KINDS:
        raise ValueError("kind must be 'abs' or 'mask'")
    if isinstance(threshold, bool) or int(threshold) != threshold or not 0 <= int(threshold) <= 255:
        raise ValueError("threshold must be an integer in 0..255")
    if isinstance(chunk_frames, bool) or int(chunk_frames) != chunk_frames or int(chunk_frames) < 1:
        raise ValueError("chunk_frames must be an integer of at least 1")
    w, h = int(resize_info["w"]), int(resize_info["h"])
    if w < 1 or h < 1:
        raise ValueError("resize_info must hold a positive w and h")
    keys = [k for k in superposition_homography_dict if k != "resize_info"]
    return keys, pair_maps(superposition_homography_dict), w, h, int(threshold), max(2, int(chunk_frames))


def _residuals(capture, keys, maps, w, h, threshold, chunk, ingest, kind, pictures):
    """Generator of (frame_no, six ints, picture or None) per pair.  The i-th frame read from `capture` goes with the i-th entry
    of the dictionary; frames are read `chunk` at a time (frames.FrameReader) and taken to w x h as the heat-map pictures' are
    (frames.DeviceLadder); a chunk's last frame is the next chunk's first, so that every pair of consecutive frames lies inside one chunk."""
    import torch
    if len(keys) < 2:
        return
    reader = FrameReader(capture, ingest)
    first = reader.first
    if not reader.planes and (first.ndim not in (2, 3) or (first.ndim == 3 and first.shape[2] != 3)):
        raise ValueError("frames must be BGR [h,w,3] or gray [h,w]")
    ctx = runtime.get_context(64, 64)             # the entries used here work on caller buffers of any size
    dev = runtime.device()
    chunk = max(2, min(chunk, len(keys), runtime.STAGING_BYTES_PER_BUFFER // max(first.nbytes, 1)))      # the host chunk stays bounded
    ladder = DeviceLadder(dev, chunk, reader.planes, (reader.w0, reader.h0), (w, h), bgr=True, gray3=True)
    stats = torch.empty((chunk - 1, 6), dtype=torch.int64, device=dev)
    out = torch.empty((chunk - 1, h, w), dtype=torch.uint8, device=dev) if pictures else None
    for done, frames in reader.chunks(chunk, 1, len(keys)):        # frames[0] is frame `done` of the dictionary's order
        n = len(frames)
        _, src, _ = ladder(ctx, torch.from_numpy(frames).to(dev))
        nos = keys[done + 1:done + n]
        mats = torch.from_numpy(np.stack([maps[k] for k in nos]).reshape(n - 1, 9)).to(dev)
        ctx.pair_residual(src, mats, stats=stats[:n - 1], out=out[:n - 1] if pictures else None, threshold=threshold, kind=kind)
        ctx.order_torch_after()
        sums = stats[:n - 1].cpu().numpy()
        pics = out[:n - 1].cpu().numpy() if pictures else None
        for k, no in enumerate(nos):
            yield no, tuple(int(v) for v in sums[k]), (pics[k] if pictures else None)


def registration_report(capture, superposition_homography_dict, resize_info, threshold=16, chunk_frames=32, ingest="auto"):
    """-> {"frames": {frame_no: {covered, sad, ssd, sad_unregistered, ssd_unregistered, moving, psnr, psnr_unregistered}},
    "itf": mean of the finite psnr, "itf_unregistered": mean of the finite psnr_unregistered, "worst": frame numbers, the least
    gain first}.  Entry frame_no scores the pair (frame before it in the dictionary's order, frame_no) under pair_maps' matrix:
    over the pixels of the resized frame the matrix keeps inside the previous frame (covered), the sums of |difference| and
    difference^2 in gray with the previous frame registered (sad, ssd) and as it is (*_unregistered), and the pixels whose
    registered difference exceeds threshold (moving).  psnr = 10 log10(65025 covered / ssd), inf for ssd == 0, None for
    covered == 0.  The i-th frame read from `capture` goes with the i-th entry of the dictionary, as in heatmap.heatmap_frames;
    it ends when either runs out.  chunk_frames (at least 2 are taken) frames are on the device at a time."""
    keys, maps, w, h, threshold, chunk = _arguments(superposition_homography_dict, resize_info, threshold, chunk_frames, ingest, "abs")
    return report_from_stats({no: s for no, s, _ in _residuals(capture, keys, maps, w, h, threshold, chunk, ingest, "abs", False)})


def residual_frames(capture, superposition_homography_dict, resize_info, threshold=16, chunk_frames=32, ingest="auto", kind="abs"):
    """Generator of (frame_no, uint8 ndarray [h,w]) per pair of registration_report: kind "abs": the registered difference in
    gray, "mask": 255 where it exceeds threshold (the moving objects), 0 elsewhere and where the pair is not covered."""
    keys, maps, w, h, threshold, chunk = _arguments(superposition_homography_dict, resize_info, threshold, chunk_frames, ingest, kind)
    return ((no, pic) for no, _, pic in _residuals(capture, keys, maps, w, h, threshold, chunk, ingest, kind, True))


# ---- direct alignment: the matrices refined on the pixels ----------------------------------------------------------------------------
def _whole(value, lo, hi, name):
    if isinstance(value, bool) or int(value) != value or not lo <= int(value) <= hi:
        raise ValueError("%s must be an integer in %d..%d" % (name, lo, hi))
    return int(value)


def _refine_arguments(superposition_homography_dict, resize_info, iters, levels, clip, fill_missing, chunk_frames, ingest):
    """The refusals of refine_pair_maps, before the capture is opened or the device touched"""
    from ._lib import REFINE_MAX_ITERS, REFINE_MAX_SIZE
    check_ingest(ingest)
    iters, levels, clip = _whole(iters, 0, REFINE_MAX_ITERS, "iters"), _whole(levels, 1, 4, "levels"), _whole(clip, 0, 255, "clip")
    if not isinstance(fill_missing, (bool, np.bool_)):
        raise ValueError("fill_missing must be True or False")
    if isinstance(chunk_frames, bool) or int(chunk_frames) != chunk_frames or int(chunk_frames) < 1:
        raise ValueError("chunk_frames must be an integer of at least 1")
    w, h = int(resize_info["w"]), int(resize_info["h"])
    if not (1 <= w <= REFINE_MAX_SIZE and 1 <= h <= REFINE_MAX_SIZE):
        raise ValueError("resize_info must hold a w and h in 1..%d" % REFINE_MAX_SIZE)
    keys = [k for k in superposition_homography_dict if k != "resize_info"]
    return keys, pair_maps(superposition_homography_dict), w, h, iters, levels, clip, bool(fill_missing), max(2, int(chunk_frames))


def level_map(w, h, lw, lh):
    """S: pixel of a level of lw x lh -> pixel of the full frame of w x h (pixel centres: f x + (f - 1) / 2, f the true ratio)"""
    fx, fy = w / lw, h / lh
    return np.array([[fx, 0, (fx - 1) / 2], [0, fy, (fy - 1) / 2], [0, 0, 1]], np.float64)


def _refine_chunk(ctx, pyramid, mats, iters, clip):
    """pyramid: the chunk's frames coarse to fine, [(frames [n,lh,lw,3], S)], the last being the full size with S = I; mats
    f64[npairs,3,3] on the host -> (mats refined, info rows int64[npairs,8] of the full size, accepted int64[npairs,levels]).
    A level hands a map on only where it accepted a step: the bytes of an untouched map survive the way down and up."""
    import torch
    from ._lib import REFINE_INFO
    dev, mats = pyramid[0][0].device, np.array(mats, np.float64).reshape(-1, 3, 3)
    accepted = np.zeros((len(mats), len(pyramid)), np.int64)
    for l, (frames, S) in enumerate(pyramid):
        with np.errstate(all="ignore"):
            start = np.stack([np.linalg.solve(S, np.dot(M, S)) if np.isfinite(M).all() else M for M in mats]) if S is not None else mats
        out, info = ctx.pair_refine(frames, torch.from_numpy(start.reshape(-1, 9).copy()).to(dev), iters=iters, clip=clip)
        ctx.order_torch_after()
        out, info = out.cpu().numpy().reshape(-1, 3, 3), info.cpu().numpy()
        accepted[:, l] = info[:, REFINE_INFO.index("accepted")]
        for p in np.nonzero(accepted[:, l])[0]:
            T = out[p] if S is None else np.dot(np.dot(S, out[p]), np.linalg.inv(S))
            mats[p] = T / T[2, 2]
    return mats, info, accepted


def refine_pair_maps(capture, superposition_homography_dict, resize_info, iters=8, levels=1, clip=255, fill_missing=False,
                     chunk_frames=32, ingest="auto"):
    """pair_maps' matrices refined on the pixels of the video (evh_pair_refine: damped Gauss-Newton steps on the photometric
    residual; a matrix is only ever replaced by one that scores better).  Frames are read and laid out as registration_report
    does.  levels (1..4): coarse to fine, level l on the chunk's frames downsized by 2^l with the area resize, the map taken
    there and back with level_map's S (M_l = S^-1 M S); iters steps per level; clip: pixels whose residual exceeds it stay out
    of the normal equations (255: none).  fill_missing: a pair whose map is NaN (matching failed) starts from the previous
    pair's refined map, the first pair from the identity -- the reference repeats the previous H there -- and keeps what it
    reaches if that registers anything; without it such a pair stays NaN.
    -> ({frame_no: f64[3,3] M'}, {frame_no: {status, evals, accepted, covered_in, ssd_in, covered_out, ssd_out, n_in (the
    full-size level's row of d_info), accepted_by_level (coarse to fine), filled}})."""
    import torch
    from ._lib import REFINE_INFO
    keys, maps, w, h, iters, levels, clip, fill_missing, chunk = _refine_arguments(
        superposition_homography_dict, resize_info, iters, levels, clip, fill_missing, chunk_frames, ingest)
    refined, infos = {}, {}
    if len(keys) < 2:
        return refined, infos
    reader = FrameReader(capture, ingest)
    first = reader.first
    if not reader.planes and (first.ndim not in (2, 3) or (first.ndim == 3 and first.shape[2] != 3)):
        raise ValueError("frames must be BGR [h,w,3] or gray [h,w]")
    ctx = runtime.get_context(64, 64)
    dev = runtime.device()
    chunk = max(2, min(chunk, len(keys), runtime.STAGING_BYTES_PER_BUFFER // max(first.nbytes, 1)))
    ladder = DeviceLadder(dev, chunk, reader.planes, (reader.w0, reader.h0), (w, h), bgr=True, gray3=True)
    sizes = [(max(1, w >> l), max(1, h >> l)) for l in range(levels - 1, 0, -1)]
    small = [torch.empty((chunk, lh, lw, 3), dtype=torch.uint8, device=dev) for lw, lh in sizes]
    last = np.eye(3)                                           # what a missing pair starts from
    for done, frames in reader.chunks(chunk, 1, len(keys)):
        n = len(frames)
        _, src, _ = ladder(ctx, torch.from_numpy(frames).to(dev))
        src = src.contiguous()
        pyramid = []
        for buf, (lw, lh) in zip(small, sizes):
            ctx.resize_area(src, buf[:n])
            pyramid.append((buf[:n], level_map(w, h, lw, lh)))
        pyramid.append((src, None))
        nos = keys[done + 1:done + n]
        mats, info, accepted = _refine_chunk(ctx, pyramid, np.stack([maps[k] for k in nos]), iters, clip)
        for p, no in enumerate(nos):
            filled = False
            if fill_missing and not np.isfinite(maps[no]).all():
                one = [(f[p:p + 2], S) for f, S in pyramid]
                m1, i1, a1 = _refine_chunk(ctx, one, last[None], iters, clip)
                if i1[0, REFINE_INFO.index("covered_out")] > 0:
                    mats[p], info[p], accepted[p], filled = m1[0], i1[0], a1[0], True
            if np.isfinite(mats[p]).all():
                last = mats[p]
            refined[no] = mats[p].copy()
            infos[no] = dict(zip(REFINE_INFO, (int(v) for v in info[p])), accepted_by_level=[int(v) for v in accepted[p]], filled=filled)
    return refined, infos


def compose_refined(superposition_homography_dict, refined_maps):
    """The refined maps recomposed into the reference's two dictionaries, float64 on the host: S'_first = the first entry's S
    (the identity in the reference's dictionaries), S'_k = S'_{k-1} . M'_k / [2][2], H'_k = S'_k . S'_{k-1}^-1 / [2][2]; a
    pair whose map is not finite gets H = None and keeps the running S', as the reference's superposition does.
    -> ({frame_no: {"H": 3x3 list or None}}, {frame_no: S' f64[3,3]})"""
    keys = [k for k in superposition_homography_dict if k != "resize_info"]
    hd, sup = {}, {}
    if not keys:
        return hd, sup
    S = entry_matrix(superposition_homography_dict[keys[0]])
    S = S if np.isfinite(S).all() else np.eye(3)
    sup[keys[0]] = S
    for no in keys[1:]:
        M = refined_maps.get(no)
        H = None
        if M is not None and np.isfinite(M).all():
            T = np.dot(S, np.asarray(M, np.float64).reshape(3, 3))
            T = T / T[2, 2]
            with np.errstate(all="ignore"):
                H = np.dot(T, np.linalg.inv(S))
                H = H / H[2, 2]
            if np.isfinite(T).all() and np.isfinite(H).all():
                S = T
            else:
                H = None
        hd[no] = {"H": None if H is None else H.tolist()}
        sup[no] = S
    return hd, sup


def refined_homography_dict(capture_factory, superposition_homography_dict, resize_info, iters=8, levels=1, clip=255,
                            fill_missing=False, threshold=16, chunk_frames=32, ingest="auto"):
    """refine_pair_maps, its maps recomposed (compose_refined) into a dictionary in the reference's format, and the score of
    both.  capture_factory() opens the video; it is called three times (the refinement and the two reports read it once each).
    -> {"homography": {frame_no: {"H": ...}}, "superposition": {frame_no: S'}, "info": refine_pair_maps' rows,
        "report_before": registration_report of the dictionary handed in, "report_after": of the refined one}"""
    _refine_arguments(superposition_homography_dict, resize_info, iters, levels, clip, fill_missing, chunk_frames, ingest)
    _arguments(superposition_homography_dict, resize_info, threshold, chunk_frames, ingest, "abs")
    maps, info = refine_pair_maps(capture_factory(), superposition_homography_dict, resize_info, iters, levels, clip, fill_missing,
                                  chunk_frames, ingest)
    hd, sup = compose_refined(superposition_homography_dict, maps)
    before = registration_report(capture_factory(), superposition_homography_dict, resize_info, threshold, chunk_frames, ingest)
    after = registration_report(capture_factory(), sup, resize_info, threshold, chunk_frames, ingest)
    return {"homography": hd, "superposition": sup, "info": info, "report_before": before, "report_after": after}


# ---- frame-to-mosaic registration: every frame aligned against what the plane already holds -----------------------------------------
def _anchor_arguments(superposition_homography_dict, resize_info, iters, clip, group, blend, feather_px, min_overlap, margin,
                      chunk_frames, ingest):
    """The refusals of anchor_superposition, before the capture is opened or the device touched"""
    from ._lib import BLEND_MODES, REFINE_MAX_ITERS, REFINE_MAX_SIZE
    from .blend import MAX_FEATHER_PX
    check_ingest(ingest)
    iters, clip = _whole(iters, 0, REFINE_MAX_ITERS, "iters"), _whole(clip, 0, 255, "clip")
    group, margin = _whole(group, 1, 65535, "group"), _whole(margin, 0, 4096, "margin")
    if blend not in BLEND_MODES:
        raise ValueError("blend must be 'feather' or 'seam'")
    if isinstance(feather_px, bool) or not isinstance(feather_px, (int, float)) or not 0 <= feather_px <= MAX_FEATHER_PX:
        raise ValueError("feather_px must lie in 0..%g" % MAX_FEATHER_PX)
    if isinstance(min_overlap, bool) or not isinstance(min_overlap, (int, float)) or not 0 <= min_overlap <= 1:
        raise ValueError("min_overlap must lie in 0..1")
    if isinstance(chunk_frames, bool) or int(chunk_frames) != chunk_frames or int(chunk_frames) < 1:
        raise ValueError("chunk_frames must be an integer of at least 1")
    w, h = int(resize_info["w"]), int(resize_info["h"])
    if not (1 <= w <= REFINE_MAX_SIZE and 1 <= h <= REFINE_MAX_SIZE):
        raise ValueError("resize_info must hold a w and h in 1..%d" % REFINE_MAX_SIZE)
    keys = [k for k in superposition_homography_dict if k != "resize_info"]
    chunk = max(group, int(chunk_frames) // group * group)              # a group never straddles two chunks
    return keys, w, h, iters, clip, group, int(round(float(feather_px) * 32)), float(min_overlap), margin, chunk


def _normalised(M):
    with np.errstate(all="ignore"):
        return M / M[2, 2]


def anchor_groups(S, T, w, h, group, min_overlap, refine, paint):
    """The loop of anchor_superposition on the host, float64.  S: the frames' matrices f64[3,3] in order (NaN = missing), frame
    pixel -> plane point; T: plane point -> canvas pixel.  refine(first, start f64[n,3,3]) -> (mats f64[n,3,3], info rows
    int[n,8]) aligns frames first .. first+n-1 against the canvas; paint(first, mats) paints them into it.  D, the running
    correction, starts as the identity.  Per group of `group` frames: frame k starts at M_k = T D S_k / [2][2]; the first group is
    taken as it stands; a later frame keeps refine's matrix when its status is REFINED and covered_in >= min_overlap w h, else
    its start; then D is chosen so that T D S_last = M'_last (the group's last frame with a matrix) and the group is painted.
    S'_k = T^-1 M'_k / [2][2]; a frame without a matrix repeats the running S'.
    -> ([S'_k], [info dict: d_info's row by name, used, overlap])"""
    from ._lib import REFINE_INFO, REFINE_REFINED, REFINE_UNCHANGED
    T = np.asarray(T, np.float64).reshape(3, 3)
    Tinv = np.linalg.inv(T)
    nan = np.full((3, 3), np.nan)
    D, running = np.eye(3), None
    out, infos = [], []
    for first in range(0, len(S), group):
        Sg = [np.asarray(m, np.float64).reshape(3, 3) for m in S[first:first + group]]
        ok = [bool(np.isfinite(m).all()) for m in Sg]
        start = np.stack([_normalised(np.dot(np.dot(T, D), m)) if good else nan for m, good in zip(Sg, ok)])
        kept = start.copy()
        rows = np.zeros((len(Sg), len(REFINE_INFO)), np.int64)
        rows[:, 0] = REFINE_UNCHANGED
        if first > 0:
            mats, rows = refine(first, start)
            mats, rows = np.asarray(mats, np.float64).reshape(-1, 3, 3), np.asarray(rows)
        for p in range(len(Sg)):
            info = dict(zip(REFINE_INFO, (int(v) for v in rows[p])))
            info["used"] = bool(first > 0 and info["status"] == REFINE_REFINED and info["covered_in"] >= min_overlap * w * h
                                and np.isfinite(mats[p]).all())
            info["overlap"] = info["covered_in"] / float(w * h)
            if info["used"]:
                kept[p] = mats[p]
            infos.append(info)
        have = [p for p in range(len(Sg)) if ok[p] and np.isfinite(kept[p]).all()]
        if have:
            with np.errstate(all="ignore"):
                try:
                    Dn = _normalised(np.dot(np.dot(Tinv, kept[have[-1]]), np.linalg.inv(Sg[have[-1]])))
                except np.linalg.LinAlgError:
                    Dn = nan
            if np.isfinite(Dn).all():
                D = Dn
        for p in range(len(Sg)):
            if ok[p] and np.isfinite(kept[p]).all():
                running = _normalised(np.dot(Tinv, kept[p]))
            out.append(nan if running is None else running)
        paint(first, kept)
    return out, infos


def anchor_superposition(capture, superposition_homography_dict, resize_info, iters=8, clip=255, group=1, blend="feather",
                         feather_px=32, min_overlap=0.25, margin=32, chunk_frames=32, ingest="auto"):
    """Frame-to-mosaic registration: every frame aligned against the blended picture of the frames before it
    (evh_canvas_refine), so that ground the camera comes back to pulls the chain of pair matrices into place again.  The canvas
    is stabilization.fixed_plane_bounds of the dictionary, `margin` pixels wider on every side; frames are read and taken to the
    working size as registration_report does; the loop is anchor_groups' (group = 1: strictly frame by frame); a group is painted
    with evh_blend_fixed_plane (blend, feather_px as in blend.blended_mosaic, no gains) and aligned against that picture where a
    frame has been painted.  iters = 0 scores the dictionary against its own mosaic and changes nothing.  The i-th frame read
    goes with the i-th entry of the dictionary; a capture that ends before the dictionary does is a ValueError.
    -> ({frame_no: S'_k f64[3,3]}, {frame_no: {status, evals, accepted, covered_in, ssd_in, covered_out, ssd_out, n_in, used,
    overlap = covered_in / (w h)}})."""
    import torch
    keys, w, h, iters, clip, group, feather, min_overlap, margin, chunk = _anchor_arguments(
        superposition_homography_dict, resize_info, iters, clip, group, blend, feather_px, min_overlap, margin, chunk_frames, ingest)
    if not keys:
        return {}, {}
    from .blend import CanvasPainter
    from .stabilization import fixed_plane_bounds
    ox, oy, dw, dh = fixed_plane_bounds(superposition_homography_dict, resize_info)
    ox, oy, dw, dh = ox - margin, oy - margin, dw + 2 * margin, dh + 2 * margin
    T = np.array([[1, 0, -ox], [0, 1, -oy], [0, 0, 1]], np.float64)
    S = [entry_matrix(superposition_homography_dict[k]) for k in keys]
    reader = FrameReader(capture, ingest)
    first = reader.first
    if not reader.planes and (first.ndim not in (2, 3) or (first.ndim == 3 and first.shape[2] != 3)):
        raise ValueError("frames must be BGR [h,w,3] or gray [h,w]")
    ctx = runtime.get_context(64, 64)
    dev = runtime.device()
    chunk = max(group, min(chunk, runtime.STAGING_BYTES_PER_BUFFER // max(first.nbytes, 1)) // group * group)
    ladder = DeviceLadder(dev, chunk, reader.planes, (reader.w0, reader.h0), (w, h), bgr=True, gray3=True)
    painter = CanvasPainter(dev, dw, dh, blend, feather)
    chunks = reader.chunks(chunk, 0, len(keys))
    held = {"start": 0, "src": None}

    def frames_of(first_no, n):
        """frames first_no .. first_no+n-1 on the device; groups come in order and never straddle two chunks"""
        while held["src"] is None or first_no >= held["start"] + held["src"].shape[0]:
            start, frames = next(chunks)
            held["start"], held["src"] = start, ladder(ctx, torch.from_numpy(frames).to(dev))[1].contiguous()
        at = first_no - held["start"]
        return held["src"][at:at + n]

    def refine(first_no, start):
        src = frames_of(first_no, len(start))
        n = src.shape[0]
        out, info = ctx.canvas_refine(src, painter.picture, torch.from_numpy(start[:n].reshape(-1, 9).copy()).to(dev),
                                      count=painter.cover, min_cover=1, iters=iters, clip=clip)
        ctx.order_torch_after()
        return out.cpu().numpy().reshape(-1, 3, 3), info.cpu().numpy()

    def paint(first_no, mats):
        src = frames_of(first_no, len(mats))
        painter.paint(ctx, src, torch.from_numpy(mats[:src.shape[0]].reshape(-1, 9).copy()).to(dev))

    sup, infos = {}, {}
    try:
        out, rows = anchor_groups(S, T, w, h, group, min_overlap, refine, paint)
    except StopIteration:
        raise ValueError("the capture holds fewer frames than the dictionary")
    for k, Sk, info in zip(keys, out, rows):
        sup[k], infos[k] = Sk, info
    return sup, infos


def anchored_homography_dict(capture_factory, superposition_homography_dict, resize_info, iters=8, clip=255, group=1, blend="feather",
                             feather_px=32, min_overlap=0.25, margin=32, threshold=16, chunk_frames=32, ingest="auto"):
    """anchor_superposition, its matrices turned into a dictionary in the reference's format, and the score of both.
    capture_factory() opens the video; it is called three times.  H'_k = S'_k . S'_{k-1}^-1 / [2][2], None where that is not finite.
    -> {"homography": {frame_no: {"H": ...}} for every entry but the first, "superposition": {frame_no: S'}, "info":
        anchor_superposition's rows, "report_before" / "report_after": registration_report of the dictionary handed in and of the
        anchored one, "canvas_score_before" / "canvas_score_after": the sums over the frames of ssd_in / covered_in and of
        ssd_out / covered_out (frames that cover nothing of the canvas add nothing)}"""
    _anchor_arguments(superposition_homography_dict, resize_info, iters, clip, group, blend, feather_px, min_overlap, margin, chunk_frames,
                      ingest)
    _arguments(superposition_homography_dict, resize_info, threshold, chunk_frames, ingest, "abs")
    sup, info = anchor_superposition(capture_factory(), superposition_homography_dict, resize_info, iters, clip, group, blend, feather_px,
                                     min_overlap, margin, chunk_frames, ingest)
    keys = list(sup)
    hd = {}
    for k0, k1 in zip(keys, keys[1:]):
        H = None
        with np.errstate(all="ignore"):
            try:
                H = _normalised(np.dot(sup[k1], np.linalg.inv(sup[k0])))
            except np.linalg.LinAlgError:
                H = None
        hd[k1] = {"H": H.tolist() if H is not None and np.isfinite(H).all() else None}
    before = registration_report(capture_factory(), superposition_homography_dict, resize_info, threshold, chunk_frames, ingest)
    after = registration_report(capture_factory(), sup, resize_info, threshold, chunk_frames, ingest)
    score = lambda a, b: float(sum(e[a] / e[b] for e in info.values() if e[b] > 0))
    return {"homography": hd, "superposition": sup, "info": info, "report_before": before, "report_after": after,
            "canvas_score_before": score("ssd_in", "covered_in"), "canvas_score_after": score("ssd_out", "covered_out")}
