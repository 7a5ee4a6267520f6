"""A second source of correspondences: points followed from frame to frame on the pixels.

The reference's known-issues.md names "H=None" as an open problem: a pair whose descriptor matching fails ("the 4 points can't be
found") repeats the previous matrix.  A frame pair with gradients but no corners -- defocus, motion blur, fog, a wall, low contrast
-- never gets a row from detect / describe / match.  Here such a pair gets its rows from evh_track_seeds (the best-conditioned
pixel of every cell) and evh_track_points (sparse pyramidal Lucas-Kanade, forward-backward checked), in the (ax, ay, bx, by)
layout every solver of this library takes, and recover_homography_dict solves them with the reference's running superposition
(evh_stream_scan).  Rows and flags stay on the device; the matrices, the statuses and the counts come back.
"""
import numpy as np

from . import runtime
from ._lib import PAIR_CAPACITY, PAIR_OK, TRACK_FLAGS
from .frames import DeviceLadder, FrameReader, check_ingest, entry_matrix
from .processing.video_processing import CHUNK_FRAMES

# The smaller eigenvalue of the mean structure tensor a seed and a tracked window must reach, in gray levels^2 per pixel^2.
# Measured on the crafted low-contrast family of tests/track_families.py (Gaussian-filtered noise, sigma 2 px, gray 100..120,
# 128 x 96, seeds 11..13; radius 2, cell 16, border 8): 35 of 35 cells give a seed at 0.5, 25..30 at 1.0, 1..9 at 2.0.
MIN_EIG = 0.5
MIN_ROWS = 4            # a homography takes four rows; fewer tracked rows leave the pair as the first pass left it


def _integer(name, value, lo, hi):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not lo <= value <= hi:
        raise ValueError("%s must be an integer in %d..%d" % (name, lo, hi))
    return int(value)


def _number(name, value, allow_none=False):
    if value is None and allow_none:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) or not np.isfinite(value) or value < 0:
        raise ValueError("%s must be a finite number, not negative" % name)
    return float(value)


def check_track_arguments(levels=3, radius=7, iters=20, cell=16, seed_radius=2, min_eig=MIN_EIG, fb_max=0.5, max_err=None):
    """The refusals of the drivers below, before a capture is opened or the device touched."""
    _integer("levels", levels, 1, 4)
    _integer("radius", radius, 1, 10)
    _integer("iters", iters, 1, 64)
    _integer("cell", cell, 8, 64)
    _integer("seed_radius", seed_radius, 1, 3)
    _number("min_eig", min_eig)
    _number("fb_max", fb_max, allow_none=True)
    if max_err is not None:
        _integer("max_err", max_err, 0, 255)


def seed_points(ctx, frames, cell=16, seed_radius=2, border=None, min_eig=MIN_EIG, pt_cap=None, size=None):
    """The seeds of every frame -> (pts f32[n,pt_cap,2], npts i32[n]) CUDA tensors.  frames: as Context.track_seeds takes them
    (size=(w, h) for packed I420 frames).  border: None = half a cell (at least seed_radius + 1), so that a tracked window finds
    room; pt_cap: None = one slot per cell."""
    check_track_arguments(cell=cell, seed_radius=seed_radius, min_eig=min_eig)
    planes = isinstance(frames, (tuple, list)) or frames.dim() == 2
    if planes:
        _, _, w, h = ctx._yuv420(frames, size, ctx.device)
    else:
        h, w = int(frames.shape[1]), int(frames.shape[2])
    border = max(int(cell) // 2, int(seed_radius) + 1) if border is None else int(border)
    if pt_cap is None:
        pt_cap = max(1, -(-max(w - 2 * border, 0) // int(cell)) * -(-max(h - 2 * border, 0) // int(cell)))
    method = ctx.track_seeds_yuv420 if planes else ctx.track_seeds
    kw = {"size": size} if planes else {}
    return method(frames, radius=int(seed_radius), cell=int(cell), border=border, min_eig=float(min_eig), pt_cap=int(pt_cap), **kw)


def _track_chunk(ctx, frames, size, mats, levels, radius, iters, cell, seed_radius, min_eig, fb_max, max_err, row_cap):
    """frames: (prev, cur) per pair, frame_step 2, as torch left them -> (rows f32[m,row_cap,4], counts i32[m], seeds i32[m],
    flags u8[m,pt_cap]) on the device; the seeds are those of each pair's current frame.  row_cap: None = one row per seed slot."""
    import torch
    planes = size is not None
    ctx.order_after_torch()                                  # the frames and the guesses were gathered by torch
    pts, npts = seed_points(ctx, frames[1::2], cell, seed_radius, None, min_eig, None, size)
    row_cap = int(pts.shape[1]) if row_cap is None else row_cap
    pt_cap = min(int(pts.shape[1]), row_cap)
    if pt_cap < pts.shape[1]:
        ctx.order_torch_after()
        pts = pts[:, :pt_cap].contiguous()
    m = pts.shape[0]
    rows = torch.zeros((m, row_cap, 4), dtype=torch.float32, device=pts.device)
    flags = torch.zeros((m, pt_cap), dtype=torch.uint8, device=pts.device)
    ctx.order_after_torch()
    method = ctx.track_points_yuv420 if planes else ctx.track_points
    kw = {"size": size} if planes else {}
    _, counts = method(frames, pts, npts, mats, levels=levels, radius=radius, iters=iters, min_eig=min_eig, fb_max=fb_max,
                       max_err=max_err, rows=rows, flags=flags, frame_step=2, **kw)
    return rows, counts, npts, flags


def track_rows(capture, resize_info, pair_maps=None, levels=3, radius=7, iters=20, cell=16, seed_radius=2, min_eig=MIN_EIG, fb_max=0.5,
               max_err=None, chunk_frames=CHUNK_FRAMES, ingest="auto"):
    """Every pair of consecutive frames of `capture` tracked on the frames resized to resize_info -> {frame_no: {"rows": f32[k,4]
    as (ax, ay, bx, by), a on frame frame_no, b on the frame before, "seeds": int, "flags": {name: count}}}.  pair_maps:
    {frame_no: 3x3 taking pixels of frame frame_no to pixels of the frame before} as registration.pair_maps returns it, the first
    guess of a pair (missing or not finite: the identity), or None."""
    import torch
    check_track_arguments(levels, radius, iters, cell, seed_radius, min_eig, fb_max, max_err)
    check_ingest(ingest)
    reader = FrameReader(capture, ingest)
    w, h = int(resize_info["w"]), int(resize_info["h"])
    chunk = runtime.chunk_frames_for(reader.first.nbytes, max(2, int(chunk_frames)))
    ctx = runtime.get_context(w, h, chunk, runtime.NFEATURES)
    dev = runtime.device()
    ladder = DeviceLadder(dev, chunk, reader.planes, (reader.w0, reader.h0), (w, h), gray3=True)
    out = {}
    for start, frames in reader.chunks(chunk, 1):
        frame_no, npairs = start + 1, len(frames) - 1
        _, small, size = ladder(ctx, torch.from_numpy(frames).to(dev))
        index = torch.tensor([j for k in range(npairs) for j in (k, k + 1)], dtype=torch.int64, device=dev)
        ctx.order_torch_after()                              # the ladder's frames, before torch gathers them
        guess = np.stack([_guess(pair_maps, frame_no + 1 + k) for k in range(npairs)])
        rows, counts, seeds, flags = _track_chunk(ctx, small[index], size, torch.from_numpy(guess).to(dev), levels, radius, iters, cell,
                                                  seed_radius, float(min_eig), fb_max, max_err, None)
        ctx.order_torch_after()
        rows_h, counts_h, seeds_h, flags_h = (t.cpu().numpy() for t in (rows, counts, seeds, flags))
        for k in range(npairs):
            out[frame_no + 1 + k] = {"rows": rows_h[k, :counts_h[k]].copy(), "seeds": int(seeds_h[k]),
                                     "flags": _histogram(flags_h[k], seeds_h[k])}
    return out


def _guess(pair_maps, frame_no):
    M = None if pair_maps is None else pair_maps.get(frame_no)
    M = entry_matrix(M)
    return (M if np.isfinite(M).all() else np.eye(3)).reshape(9)


def _histogram(flags, seeds):
    counts = np.bincount(flags[:min(int(seeds), len(flags))], minlength=len(TRACK_FLAGS))
    return {name: int(counts[i]) for i, name in enumerate(TRACK_FLAGS) if counts[i]}


def recover_homography_dict(capture, homography_dict, levels=3, radius=7, iters=20, cell=16, seed_radius=2, min_eig=MIN_EIG,
                            fb_max=0.5, max_err=None, nfeatures=runtime.NFEATURES, chunk_frames=CHUNK_FRAMES,
                            features_type_list=("ORB",), ingest="auto", none_H_processing=True):
    """-> (recovered_dict, report).  capture: the video of the first pass, opened again.  homography_dict: the first pass's result
    ({frame_no: {"H": 3x3}, ..., "resize_info"}, keys int or str); a first pass that could not finish may hand over
    {"resize_info": ...} alone.

    The capture is read chunk by chunk as moving.refine_homography_dict reads it (the same synchronous loop, ["ORB"] only,
    EVH_PAIR_CAPACITY raising as there).  Per chunk the batch entry get_homography_dict runs, then batch_static_rows; every pair
    whose front status or first-pass final status is not EVH_PAIR_OK gets the seeds of its current frame (Context.track_seeds) and
    their tracks into its previous frame (Context.track_points, both on the frames resized to resize_info).  The first guess of
    such a pair is the pair map of its own entry of homography_dict -- under none_H_processing that entry repeats the nearest
    earlier pair that had a matrix -- and the identity where there is none.  With at least four tracked rows these replace the
    pair's rows and its front status becomes EVH_PAIR_OK; then stream_scan runs over all pairs with its own carried state.  Pairs
    that were fine keep their own rows: their matrices up to the first recovered pair are the first pass's byte for byte.

    recovered_dict has the format and the none_H_processing rule of get_homography_dict.  report[frame_no] = {"first_status",
    "seeds", "tracked", "flags": {name: count}, "final_status"} for every pair that was tracked."""
    import torch
    from . import registration
    from .processing.utils import superposition_dict
    from .processing.video_processing import _feature_list, _pairs_into, resized_shape
    check_track_arguments(levels, radius, iters, cell, seed_radius, min_eig, fb_max, max_err)
    check_ingest(ingest)
    if isinstance(nfeatures, bool) or not isinstance(nfeatures, (int, np.integer)) or nfeatures < 1:
        raise ValueError("nfeatures must be an integer of at least 1")
    if isinstance(chunk_frames, bool) or not isinstance(chunk_frames, (int, np.integer)) or chunk_frames < 2:
        raise ValueError("chunk_frames must be an integer of at least 2")
    if _feature_list(features_type_list) != ["ORB"]:
        raise ValueError('features_type_list must be ["ORB"]: the second pass is built on the fused ORB path only')
    if not isinstance(homography_dict, dict) or "resize_info" not in homography_dict:
        raise ValueError("homography_dict must be the first pass's dictionary, with its resize_info")
    resize_info = homography_dict["resize_info"]
    per_frame = {int(k): v for k, v in homography_dict.items() if k != "resize_info"}
    guesses = registration.pair_maps(superposition_dict(per_frame)) if len(per_frame) > 1 else {}
    reader = FrameReader(capture, ingest)
    first, planes, w0, h0 = reader.first, reader.planes, reader.w0, reader.h0
    w, h = int(resize_info["w"]), int(resize_info["h"])
    if (w, h) != resized_shape((h0, w0), w):
        raise ValueError("resize_info %dx%d is not what frames of %dx%d resize to" % (w, h, w0, h0))
    method, size0 = ("stream_homography_batch_yuv420", ((w0, h0),)) if planes else ("stream_homography_batch", ())
    chunk = runtime.chunk_frames_for(first.nbytes, max(2, int(chunk_frames)))
    ctx = runtime.get_context(w, h, chunk, nfeatures)
    dev = runtime.device()
    ladder = DeviceLadder(dev, chunk, planes, (w0, h0), (w, h), gray3=True)
    H_dev = torch.zeros((chunk - 1, 9), dtype=torch.float64, device=dev)
    st_dev = torch.zeros(chunk - 1, dtype=torch.int32, device=dev)
    first_state = torch.zeros(18, dtype=torch.float64, device=dev)      # {H_sup, H_prev} of the first pass's solve, as it ran
    state = torch.zeros(18, dtype=torch.float64, device=dev)            # and of the recovered one
    recovered, report = {}, {}
    have_state = False
    for start, frames in reader.chunks(chunk, 1):            # consecutive chunks overlap by one frame
        frame_no, npairs = start + 1, len(frames) - 1        # frames[0] is frame `frame_no`, the newest frame already paired
        src = torch.from_numpy(frames).to(dev)
        getattr(ctx, method)(src, *size0, H_dev, st_dev, state_in=first_state if have_state else None,
                             state_out=first_state, nfeatures=nfeatures, resize_to=(w, h))
        rows, counts, st1 = ctx.batch_static_rows(0, npairs)
        cap = rows.shape[1]
        ctx.order_torch_after()
        st1_h, stf_h = st1.cpu().numpy(), st_dev[:npairs].cpu().numpy()
        if (st1_h == PAIR_CAPACITY).any() or (stf_h == PAIR_CAPACITY).any():
            raise RuntimeError("frames %d..%d: more tied key points than a frame slot holds (EVH_PAIR_CAPACITY); the re-run on "
                               "larger slots is not built for the second pass" % (frame_no, frame_no + npairs))
        lost = [k for k in range(npairs) if st1_h[k] != PAIR_OK or stf_h[k] != PAIR_OK]
        if lost:
            _, small, size = ladder(ctx, src)
            at = torch.tensor([j for k in lost for j in (k, k + 1)], dtype=torch.int64, device=dev)
            guess = torch.from_numpy(np.stack([_guess(guesses, frame_no + 1 + k) for k in lost])).to(dev)
            ctx.order_torch_after()                          # the ladder's frames, before torch gathers them
            t_rows, t_counts, seeds, flags = _track_chunk(ctx, small[at], size, guess, levels, radius, iters, cell, seed_radius,
                                                          float(min_eig), fb_max, max_err, cap)
            ctx.order_torch_after()
            which = torch.tensor(lost, dtype=torch.int64, device=dev)
            enough = t_counts >= MIN_ROWS
            rows[which[enough]] = t_rows[enough]
            counts[which[enough]] = t_counts[enough]
            st1[which[enough]] = PAIR_OK
            t_counts_h, seeds_h, flags_h = t_counts.cpu().numpy(), seeds.cpu().numpy(), flags.cpu().numpy()
        Hs, sts = ctx.stream_scan(rows, counts, st1, state_in=state if have_state else None, state_out=state)
        have_state = True
        sts_h = sts.cpu().numpy()
        if (sts_h == PAIR_CAPACITY).any():
            raise RuntimeError("frames %d..%d: EVH_PAIR_CAPACITY in the recovered solve" % (frame_no, frame_no + npairs))
        for i, k in enumerate(lost):
            report[frame_no + 1 + k] = {"first_status": int(st1_h[k] if st1_h[k] != PAIR_OK else stf_h[k]), "seeds": int(seeds_h[i]),
                                        "tracked": int(t_counts_h[i]), "flags": _histogram(flags_h[i], seeds_h[i]),
                                        "final_status": int(sts_h[k])}
        _pairs_into(recovered, frame_no, Hs.cpu().numpy().reshape(-1, 3, 3), sts_h, none_H_processing)
    recovered["resize_info"] = {"h": h, "w": w}
    return recovered, report
