"""numpy restatement of evh_rows_moving_filter (include/evhip.h), built on warp_checks.warp_frame, which gives a frame's samples
and coverage on the whole canvas exactly as evh_warp_fixed_plane states them, and plate_checks.gray.

    hit_map(frame, M, plate, count, origin, min_cover, threshold)  -> bool[dh,dw]: the pixels that are hits for this frame
    canvas_points(xy, M, row_scale)                                -> (cx i64[n], cy i64[n], usable bool[n])
    moving_points(xy, M, hits, origin, radius, min_hits, row_scale) -> bool[n]
    rows_filter(frames, mats, plate, count, origin, rows, counts, status1, out_rows, out_counts, moving, flags, ...)
                                                                   -> the four outputs as the entry leaves them (copies)

Every operation on coordinates is one IEEE float64 operation on arrays, in the order the header states.
"""
import numpy as np

import plate_checks as P
import warp_checks as W

PAIR_OK = 0
LIMIT = float(1 << 30)


def hit_map(frame, M, plate, count, origin, min_cover, threshold):
    plate = np.asarray(plate)
    dh, dw = plate.shape[:2]
    val, cov = W.warp_frame(frame, M, dw, dh, origin)
    return cov & (np.asarray(count) >= min_cover) & (np.abs(P.gray(val) - P.gray(plate)) > threshold)


def canvas_points(xy, M, row_scale=(1.0, 1.0)):
    m = np.asarray(M, np.float64).reshape(9)
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    with np.errstate(all="ignore"):
        px = xy[:, 0].astype(np.float64) * np.float64(row_scale[0])
        py = xy[:, 1].astype(np.float64) * np.float64(row_scale[1])
        tx = (m[0] * px + m[1] * py) + m[2]
        ty = (m[3] * px + m[4] * py) + m[5]
        tw = (m[6] * px + m[7] * py) + m[8]
        cx, cy = np.rint(tx / tw), np.rint(ty / tw)
        usable = (np.abs(cx) <= LIMIT) & (np.abs(cy) <= LIMIT)                  # NaN fails
    return np.where(usable, cx, 0).astype(np.int64), np.where(usable, cy, 0).astype(np.int64), usable


def moving_points(xy, M, hits, origin, radius, min_hits, row_scale=(1.0, 1.0)):
    dh, dw = hits.shape
    cx, cy, usable = canvas_points(xy, M, row_scale)
    total = np.zeros(len(cx), np.int64)
    for j in range(-radius, radius + 1):
        for i in range(-radius, radius + 1):
            X, Y = cx - int(origin[0]) + i, cy - int(origin[1]) + j
            inside = usable & (X >= 0) & (X < dw) & (Y >= 0) & (Y < dh)
            total += inside & hits[np.where(inside, Y, 0), np.where(inside, X, 0)]
    return total >= min_hits


def rows_filter(frames, mats, plate, count, origin, rows, counts, status1, out_rows, out_counts, moving=None, flags=None, *,
                threshold=16, min_cover=1, radius=1, min_hits=1, row_scale=(1.0, 1.0), frame_step=1, min_keep=8):
    """frames u8[n,sh,sw(,3)], mats f64[n,9]; rows f32[npairs,cap,4]; the outputs are taken as they stand before the call."""
    mats = np.asarray(mats, np.float64).reshape(-1, 9)
    rows = np.ascontiguousarray(rows, np.float32)
    npairs, cap = rows.shape[:2]
    out_rows = np.array(out_rows, np.float32).reshape(npairs, cap, 4)
    out_counts = np.array(out_counts, np.int32)
    moving = None if moving is None else np.array(moving, np.int32)
    flags = None if flags is None else np.array(flags, np.uint8).reshape(npairs, cap)
    bits, out_bits = rows.view(np.uint32), out_rows.view(np.uint32)
    maps = {}

    def hits_of(f):
        if f not in maps:
            maps[f] = hit_map(frames[f], mats[f], plate, count, origin, min_cover, threshold)
        return maps[f]

    for p in range(npairs):
        n = min(max(int(counts[p]), 0), cap)
        if status1[p] != PAIR_OK or n == 0:
            out_counts[p] = counts[p]
            if moving is not None:
                moving[p] = 0
            continue
        fp, fc = p * frame_step, p * frame_step + 1
        a = moving_points(rows[p, :n, 0:2], mats[fc], hits_of(fc), origin, radius, min_hits, row_scale)
        b = moving_points(rows[p, :n, 2:4], mats[fp], hits_of(fp), origin, radius, min_hits, row_scale)
        gone = a | b
        if flags is not None:
            flags[p, :n] = a.astype(np.uint8) | (b.astype(np.uint8) << 1)
        left = n - int(gone.sum())
        if left >= min_keep:
            out_bits[p, :left] = bits[p, :n][~gone]
            out_counts[p] = left
        else:
            out_bits[p, :n] = bits[p, :n]
            out_counts[p] = n
        if moving is not None:
            moving[p] = n - left
    return out_rows, out_counts, moving, flags


def scene_rows():
    """The rows of plate_checks.panning_scene() -> (rows f32[8,cap,4], counts i32[8], background rows per pair (a list of
    f32[k,4]), cap).  Pair p is (frame p + 1, frame p).  A square row has a on the bright square of the current frame and b at the
    same offset on the square of the previous one; a background row is a plane point on a 3-pixel grid inside both windows and
    inside neither square, mapped into the two frames.  Square and background rows are interleaved."""
    _, frames, mats, squares = P.panning_scene()
    per_pair, background = [], []
    for p in range(8):
        def window(k):
            return 2 * k + 1, k + 2                           # dx, dy of frame k's translation

        def square(k):
            return (5 * k) % 20, (3 * k) % 12

        (cdx, cdy), (pdx, pdy) = window(p + 1), window(p)
        (csx, csy), (psx, psy) = square(p + 1), square(p)
        sq = [(csx + i, csy + j, psx + i, psy + j) for j in range(4) for i in range(4)]
        bg = []
        for Y in range(cdy, 40, 3):                           # the grid starts at the corner the two windows share
            for X in range(cdx, 60, 3):
                inside = cdx <= X < cdx + 24 and cdy <= Y < cdy + 16 and pdx <= X < pdx + 24 and pdy <= Y < pdy + 16
                if inside and not squares[p + 1, Y, X] and not squares[p, Y, X]:
                    bg.append((X - cdx, Y - cdy, X - pdx, Y - pdy))
        mixed, s, b = [], list(sq), list(bg)
        while s or b:
            if b:
                mixed.append(b.pop(0))
            if s:
                mixed.append(s.pop(0))
            if b:
                mixed.append(b.pop(0))
        per_pair.append(np.array(mixed, np.float32))
        background.append(np.array(bg, np.float32))
    cap = max(len(r) for r in per_pair) + 3
    rows = np.zeros((8, cap, 4), np.float32)
    for p, r in enumerate(per_pair):
        rows[p, :len(r)] = r
    return rows, np.array([len(r) for r in per_pair], np.int32), background, cap
