"""numpy restatement of evh_plate_fixed_plane (include/evhip.h), built on warp_checks.warp_frame, which gives every frame's
samples and coverage exactly as evh_warp_fixed_plane states them.

    plate(frames, mats, dw, dh, origin, background, inverse_map, min_cover, threshold) -> (plate u8[dh,dw(,c)], count u8[dh,dw],
                                                                                          masks u8[n,dh,dw])
    gray(bgr)                                                                          -> the integer gray of the masks
    panning_scene(), check_panning_scene(plate_of, mosaic_of)                          -> what the plate is for, host and device

Uncovered samples are keyed 256 and sorted last, so the covering ones fill ranks 0 .. n-1 and the plate is the key at rank
(n - 1) >> 1, per channel.
"""
import numpy as np

import warp_checks as W


def gray(a):
    """(b*1868 + g*9617 + r*4899 + 8192) >> 14 over the last axis of [...,3]; a gray array is its own gray."""
    a = np.asarray(a).astype(np.int64)
    return a if a.shape[-1:] != (3,) else (a[..., 0] * 1868 + a[..., 1] * 9617 + a[..., 2] * 4899 + 8192) >> 14


def plate(frames, mats, dw, dh, origin=(0, 0), background=None, inverse_map=False, min_cover=1, threshold=16):
    """frames u8[n,sh,sw] or u8[n,sh,sw,3], mats f64[n,9] (or [n,3,3]); n may be 0 (frames then only gives the channels)."""
    frames = np.asarray(frames)
    mats = np.asarray(mats, np.float64).reshape(-1, 9)
    n = len(frames)
    assert len(mats) == n and 1 <= min_cover <= 255 and 0 <= threshold <= 255 and n <= 255
    bgr = frames.ndim == 4
    shape = (dh, dw, 3) if bgr else (dh, dw)
    bg = np.zeros(shape, np.uint8) if background is None else np.array(background, np.uint8).reshape(shape)
    if n == 0:
        return bg, np.zeros((dh, dw), np.uint8), np.zeros((0, dh, dw), np.uint8)
    warped = [W.warp_frame(frames[k], mats[k], dw, dh, origin, inverse_map) for k in range(n)]
    val = np.stack([w[0] for w in warped]).astype(np.int64)                  # [n,dh,dw(,3)]
    cov = np.stack([w[1] for w in warped])                                   # [n,dh,dw]
    count = cov.sum(axis=0)
    per_channel = (lambda a: a[..., None]) if bgr else (lambda a: a)
    key = np.sort(np.where(per_channel(cov), val, 256), axis=0)
    rank = np.maximum(count - 1, 0) >> 1
    median = np.take_along_axis(key, per_channel(rank)[None], axis=0)[0]
    settled = count >= min_cover
    assert (median[settled] <= 255).all()
    out = np.where(per_channel(settled), median, bg).astype(np.uint8)
    masks = cov & settled[None] & (np.abs(gray(val) - gray(out)[None]) > threshold)
    return out, count.astype(np.uint8), np.where(masks, 255, 0).astype(np.uint8)


def panning_scene():
    """A 24 x 16 window panning over a fixed background, with a bright 4 x 4 square that moves inside the window."""
    B = np.random.default_rng(5).integers(0, 255, (40, 60, 3)).astype(np.uint8)
    frames, mats, squares = [], [], np.zeros((9, 40, 60), bool)
    for k in range(9):
        dx, dy = 2 * k + 1, k + 2
        f = B[dy:dy + 16, dx:dx + 24].copy()
        sx, sy = (5 * k) % 20, (3 * k) % 12
        f[sy:sy + 4, sx:sx + 4] = 255
        squares[k, dy + sy:dy + sy + 4, dx + sx:dx + sx + 4] = True
        frames.append(f)
        mats.append(W.translation(dx, dy))
    return B, np.stack(frames), np.stack(mats), squares


def check_panning_scene(plate_of, mosaic_of):
    """The three equalities of the panning scene, for whatever computes a plate and a mosaic."""
    B, frames, mats, squares = panning_scene()
    plate, count, masks = plate_of(frames, mats, 60, 40, min_cover=2, threshold=0)
    twice = count >= 2
    assert (count >= 1).sum() == 816 and twice.sum() == 680
    assert np.array_equal(plate[twice], B[twice]) and not plate[~twice].any()     # the square is gone wherever two frames meet
    mosaic = mosaic_of(frames, mats, 60, 40)
    assert ((mosaic != B).any(axis=2) & (count >= 1)).sum() == 36                 # the last covering frame keeps its square
    assert np.array_equal(masks != 0, squares & twice[None]) and (masks != 0).sum() == 134
    assert set(np.unique(masks)) == {0, 255}
