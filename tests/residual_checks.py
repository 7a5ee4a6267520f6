"""numpy restatement of evh_pair_residual (include/evhip.h) on top of warp_checks.warp_frame: the previous frame sampled where
the matrix sends each pixel of the current frame, both taken to gray with the ingest's weights, differenced and summed over the
covered pixels.  Every figure is an exact integer, so the device must agree with it to the last unit and byte.

    gray_of(img)                                   -> u8[h,w]: (b*1868 + g*9617 + r*4899 + 8192) >> 14, or the byte itself
    residual(prev, cur, M, threshold)              -> (stats: six Python ints, abs picture u8[h,w], mask picture u8[h,w])
    residual_pairs(frames, mats, threshold, frame_step)
                                                   -> (stats int64[npairs,6], abs u8[npairs,h,w], mask u8[npairs,h,w])
"""
import numpy as np

import warp_checks as W

COVERED, SAD, SSD, SAD0, SSD0, MOVING = range(6)


def gray_of(img):
    img = np.asarray(img)
    if img.ndim == 2:
        return img.astype(np.uint8)
    p = img.astype(np.int64)
    return ((p[..., 0] * 1868 + p[..., 1] * 9617 + p[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def residual(prev, cur, M, threshold=16):
    """One pair.  M maps pixels of `cur` to pixels of `prev` and is used as it is (inverse_map)."""
    prev, cur = np.asarray(prev), np.asarray(cur)
    assert prev.shape == cur.shape and prev.dtype == np.uint8 and cur.dtype == np.uint8
    h, w = cur.shape[:2]
    val, cov = W.warp_frame(prev, M, w, h, (0, 0), inverse_map=True)      # interpolated per channel, converted afterwards
    g_cur, g_reg, g_prev = (gray_of(a).astype(np.int64) for a in (cur, val, prev))
    d = np.where(cov, np.abs(g_cur - g_reg), 0)
    d0 = np.where(cov, np.abs(g_cur - g_prev), 0)
    moving = cov & (d > int(threshold))
    stats = (int(cov.sum()), int(d.sum()), int((d * d).sum()), int(d0.sum()), int((d0 * d0).sum()), int(moving.sum()))
    return stats, d.astype(np.uint8), np.where(moving, 255, 0).astype(np.uint8)


def residual_pairs(frames, mats, threshold=16, frame_step=1):
    frames = np.asarray(frames)
    mats = np.asarray(mats, np.float64).reshape(-1, 9)
    h, w = frames.shape[1:3]
    stats = np.zeros((len(mats), 6), np.int64)
    pics = np.zeros((2, len(mats), h, w), np.uint8)
    for p, M in enumerate(mats):
        s, pics[0, p], pics[1, p] = residual(frames[p * frame_step], frames[p * frame_step + 1], M, threshold)
        stats[p] = s
    return stats, pics[0], pics[1]
