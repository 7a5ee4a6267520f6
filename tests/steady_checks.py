"""numpy restatement of evh_steady_frames (include/evhip.h): position, cover and value are warp_checks.warp_frame's with
inverse_map, the edge distance and the feather are added here, every step in the order the header states, so the device must
agree with it byte for byte.

    edge_distance(M, sw, sh, dw, dh)                                   -> i64[dh,dw], valid where the tap covers
    steady_frames(frames, tap_frame, tap_M, dw, dh, feather, background)
                                                                       -> (pictures u8[nout,dh,dw(,c)], tap_of u8[nout,dh,dw],
                                                                           counts i64[nout,ntaps+1])
"""
import numpy as np

import warp_checks as W


def edge_distance(M, sw, sh, dw, dh):
    """min(U, 32(sw-1) - U, V, 32(sh-1) - V) of the map M at every output pixel; U and V formed as warp_frame forms them."""
    a = np.asarray(M, np.float64).reshape(9)
    with np.errstate(all="ignore"):
        X = np.arange(dw, dtype=np.float64)[None, :]
        Y = np.arange(dh, dtype=np.float64)[:, None]
        tx = (a[0] * X + a[1] * Y) + a[2]
        ty = (a[3] * X + a[4] * Y) + a[5]
        tw = (a[6] * X + a[7] * Y) + a[8]
        U = np.rint(tx / tw * 32)
        V = np.rint(ty / tw * 32)
        ok = (U >= 0) & (U <= 32 * (sw - 1)) & (V >= 0) & (V <= 32 * (sh - 1))
    U = np.where(ok, U, 0).astype(np.int64)
    V = np.where(ok, V, 0).astype(np.int64)
    return np.minimum(np.minimum(U, 32 * (sw - 1) - U), np.minimum(V, 32 * (sh - 1) - V))


def steady_frames(frames, tap_frame, tap_M, dw, dh, feather=0, background=None):
    frames = np.asarray(frames)
    nframes, sh, sw = frames.shape[:3]
    tail = frames.shape[3:]
    tap_frame = np.asarray(tap_frame, np.int64)
    nout, ntaps = tap_frame.shape
    tap_M = np.asarray(tap_M, np.float64).reshape(nout, ntaps, 9)
    assert 1 <= ntaps <= 16 and 0 <= feather <= 8160
    bg = np.zeros((dh, dw) + tail, np.uint8) if background is None else np.asarray(background, np.uint8).reshape((dh, dw) + tail)
    pictures = np.zeros((nout, dh, dw) + tail, np.uint8)
    tap_of = np.zeros((nout, dh, dw), np.uint8)
    counts = np.zeros((nout, ntaps + 1), np.int64)
    wide = (lambda a_: a_[..., None]) if tail else (lambda a_: a_)
    for j in range(nout):
        vals, covs = [], []
        for t in range(ntaps):
            f = int(tap_frame[j, t])
            if 0 <= f < nframes:
                val, cov = W.warp_frame(frames[f], tap_M[j, t], dw, dh, (0, 0), True)
            else:                                                     # not live: covers nothing
                val, cov = np.zeros((dh, dw) + tail, np.uint8), np.zeros((dh, dw), bool)
            vals.append(val.astype(np.int64))
            covs.append(cov)
        pic = bg.astype(np.int64)
        first = np.zeros((dh, dw), np.int64)                           # 0: none, else t + 1
        for t in range(ntaps - 1, -1, -1):
            pic = np.where(wide(covs[t]), vals[t], pic)
            first = np.where(covs[t], t + 1, first)
        if feather > 0:
            d = edge_distance(tap_M[j, 0], sw, sh, dw, dh)
            todo = (first == 1) & (d < feather)                        # tap 0's band, still without its second tap
            for t in range(1, ntaps):
                take = todo & covs[t]
                mixed = (vals[0] * wide(d) + vals[t] * wide(feather - d) + (feather >> 1)) // feather
                pic = np.where(wide(take), mixed, pic)
                todo = todo & ~covs[t]
        assert pic.min() >= 0 and pic.max() <= 255
        pictures[j] = pic.astype(np.uint8)
        tap_of[j] = first.astype(np.uint8)
        counts[j] = np.bincount(first.reshape(-1), minlength=ntaps + 1)
    return pictures, tap_of, counts
