"""numpy restatement of evh_warp_fixed_plane (include/evhip.h), vectorised over the canvas: every operation below is one
IEEE float64 operation on arrays, in the order the header states, so the device must agree with it byte for byte.

    warp_frame(src, M, dw, dh, origin, inverse_map)            -> (values u8[dh,dw(,c)], covered bool[dh,dw])
    warp_canvases(frames, mats, mode, dw, dh, origin, background, inverse_map)
                                                               -> u8[n,dh,dw(,c)] ("each", "history") or u8[dh,dw(,c)] ("mosaic")
    planes_to_bgr(planes)                                      -> the BGR frames a list of (y, cb, cr) converts to
    translation(dx, dy)                                        -> the 3x3 of a paste at (dx, dy)
"""
import numpy as np

FRACTION_BITS = 5   # positions in 1/32 pixels (OpenCV's INTER_BITS)


def adjugate(M):
    m = np.asarray(M, np.float64).reshape(9)
    return np.array([m[4] * m[8] - m[5] * m[7], m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
                     m[5] * m[6] - m[3] * m[8], m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
                     m[3] * m[7] - m[4] * m[6], m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]], np.float64)


def translation(dx, dy):
    return np.array([[1, 0, dx], [0, 1, dy], [0, 0, 1]], np.float64)


def warp_frame(src, M, dw, dh, origin=(0, 0), inverse_map=False):
    """One frame u8[sh,sw] or u8[sh,sw,c] at every canvas pixel: its interpolated bytes and whether it covers the pixel."""
    src = np.asarray(src)
    sh, sw = src.shape[:2]
    with np.errstate(all="ignore"):
        a = np.asarray(M, np.float64).reshape(9) if inverse_map else adjugate(M)
        X = (np.arange(dw, dtype=np.int64) + int(origin[0])).astype(np.float64)[None, :]
        Y = (np.arange(dh, dtype=np.int64) + int(origin[1])).astype(np.float64)[:, None]
        tx = (a[0] * X + a[1] * Y) + a[2]
        ty = (a[3] * X + a[4] * Y) + a[5]
        tw = (a[6] * X + a[7] * Y) + a[8]
        U = np.rint(tx / tw * 32)
        V = np.rint(ty / tw * 32)
        covered = (U >= 0) & (U <= 32 * (sw - 1)) & (V >= 0) & (V <= 32 * (sh - 1))      # NaN and +-inf fail
    Ui = np.where(covered, U, 0).astype(np.int64)
    Vi = np.where(covered, V, 0).astype(np.int64)
    sx, fx, sy, fy = Ui >> 5, Ui & 31, Vi >> 5, Vi & 31
    # a tap of weight 0 is not read: its index is only clamped here to keep numpy's gather inside the array
    sx1, sy1 = np.minimum(sx + 1, sw - 1), np.minimum(sy + 1, sh - 1)
    assert not ((sx + 1 >= sw) & (fx != 0) & covered).any() and not ((sy + 1 >= sh) & (fy != 0) & covered).any()
    s = src.astype(np.int64)
    wgt = (lambda a_: a_[..., None]) if src.ndim == 3 else (lambda a_: a_)
    val = (s[sy, sx] * wgt((32 - fx) * (32 - fy)) + s[sy, sx1] * wgt(fx * (32 - fy)) + s[sy1, sx] * wgt((32 - fx) * fy)
           + s[sy1, sx1] * wgt(fx * fy) + 512) >> 10
    assert val.min() >= 0 and val.max() <= 255
    return val.astype(np.uint8), covered


def warp_canvases(frames, mats, mode, dw, dh, origin=(0, 0), background=None, inverse_map=False):
    """The three modes over frames u8[n,sh,sw(,c)] and mats f64[n,9] (or [n,3,3]), frames taken in order."""
    frames = np.asarray(frames)
    mats = np.asarray(mats, np.float64).reshape(-1, 9)
    n = len(frames)
    assert len(mats) == n and mode in ("each", "history", "mosaic")
    shape = (dh, dw) + frames.shape[3:]
    canvas = np.zeros(shape, np.uint8) if background is None else np.array(background, np.uint8).reshape(shape)
    outs = []
    for k in range(n):
        val, cov = warp_frame(frames[k], mats[k], dw, dh, origin, inverse_map)
        base = canvas.copy()
        base[cov] = val[cov]
        outs.append(base)
        if mode != "each":
            canvas = base                     # the last covering frame wins
    if mode == "mosaic":
        return canvas
    return np.stack(outs) if outs else np.zeros((0,) + shape, np.uint8)


def planes_to_bgr(planes):
    from evenvizion_amd.synthetic import yuv420_to_bgr_host
    return np.stack([yuv420_to_bgr_host(*p) for p in planes])
