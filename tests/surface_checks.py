"""numpy restatement of evh_warp_ray_surface (include/evhip.h), vectorised over the canvas: every operation below is one IEEE
float64 operation on arrays, in the order the header states, so the device must agree with it byte for byte.

    ray_frame(src, A, cols, rows)                       -> (values u8[dh,dw(,c)], covered bool[dh,dw], tw f64[dh,dw])
    ray_canvases(frames, mats, cols, rows, mode, background)
                                                        -> u8[n,dh,dw(,c)] ("each", "history") or u8[dh,dw(,c)] ("mosaic")
    plane_tables(dw, dh, origin)                        -> the tables (X, 1), Y of the plane with canvas origin (ox, oy)

From the rounded position on the bytes are warp_checks' (the same 1/32-pixel taps, weights and >> 10).  warp_checks.warp_frame
forms its position from a matrix and an integer grid in one piece, so it cannot be handed a position: `taps` below restates its
last lines, and tests/test_surface_host.py holds the two together (the plane's tables against warp_frame, byte for byte).
"""
import numpy as np

from warp_checks import FRACTION_BITS, planes_to_bgr  # noqa: F401  (planes_to_bgr: for the tests that import this module)

ONE = 1 << FRACTION_BITS          # 32


def taps(src, U, V, covered):
    """The bytes of src u8[sh,sw(,c)] at the positions (U, V) in 1/32 pixels where `covered` (anything elsewhere)."""
    src = np.asarray(src)
    sh, sw = src.shape[:2]
    Ui = np.where(covered, U, 0).astype(np.int64)
    Vi = np.where(covered, V, 0).astype(np.int64)
    sx, fx, sy, fy = Ui >> FRACTION_BITS, Ui & (ONE - 1), Vi >> FRACTION_BITS, Vi & (ONE - 1)
    # a tap of weight 0 is not read: its index is only clamped here to keep numpy's gather inside the array
    sx1, sy1 = np.minimum(sx + 1, sw - 1), np.minimum(sy + 1, sh - 1)
    assert not ((sx + 1 >= sw) & (fx != 0) & covered).any() and not ((sy + 1 >= sh) & (fy != 0) & covered).any()
    s = src.astype(np.int64)
    wgt = (lambda a_: a_[..., None]) if src.ndim == 3 else (lambda a_: a_)
    val = (s[sy, sx] * wgt((ONE - fx) * (ONE - fy)) + s[sy, sx1] * wgt(fx * (ONE - fy)) + s[sy1, sx] * wgt((ONE - fx) * fy)
           + s[sy1, sx1] * wgt(fx * fy) + 512) >> 10
    assert val.min() >= 0 and val.max() <= 255
    return val.astype(np.uint8)


def ray_frame(src, A, cols, rows):
    """One frame u8[sh,sw] or u8[sh,sw,c] at every canvas ray: its interpolated bytes, whether it covers the pixel, and tw."""
    src = np.asarray(src)
    sh, sw = src.shape[:2]
    A = np.asarray(A, np.float64).reshape(9)
    cols = np.asarray(cols, np.float64)
    a, c = cols[:, 0][None, :], cols[:, 1][None, :]
    b = np.asarray(rows, np.float64)[:, None]
    with np.errstate(all="ignore"):
        tx = (A[0] * a + A[1] * b) + A[2] * c
        ty = (A[3] * a + A[4] * b) + A[5] * c
        tw = (A[6] * a + A[7] * b) + A[8] * c
        U = np.rint(tx / tw * 32)
        V = np.rint(ty / tw * 32)
        covered = (tw > 0) & (U >= 0) & (U <= 32 * (sw - 1)) & (V >= 0) & (V <= 32 * (sh - 1))      # NaN and +-inf fail
    return taps(src, U, V, covered), covered, tw


def ray_canvases(frames, mats, cols, rows, mode, background=None):
    """The three modes over frames u8[n,sh,sw(,c)] and mats f64[n,9] (or [n,3,3]), frames taken in order."""
    frames = np.asarray(frames)
    mats = np.asarray(mats, np.float64).reshape(-1, 9)
    n, dw, dh = len(frames), len(cols), len(rows)
    assert len(mats) == n and mode in ("each", "history", "mosaic")
    shape = (dh, dw) + frames.shape[3:]
    canvas = np.zeros(shape, np.uint8) if background is None else np.array(background, np.uint8).reshape(shape)
    outs = []
    for k in range(n):
        val, cov, _ = ray_frame(frames[k], mats[k], cols, rows)
        base = canvas.copy()
        base[cov] = val[cov]
        outs.append(base)
        if mode != "each":
            canvas = base                     # the last covering frame wins
    if mode == "mosaic":
        return canvas
    return np.stack(outs) if outs else np.zeros((0,) + shape, np.uint8)


def plane_tables(dw, dh, origin=(0, 0)):
    """(cols, rows) of the plane: a = X = x + ox, c = 1, b = Y = y + oy, the sums formed in int64 as evh_warp_fixed_plane does."""
    X = (np.arange(dw, dtype=np.int64) + int(origin[0])).astype(np.float64)
    Y = (np.arange(dh, dtype=np.int64) + int(origin[1])).astype(np.float64)
    return np.stack([X, np.ones(dw)], axis=1), Y
