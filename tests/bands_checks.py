"""numpy restatement of evh_seam_labels_* and evh_blend_bands_* (include/evhip.h).  No product code: positions are formed as
blend_checks / surface_checks form them (one IEEE float64 operation at a time, in the header's order), the taps come from
surface_checks.taps, and everything after them is int64 -- the header's bounds keep |A| below 2^43, and the crafted states of the
tests stay below 2^52, so nothing wraps.

    level_sizes(dw, dh, levels)                           -> [(dw_l, dh_l)] for l = 0 .. levels
    state_elems(dw, dh, cn, levels), frame_ws_bytes(...)  -> what the sizing helpers return
    labels_plane(mats, sw, sh, dw, dh, origin, feather, first_label, best, label, inverse_map)   -> (best u32, label u16)
    labels_ray(mats, cols, rows, sw, sh, feather, first_label, best, label)                      -> (best u32, label u16)
    plane_positions / ray_positions                       -> [(U, V, valid)] per frame: the position before any coverage test
    extended_sample(frame, U, V, valid)                   -> int64[dh,dw,cn]: the frame continued by its edge pixels
    pyramid(G0, W0, levels)                               -> ([L^l], [W^l])
    bands(frames, positions, label, levels, first_label, gains, state, background, order)        -> (picture, state)
    picture(state, dw, dh, cn, levels, background)        -> u8[dh,dw(,c)] of a state

A state is int64, flat: per level [dh_l][dw_l][cn+1], levels 0..n one after the other, as the device holds it.
"""
import numpy as np

import blend_checks as BC
from surface_checks import taps

NOBODY = 65535
K5 = (1, 4, 6, 4, 1)


def level_sizes(dw, dh, levels):
    out = []
    for _ in range(levels + 1):
        out.append((dw, dh))
        dw, dh = (dw + 1) >> 1, (dh + 1) >> 1
    return out


def state_elems(dw, dh, cn, levels):
    return sum(w * h for w, h in level_sizes(dw, dh, levels)) * (cn + 1)


def frame_ws_bytes(dw, dh, cn, levels):
    return 4 * state_elems(dw, dh, cn, levels)


# ---- labels ---------------------------------------------------------------------------------------------------------------------------
def _labels(covering, sw, sh, shape, feather, first_label, best, label):
    best = np.zeros(shape, np.int64) if best is None else np.asarray(best).astype(np.int64).copy()
    label = np.full(shape, NOBODY, np.int64) if label is None else np.asarray(label).astype(np.int64).copy()
    for k, (U, V, covered) in enumerate(covering):
        w = BC.weight(U, V, covered, sw, sh, feather)
        take = w > best                                    # strict: the earliest frame holds among equal weights
        best[take] = w[take]
        label[take] = first_label + k
    return best.astype(np.uint32), label.astype(np.uint16)


def labels_plane(mats, sw, sh, dw, dh, origin=(0, 0), feather=1024, first_label=0, best=None, label=None, inverse_map=False):
    mats = np.asarray(mats, np.float64).reshape(-1, 9)
    return _labels([BC.position(m, sw, sh, dw, dh, origin, inverse_map) for m in mats], sw, sh, (dh, dw), feather, first_label, best,
                   label)


def labels_ray(mats, cols, rows, sw, sh, feather=1024, first_label=0, best=None, label=None):
    mats = np.asarray(mats, np.float64).reshape(-1, 9)
    return _labels([BC.ray_position(m, cols, rows, sw, sh) for m in mats], sw, sh, (len(rows), len(cols)), feather, first_label, best,
                   label)


# ---- the extended sample --------------------------------------------------------------------------------------------------------------
def plane_positions(mats, sw, sh, dw, dh, origin=(0, 0), inverse_map=False):
    out = []
    for m in np.asarray(mats, np.float64).reshape(-1, 9):
        U, V, _ = BC.position(m, sw, sh, dw, dh, origin, inverse_map)
        out.append((U, V, ~np.isnan(U) & ~np.isnan(V)))
    return out


def ray_positions(mats, cols, rows):
    cols = np.asarray(cols, np.float64)
    a, c = cols[:, 0][None, :], cols[:, 1][None, :]
    b = np.asarray(rows, np.float64)[:, None]
    out = []
    for A in np.asarray(mats, np.float64).reshape(-1, 9):
        with np.errstate(all="ignore"):
            tx = (A[0] * a + A[1] * b) + A[2] * c
            ty = (A[3] * a + A[4] * b) + A[5] * c
            tw = (A[6] * a + A[7] * b) + A[8] * c
            U, V = np.rint(tx / tw * 32), np.rint(ty / tw * 32)
        out.append((U, V, ~np.isnan(U) & ~np.isnan(V) & (tw > 0)))
    return out


def extended_sample(frame, U, V, valid):
    frame = np.asarray(frame)
    sh, sw = frame.shape[:2]
    cn = 1 if frame.ndim == 2 else frame.shape[2]
    with np.errstate(all="ignore"):
        Uc = np.minimum(np.maximum(U, 0.0), 32.0 * (sw - 1))
        Vc = np.minimum(np.maximum(V, 0.0), 32.0 * (sh - 1))
    s = taps(frame, Uc, Vc, valid).astype(np.int64).reshape(valid.shape + (cn,))
    s[~valid] = 0
    return s


# ---- pyramids -------------------------------------------------------------------------------------------------------------------------
def reduce(a, add):
    """a: int64[h,w(,c)] one level down; add = 128 (G) or 255 (W)"""
    h, w = a.shape[:2]
    ys = np.clip(2 * np.arange((h + 1) >> 1)[:, None] + np.arange(5)[None, :] - 2, 0, h - 1)
    xs = np.clip(2 * np.arange((w + 1) >> 1)[:, None] + np.arange(5)[None, :] - 2, 0, w - 1)
    rows = sum(K5[j] * a[ys[:, j]] for j in range(5))
    out = sum(K5[i] * rows[:, xs[:, i]] for i in range(5))
    assert out.min() >= 0 and out.max() + add < (1 << 32)
    return (out + add) >> 8


def _expand_axis(g, n, axis):
    i = np.arange(n)
    j, m = i >> 1, g.shape[axis]
    lo, hi = np.clip(j - 1, 0, m - 1), np.clip(j + 1, 0, m - 1)
    even = np.take(g, lo, axis) + 6 * np.take(g, j, axis) + np.take(g, hi, axis)
    odd = 4 * np.take(g, j, axis) + 4 * np.take(g, hi, axis)
    pick = (i & 1).reshape([-1 if d == axis else 1 for d in range(g.ndim)]).astype(bool)
    return np.where(pick, odd, even)


def expand(g, w, h):
    """g: int64[h1,w1(,c)] -> [h,w(,c)]: rows, then columns, then (. + 32) >> 6 (an arithmetic shift: it rounds down)"""
    assert g.shape[0] == (h + 1) >> 1 and g.shape[1] == (w + 1) >> 1
    return (_expand_axis(_expand_axis(g, w, 1), h, 0) + 32) >> 6


def pyramid(G0, W0, levels):
    G, W = [np.asarray(G0, np.int64)], [np.asarray(W0, np.int64)]
    for _ in range(levels):
        G.append(reduce(G[-1], 128))
        W.append(reduce(W[-1], 255))
    L = [G[l] - expand(G[l + 1], G[l].shape[1], G[l].shape[0]) for l in range(levels)] + [G[levels]]
    return L, W


def split(state, dw, dh, cn, levels):
    """the per-level views [dh_l, dw_l, cn+1] of a flat state"""
    out, at = [], 0
    for w, h in level_sizes(dw, dh, levels):
        out.append(state[at:at + w * h * (cn + 1)].reshape(h, w, cn + 1))
        at += w * h * (cn + 1)
    assert at == state.size
    return out


def picture(state, dw, dh, cn, levels, background=None):
    lv = split(np.asarray(state, np.int64), dw, dh, cn, levels)
    R = None
    for l in range(levels, -1, -1):
        A, D = lv[l][..., :cn], lv[l][..., cn:]
        q = np.where(D > 0, (2 * A + D) // np.where(D > 0, 2 * D, 1), 0)             # // rounds down, also below zero
        R = q if R is None else q + expand(R, lv[l].shape[1], lv[l].shape[0])
    out = np.zeros((dh, dw, cn), np.uint8) if background is None else np.array(background, np.uint8).reshape(dh, dw, cn).copy()
    byte = np.clip((R + 2048) >> 12, 0, 255).astype(np.uint8)
    have = lv[0][..., cn] > 0
    out[have] = byte[have]
    return out[..., 0] if cn == 1 else out


def bands(frames, positions, label, levels, first_label=0, gains=None, state=None, background=None, order=None):
    """frames u8[n,sh,sw(,3)], positions: plane_positions / ray_positions of their matrices, label u16[dh,dw]"""
    frames = np.asarray(frames)
    cn = 1 if frames.ndim == 3 else frames.shape[3]
    label = np.asarray(label)
    dh, dw = label.shape
    st = np.zeros(state_elems(dw, dh, cn, levels), np.int64) if state is None else np.array(state, np.int64).reshape(-1).copy()
    lv = split(st, dw, dh, cn, levels)
    for k in (range(len(frames)) if order is None else order):
        g = np.full(3, 4096, np.int64) if gains is None else np.asarray(gains)[k].astype(np.int64)
        U, V, valid = positions[k]
        G0 = extended_sample(frames[k], U, V, valid) * g[:cn]
        assert G0.max(initial=0) < (1 << 24)
        W0 = np.where(label == first_label + k, 65536, 0).astype(np.int64)
        L, W = pyramid(G0, W0, levels)
        for l in range(levels + 1):
            assert np.abs(L[l]).max(initial=0) < (1 << 25) and W[l].max(initial=0) <= 65536
            lv[l][..., :cn] += W[l][..., None] * L[l]
            lv[l][..., cn] += W[l]
    return picture(st, dw, dh, cn, levels, background), st


def bands_plane(frames, mats, dw, dh, origin, label, levels, inverse_map=False, **kw):
    frames = np.asarray(frames)
    return bands(frames, plane_positions(mats, frames.shape[2], frames.shape[1], dw, dh, origin, inverse_map), label, levels, **kw)


def bands_ray(frames, mats, cols, rows, label, levels, **kw):
    return bands(frames, ray_positions(mats, cols, rows), label, levels, **kw)
