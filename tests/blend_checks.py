"""numpy restatement of evh_blend_fixed_plane, evh_blend_ray_surface and evh_pair_exposure (include/evhip.h), and of the cost
blend.solve_gains minimises.  No product code: the positions are formed as warp_checks / surface_checks form them (one IEEE
float64 operation at a time, in the header's order), the bytes come from surface_checks.taps, and the state of a canvas pixel is
held in Python integers (object arrays), which cannot wrap.

    position(M, sw, sh, dw, dh, origin, inverse_map)      -> (U, V, covered) of the plane form
    ray_position(A, cols, rows, sw, sh)                   -> (U, V, covered) of the ray form (tw > 0 included)
    weight(U, V, covered, sw, sh, feather)                -> int64[dh,dw]: min(d, F) + 1 where covered
    blend(frames, mats, dw, dh, origin, mode, feather, gains, state, background, inverse_map)   -> (picture, state)
    blend_ray(frames, mats, cols, rows, mode, feather, gains, state, background)                -> (picture, state)
    picture(state, mode, background)                      -> u8[dh,dw(,c)] of a state
    exposure(frames, pairs, maps, step, lo, hi)           -> object[npairs,7]
    gain_cost(g, pairs, stats, channel, sigma_n, sigma_g, min_pixels) -> float

A state is an object array [dh,dw,c+1]; frames u8[n,sh,sw] are gray (c = 1), u8[n,sh,sw,3] BGR.
"""
import numpy as np

from surface_checks import taps
from warp_checks import adjugate, warp_frame

FEATHER, SEAM = "feather", "seam"


def position(M, sw, sh, dw, dh, origin=(0, 0), inverse_map=False):
    with np.errstate(all="ignore"):
        a = np.asarray(M, np.float64).reshape(9) if inverse_map else adjugate(M)
        X = (np.arange(dw, dtype=np.int64) + int(origin[0])).astype(np.float64)[None, :]
        Y = (np.arange(dh, dtype=np.int64) + int(origin[1])).astype(np.float64)[:, None]
        tx = (a[0] * X + a[1] * Y) + a[2]
        ty = (a[3] * X + a[4] * Y) + a[5]
        tw = (a[6] * X + a[7] * Y) + a[8]
        U = np.rint(tx / tw * 32)
        V = np.rint(ty / tw * 32)
        covered = (U >= 0) & (U <= 32 * (sw - 1)) & (V >= 0) & (V <= 32 * (sh - 1))
    return U, V, covered


def ray_position(A, cols, rows, sw, sh):
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
        covered = (tw > 0) & (U >= 0) & (U <= 32 * (sw - 1)) & (V >= 0) & (V <= 32 * (sh - 1))
    return U, V, covered


def weight(U, V, covered, sw, sh, feather):
    """min(d, F) + 1 with d the distance of (U, V) to the nearest frame edge, in 1/32 pixels (0 where not covered)."""
    Ui = np.where(covered, U, 0).astype(np.int64)
    Vi = np.where(covered, V, 0).astype(np.int64)
    d = np.minimum(np.minimum(Ui, 32 * (sw - 1) - Ui), np.minimum(Vi, 32 * (sh - 1) - Vi))
    assert (d[covered] >= 0).all()
    return np.where(covered, np.minimum(d, int(feather)) + 1, 0)


def _empty_state(dh, dw, cn):
    s = np.empty((dh, dw, cn + 1), object)
    s[...] = 0
    return s


def _reduce(state, frame, U, V, covered, mode, feather, g):
    """One frame into the state, pixel by pixel in Python integers."""
    sh, sw = frame.shape[:2]
    cn = state.shape[2] - 1
    val = taps(frame, U, V, covered).reshape(covered.shape + (cn,))
    w = weight(U, V, covered, sw, sh, feather)
    for y, x in zip(*np.nonzero(covered)):
        wk = int(w[y, x])
        t = [int(val[y, x, c]) * int(g[c]) for c in range(cn)]
        if mode == FEATHER:
            for c in range(cn):
                state[y, x, c] += wk * t[c]
            state[y, x, cn] += wk
        elif wk > state[y, x, cn]:
            for c in range(cn):
                state[y, x, c] = t[c]
            state[y, x, cn] = wk


def picture(state, mode, background=None):
    dh, dw, ns = state.shape
    cn = ns - 1
    out = np.zeros((dh, dw, cn), np.uint8) if background is None else np.array(background, np.uint8).reshape(dh, dw, cn).copy()
    for y in range(dh):
        for x in range(dw):
            den = int(state[y, x, cn])
            if den == 0:
                continue
            for c in range(cn):
                a = int(state[y, x, c])
                out[y, x, c] = min(255, (a + (den << 11)) // (den << 12)) if mode == FEATHER else min(255, (a + 2048) >> 12)
    return out[..., 0] if cn == 1 else out


def _run(frames, positions, shape, mode, feather, gains, state, background):
    frames = np.asarray(frames)
    assert mode in (FEATHER, SEAM)
    cn = 1 if frames.ndim == 3 else frames.shape[3]
    dh, dw = shape
    st = _empty_state(dh, dw, cn) if state is None else np.array(state, object).reshape(dh, dw, cn + 1).copy()
    for k, frame in enumerate(frames):
        g = [4096] * 3 if gains is None else [int(v) for v in np.asarray(gains)[k]]
        U, V, covered = positions(k, frame.shape[1], frame.shape[0])
        _reduce(st, frame, U, V, covered, mode, feather, g)
    return picture(st, mode, background), st


def blend(frames, mats, dw, dh, origin=(0, 0), mode=FEATHER, feather=1024, gains=None, state=None, background=None,
          inverse_map=False):
    mats = np.asarray(mats, np.float64).reshape(-1, 9)
    assert len(mats) == len(frames)
    return _run(frames, lambda k, sw, sh: position(mats[k], sw, sh, dw, dh, origin, inverse_map), (dh, dw), mode, feather, gains,
                state, background)


def blend_ray(frames, mats, cols, rows, mode=FEATHER, feather=1024, gains=None, state=None, background=None):
    mats = np.asarray(mats, np.float64).reshape(-1, 9)
    assert len(mats) == len(frames)
    return _run(frames, lambda k, sw, sh: ray_position(mats[k], cols, rows, sw, sh), (len(rows), len(cols)), mode, feather, gains,
                state, background)


def state_to_i64(state):
    """The state as the int64 view of the device's u64 values."""
    return np.array([int(v) - (1 << 64) if int(v) >= (1 << 63) else int(v) for v in state.reshape(-1)], np.int64).reshape(state.shape)


def exposure(frames, pairs, maps, step, lo, hi):
    frames = np.asarray(frames)
    n, h, w = frames.shape[:3]
    cn = 1 if frames.ndim == 3 else frames.shape[3]
    maps = np.asarray(maps, np.float64).reshape(-1, 9)
    out = np.empty((len(pairs), 7), object)
    out[...] = 0
    for p, (i, j) in enumerate(pairs):
        if not (0 <= i < n and 0 <= j < n):
            continue
        b, cov = warp_frame(frames[j], maps[p], w, h, (0, 0), inverse_map=True)
        a = frames[i].reshape(h, w, cn)[::step, ::step].astype(np.int64)
        b = b.reshape(h, w, cn)[::step, ::step].astype(np.int64)
        ok = cov[::step, ::step] & ((a >= lo) & (a <= hi) & (b >= lo) & (b <= hi)).all(axis=2)
        out[p, 0] = int(ok.sum())
        for c in range(cn):
            out[p, 1 + c] = int(a[..., c][ok].sum())
            out[p, 4 + c] = int(b[..., c][ok].sum())
    return out


def gain_cost(g, pairs, stats, channel=0, sigma_n=10.0, sigma_g=0.1, min_pixels=64):
    """sum_p N_p * [(g_i * abar_p - g_j * bbar_p)^2 / sigma_n^2 + ((1 - g_i)^2 + (1 - g_j)^2) / sigma_g^2] over the pairs with
    N_p >= min_pixels, for one channel; g: float64[n]."""
    cost = 0.0
    for (i, j), s in zip(pairs, stats):
        N = float(s[0])
        if N < min_pixels or N <= 0:
            continue
        abar, bbar = float(s[1 + channel]) / N, float(s[4 + channel]) / N
        cost += N * ((g[i] * abar - g[j] * bbar) ** 2 / sigma_n ** 2 + ((1 - g[i]) ** 2 + (1 - g[j]) ** 2) / sigma_g ** 2)
    return cost
