"""numpy restatement of evh_trail_fixed_plane (include/evhip.h): the colour step in the arithmetic the header states -- int32 for
BGR -> HSV, float32 arrays for HSV -> BGR, so that every operation rounds once -- and the trail itself, once literally (a pixel
and a frame at a time) and once vectorised over the canvas.  Coverage and sampling come from warp_checks.warp_frame.

    to_hsv(p) -> (h, s, v)            from_hsv(h, s, v) -> u8[..., 3]            keep(p), show(p) -> u8[..., 3]
    trail_literal / trail(frames, mats, canvas, origin, rects, inverse_map) -> (pictures u8[n,dh,dw,3], canvas u8[dh,dw,3])
    every_colour() -> (frame u8[4096,4096,3] holding all 2^24 colours, keep of it, show of it, its V), computed once
"""
import functools

import numpy as np

import warp_checks as W

_I = np.arange(1, 256, dtype=np.float64)
S_TAB = np.concatenate([[0], np.rint(1044480.0 / _I)]).astype(np.int32)            # 255 << 12
H_TAB = np.concatenate([[0], np.rint(737280.0 / (6.0 * _I))]).astype(np.int32)     # 180 << 12
C6 = np.array([0x3D088889], np.uint32).view(np.float32)[0]                         # 6.f / 180.f
K255 = np.array([0x3B808081], np.uint32).view(np.float32)[0]                       # 1.f / 255.f
SECTOR = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])
ONE, SIX, F255 = np.float32(1), np.float32(6), np.float32(255)
DARK_HSV = (222, 12, 31)          # [222, 12.35, 31.76] stored into a uint8 array
DARK = (30, 31, 30)               # what from_hsv makes of it (test_trail_host.py checks that)
WHITE = (255, 255, 255)


def to_hsv(p):
    """p u8[..., 3] in BGR order -> (h, s, v) int32[...]"""
    p = np.asarray(p)
    b, g, r = (p[..., i].astype(np.int32) for i in range(3))
    v = np.maximum(b, np.maximum(g, r))
    d = v - np.minimum(b, np.minimum(g, r))
    s = (d * S_TAB[v] + 2048) >> 12
    t = np.where(v == r, g - b, np.where(v == g, b - r + 2 * d, r - g + 4 * d))
    h = (t * H_TAB[d] + 2048) >> 12                     # >> of a negative int32 is arithmetic: a floor
    return np.where(h < 0, h + 180, h), s, v


def from_hsv(h, s, v):
    """(h, s, v) integer arrays of one shape -> u8[..., 3] in BGR order"""
    h, s, v = (np.asarray(a, np.int32) for a in (h, s, v))
    hf = h.astype(np.float32) * C6
    while (hf >= SIX).any():
        hf = np.where(hf >= SIX, hf - SIX, hf)
    k = np.floor(hf)
    f = hf - k
    sf, vf = s.astype(np.float32) * K255, v.astype(np.float32) * K255
    tab = np.stack([vf, vf * (ONE - sf), vf * (ONE - sf * f), vf * (ONE - sf * (ONE - f))], axis=-1)
    assert tab.dtype == np.float32 and f.dtype == np.float32
    bgr = np.take_along_axis(tab, SECTOR[k.astype(np.int64)], axis=-1)
    bgr = np.where((s == 0)[..., None], vf[..., None], bgr)
    return np.clip(np.rint(bgr * F255), 0, 255).astype(np.uint8)


def keep_hsv(h, s, v):
    return from_hsv(h, s, np.maximum(v - 2, 0))


def show_hsv(h, s, v):
    lit = v >= 2
    return from_hsv(np.where(lit, h, DARK_HSV[0]), np.where(lit, s, DARK_HSV[1]), np.where(lit, v - 2, DARK_HSV[2]))


def keep(p):
    return keep_hsv(*to_hsv(p))


def show(p):
    return show_hsv(*to_hsv(p))


def on_outline(x, y, rect):
    x0, y0, x1, y1 = (int(a) for a in rect)
    return x0 <= x <= x1 and y0 <= y <= y1 and (x == x0 or x == x1 or y == y0 or y == y1)


def trail_literal(frames, mats, canvas, origin=(0, 0), rects=None, inverse_map=False):
    """The header's three steps, a pixel and a frame at a time."""
    c = np.array(canvas, np.uint8)
    dh, dw = c.shape[:2]
    pictures = np.zeros((len(frames), dh, dw, 3), np.uint8)
    for k in range(len(frames)):
        val, cov = W.warp_frame(frames[k], mats[k], dw, dh, origin, inverse_map)
        for y in range(dh):
            for x in range(dw):
                if cov[y, x]:
                    c[y, x] = val[y, x]
                q = c[y, x]
                if rects is not None and on_outline(x, y, rects[k]):
                    q = np.array(WHITE, np.uint8)
                pictures[k, y, x] = show(q)
                c[y, x] = keep(c[y, x])
    return pictures, c


def outline_mask(dw, dh, rect):
    x0, y0, x1, y1 = (int(a) for a in rect)
    x, y = np.arange(dw)[None, :], np.arange(dh)[:, None]
    return (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1) & ((x == x0) | (x == x1) | (y == y0) | (y == y1))


def trail(frames, mats, canvas, origin=(0, 0), rects=None, inverse_map=False):
    """The same over whole canvases."""
    c = np.array(canvas, np.uint8)
    dh, dw = c.shape[:2]
    pictures = np.zeros((len(frames), dh, dw, 3), np.uint8)
    for k in range(len(frames)):
        val, cov = W.warp_frame(frames[k], mats[k], dw, dh, origin, inverse_map)
        c[cov] = val[cov]
        q = c.copy()
        if rects is not None:
            q[outline_mask(dw, dh, rects[k])] = WHITE
        pictures[k] = show(q)
        c = keep(c)
    return pictures, c


@functools.lru_cache(maxsize=1)
def every_colour():
    """All 2^24 colours as one frame (pixel i holds b = i & 255, g = (i >> 8) & 255, r = i >> 16), with keep, show and V of
    every pixel; a quarter at a time to bound the float32 temporaries.  Read-only: shared by the tests that need it."""
    i = np.arange(1 << 24, dtype=np.uint32)
    frame = np.stack([i & 255, (i >> 8) & 255, i >> 16], axis=-1).astype(np.uint8)
    kept, shown, value = np.empty_like(frame), np.empty_like(frame), np.empty(1 << 24, np.int32)
    for a in range(0, 1 << 24, 1 << 22):
        h, s, v = to_hsv(frame[a:a + (1 << 22)])
        assert h.min() >= 0 and h.max() <= 179 and s.min() >= 0 and s.max() <= 255
        kept[a:a + (1 << 22)] = keep_hsv(h, s, v)
        shown[a:a + (1 << 22)] = show_hsv(h, s, v)
        value[a:a + (1 << 22)] = v
    out = tuple(a.reshape((4096, 4096) + a.shape[1:]) for a in (frame, kept, shown, value))
    for a in out:
        a.setflags(write=False)
    return out
