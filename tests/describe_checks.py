"""ORB's describe stage restated plainly in numpy (int64 / float64), from the definitions: the Harris response, the
intensity-centroid orientation, the 7 x 7 sigma-2 fixed-point Gaussian and the steered BRIEF tests.  Shares no code with the
oracle or the kernels; tests/test_oracle_describe_edges.py holds the oracle to it, tests/test_gpu_describe_edges.py the device."""
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF_PATCH = 15          # radius of the orientation disc
TAP_REACH = 19           # |rotated tap coordinate| <= round(13 * sqrt(2)) + 0 = 18, plus the rounding: the kernel's DB_R
HARRIS_K = 0.04
HARRIS_SCALE = (1.0 / (4 * 7 * 255.0)) ** 4
# fastAtan2 (a degree-7 polynomial in the ratio of the moments) against atan2: the largest error measured is 0.009552 degrees
# (tests/test_oracle_describe_edges.py::test_fast_atan2_error_is_the_polynomials); the bound is twice that
ANGLE_BOUND = 2 * 0.009552


def _pattern():
    rows = []
    with open(os.path.join(ROOT, "evenvizion_amd", "data", "orb_pattern_31.txt")) as f:
        for line in f:
            line = line.split("#")[0].split()
            if line:
                rows.append([int(v) for v in line])
    p = np.array(rows, np.int64)
    assert p.shape == (256, 4) and np.abs(p).max() <= 13
    return p


PATTERN = _pattern()


def gauss_taps():
    """exp(-x^2 / (2 sigma^2)), sigma 2, x = -3 .. 3, normalised to sum 1 and rounded at 8 fractional bits"""
    g = np.exp(-np.arange(-3, 4, dtype=np.float64) ** 2 / 8.0)
    return np.rint(g / g.sum() * 256.0).astype(np.int64)


def reflect101(i, n):
    """index i of an axis of n samples under BORDER_REFLECT_101: ... 2 1 | 0 1 2 ... n-1 | n-2 n-3 ..."""
    i = np.abs(i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def blur7_u8(level):
    """(blurred, clipped): the separable 7-tap blur in exact int64 sums, ONE rounding (s + 32768) >> 16 after both passes,
    clipped to 0 .. 255; `clipped` marks the pixels where the clip acted"""
    k = gauss_taps()
    a = np.asarray(level).astype(np.int64)
    h, w = a.shape
    assert h >= 4 and w >= 4
    cols = reflect101(np.arange(w)[None, :] + np.arange(-3, 4)[:, None], w)          # [7, w]
    rows = reflect101(np.arange(h)[None, :] + np.arange(-3, 4)[:, None], h)          # [7, h]
    hp = sum(k[t] * a[:, cols[t]] for t in range(7))
    s = sum(k[t] * hp[rows[t], :] for t in range(7))
    v = (s + 32768) >> 16
    return np.clip(v, 0, 255).astype(np.uint8), (v > 255) | (v < 0)


def disc_half_widths():
    """half-width of the radius-15 disc in row |v|, v = 0 .. 15, by the circle rule: where |u| >= |v| a pixel belongs when
    |u| <= round(sqrt(15^2 - v^2)); the other octants are the mirror image about the diagonal"""
    r = HALF_PATCH
    inside = np.zeros((r + 1, r + 1), bool)
    for v in range(r + 1):
        for u in range(r + 1):
            lo, hi = min(u, v), max(u, v)
            inside[v, u] = hi <= int(round(math.sqrt(r * r - lo * lo)))
    hw = [int(np.nonzero(inside[v])[0].max()) for v in range(r + 1)]
    assert all(inside[v, :hw[v] + 1].all() for v in range(r + 1))
    return hw


DISC = disc_half_widths()


def moments(level, x, y):
    """(m10, m01) = sum of u I and of v I over the disc centred on (x, y), Python integers"""
    a = np.asarray(level).astype(np.int64)
    m10 = m01 = 0
    for v in range(-HALF_PATCH, HALF_PATCH + 1):
        d = DISC[abs(v)]
        row = a[y + v, x - d:x + d + 1]
        m10 += int((np.arange(-d, d + 1) * row).sum())
        m01 += v * int(row.sum())
    return m10, m01


def angle_exact(m10, m01):
    """atan2(m01, m10) in float64, degrees in [0, 360)"""
    a = math.degrees(math.atan2(float(m01), float(m10)))
    if a < 0:
        a += 360.0
    return 0.0 if a >= 360.0 else a


def moment_class(m10, m01):
    """sign / ordering class of a moment pair: the eight open octants '+x+y>' ... (sign of m10, sign of m01, '>' when |m10| >
    |m01|), the four axes, the four diagonals and 'zero'"""
    if m10 == 0 and m01 == 0:
        return "zero"
    sx = "+x" if m10 > 0 else "-x" if m10 < 0 else "0x"
    sy = "+y" if m01 > 0 else "-y" if m01 < 0 else "0y"
    o = ">" if abs(m10) > abs(m01) else "<" if abs(m10) < abs(m01) else "="
    return sx + sy + o


def exact_angle_of(m10, m01):
    """the angle a zero moment fixes exactly, else None"""
    if m01 == 0:
        return 0.0 if m10 >= 0 else 180.0
    if m10 == 0:
        return 90.0 if m01 > 0 else 270.0
    return None


def check_angles(angles, moment_pairs, what):
    """asserts of angles (float32, degrees) given the plain moments [(m10, m01)]: exactly 0 / 90 / 180 / 270 where a moment is
    exactly zero (0 for (0, 0)), within ANGLE_BOUND of atan2 elsewhere; returns the largest error"""
    worst = 0.0
    for a, (m10, m01) in zip(angles, moment_pairs):
        exact = exact_angle_of(m10, m01)
        if exact is not None:
            assert float(a) == exact, (what, m10, m01, float(a))
        else:
            e = abs(float(a) - angle_exact(m10, m01))
            worst = max(worst, min(e, 360.0 - e))
    assert worst <= ANGLE_BOUND, (what, worst)
    return worst


def _pack(bits):
    return np.packbits(bits.astype(np.uint8), bitorder="little")


def brief_bits(blurred, x, y, angle_f32):
    """(desc_a, desc_b, near_half): the 256 tests blurred[tap0] < blurred[tap1] as 32 bytes (bit b of byte i = test 8 i + b),
    taps rotated by the angle (degrees)
      (a) in float32, one rounded operation at a time: rad = angle * (float)(pi / 180), c = (float)cos(rad), s = (float)sin(rad)
          (cos and sin of the float32 angle taken in float64), fx = px c - py s, fy = px s + py c, rounded half-to-even;
      (b) in float64 throughout, from the same float32 angle;
    near_half[256]: tests with a float64 tap coordinate within 1e-4 of a half-integer (where (a) and (b) may round apart)"""
    b = np.asarray(blurred)
    ang = np.float32(angle_f32)
    rad32 = np.float32(ang * np.float32(math.pi / 180.0))
    c32, s32 = np.float32(math.cos(float(rad32))), np.float32(math.sin(float(rad32)))
    p32 = PATTERN.astype(np.float32)
    out = []
    for k in (0, 2):
        px, py = p32[:, k], p32[:, k + 1]
        fx = (px * c32).astype(np.float32) - (py * s32).astype(np.float32)
        fy = (px * s32).astype(np.float32) + (py * c32).astype(np.float32)
        assert fx.dtype == np.float32 and fy.dtype == np.float32
        out.append(b[y + np.rint(fy).astype(np.int64), x + np.rint(fx).astype(np.int64)].astype(np.int64))
    desc_a = _pack(out[0] < out[1])
    rad = math.radians(float(ang))
    c, s = math.cos(rad), math.sin(rad)
    p = PATTERN.astype(np.float64)
    out, near = [], np.zeros(256, bool)
    for k in (0, 2):
        fx, fy = p[:, k] * c - p[:, k + 1] * s, p[:, k] * s + p[:, k + 1] * c
        for v in (fx, fy):
            near |= np.abs(np.abs(v - np.floor(v)) - 0.5) <= 1e-4
        out.append(b[y + np.rint(fy).astype(np.int64), x + np.rint(fx).astype(np.int64)].astype(np.int64))
    return desc_a, _pack(out[0] < out[1]), near


def sobel_sums(level, x, y):
    """(a, b, c) = sums of Ix^2, Iy^2, Ix Iy over the 7 x 7 block centred on (x, y), 3 x 3 Sobel gradients, Python integers"""
    p = np.asarray(level).astype(np.int64)[y - 4:y + 5, x - 4:x + 5]
    ix = (p[1:-1, 2:] - p[1:-1, :-2]) * 2 + (p[:-2, 2:] - p[:-2, :-2]) + (p[2:, 2:] - p[2:, :-2])
    iy = (p[2:, 1:-1] - p[:-2, 1:-1]) * 2 + (p[2:, :-2] - p[:-2, :-2]) + (p[2:, 2:] - p[:-2, 2:])
    return int((ix * ix).sum()), int((iy * iy).sum()), int((ix * iy).sum())


def harris_f64(level, x, y):
    """det M - 0.04 trace(M)^2 of the block's gradient matrix, scaled by (1 / (4 * 7 * 255))^4; the integer part exactly, then
    float64"""
    a, b, c = sobel_sums(level, x, y)
    return (float(a * b - c * c) - HARRIS_K * float((a + b) * (a + b))) * HARRIS_SCALE


def unpack_bits(desc):
    """[n, 32] descriptor bytes -> [n, 256] bits in test order"""
    return np.unpackbits(np.asarray(desc, np.uint8), axis=-1, bitorder="little")
