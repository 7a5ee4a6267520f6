"""The image front end in plain numpy: gray conversion, resize(INTER_AREA) in its four forms, resize(INTER_LINEAR_EXACT)
and ORB's eight level sizes, written from the published OpenCV 3.4 definitions (imgproc color.cpp / resize.cpp,
features2d orb.cpp).  It imports neither the oracle nor the library: tests/test_oracle_front_edges.py holds the oracle to
it on the CPU, tests/test_gpu_front_edges.py the kernels.

Two kinds of statement.
(a) The operator's own arithmetic, bit for bit: `gray`, `resize_area` (which picks among a copy, `area_int`,
    `area_tables` and `area_enlarge` through `area_form`), `linear_exact`, `orb_sizes`, `orb_pyramid`.
(b) The definition in float64 with a derived bound: `gray_true` / `GRAY_BOUND`, `area_true` / `area_bound`,
    `bilinear_true` / `LINEAR_BOUND`.  The bounds are derived in the docstrings, none is measured.

Images are uint8 arrays [h, w] or [h, w, cn]."""
import functools
import math

import numpy as np

F32 = np.float32
DBL_EPSILON = 2.220446049250313e-16


# ---------------------------------------------------------------------------------------------------------------- gray
def gray(bgr):
    """cvtColor(BGR2GRAY) on 8-bit pixels: 14-bit fixed point, Y = (B*1868 + G*9617 + R*4899 + 8192) >> 14."""
    p = bgr.astype(np.int64)
    return ((p[..., 0] * 1868 + p[..., 1] * 9617 + p[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def gray_true(bgr):
    """Y = 0.114 B + 0.587 G + 0.299 R in float64."""
    p = bgr.astype(np.float64)
    return 0.114 * p[..., 0] + 0.587 * p[..., 1] + 0.299 * p[..., 2]


# Each 14-bit weight is the rounded real one: it is off by at most half a unit of 2^-14, that is 2^-15, and multiplies a
# byte of at most 255: three of them move the sum by at most 3 * 255 * 2^-15.  The + 8192 >> 14 is round-half-up of the
# fixed-point sum: another 0.5.
GRAY_BOUND = 0.5 + 3 * 255 * 2.0 ** -15


# ------------------------------------------------------------------------------------------------------ INTER_AREA
def _scales(s, d):
    """resize() forms inv_scale = d / s in double and scale = 1 / inv_scale, in this order"""
    inv = float(d) / float(s)
    return 1.0 / inv, inv


def area_form(sw, sh, dw, dh):
    """Which of INTER_AREA's forms resize() takes, from the geometry alone: 'copy'; ('int', isx, isy) when both scales are
    >= 1 and within DBL_EPSILON of their rounded value; 'tables' when both are >= 1 otherwise; 'enlarge' as soon as one
    scale is below 1 (both axes then go through the bilinear machinery with area-mode coefficients)."""
    if (sw, sh) == (dw, dh):
        return "copy"
    sx, sy = _scales(sw, dw)[0], _scales(sh, dh)[0]
    if sx >= 1 and sy >= 1:
        ix, iy = int(np.rint(sx)), int(np.rint(sy))
        if abs(sx - ix) < DBL_EPSILON and abs(sy - iy) < DBL_EPSILON:
            return ("int", ix, iy)
        return "tables"
    return "enlarge"


def _as3(img):
    return img[:, :, None] if img.ndim == 2 else img


def _like(out, img):
    return out[:, :, 0] if img.ndim == 2 else out


def block_sums(img, isx, isy, dw, dh):
    """integer sums of the isx x isy source blocks, int64 [dh, dw, cn]"""
    a = _as3(img)[:dh * isy, :dw * isx].astype(np.int64)
    return a.reshape(dh, isy, dw, isx, a.shape[2]).sum(axis=(1, 3))


def area_int_product(sums, area):
    """the float32 product an integer-ratio block other than 2 x 2 is rounded from: float32(sum) * (1.f / area)"""
    return sums.astype(F32) * (F32(1.0) / F32(area))


def area_int(img, isx, isy, dw, dh):
    """Integer ratios: block sums in integers; 2 x 2 rounds as (s + 2) >> 2, every other block is
    rint(float32(s) * float32(1 / area)), half to even, saturated."""
    s = block_sums(img, isx, isy, dw, dh)
    if (isx, isy) == (2, 2):
        v = (s + 2) >> 2
    else:
        v = np.rint(area_int_product(s, isx * isy)).astype(np.int64)
    return _like(np.clip(v, 0, 255).astype(np.uint8), img)


def area_tab(ssize, dsize):
    """One axis of the fractional form: per destination index the list of (source index, float32 weight).  The cell of d is
    [d * scale, (d + 1) * scale); its width is cut at the source's end.  A partial pixel on either side enters only when
    it is wider than 1e-3; whole pixels weigh 1 / cell."""
    scale = _scales(ssize, dsize)[0]
    tab = []
    for d in range(dsize):
        f1 = d * scale
        f2 = f1 + scale
        cell = min(scale, ssize - f1)
        s1, s2 = int(math.ceil(f1)), int(math.floor(f2))
        s2 = min(s2, ssize - 1)
        s1 = min(s1, s2)
        e = []
        if s1 - f1 > 1e-3:
            e.append((s1 - 1, F32((s1 - f1) / cell)))
        for s in range(s1, s2):
            e.append((s, F32(1.0 / cell)))
        if f2 - s2 > 1e-3:
            e.append((s2, F32(min(min(f2 - s2, 1.0), cell) / cell)))
        tab.append(e)
    return tab


def _padded(tab):
    """a table as rectangular arrays: counts [d], source indices [d, kmax], float32 weights [d, kmax]"""
    cnt = np.array([len(e) for e in tab])
    si = np.zeros((len(tab), cnt.max()), np.int64)
    al = np.zeros((len(tab), cnt.max()), F32)
    for d, e in enumerate(tab):
        for k, (s, a) in enumerate(e):
            si[d, k], al[d, k] = s, a
    return cnt, si, al


def area_tables(img, dw, dh):
    """The fractional form.  Every operation is one float32 operation.  Inner sum: along a source row, the entries of a
    destination column in table order, buf = buf + float32(pixel) * alpha from buf = 0.  Outer sum: the rows of a
    destination row in table order, the first term beta * buf ASSIGNED, every later one added.  Then rint (half to even)
    and saturation."""
    a = _as3(img)
    sh, sw = a.shape[:2]
    xc, xs, xa = _padded(area_tab(sw, dw))
    yc, ys, ya = _padded(area_tab(sh, dh))
    buf = np.zeros((sh, dw, a.shape[2]), F32)
    for k in range(xs.shape[1]):
        m = xc > k
        buf[:, m] = buf[:, m] + a[:, xs[m, k]].astype(F32) * xa[m, k][None, :, None]
    out = np.zeros((dh, dw, a.shape[2]), F32)
    for k in range(ys.shape[1]):
        m = yc > k
        term = ya[m, k][:, None, None] * buf[ys[m, k]]
        out[m] = term if k == 0 else out[m] + term
    return _like(np.clip(np.rint(out), 0, 255).astype(np.uint8), img)


def _enlarge_axis(ssize, dsize):
    """Area-mode coefficients of the bilinear machinery for one axis: s = floor(d * scale),
    f = float32((d + 1) - (s + 1) * inv_scale), f = 0 where f <= 0, else f - floor(f); s < 0 and s >= ssize - 1 pin the tap
    to the edge with f = 0; the two coefficients are saturate_cast<short>((1 - f) * 2048) and (f * 2048), products in
    float32, rounded half to even.  `first_edge` is the first d with s + 1 >= ssize (xmax), dsize when there is none."""
    scale, inv = _scales(ssize, dsize)
    s_, c0, c1 = np.zeros(dsize, np.int64), np.zeros(dsize, np.int64), np.zeros(dsize, np.int64)
    first_edge = dsize
    for d in range(dsize):
        s = int(math.floor(d * scale))
        f = F32((d + 1) - (s + 1) * inv)
        f = F32(0) if f <= 0 else F32(f - np.floor(f))
        if s < 0:
            f, s = F32(0), 0
        if s + 1 >= ssize:
            first_edge = min(first_edge, d)
            if s >= ssize - 1:
                f, s = F32(0), ssize - 1
        s_[d] = s
        c0[d] = int(np.clip(np.rint((F32(1) - f) * F32(2048)), -32768, 32767))
        c1[d] = int(np.clip(np.rint(f * F32(2048)), -32768, 32767))
    return s_, c0, c1, first_edge


def area_enlarge(img, dw, dh):
    """INTER_AREA with a scale below 1 on either axis: the 8-bit bilinear resize with area-mode coefficients, in integers.
    Horizontal pass: S[s] * a0 + S[s + 1] * a1 for d < xmax, S[s] * 2048 from xmax on (the substitution).  The two source
    rows of a destination row are s and s + 1 CLIPPED to the image.  Vertical pass:
    (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2, saturated."""
    a = _as3(img).astype(np.int64)
    sh, sw = a.shape[:2]
    xs, a0, a1, xmax = _enlarge_axis(sw, dw)
    ys, b0, b1, _ = _enlarge_axis(sh, dh)
    a0, a1 = a0.copy(), a1.copy()
    a0[xmax:], a1[xmax:] = 2048, 0
    x1 = np.minimum(xs + 1, sw - 1)                       # read only where a1 != 0, i.e. below xmax, where s + 1 < sw
    hor = a[:, xs] * a0[None, :, None] + a[:, x1] * a1[None, :, None]
    r0, r1 = np.clip(ys, 0, sh - 1), np.clip(ys + 1, 0, sh - 1)
    v = (((b0[:, None, None] * (hor[r0] >> 4)) >> 16) + ((b1[:, None, None] * (hor[r1] >> 4)) >> 16) + 2) >> 2
    return _like(np.clip(v, 0, 255).astype(np.uint8), img)


def resize_area(img, dw, dh):
    """resize(img, (dw, dh), INTER_AREA)"""
    sh, sw = img.shape[:2]
    form = area_form(sw, sh, dw, dh)
    if form == "copy":
        return img.copy()
    if form == "tables":
        return area_tables(img, dw, dh)
    if form == "enlarge":
        return area_enlarge(img, dw, dh)
    return area_int(img, form[1], form[2], dw, dh)


def _true_axis(ssize, dsize):
    """float64 weights [dsize, ssize] of the true area mean over [d * scale, (d + 1) * scale) clipped to the source"""
    scale = float(ssize) / float(dsize)
    w = np.zeros((dsize, ssize))
    for d in range(dsize):
        lo, hi = d * scale, min((d + 1) * scale, float(ssize))
        for s in range(int(math.floor(lo)), min(int(math.ceil(hi)), ssize)):
            w[d, s] = max(0.0, min(hi, s + 1.0) - max(lo, float(s)))
        w[d] /= hi - lo
    return w


def area_true(img, dw, dh):
    """The definition of shrinking by area: the mean of the source over the destination pixel's cell, float64."""
    a = _as3(img).astype(np.float64)
    sh, sw = a.shape[:2]
    out = np.einsum("ys,sxc->yxc", _true_axis(sh, dh), np.einsum("xs,ysc->yxc", _true_axis(sw, dw), a))
    return _like(out, img)


def area_bound(sw, sh, dw, dh):
    """How far a shrinking form (integer ratios or tables) may lie from `area_true`.
      0.5                          the final rounding to a byte;
      255 * 2e-3 * (1/sx + 1/sy)   the table form drops a partial pixel of width <= 1e-3 on either side of a cell, so on
                                   an axis of scale s up to 2e-3 / s of the weight is missing, and a weight w missing
                                   moves a mean of bytes by at most 255 w (integer ratios drop nothing, the term only
                                   loosens their bound);
      255 * (nx + ny + 6) * 2^-24  float32: a sequential sum of n products of a byte and a rounded weight carries a
                                   relative error of at most (n + 2) u of the sum of the magnitudes, u = 2^-24 (one u for
                                   the weight, one for the product, n - 1 additions, to first order), the magnitudes sum
                                   to at most 255; nx = ceil(sx) + 2 and ny = ceil(sy) + 2 bound the entries of a cell
                                   (whole pixels plus two partial ones); the outer sum multiplies by beta once more.
                                   The integer-ratio product float32(sum) * float32(1 / area) has two roundings and
                                   is covered with room to spare."""
    sx, sy = float(sw) / dw, float(sh) / dh
    nx, ny = math.ceil(sx) + 2, math.ceil(sy) + 2
    return 0.5 + 255 * 2e-3 * (1 / sx + 1 / sy) + 255 * (nx + ny + 6) * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ INTER_LINEAR_EXACT
def linear_taps(ssize, dsize):
    """One axis of the bit-exact bilinear resize: the sample position of d is scale * (d + 0.5) - 0.5 in double.  Inside
    the source the taps are floor and floor + 1 with the 8.8 weight rint(fraction * 256) on the second (half to even) and
    256 minus it on the first; a position before the first sample (or a source of one sample) is the first sample at full
    weight, a position at or past the last sample is the last one at full weight.
    -> (i0, i1, w0, w1) with w0 + w1 == 256."""
    scale = _scales(ssize, dsize)[0]
    f = scale * (np.arange(dsize) + 0.5) - 0.5
    i = np.floor(f).astype(np.int64)
    inside = (i >= 0) & (i < ssize - 1) & (ssize > 1)
    last = (i >= 0) & (i >= ssize - 1) & (ssize > 1)
    i0 = np.where(inside, i, np.where(last, ssize - 1, 0))
    i1 = np.where(inside, i + 1, i0)
    w1 = np.where(inside, np.rint((f - i) * 256.0).astype(np.int64), 0)
    return i0, i1, 256 - w1, w1


def linear_exact_wide(img, dw, dh):
    """The 16.16 value of every destination pixel before the final rounding: horizontal pass in 8.8 (exact integers),
    vertical pass of the two 8.8 rows with 8.8 weights."""
    a = img.astype(np.int64)
    sh, sw = a.shape
    x0, x1, c0, c1 = linear_taps(sw, dw)
    y0, y1, m0, m1 = linear_taps(sh, dh)
    hor = a[:, x0] * c0[None, :] + a[:, x1] * c1[None, :]
    return hor[y0] * m0[:, None] + hor[y1] * m1[:, None]


def linear_exact(img, dw, dh):
    """resize(gray, (dw, dh), INTER_LINEAR_EXACT): (v + 32768) >> 16 of the 16.16 value"""
    return np.clip((linear_exact_wide(img, dw, dh) + 32768) >> 16, 0, 255).astype(np.uint8)


def bilinear_true(img, dw, dh):
    """Centre-aligned bilinear interpolation in float64, samples clamped to the image."""
    a = img.astype(np.float64)
    sh, sw = a.shape

    def axis(ssize, dsize):
        f = np.clip((np.arange(dsize) + 0.5) * (float(ssize) / dsize) - 0.5, 0.0, ssize - 1.0)
        i = np.minimum(np.floor(f).astype(np.int64), max(ssize - 2, 0))
        return i, np.minimum(i + 1, ssize - 1), f - i
    x0, x1, fx = axis(sw, dw)
    y0, y1, fy = axis(sh, dh)
    hor = a[:, x0] * (1 - fx)[None, :] + a[:, x1] * fx[None, :]
    return hor[y0] * (1 - fy)[:, None] + hor[y1] * fy[:, None]


# An 8.8 weight is the real one rounded to a multiple of 2^-8: off by at most 2^-9.  The horizontal pass is
# a + w (b - a) with |b - a| <= 255, so the weight's error moves it by at most 255 * 2^-9, and it is then held exactly (8.8
# times a byte is an integer).  The vertical pass does the same to two such values, themselves within [0, 255]: another
# 255 * 2^-9, plus the horizontal error carried through a convex combination unchanged.  (v + 32768) >> 16 rounds half up: 0.5.
LINEAR_BOUND = 0.5 + 2 * 255 * 2.0 ** -9


# ------------------------------------------------------------------------------------------------------------- ORB
NLEVELS = 8


@functools.lru_cache(maxsize=None)
def orb_sizes(w, h):
    """ORB_create() defaults: level l has scale float32(pow(double(1.2f), l)) and size cvRound(w / scale), cvRound(h / scale),
    the division in float32, the rounding half to even."""
    out = []
    for l in range(NLEVELS):
        s = F32(float(F32(1.2)) ** l)
        out.append((int(np.rint(F32(w) / s)), int(np.rint(F32(h) / s))))
    return tuple(out)


def orb_pyramid(gray_img):
    """Level 0 is the image; level l is resize(level l - 1, size of l, INTER_LINEAR_EXACT)."""
    h, w = gray_img.shape
    pyr = [gray_img]
    for (lw, lh) in orb_sizes(w, h)[1:]:
        pyr.append(linear_exact(pyr[-1], lw, lh))
    return pyr
