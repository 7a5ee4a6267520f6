"""SIFT's stages after the scale space restated plainly in numpy (float64), from the operator's definitions: the 26-neighbour
extrema of the difference of Gaussians, the quadratic (Newton) fit with its contrast and edge tests, the 36-bin orientation
histogram, the 4 x 4 x 8 descriptor and the final order.  Shares no code with the oracle or the kernels and imports neither;
tests/test_oracle_sift_edges.py holds the oracle to it, tests/test_gpu_sift_edges.py the device.

The input is a Gaussian pyramid: a list of octaves of six float32 layers [6, h, w].  The sides under test work in float32, this
file in float64, so every branch they take is compared only where its MARGIN exceeds an ERROR BAR derived below from float32
rounding analysis; the rest is `undecided` and compared on neither side.  EPS32 = 2^-23 is twice float32's unit roundoff: the
bars are first-order bounds in the unit roundoff written with EPS32, and that factor of two covers the second-order terms."""
import hashlib
import math

import numpy as np

EPS32 = 2.0 ** -23
FLT_EPSILON = EPS32
BORDER = 5
MAX_STEPS = 5
LAYERS = 3
SIGMA = 1.6
CONTRAST = 0.04
EDGE_R = 10.0
INT_MAX_3 = float((2 ** 31 - 1) // 3)
# fastAtan2 against atan2: the largest error measured is 0.009552 degrees over both branches and all quadrants
# (tests/test_oracle_sift_edges.py::test_fast_atan2_error_is_the_polynomials measures it again at the magnitudes of float
# gradients); the bound is twice that -- the same figure as describe_checks.ANGLE_BOUND, asserted equal there
ANGLE_BOUND = 2 * 0.009552
# hal::exp32f against exp: relative error at most 4e-7 (tests/test_oracle_ops.py, asserted again in test_oracle_sift_edges.py)
EXP_REL = 4e-7
# the rotated window coordinates c_rot, r_rot of the descriptor in float32: the angle ori * (float)(pi / 180) carries two roundings
# of a value below 2 pi (4 pi EPS32 = 1.5e-6 rad), cos / sin, the division by hist_width and the two products and one sum of
# j cos - i sin five more (5 EPS32 = 6e-7 relative); |(j, i)| / hist_width <= 2.5 sqrt(2) = 3.6, so
# |delta| <= 3.6 * (1.5e-6 + 6e-7) = 7.6e-6
ROT_SLACK = 7.6e-6
# bin = round((36 / 360.f) * Ori) in float32: the constant's rounding and the product's move the bin by at most 2 * 36 EPS32 bins
# = 8.6e-5 degrees of Ori; rounded up to
BIN_SLACK_DEG = 1e-4
# Limits of the enumeration of a fit's alternatives (no tolerances: beyond them a candidate is `wild`, hence undecided, and its
# octave's records are counted, not judged).  A component whose bar reaches a quarter sample can round to more than two values;
# five steps of at most 2^3 alternatives each are cut off at 64 outcomes.
WILD_BAR = 0.25
WILD_OUTCOMES = 64


# ---------------------------------------------------------------------------------------------------------------- extrema
def dog(octave):
    """D[l] = G[l + 1] - G[l], l = 0 .. 4: one float32 subtraction each, the same IEEE operation on every side"""
    g = np.asarray(octave, np.float32)
    d = g[1:] - g[:-1]
    assert d.dtype == np.float32
    return d


def extrema(pyr):
    """[(octave, layer, row, col)] in scan order: |D| > floor(0.5 * 0.04 / 3 * 255), D >= (maxima, D > 0) or <= (minima, D < 0)
    all 26 neighbours, layers 1 .. 3, 5 pixels off every border.  Comparisons of float32 values: exact, no tolerance."""
    thr = math.floor(0.5 * CONTRAST / LAYERS * 255)
    out = []
    for o, octave in enumerate(pyr):
        d = dog(octave)
        h, w = d.shape[1:]
        if h <= 2 * BORDER or w <= 2 * BORDER:
            continue
        for l in range(1, LAYERS + 1):
            v = d[l, BORDER:h - BORDER, BORDER:w - BORDER]
            hi = np.full(v.shape, -np.inf, np.float32)
            lo = np.full(v.shape, np.inf, np.float32)
            for s in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        nb = d[l + s, BORDER + dy:h - BORDER + dy, BORDER + dx:w - BORDER + dx]
                        hi = np.maximum(hi, nb); lo = np.minimum(lo, nb)
            ok = (np.abs(v) > thr) & (((v > 0) & (v >= hi)) | ((v < 0) & (v <= lo)))
            rr, cc = np.nonzero(ok)
            out.extend((o, l, int(r) + BORDER, int(c) + BORDER) for r, c in zip(rr, cc))
    return out


# ----------------------------------------------------------------------------------------------------------------- refine
_PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))


def _perm_abs(m):
    """sum over the six permutations of |m[0, p0] m[1, p1] m[2, p2]|: the size of the terms a 3 x 3 determinant sums"""
    a = np.abs(m)
    return float(sum(a[0, p[0]] * a[1, p[1]] * a[2, p[2]] for p in _PERMS))


def _system(d, l, r, c):
    """gradient g and Hessian H of D at (l, r, c) in the order (x, y, s), central differences of the float32 values taken in
    float64 and scaled by 1 / 255, the value v / 255 and E, the bound of the error of one float32 entry:
    an entry is a sum of at most four values (three additions) times a scale (one product), every rounding relative to at most the
    sum of the magnitudes <= 4 Dmax: E = 4 * EPS32 * 4 * Dmax / 255.  (The scales are 1.f / 255 times a power of two: that
    constant's own rounding multiplies H and g alike and leaves the solution alone.)"""
    q = d[l - 1:l + 2, r - 1:r + 2, c - 1:c + 2].astype(np.float64)
    v = q[1, 1, 1]
    g = np.array([(q[1, 1, 2] - q[1, 1, 0]) / 2, (q[1, 2, 1] - q[1, 0, 1]) / 2, (q[2, 1, 1] - q[0, 1, 1]) / 2]) / 255
    dxx = q[1, 1, 2] + q[1, 1, 0] - 2 * v
    dyy = q[1, 2, 1] + q[1, 0, 1] - 2 * v
    dss = q[2, 1, 1] + q[0, 1, 1] - 2 * v
    dxy = (q[1, 2, 2] - q[1, 2, 0] - q[1, 0, 2] + q[1, 0, 0]) / 4
    dxs = (q[2, 1, 2] - q[2, 1, 0] - q[0, 1, 2] + q[0, 1, 0]) / 4
    dys = (q[2, 2, 1] - q[2, 0, 1] - q[0, 2, 1] + q[0, 0, 1]) / 4
    hm = np.array([[dxx, dxy, dxs], [dxy, dyy, dys], [dxs, dys, dss]]) / 255
    return g, hm, v / 255, 16 * EPS32 * float(np.abs(q).max()) / 255


def _solve(g, hm, e):
    """-> (x, bar, det, det_bar, cond): x = -H^-1 g by numpy.linalg.solve, and per component the bar of the float32 Cramer's rule.

    Derivation.  (1) The entries of H and g carry an absolute error <= E (see _system); to first order that moves x_i by at most
    sum_j |H^-1|_ij E (|x|_1 + 1).  (2) Cramer's rule forms every determinant as products of products: an expression five
    operations deep (product, difference, product, sum, sum), so its error is at most 5 EPS32 times the sum of the magnitudes of
    its six triple products, perm|M|; x_i = N_i (1 / det) adds two roundings.  Hence
        bar_i = sum_j |H^-1|_ij E (|x|_1 + 1)  +  5 EPS32 (perm|H_i| + |x_i| perm|H|) / |det|  +  2 EPS32 |x_i|.
    In the words of a condition number: perm|H| / |det| and |H^-1| |H| are both at most 6 kappa_inf(H) up to the cancellation
    inside the 2 x 2 minors, so the bar is of the form K EPS32 kappa |x| with K = 5 * 6 + 2 + 16 * 4 -- but Cramer's rule for
    n = 3 is not bounded by kappa alone, so the terms are evaluated as they stand, in float64, not through kappa.
    det_bar = 5 EPS32 perm|H| + E sum|adj H| is the bar of the decision det != 0."""
    det = float(np.linalg.det(hm))
    perm = _perm_abs(hm)
    adj = np.array([[abs(float(np.linalg.det(np.delete(np.delete(hm, i, 0), j, 1)))) for j in range(3)] for i in range(3)])
    det_bar = 5 * EPS32 * perm + e * float(adj.sum())
    if det == 0 or not np.isfinite(det):
        return np.zeros(3), np.full(3, np.inf), 0.0, det_bar, np.inf
    try:
        x = np.linalg.solve(hm, -g)
        inv = np.linalg.inv(hm)
    except np.linalg.LinAlgError:
        return np.zeros(3), np.full(3, np.inf), 0.0, det_bar, np.inf
    bar = np.zeros(3)
    for i in range(3):
        hi = hm.copy(); hi[:, i] = g
        bar[i] = (float(np.abs(inv[i]).sum()) * e * (float(np.abs(x).sum()) + 1)
                  + 5 * EPS32 * (_perm_abs(hi) + abs(x[i]) * perm) / abs(det) + 2 * EPS32 * abs(x[i]))
    return x, bar, det, det_bar, float(np.linalg.cond(hm, np.inf))


def _finish(d, o, l, r, c, x, bar, e, note=None):
    """the contrast test, the edge test and the record at the sample the fit stopped on -> (status, decided, record or None).

    contr = v / 255 + (g . x) / 2: three products and three sums, a halving, one sum.  bar_c = sum(|g_i| bar_i + E |x_i|) / 2
    + 2 EPS32 sum|g_i x_i| + 2 EPS32 |v| / 255 + EPS32 |contr|.  The test |contr| * 3 >= (float)0.04 adds one product and the
    rounding of 0.04: its bar is 3 bar_c + 2 EPS32 * 0.04.
    Edge test on tr = dxx + dyy, det = dxx dyy - dxy^2 (entries within E): bar_det = E (|dxx| + |dyy| + 2 |dxy|) + 3 EPS32 (|dxx dyy|
    + dxy^2) for det <= 0, and for q = 10 tr^2 - 121 det: bar_q = 10 (4 E |tr| + 4 EPS32 tr^2) + 121 (bar_det + 2 EPS32 |det|)."""
    g, hm, v, _ = _system(d, l, r, c)
    contr = v + 0.5 * float(g @ x)
    bar_c = (0.5 * float((np.abs(g) * bar + e * np.abs(x)).sum()) + 2 * EPS32 * float(np.abs(g * x).sum())
             + 2 * EPS32 * abs(v) + EPS32 * abs(contr))
    decided = abs(abs(contr) * LAYERS - CONTRAST) > 3 * bar_c + 2 * EPS32 * CONTRAST
    if note is not None:
        note["contr"] = contr
    if abs(contr) * LAYERS < CONTRAST:
        return "contrast", decided, None
    dxx, dyy, dxy = hm[0, 0], hm[1, 1], hm[0, 1]
    tr, det2 = dxx + dyy, dxx * dyy - dxy * dxy
    bar_det = e * (abs(dxx) + abs(dyy) + 2 * abs(dxy)) + 3 * EPS32 * (abs(dxx * dyy) + dxy * dxy)
    decided = decided and abs(det2) > bar_det
    if det2 <= 0:
        return "edge_det", decided, None
    qv = EDGE_R * tr * tr - (EDGE_R + 1) ** 2 * det2
    bar_q = EDGE_R * (4 * e * abs(tr) + 4 * EPS32 * tr * tr) + (EDGE_R + 1) ** 2 * (bar_det + 2 * EPS32 * abs(det2))
    decided = decided and abs(qv) > bar_q
    if qv >= 0:
        return "edge_ratio", decided, None
    xc, xr, xi = (float(t) for t in x)
    scl = SIGMA * 2.0 ** ((l + xi) / LAYERS)              # the scale inside the octave; the record's size is scl * 2^octave * 2 / 2
    k = 2.0 ** o * 0.5                                    # octave 0 is the doubled image: the first octave counts as -1
    rec = dict(o=o, layer=l, r=r, c=c, xi=xi, xr=xr, xc=xc, scl=scl,
               x=(c + xc) * k, y=(r + xr) * k, size=scl * k * 2, response=abs(contr), byte=(xi + 0.5) * 255,
               # (c + xc) * 2^o: one sum, one product; 2^(..): the quotient by 3, the power rounded to float, two products
               bar_x=bar[0] * k + 2 * EPS32 * abs(c + xc) * k, bar_y=bar[1] * k + 2 * EPS32 * abs(r + xr) * k,
               rel_size=math.log(2.0) / LAYERS * (bar[2] + EPS32 * (l + abs(xi))) + 4 * EPS32,
               bar_response=bar_c, bar_byte=255 * bar[2])
    return "kp", decided, rec


def _walk(d, o, l, r, c, step, out, primary, state):
    """the Newton fit from (l, r, c): at most 5 steps; a step ends the fit when |x| < 0.5 in all three components, else moves
    the sample by the rounded x and leaves when a component exceeds INT_MAX / 3 or the sample leaves layers 1 .. 3 or the border.
    Every outcome reachable within the bars is appended to `out` as (status, decided, record, steps); the float64 path is the
    primary one (primary = True), and state['decided'] falls when a decision on it has a margin within its bar.
    state['wild'] rises when the alternatives are not enumerated: det != 0 undecided, a bar of a quarter sample or more (the
    rounded move then has more than two outcomes per component), or more than 64 outcomes.  These two figures limit the
    enumeration (WILD_BAR, WILD_OUTCOMES), they are no tolerances.  state['contr'] receives the contrast of the primary exit."""
    if step >= MAX_STEPS:
        out.append(("steps", primary, None, step, primary))
        return
    g, hm, _, e = _system(d, l, r, c)
    x, bar, det, det_bar, _ = _solve(g, hm, e)
    if abs(det) <= det_bar:
        # det != 0 is not decided: either x = 0 (the fit stops here) or anything
        if primary:
            state["decided"] = False
        state["wild"] = True
        if det == 0:
            st, dec, rec = _finish(d, o, l, r, c, np.zeros(3), np.zeros(3), e, state if primary else None)
            out.append((st, False, rec, step, primary))
            return
    if not np.all(np.isfinite(bar)) or bar.max() >= WILD_BAR:
        state["wild"] = True
        if primary:
            state["decided"] = False
    ax = np.abs(x)
    stop = bool(np.all(ax < 0.5))
    stop_sure = bool(np.all(ax + bar < 0.5))
    move_sure = bool(np.any(ax - bar >= 0.5))
    if primary and not (stop_sure or move_sure):
        state["decided"] = False
    if stop or not move_sure:
        p = primary and stop
        st, dec, rec = _finish(d, o, l, r, c, x, bar, e, state if p else None)
        if p and not dec:
            state["decided"] = False
        out.append((st, dec, rec, step, p))
    if stop_sure:
        return
    if np.any(ax - bar > INT_MAX_3) or not np.all(np.isfinite(x)):
        out.append(("overflow", True, None, step + 1, primary and not stop))
        return
    if np.any(ax + bar > INT_MAX_3) and primary:
        state["decided"] = False
    if state["wild"] and (not np.all(np.isfinite(bar)) or bar.max() >= WILD_BAR):
        if not stop:
            mv = np.rint(x).astype(np.int64)
            l2, r2, c2 = l + int(mv[2]), r + int(mv[1]), c + int(mv[0])
            _leave_or_go(d, o, l2, r2, c2, step, out, primary, state)
        return
    # the rounded move: a component within its bar of a half-integer may round either way
    opts = []
    for i in range(3):
        a = {int(np.rint(x[i] - bar[i])), int(np.rint(x[i])), int(np.rint(x[i] + bar[i]))}
        if abs(abs(x[i] - math.floor(x[i])) - 0.5) <= bar[i]:
            a |= {int(math.floor(x[i])), int(math.floor(x[i])) + 1}
        opts.append(sorted(a))
    main = tuple(int(t) for t in np.rint(x))
    if primary and not stop and any(len(a) > 1 for a in opts):
        state["decided"] = False
    for mc in opts[0]:
        for mr in opts[1]:
            for ml in opts[2]:
                p = primary and not stop and (mc, mr, ml) == main
                if mc == 0 and mr == 0 and ml == 0 and not p:
                    continue                  # no move: that is the stop outcome above (a primary 0.5 rounds to even and stays)
                _leave_or_go(d, o, l + ml, r + mr, c + mc, step, out, p, state)


def _leave_or_go(d, o, l, r, c, step, out, primary, state):
    h, w = d.shape[1:]
    if l < 1 or l > LAYERS:
        out.append(("layer", True, None, step + 1, primary))
    elif c < BORDER or c >= w - BORDER or r < BORDER or r >= h - BORDER:
        out.append(("border", True, None, step + 1, primary))
    elif primary or len(out) < WILD_OUTCOMES:
        _walk(d, o, l, r, c, step + 1, out, primary, state)
    else:
        state["wild"] = True


def refine(pyr, cand):
    """per candidate (octave, layer, row, col) a dict:
      status   the exit of the float64 fit: 'kp', 'layer', 'border', 'overflow', 'steps' (used up after 5), 'contrast',
               'edge_det' (det <= 0), 'edge_ratio'
      steps    the moves made before that exit
      decided  every decision on the way had a margin beyond its bar (_solve, _finish): |x| < 0.5 per step, the rounded move,
               det != 0, the contrast and the edge test
      rec      for 'kp' the record in float64 with its bars: x, y, size (rel_size relative), response, byte = (xi + 0.5) * 255
      contr    the contrast v / 255 + (g . x) / 2 where the fit stopped (None where it left before the contrast test)
      maybe    the records of every other outcome reachable within the bars;  wild: the alternatives could not be enumerated"""
    dogs = {}
    res = []
    for o, l, r, c in cand:
        if o not in dogs:
            dogs[o] = dog(pyr[o])
        out, state = [], dict(decided=True, wild=False)
        _walk(dogs[o], o, l, r, c, 0, out, True, state)
        prim = [t for t in out if t[4]]
        assert len(prim) == 1, (o, l, r, c, out)
        st, dec, rec, steps, _ = prim[0]
        res.append(dict(cand=(o, l, r, c), status=st, steps=steps, decided=bool(state["decided"] and dec and not state["wild"]),
                        rec=rec, maybe=[t[2] for t in out if t[2] is not None and not t[4]], wild=state["wild"],
                        contr=state.get("contr")))
    return res


# ------------------------------------------------------------------------------------------------------------ orientations
def _smooth(t):
    return ((np.roll(t, 2) + np.roll(t, -2)) / 16 + (np.roll(t, 1) + np.roll(t, -1)) * 4 / 16 + t * 6 / 16)


def orientations(pyr, rec):
    """the orientations of one refined key point `rec` (a record of refine) -> dict(radius, decided, peaks, hist):
    36 bins over the window of radius round(4.5 scl) around (c, r) in layer G[layer] of its octave, pixels with 0 < x < w - 1 and
    0 < y < h - 1, weight exp(-(i^2 + j^2) / (2 (1.5 scl)^2)) times the gradient magnitude into bin round(atan2 / 10 degrees);
    circular 1-4-6-4-1 smoothing; peaks are strict local maxima >= 0.8 max; bin = j + (l - r) / 2 / (l - 2 h + r), wrapped into
    [0, 36); angle = 360 - 10 bin, 360 -> 0.

    Exactness.  fastAtan2 is within ANGLE_BOUND of atan2, and (36 / 360.f) * Ori adds 36 EPS32 bins = 4e-5 degrees: a sample
    whose angle lies within ANGLE_BOUND + BIN_SLACK_DEG degrees of a bin edge is carried on BOTH bins as an interval [0, weight].  A
    weight's relative error is at most REL = EXP_REL + 4 EPS32 (exp32f; magnitude, exponent and product), a bin's float32 sum of n
    terms adds n EPS32, the smoothing 5 EPS32: every bin is an interval [lo (1 - rel), hi (1 + rel)], rel = REL + (n + 5) EPS32.
    The smoothing has positive weights, so it maps intervals to intervals.  The scale enters through sigma = 1.5 scl, known to
    rel_size: every weight is monotone in sigma, and moving sigma moves all bins together, so -- instead of widening every bin on
    its own, which forgets that -- the intervals are formed at sigma (1 - rel_size), sigma and sigma (1 + rel_size), and a test
    counts as holding only where it holds at all three.  A peak is `sure` when the three tests (above the left neighbour, above
    the right one, >= 0.8 max) hold over the whole intervals, impossible when one fails over the whole intervals, else `maybe`.
    The parabola's offset is monotone in each of its three arguments (its partial derivatives (r - h) / den^2, (h - l) / den^2,
    (l - r) / den^2 keep their sign where h > l, r), so its range is spanned by the eight corners: `tol` is the largest distance
    from the plain offset to a corner, over the three sigmas, in degrees, plus 360 * 4 EPS32 for the float32 evaluation.
    radius: undecided when 4.5 scl lies within 4.5 scl (rel_size + 2 EPS32) of a half-integer."""
    img = np.asarray(pyr[rec["o"]][rec["layer"]], np.float32)
    h, w = img.shape
    scl, px, py = rec["scl"], rec["c"], rec["r"]
    rv = 4.5 * scl
    radius = int(np.rint(rv))
    decided = abs(abs(rv - math.floor(rv)) - 0.5) > rv * (rec["rel_size"] + 2 * EPS32)
    ii, jj = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    y, x = py + ii, px + jj
    ok = (y > 0) & (y < h - 1) & (x > 0) & (x < w - 1)
    y, x, ii, jj = y[ok], x[ok], ii[ok], jj[ok]
    dx = (img[y, x + 1] - img[y, x - 1]).astype(np.float64)          # one float32 subtraction, then exact
    dy = (img[y - 1, x] - img[y + 1, x]).astype(np.float64)
    mag = np.hypot(dx, dy)
    ang = np.degrees(np.arctan2(dy, dx)) % 360.0
    ang[(dx == 0) & (dy == 0)] = 0.0
    pos = ang / 10.0
    b = np.rint(pos).astype(np.int64)
    edge = np.abs(np.abs(pos - np.floor(pos)) - 0.5) <= (ANGLE_BOUND + BIN_SLACK_DEG) / 10.0
    other = np.where(pos - np.floor(pos) >= 0.5, b - 1, b + 1)          # the bin across the near edge
    cnt = np.zeros(36)
    np.add.at(cnt, b % 36, 1); np.add.at(cnt, other[edge] % 36, 1)
    rel = EXP_REL + 4 * EPS32 + (cnt + 5) * EPS32

    def at(sig):
        wgt = np.exp(-(ii * ii + jj * jj) / (2 * sig * sig)) * mag
        lo, hi, plain = np.zeros(36), np.zeros(36), np.zeros(36)
        np.add.at(lo, b[~edge] % 36, wgt[~edge])
        np.add.at(hi, b % 36, wgt)
        np.add.at(hi, other[edge] % 36, wgt[edge])
        np.add.at(plain, b % 36, wgt)
        return _smooth(lo * (1 - rel)), _smooth(hi * (1 + rel)), _smooth(plain)

    sig = 1.5 * scl
    forms = [at(sig * (1 - rec["rel_size"])), at(sig), at(sig * (1 + rec["rel_size"]))]
    hist = forms[1][2]
    peaks = []
    for j in range(36):
        l, r = (j - 1) % 36, (j + 1) % 36
        if hist.max() <= 0:
            break
        if all(hi[j] <= lo[l] or hi[j] <= lo[r] or hi[j] < 0.8 * lo.max() * (1 - 2 * EPS32) for lo, hi, _ in forms):
            continue                                                   # cannot be a peak
        sure = all(lo[j] > hi[l] and lo[j] > hi[r] and lo[j] >= 0.8 * hi.max() * (1 + 2 * EPS32) for lo, hi, _ in forms)
        den = hist[l] - 2 * hist[j] + hist[r]
        if den >= 0:
            off, tol, sure = 0.0, 10.0, False
        else:
            off = 0.5 * (hist[l] - hist[r]) / den
            offs = []
            for lo, hi, _ in forms:
                for a in (lo[l], hi[l]):
                    for m in (lo[j], hi[j]):
                        for c in (lo[r], hi[r]):
                            dn = a - 2 * m + c
                            offs.append(0.5 * (a - c) / dn if dn < 0 else np.inf)
            if not np.all(np.isfinite(offs)):
                tol, sure = 10.0, False
            else:
                tol = 10.0 * max(max(offs) - off, off - min(offs)) + 360 * 4 * EPS32
        bn = (j + off) % 36.0
        angle = 360.0 - 10.0 * bn
        peaks.append(dict(bin=j, offset=off, wrapped=int(j + off < 0) - int(j + off >= 36), angle=0.0 if angle >= 360.0 else angle,
                          tol=tol, sure=bool(sure)))
    return dict(radius=radius, decided=bool(decided), peaks=peaks, hist=hist, flat=bool(hist.max() <= 0), cut=bool(ok.size != ok.sum()),
                zeros=int(((dx == 0) & (dy == 0)).sum()))


# -------------------------------------------------------------------------------------------------------------- descriptor
def unpack_octave(packed):
    """(octave with -1 for the doubled image, layer, byte) of the packed word"""
    o = int(packed) & 255
    return (o - 256 if o >= 128 else o), (int(packed) >> 8) & 255, (int(packed) >> 16) & 255


def descriptor(pyr, x, y, size, angle, packed):
    """the 128 values of one emitted record (float32 x, y, size, angle and the packed octave, exactly as emitted) BEFORE the
    final rounding -> dict(value[128], bound[128], decided, radius, samples, clipped):
    the point, the size and the layer of the record's own octave (unpack_octave; the scale is a power of two: exact);
    ori = 360 - angle (one float32 subtraction), 360 -> 0; radius round(3 scl sqrt(2) 2.5) capped by the image diagonal; over the
    FULL (2 radius + 1)^2 window the samples with -1 < rbin, cbin < 4 (rbin = r_rot + 1.5, the offsets turned by ori and divided
    by 3 scl) on an interior pixel; Gaussian weight exp(-(c_rot^2 + r_rot^2) / 8) times the gradient magnitude, shared trilinearly
    over the 6 x 6 spatial cells and, circularly, the 8 orientation bins of (atan2 - ori) / 45 degrees -- the two wrap-around bins
    fall on bins 0 and 1 by the modulus; the inner 4 x 4 x 8; norm, clip at 0.2 norm, 512 / max(norm', FLT_EPSILON).

    Bound of a byte.  The shares are continuous in rbin, cbin and obin (a trilinear weight vanishes where the operator's tests
    cut it off), so an input error moves weight, it never drops a sample.  obin carries fastAtan2's ANGLE_BOUND / 45 = 4.2e-4 bins
    (plus 4 EPS32 * 8 for its float32 evaluation), rbin and cbin carry ROT_SLACK, the sample weight a relative EXP_REL + 3
    ROT_SLACK (the exponent (c_rot^2 + r_rot^2) / 8 moves by at most 2 * 3.6 * sqrt(2) ROT_SLACK / 8 = 1.3 ROT_SLACK, its own
    three operations and the magnitude's by the rest) + 4 EPS32, a cell's float32 sum of n shares n EPS32.  With S the
    spatial share of every sample added to BOTH orientation bins it touches and T the plain magnitudes of the samples touching a
    cell:  err_hist = (ANGLE_BOUND / 45 + 32 EPS32) S + 2 ROT_SLACK T + (EXP_REL + 3 ROT_SLACK + (n + 4) EPS32) hist.
    Through the normalisation, to first order: the norm moves by at most e_norm = sum(dst_i err_i) / norm (the values are not
    negative); a clipped value is 0.2 norm and moves with it, by 0.2 e_norm, an unclipped one by its own err_k, one within these
    of the clip by the larger of the two: err_clip_k.  The second norm moves by at most e_norm' = sum(val_i err_clip_i) / norm', so
    bound_k = 512 err_clip_k / norm' + value_k e_norm' / norm' + (128 + 8) EPS32 value_k.
    A byte may differ from rint(value) only where value lies within bound of a half-integer, and then by 1.
    decided: round(ptx), round(pty) are roundings of exact products (slack EPS32 of the value), the radius of three float32
    products (slack 4 EPS32 of the value); the record is undecided when one lies within its slack of a half-integer."""
    oct_, layer, _ = unpack_octave(packed)
    scale = 2.0 ** -oct_
    img = np.asarray(pyr[oct_ + 1][layer], np.float32)
    rows, cols = img.shape
    ptx, pty, scl = float(x) * scale, float(y) * scale, float(size) * scale * 0.5
    ori32 = np.float32(360.0) - np.float32(angle)
    ori = float(ori32)
    if abs(ori - 360.0) < FLT_EPSILON:
        ori = 0.0
    hw = 3.0 * scl
    rv = hw * math.sqrt(2.0) * 2.5
    half = lambda v, s: abs(abs(v - math.floor(v)) - 0.5) <= s
    decided = not (half(ptx, EPS32 * abs(ptx)) or half(pty, EPS32 * abs(pty)) or half(rv, 4 * EPS32 * rv))
    px, py = int(np.rint(ptx)), int(np.rint(pty))
    radius = min(int(np.rint(rv)), int(math.sqrt(float(cols) * cols + float(rows) * rows)))
    ct, st = math.cos(math.radians(ori)) / hw, math.sin(math.radians(ori)) / hw
    ii, jj = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    c_rot, r_rot = jj * ct - ii * st, jj * st + ii * ct
    rbin, cbin = r_rot + 1.5, c_rot + 1.5
    r, c = py + ii, px + jj
    ok = (rbin > -1) & (rbin < 4) & (cbin > -1) & (cbin < 4) & (r > 0) & (r < rows - 1) & (c > 0) & (c < cols - 1)
    r, c, rbin, cbin, c_rot, r_rot = r[ok], c[ok], rbin[ok], cbin[ok], c_rot[ok], r_rot[ok]
    dx = (img[r, c + 1] - img[r, c - 1]).astype(np.float64)
    dy = (img[r - 1, c] - img[r + 1, c]).astype(np.float64)
    th = np.degrees(np.arctan2(dy, dx)) % 360.0
    th[(dx == 0) & (dy == 0)] = 0.0
    mag = np.hypot(dx, dy) * np.exp(-(c_rot * c_rot + r_rot * r_rot) / 8.0)
    obin = (th - ori) / 45.0
    r0, c0, o0 = np.floor(rbin).astype(np.int64), np.floor(cbin).astype(np.int64), np.floor(obin).astype(np.int64)
    fr, fc, fo = rbin - r0, cbin - c0, obin - o0
    hist, sens, tot, cnt = (np.zeros((6, 6, 8)) for _ in range(4))
    for ar, wr in ((0, 1 - fr), (1, fr)):
        for ac, wc in ((0, 1 - fc), (1, fc)):
            for ao, wo in ((0, 1 - fo), (1, fo)):
                idx = (r0 + 1 + ar, c0 + 1 + ac, (o0 + ao) % 8)
                np.add.at(hist, idx, mag * wr * wc * wo)
                np.add.at(sens, idx, mag * wr * wc)
                np.add.at(tot, idx, mag)
                np.add.at(cnt, idx, 1)
    inner = lambda a: a[1:5, 1:5, :].reshape(128)
    dst = inner(hist)
    err = ((ANGLE_BOUND / 45.0 + 32 * EPS32) * inner(sens) + 2 * ROT_SLACK * inner(tot)
           + (EXP_REL + 3 * ROT_SLACK + (inner(cnt) + 4) * EPS32) * dst)
    norm = math.sqrt(float((dst * dst).sum()))
    thr = 0.2 * norm
    clipped = dst > thr
    val = np.minimum(dst, thr)
    e_norm = float((dst * err).sum()) / max(norm, FLT_EPSILON)
    err_clip = np.where(clipped, 0.2 * e_norm, err)
    err_clip = np.where(np.abs(dst - thr) <= err + 0.2 * e_norm, np.maximum(err, 0.2 * e_norm), err_clip)
    n2 = max(math.sqrt(float((val * val).sum())), FLT_EPSILON)
    e2 = float((val * err_clip).sum()) / n2
    value = val * 512.0 / n2
    bound = 512.0 * err_clip / n2 + value * e2 / n2 + 136 * EPS32 * value
    return dict(value=value, bound=bound, decided=decided, radius=radius, samples=int(ok.sum()), clipped=int(clipped.sum()),
                ori=ori, sides=(px - radius < 1, py - radius < 1, px + radius > cols - 2, py + radius > rows - 2),
                capped=radius < int(np.rint(rv)))


def check_descriptor(desc, d, what):
    """asserts the byte rule for one descriptor `desc` (128 values 0 .. 255) given descriptor()'s `d`; returns the number of
    bytes that differ from rint(value) (all of them within their bound of a half-integer)"""
    want = np.clip(np.rint(d["value"]), 0, 255)
    got = np.asarray(desc, np.float64)
    diff = got - want
    near = np.abs(np.abs(d["value"] - np.floor(d["value"])) - 0.5) <= d["bound"]
    near |= (d["value"] >= 255.5 - d["bound"]) & (d["value"] <= 255.5 + d["bound"])
    bad = (diff != 0) & ~(near & (np.abs(diff) == 1))
    assert not bad.any(), "%s: bytes %s are %s, the values %s (bounds %s)" % (
        what, np.nonzero(bad)[0].tolist(), got[bad].tolist(), d["value"][bad].tolist(), d["bound"][bad].tolist())
    return int((diff != 0).sum())


# -------------------------------------------------------------------------------------------------------------- final order
def _order_key(t):
    return (t[0], t[1], -t[2], t[3], -t[4], -t[5])


def final_order(records):
    """records: (x, y, size, angle, response, packed octave) as exact float32 / integer values -> sorted by (x, y, size
    descending, angle, response descending, octave descending), then every record dropped that equals the last kept one in
    (x, y, size, angle).  Exact on exact values."""
    out = []
    for t in sorted(records, key=_order_key):
        if not out or t[:4] != out[-1][:4]:
            out.append(t)
    return out


def records_of(kp):
    """the emitted dict (xy, size, angle, response, octave) as a list of tuples of Python numbers (float32 values exactly)"""
    return [(float(kp["xy"][i, 0]), float(kp["xy"][i, 1]), float(kp["size"][i]), float(kp["angle"][i]), float(kp["response"][i]),
             int(kp["octave"][i])) for i in range(len(kp["xy"]))]


def check_order(kp, what):
    """the emitted list is strictly increasing under the comparator, no two neighbours are equal in (x, y, size, angle), and
    final_order leaves it as it is"""
    rec = records_of(kp)
    for a, b in zip(rec, rec[1:]):
        assert _order_key(a) < _order_key(b), (what, a, b)
        assert a[:4] != b[:4], (what, a, b)
    assert final_order(rec) == rec, what


# ----------------------------------------------------------------------------------------------------- the whole reference
_CACHE = {}


def reference(pyr):
    """extrema -> refine -> orientations of a pyramid, computed once per pyramid CONTENT (keyed by a digest of its bytes: a
    device pyramid that equals another bit for bit shares the entry).  -> dict(cand, fits, ori): ori[k] for the fits with a
    record.  Treat as read-only."""
    hsh = hashlib.sha1()
    for octave in pyr:
        a = np.ascontiguousarray(octave, np.float32)
        hsh.update(repr(a.shape).encode()); hsh.update(a.tobytes())
    key = hsh.hexdigest()
    if key not in _CACHE:
        cand = extrema(pyr)
        fits = refine(pyr, cand)
        ori = {k: orientations(pyr, f["rec"]) for k, f in enumerate(fits) if f["rec"] is not None}
        _CACHE[key] = dict(cand=cand, fits=fits, ori=ori)
    return _CACHE[key]


def sample_of(rec_tuple):
    """(octave index, layer, row, col) of an emitted record: its point in the octave's own pixels, rounded"""
    x, y, _, _, _, packed = rec_tuple
    oct_, layer, _ = unpack_octave(packed)
    s = 2.0 ** -oct_
    return oct_ + 1, layer, int(np.rint(y * s)), int(np.rint(x * s))


def _angle_gap(a, b):
    d = abs(a - b) % 360.0
    return min(d, 360.0 - d)


def check_keypoints(pyr, kp, what):
    """holds an emitted key-point list to the reference of `pyr`:
      * every decided reference key point (decided fit, decided radius, sure peak) is present: a record on its sample whose x, y,
        size, response and octave byte lie within the fit's bars and whose angle lies within the peak's tolerance;
      * nothing extra: every emitted record sits on the sample of a reference record, decided or undecided or reachable within the
        bars (`maybe`), and -- where that fit is decided -- its angle is one of the peaks the reference holds possible; a record in
        an octave with a `wild` candidate (alternatives not enumerable) is counted, not judged;
      * the order (check_order).
    Returns dict(present, judged, unjudged, worst, worst_what): counts, the largest error in units of its bar, and
    the quantity and candidate that has it."""
    ref = reference(pyr)
    emitted = records_of(kp)
    check_order(kp, what)
    by_sample = {}
    for i, t in enumerate(emitted):
        by_sample.setdefault(sample_of(t), []).append(i)
    worst, worst_what, present = 0.0, None, 0
    sure_samples, maybe_samples, wild_octaves = {}, set(), set()
    for k, f in enumerate(ref["fits"]):
        if f["wild"]:
            wild_octaves.add(f["cand"][0])
        for m in f["maybe"]:
            maybe_samples.add((m["o"], m["layer"], m["r"], m["c"]))
        rec = f["rec"]
        if rec is None:
            continue
        s = (rec["o"], rec["layer"], rec["r"], rec["c"])
        o = ref["ori"][k]
        if not (f["decided"] and o["decided"]):
            maybe_samples.add(s)
            continue
        sure_samples.setdefault(s, []).append(k)
        for p in o["peaks"]:
            if not p["sure"]:
                continue
            idx = by_sample.get(s, [])
            assert idx, "%s: the key point of candidate %s on sample %s (angle %.3f) is missing" % (what, f["cand"], s, p["angle"])
            i = min(idx, key=lambda i: _angle_gap(emitted[i][3], p["angle"]))
            x, y, size, angle, resp, packed = emitted[i]
            errs = dict(x=abs(x - rec["x"]) / (rec["bar_x"] + EPS32 * abs(x)), y=abs(y - rec["y"]) / (rec["bar_y"] + EPS32 * abs(y)),
                        size=abs(size / rec["size"] - 1) / rec["rel_size"], response=abs(resp - rec["response"]) / (rec["bar_response"] + EPS32 * resp),
                        angle=_angle_gap(angle, p["angle"]) / p["tol"],
                        byte=abs(unpack_octave(packed)[2] - rec["byte"]) / (0.5 + rec["bar_byte"]))
            for name, e in errs.items():
                assert e <= 1.0, "%s: candidate %s sample %s: %s off by %.3g bars (emitted %r, reference %r, peak %r)" % (
                    what, f["cand"], s, name, e, emitted[i], {a: rec[a] for a in ("x", "y", "size", "response", "byte")}, p)
                if e > worst:
                    worst, worst_what = e, (name, f["cand"])
            present += 1
    judged = unjudged = 0
    for t in emitted:
        s = sample_of(t)
        if s in sure_samples:
            ok = False
            for k in sure_samples[s]:
                ok = ok or any(_angle_gap(t[3], p["angle"]) <= p["tol"] for p in ref["ori"][k]["peaks"])
            assert ok, "%s: the emitted record %r on sample %s has an angle the reference does not hold possible" % (what, t, s)
            judged += 1
        elif s in maybe_samples:
            judged += 1
        else:
            assert s[0] in wild_octaves, "%s: the emitted record %r on sample %s is not in the reference" % (what, t, s)
            unjudged += 1
    return dict(present=present, judged=judged, unjudged=unjudged, worst=worst, worst_what=worst_what)


def check_descriptors(pyr, kp, what):
    """every emitted descriptor against descriptor() of its own record; returns (records checked, undecided, bytes off by one,
    the largest bound)"""
    n = und = off = 0
    big = 0.0
    for i, t in enumerate(records_of(kp)):
        d = descriptor(pyr, t[0], t[1], t[2], t[3], t[5])
        if not d["decided"]:
            und += 1
            continue
        off += check_descriptor(kp["desc"][i], d, "%s record %d %r" % (what, i, t))
        big = max(big, float(d["bound"].max()))
        n += 1
    return n, und, off, big


def decided_shares(pyr):
    """(decided candidates, candidates, decided key points, key points) of the reference alone: a key point is a fit with a
    record, decided when the fit, the orientation radius and every possible peak are"""
    ref = reference(pyr)
    fits = ref["fits"]
    kps = [k for k, f in enumerate(fits) if f["rec"] is not None]
    dk = sum(1 for k in kps if fits[k]["decided"] and ref["ori"][k]["decided"] and all(p["sure"] for p in ref["ori"][k]["peaks"]))
    return sum(1 for f in fits if f["decided"]), len(fits), dk, len(kps)
