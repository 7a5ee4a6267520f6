"""SURF's stages restated plainly in numpy (float64), from the operator's definitions (opencv-contrib 3.4.2 SURF, 4 octaves x 3
layers, extended, rotation-aware): the integral image, the box-filter Hessian of the 20 layers, the strict 26-neighbour maxima
above the threshold, the quadratic fit, the deletion test, the dominant orientation, the 128-float descriptor and the final order.
Shares no code with the oracle or the kernels and imports neither; tests/test_oracle_surf_edges.py holds the oracle to it,
tests/test_gpu_surf_edges.py the device.

The input is the gray frame itself: the integral is exact integer arithmetic.  The sides under test work in float32, this file in
float64, so every branch they take is compared only where its MARGIN exceeds an ERROR BAR derived below from float32 rounding
analysis; the rest is `undecided`, counted, and compared on neither side.  EPS32 = 2^-23 is twice float32's unit roundoff u: the
bars are first-order bounds in u written with EPS32, and that factor of two covers the second-order terms.

Three scalars of a key point -- s = size * 1.2f / 9.0f, the wavelet side g = 2 round(2 s) and the window side int(21 s) -- and the
rounded positions of the 113 orientation samples are DEFINED by the operator as float32 expressions of a few operations; 21 s lies
exactly on an integer for every size that is a multiple of five, where no bar can decide it.  They are evaluated here as the
definition writes them, one IEEE float32 operation at a time (numpy.float32 scalars), and, beside that, in float64 with a bar: the
number of key points whose float64 value lies within the bar of the rounding is reported as `ties`, not hidden."""
import math
from fractions import Fraction

import numpy as np

from sift_checks import ANGLE_BOUND, EPS32, _solve   # fastAtan2's measured 0.009552 degrees, doubled; the Cramer's-rule bars

F32 = np.float32
OCTAVES, LAYERS = 4, 3
NL = OCTAVES * (LAYERS + 2)
THRESHOLD = 400.0
HESSIAN_W = 0.81
ORI_RADIUS, ORI_N = 6, 113
PATCH = 20
# a Haar value sums 2 .. 4 products (exact integer box sum) * (float32 weight), in double, and is rounded to float32 once: the
# weight carries one rounding (u), the product one (u), the final rounding one (u of the value <= u A), A = sum |box| |w|; the
# double sum adds 4 * 2^-53 A.  3 u A = 1.5 EPS32 A; written as
HAAR_K = 2.0
# an orientation / descriptor Gaussian weight is (float32 exp) * (float32 1 / sum) rounded (3 u), a product of two of them rounded
# once more: 7 u, written as
GAUSS_REL = 4 * EPS32

DXX = ((0, 2, 3, 7, 1), (3, 2, 6, 7, -2), (6, 2, 9, 7, 1))             # x1, y1, x2, y2, weight on the 9 x 9 pattern
DYY = tuple((y1, x1, y2, x2, w) for x1, y1, x2, y2, w in DXX)
DXY = ((1, 1, 4, 4, 1), (5, 1, 8, 4, -1), (1, 5, 4, 8, -1), (5, 5, 8, 8, 1))
GRAD_X = ((0, 0, 2, 4, -1), (2, 0, 4, 4, 1))                           # on a 4 x 4 pattern: right half minus left half
GRAD_Y = ((0, 0, 4, 2, 1), (0, 2, 4, 4, -1))                           # upper half minus lower half


def integral(img):
    """(h + 1) x (w + 1) sums of the pixels above and left, exact (int64)"""
    img = np.asarray(img)
    out = np.zeros((img.shape[0] + 1, img.shape[1] + 1), np.int64)
    out[1:, 1:] = img.astype(np.int64).cumsum(0).cumsum(1)
    return out


def layers():
    """[(octave, layer, size, step)] of the 20 Hessian layers"""
    return [(o, l, (9 + 6 * l) << o, 1 << o) for o in range(OCTAVES) for l in range(LAYERS + 2)]


def scaled_boxes(pattern, old, new):
    """the boxes of `pattern` scaled by new / old, corners rounded to the nearest integer, weight w / area as an exact rational.
    The layer sizes are 3 (3 + 2 l) 2^o, so a corner new * c / 9 has a fractional part of 0, 1/3 or 2/3, and the wavelet's side is
    even with corners on 0, 2, 4 of 4: no corner lies on a half, the rounding is decided (asserted)."""
    out = []
    for x1, y1, x2, y2, w in pattern:
        c = []
        for v in (x1, y1, x2, y2):
            q = Fraction(new * v, old)
            assert (q - math.floor(q)) != Fraction(1, 2)
            c.append(int(round(q)))
        area = (c[2] - c[0]) * (c[3] - c[1])
        out.append((c[0], c[1], c[2], c[3], Fraction(w, area)))
    return out


def _haar_grid(ii, boxes, size, step):
    """the Haar value of `boxes` with its top-left corner on every step-th sum sample where the size x size pattern fits:
    -> (value, A = sum |box| |w|), float64 [ni, nj]"""
    h, w = ii.shape[0] - 1, ii.shape[1] - 1
    ni, nj = 1 + (h - size) // step, 1 + (w - size) // step
    val = np.zeros((ni, nj))
    mag = np.zeros((ni, nj))

    def at(y, x):
        return ii[y:y + (ni - 1) * step + 1:step, x:x + (nj - 1) * step + 1:step]
    for x1, y1, x2, y2, wgt in boxes:
        s = (at(y2, x2) + at(y1, x1) - at(y1, x2) - at(y2, x1)).astype(np.float64)
        val += s * float(wgt)
        mag += np.abs(s) * abs(float(wgt))
    return val, mag


def hessian(img):
    """the 20 layers of a frame -> list of dict(octave, layer, size, step, built, det, trace, bar, tbar): planes of (h // step) x
    (w // step) samples, zero where the layer writes nothing; a layer is built when its size fits into the frame both ways; the
    sample (i, j) of a built layer holds the pattern whose top-left corner is the sum sample step (i - m, j - m), m = (size / 2)
    / step.

    det = Dxx Dyy - 0.81 Dxy^2 in float32 is four operations (two products for the second term, one for the first, the
    difference) on Haar values within e = HAAR_K EPS32 A of the exact ones, and 0.81f is within u of 0.81:
      bar = |Dyy| e_xx + |Dxx| e_yy + 2 * 0.81 |Dxy| e_xy + EPS32 (|Dxx Dyy| + 2 * 0.81 Dxy^2) + EPS32 |det|
    trace = Dxx + Dyy: tbar = e_xx + e_yy + EPS32 |trace|."""
    ii = integral(img)
    h, w = ii.shape[0] - 1, ii.shape[1] - 1
    out = []
    for o, l, size, step in layers():
        rows, cols = h // step, w // step
        L = dict(octave=o, layer=l, size=size, step=step, built=not (size > h or size > w),
                 det=np.zeros((max(rows, 0), max(cols, 0))), trace=None, bar=None, tbar=None)
        L["trace"], L["bar"], L["tbar"] = (np.zeros_like(L["det"]) for _ in range(3))
        if L["built"]:
            dxx, axx = _haar_grid(ii, scaled_boxes(DXX, 9, size), size, step)
            dyy, ayy = _haar_grid(ii, scaled_boxes(DYY, 9, size), size, step)
            dxy, axy = _haar_grid(ii, scaled_boxes(DXY, 9, size), size, step)
            exx, eyy, exy = (HAAR_K * EPS32 * a for a in (axx, ayy, axy))
            det = dxx * dyy - HESSIAN_W * dxy * dxy
            bar = (np.abs(dyy) * exx + np.abs(dxx) * eyy + 2 * HESSIAN_W * np.abs(dxy) * exy
                   + EPS32 * (np.abs(dxx * dyy) + 2 * HESSIAN_W * dxy * dxy) + EPS32 * np.abs(det))
            m = (size // 2) // step
            ni, nj = det.shape
            L["det"][m:m + ni, m:m + nj] = det
            L["bar"][m:m + ni, m:m + nj] = bar
            L["trace"][m:m + ni, m:m + nj] = dxx + dyy
            L["tbar"][m:m + ni, m:m + nj] = exx + eyy + EPS32 * np.abs(dxx + dyy)
        out.append(L)
    return out


# ------------------------------------------------------------------------------------------------------------ candidates
def _near_half(v, bar):
    return abs(abs(v - math.floor(v)) - 0.5) <= bar


def _fit(N, B, L, Lp, i, j):
    """the quadratic fit around sample (i, j) of the middle layer: N, B = the 3 x 3 x 3 values and bars in the order (layer, row,
    column).  -> (record or None, decided).  A x = b with A the second differences and b minus the first ones, x = (column, row,
    layer) offsets; accepted when x is not all zero and every |x_i| <= 1; then x, y move by x_i step from the centre of the
    pattern, size = round(size + x_2 (size - size below)).

    Every entry of A and b combines at most four values (bars B) with at most three float32 operations relative to at most 4
    max|N|: E = 4 max B + 4 EPS32 max|N|.  The solution's bars are those of Cramer's rule in float32 (sift_checks._solve)."""
    g = np.array([(N[1, 1, 2] - N[1, 1, 0]) / 2, (N[1, 2, 1] - N[1, 0, 1]) / 2, (N[2, 1, 1] - N[0, 1, 1]) / 2])
    v = N[1, 1, 1]
    axx = N[1, 1, 0] - 2 * v + N[1, 1, 2]
    ayy = N[1, 0, 1] - 2 * v + N[1, 2, 1]
    ass = N[0, 1, 1] - 2 * v + N[2, 1, 1]
    axy = (N[1, 2, 2] - N[1, 2, 0] - N[1, 0, 2] + N[1, 0, 0]) / 4
    axs = (N[2, 1, 2] - N[2, 1, 0] - N[0, 1, 2] + N[0, 1, 0]) / 4
    ays = (N[2, 2, 1] - N[2, 0, 1] - N[0, 2, 1] + N[0, 0, 1]) / 4
    A = np.array([[axx, axy, axs], [axy, ayy, ays], [axs, ays, ass]])
    e = 4 * float(B.max()) + 4 * EPS32 * float(np.abs(N).max())
    x, bar, det, det_bar, _ = _solve(g, A, e)
    if abs(det) <= det_bar or not np.all(np.isfinite(bar)):
        return None, False                    # det != 0 undecided: x = 0 (rejected) or anything
    ax = np.abs(x)
    ok = bool(ax.max() > 0 and np.all(ax <= 1))
    decided = bool(np.all(np.abs(ax - 1) > bar) and ax.max() > bar[int(ax.argmax())])
    if not ok:
        return None, decided
    size, step, ds = L["size"], L["step"], L["size"] - Lp["size"]
    m = (size // 2) // step
    cx = step * (j - m) + (size - 1) * 0.5 + x[0] * step
    cy = step * (i - m) + (size - 1) * 0.5 + x[1] * step
    sz = size + x[2] * ds
    # size + x_2 ds: one product, one sum; the rounded size is decided away from a half
    decided = decided and not _near_half(sz, bar[2] * ds + 2 * EPS32 * abs(sz))
    rec = dict(octave=L["octave"], layer=L["layer"], i=i, j=j, x=cx, y=cy, size=float(np.rint(sz)),
               bar_x=bar[0] * step + 2 * EPS32 * abs(cx), bar_y=bar[1] * step + 2 * EPS32 * abs(cy), fit=x, fit_bar=bar)
    return rec, decided


def candidates(img, thr=THRESHOLD):
    """-> (hessian layers, list of candidates).  A candidate is a sample of a middle layer (layers 1 .. 3 of an octave), inside the
    margin (size of the layer above / 2) / step + 1 on every side, with det > thr and det > each of its 26 neighbours in the
    layers below, its own and above.  Each: dict(octave, layer, i, j, response, bar_response, sure, fit_decided, rec, laplacian).
    `sure`: the threshold test and all 26 comparisons have margins beyond their bars (|a - b| > bar_a + bar_b; a value the layer
    never wrote is an exact zero); a sample that passes only within the bars is listed with sure = False.  rec is None where the fit
    rejects.  laplacian = sign of the trace, None where |trace| <= tbar."""
    H = hessian(img)
    h, w = np.asarray(img).shape
    out = []
    for o in range(OCTAVES):
        for ml in range(1, LAYERS + 1):
            k = o * (LAYERS + 2) + ml
            Lp, L, Ln = H[k - 1], H[k], H[k + 1]
            step = L["step"]
            rows, cols = h // step, w // step
            mg = (Ln["size"] // 2) // step + 1
            if rows - 2 * mg <= 0 or cols - 2 * mg <= 0:
                continue
            sl = lambda a, di, dj: a[mg + di:rows - mg + di, mg + dj:cols - mg + dj]
            v, bv = sl(L["det"], 0, 0), sl(L["bar"], 0, 0)
            sure = v - bv > thr
            poss = v + bv > thr
            for P in (Lp, L, Ln):
                for di in (-1, 0, 1):
                    for dj in (-1, 0, 1):
                        if P is L and di == 0 and dj == 0:
                            continue
                        nb, bn = sl(P["det"], di, dj), sl(P["bar"], di, dj)
                        sure &= v - bv > nb + bn
                        poss &= v + bv >= nb - bn
            for a, b in zip(*np.nonzero(poss)):
                i, j = int(a) + mg, int(b) + mg
                N = np.stack([P["det"][i - 1:i + 2, j - 1:j + 2] for P in (Lp, L, Ln)])
                B = np.stack([P["bar"][i - 1:i + 2, j - 1:j + 2] for P in (Lp, L, Ln)])
                rec, dec = _fit(N, B, L, Lp, i, j)
                tr, tb = float(L["trace"][i, j]), float(L["tbar"][i, j])
                out.append(dict(octave=o, layer=ml, i=i, j=j, response=float(L["det"][i, j]), bar_response=float(L["bar"][i, j]),
                                sure=bool(sure[a, b]), fit_decided=dec, rec=rec,
                                laplacian=None if abs(tr) <= tb else int(tr > 0) - int(tr < 0)))
    return H, out


# ------------------------------------------------------------------------------------------------- deletion and orientation
def _gauss(n, sigma):
    x = np.arange(n) - (n - 1) * 0.5
    k = np.exp(-x * x / (2 * sigma * sigma))
    return k / k.sum()


def _ori_samples():
    g = _gauss(2 * ORI_RADIUS + 1, 2.5)
    pts = [(i, j, g[i + ORI_RADIUS] * g[j + ORI_RADIUS]) for i in range(-ORI_RADIUS, ORI_RADIUS + 1)
           for j in range(-ORI_RADIUS, ORI_RADIUS + 1) if i * i + j * j <= ORI_RADIUS * ORI_RADIUS]
    assert len(pts) == ORI_N
    return np.array([p[0] for p in pts]), np.array([p[1] for p in pts]), np.array([p[2] for p in pts])


APT_X, APT_Y, APT_W = _ori_samples()


def scalars(size):
    """s, g and win of a size as the operator defines them (float32, see the module text) and `tie`: the float64 values of 2 s or
    21 s lie within their bars (3 and 4 roundings of the value) of the rounding's edge"""
    s = F32(size) * F32(1.2) / F32(9.0)
    g = 2 * int(np.rint(F32(2) * s))
    win = int(F32(PATCH + 1) * s)
    sd = float(size) * 1.2 / 9.0
    w21 = 21 * sd
    tie = _near_half(2 * sd, 3 * EPS32 * 2 * sd) or (w21 - math.floor(w21)) <= 4 * EPS32 * w21 or (math.ceil(w21) - w21) <= 4 * EPS32 * w21
    return s, g, win, bool(tie)


def sample_positions(x, y, size, shape):
    """the 113 orientation samples of a key point: top-left corners round(c + apt * s - (g - 1) / 2) of its g x g wavelets and
    which of them lie inside (0 <= corner < sum side - g) -> (xs, ys, inside, s, g, ties).  float32 as defined; `ties` counts the
    samples whose float64 position lies within 3 EPS32 (|c| + 6 s + g / 2) -- three float32 operations on terms of that size -- of
    a half"""
    h, w = shape
    s, g, _, _ = scalars(size)
    half = F32(g - 1) / F32(2)
    xs = np.rint(F32(x) + APT_X.astype(F32) * s - half).astype(np.int64)
    ys = np.rint(F32(y) + APT_Y.astype(F32) * s - half).astype(np.int64)
    assert (F32(x) + APT_X.astype(F32) * s - half).dtype == F32
    inside = ~((ys < 0) | (ys >= h + 1 - g) | (xs < 0) | (xs >= w + 1 - g))
    sd = float(size) * 1.2 / 9.0
    ties = 0
    for c, apt in ((float(x), APT_X), (float(y), APT_Y)):
        p = c + apt * sd - (g - 1) / 2
        ties += int((np.abs(np.abs(p - np.floor(p)) - 0.5) <= 3 * EPS32 * (abs(c) + 6 * sd + g / 2)).sum())
    return xs, ys, inside, float(s), g, ties


def deleted(x, y, size, shape):
    """the operator deletes a key point whose gradient wavelet is larger than the integral or none of whose 113 samples is inside"""
    h, w = shape
    xs, ys, inside, s, g, _ = sample_positions(x, y, size, shape)
    return bool(h + 1 < g or w + 1 < g or not inside.any())


def orientation(ii, x, y, size):
    """the dominant orientation of an emitted key point (its own float32 x, y, size) -> dict(deleted, nangle, angle, tol, decided,
    alternatives, ties).

    X, Y = Gaussian-weighted Haar gradients of the inside samples; angle_k = atan2(Y, X) in degrees, rounded; 72 windows centred on
    0, 5 .. 355 degrees take the samples with |rounded angle - centre| < 30 or > 330; the window with the largest sumx^2 + sumy^2
    (the first of equals) gives atan2(-sumy, sumx).

    Bars.  A gradient is a two-box Haar value (HAAR_K EPS32 A) times a weight (GAUSS_REL, one product): e_k.  The angle of a
    sample moves by at most (e_X + e_Y) / |(X, Y)| radians and fastAtan2 by ANGLE_BOUND: a sample whose angle lies within that of a
    half may round either way, and is `loose` in the windows it then enters or leaves (in every window where the bar reaches half
    a degree).  A window's sum is a float32 running sum of n terms: U = n EPS32 sum(|X| + |Y|) / 2 plus the e_k of its members.
    Its modulus lies between the smallest and the largest |sum| over every subset of its loose samples (enumerated up to five of
    them; the triangle inequality beyond that, and where the loose vectors together are below 1e-3 of the sum), widened by U and
    4 EPS32.  The winner is decided when its lower end exceeds the upper end of every window with other members; the angle's
    tolerance is ANGLE_BOUND + degrees((U + loose vectors) / |S|) + 360 EPS32.  Otherwise every window whose upper end reaches
    the best lower end is an alternative, each with its own tolerance."""
    h, w = ii.shape[0] - 1, ii.shape[1] - 1
    xs, ys, inside, s, g, ties = sample_positions(x, y, size, (h, w))
    if h + 1 < g or w + 1 < g or not inside.any():
        return dict(deleted=True, nangle=0, ties=ties)
    xs, ys, wt = xs[inside], ys[inside], APT_W[inside]
    n = len(xs)
    vals = []
    for pat in (GRAD_X, GRAD_Y):
        v, a = np.zeros(n), np.zeros(n)
        for x1, y1, x2, y2, wgt in scaled_boxes(pat, 4, g):
            sm = (ii[ys + y2, xs + x2] + ii[ys + y1, xs + x1] - ii[ys + y1, xs + x2] - ii[ys + y2, xs + x1]).astype(np.float64)
            v += sm * float(wgt); a += np.abs(sm) * abs(float(wgt))
        vals.append((v * wt, (HAAR_K * EPS32 * a + (GAUSS_REL + EPS32) * np.abs(v)) * wt))
    (X, eX), (Y, eY) = vals
    r = np.hypot(X, Y)
    ang = np.degrees(np.arctan2(Y, X)) % 360.0
    ang[r == 0] = 0.0                                                  # exact integer zeros on every side
    with np.errstate(divide="ignore", invalid="ignore"):
        abar = np.where(r > 0, ANGLE_BOUND + np.degrees(np.minimum((eX + eY) / np.where(r > 0, r, 1), math.pi)), 0.0)
    rnd = np.rint(ang).astype(np.int64)
    frac = ang - np.floor(ang)
    loose = np.abs(frac - 0.5) <= abar
    other = np.where(frac >= 0.5, rnd - 1, rnd + 1)
    wide = abar >= 0.5                                                 # may round to more than two values: loose in every window
    centres = np.arange(0, 360, 5)

    def member(rr):
        d = np.abs(rr[None, :] - centres[:, None])
        return (d < 30) | (d > 330)
    M = member(rnd)
    Lz = (loose[None, :] & (member(other) != M)) | wide[None, :]
    fixed = M & ~Lz
    sx, sy = (fixed * X[None, :]).sum(1), (fixed * Y[None, :]).sum(1)
    U = ((M | Lz) * (eX + eY)[None, :]).sum(1) + n * EPS32 * ((M | Lz) * (np.abs(X) + np.abs(Y))[None, :]).sum(1) / 2
    px, py = (M * X[None, :]).sum(1), (M * Y[None, :]).sum(1)          # the plain path
    lo, hi = np.zeros(72), np.zeros(72)
    mass = (Lz * np.hypot(X, Y)[None, :]).sum(1)                       # the loose vectors of a window, by length
    clean = mass <= 1e-3 * np.hypot(sx, sy)                           # (any split is sound: this one only chooses the cheaper bound)
    for k in range(72):
        lz = np.nonzero(Lz[k])[0]
        if clean[k] or len(lz) > 5:
            # the triangle inequality over the loose vectors
            a, b = max(math.hypot(sx[k], sy[k]) - mass[k], 0.0), math.hypot(sx[k], sy[k]) + mass[k]
        else:
            # the window's sum over every subset of its loose samples
            mods = [math.hypot(sx[k] + sum(X[t] for b_, t in enumerate(lz) if m >> b_ & 1),
                               sy[k] + sum(Y[t] for b_, t in enumerate(lz) if m >> b_ & 1)) for m in range(1 << len(lz))]
            a, b = min(mods), max(mods)
        lo[k] = max(a - U[k], 0.0) ** 2 * (1 - 4 * EPS32)
        hi[k] = (b + U[k]) ** 2 * (1 + 4 * EPS32)
    plain = px * px + py * py
    if plain.max() <= 0 and hi.max() <= 0:
        # every window empty or exactly zero: best stays (0, 0), the angle is fastAtan2(-0, 0) = 0
        return dict(deleted=False, nangle=n, angle=0.0, tol=ANGLE_BOUND, decided=True, alternatives=[(0.0, ANGLE_BOUND)], ties=ties)
    best = int(np.argmax(plain))                                       # the first of equals
    # a window with the members of the best one, both clean, gives the best one's sums up to the loose mass: the same angle
    same = np.array([np.array_equal(M[k], M[best]) and bool(clean[k]) for k in range(72)]) & bool(clean[best])
    decided = bool(np.all(same | (hi < lo[best]))) and lo[best] > 0

    def angle_of(k):
        a = math.degrees(math.atan2(-py[k], px[k])) % 360.0
        mod = math.hypot(px[k], py[k])
        u = U[k] + mass[k]                                             # a loose sample may be in or out: its whole vector
        t = ANGLE_BOUND + 360 * EPS32 + (math.degrees(min(u / mod, math.pi)) if mod > 0 else 360.0)
        return a, t
    alts = [angle_of(k) for k in range(72) if k == best or (not same[k] and hi[k] >= lo[best])]
    a, t = angle_of(best)
    return dict(deleted=False, nangle=n, angle=a, tol=t, decided=decided, alternatives=alts, ties=ties)


# -------------------------------------------------------------------------------------------------------------- descriptor
DESC_W = np.outer(_gauss(PATCH, 3.3), _gauss(PATCH, 3.3))


def _area_weights(win):
    """[21, win]: the share of source sample k in output cell d of an area average win -> 21: |[k, k + 1] n [d t, (d + 1) t]| / t,
    t = win / 21.  (The operator drops an end tap narrower than 1e-3 of a sample; the ends d t have fractional parts that are
    multiples of 1 / 21, never in (0, 1e-3], so that never drops a real tap.)"""
    t = win / 21.0
    k = np.arange(win)
    d = np.arange(21)
    lo = np.maximum(k[None, :], (d * t)[:, None])
    hi = np.minimum(k[None, :] + 1.0, ((d + 1) * t)[:, None])
    W = np.clip(hi - lo, 0, None) / t
    W[W < 1e-9] = 0.0
    return W


def patch_of(img, x, y, size, angle):
    """the 21 x 21 byte patch of an emitted record (float32 x, y, size, angle) as three arrays lo <= nominal <= hi and the window side.

    The window of win = int(21 s) samples a side is turned by the angle about the key point: sample (i, j) lies at
      px = x + (j + off) cos - (i + off) sin,  py = y + (j + off) sin + (i + off) cos  with the IMAGE's y pointing down and
    sin = sin(angle), i.e. in the operator's words sin_dir = -sin, px += sin_dir per row; off = -(win - 1) / 2.
    A sample with 0 <= floor(px) < w - 1 and 0 <= floor(py) < h - 1 is bilinear, rounded to a byte; any other is the nearest pixel
    (round, clamped into the frame).  The bytes are area-averaged to 21 x 21 and rounded.

    Bars.  The operator walks the rows by float32 running sums (start += sin_dir, win times, each rounding u of at most M = |c| +
    win) and the columns in double; cos and sin are float32 (u each, times at most win steps), the angle in radians carries two
    roundings of at most 2 pi on a lever of at most win: pos = EPS32 ((win + 3) M / 2 + 8 win) pixels.  The bilinear surface is
    continuous, with slopes of at most Lx, Ly = the largest neighbour differences of the 4 x 4 pixels around the cell, and its
    float32 evaluation (four terms of three operations, three sums) errs by at most 8 EPS32 * 255: e_v = pos (Lx + Ly) + 8 EPS32
    * 255.  A sample within pos of the frame where bilinear and nearest-pixel meet, or of a half outside it, takes the range of the
    3 x 3 pixels around it.  Sample bytes lie in [rint(v - e_v), rint(v + e_v)].  The area average has positive weights, so it maps
    ranges to ranges: ratio 2 is (acc + 2) >> 2 on exact integers, an integer ratio k is rint(acc / k^2) of an exact numerator
    (the float32 product errs by 2 u 255 = 3e-5, below the 1 / (2 k^2) >= 4e-4 that separates a non-tie from a half for k <= 35,
    so only an exact half is accepted either way), any other ratio a float32 sum of at most (win / 21 + 2) taps twice:
    (2 (win / 21 + 2) + 4) EPS32 * 255."""
    img = np.asarray(img)
    h, w = img.shape
    s, g, win, tie = scalars(size)
    assert 1 <= win
    off = -(win - 1) / 2.0
    a = float(F32(angle)) * math.pi / 180.0
    ca, sa = math.cos(a), math.sin(a)
    jj, ii_ = np.meshgrid(np.arange(win) + off, np.arange(win) + off)
    px = float(x) + jj * ca - ii_ * sa
    py = float(y) + jj * sa + ii_ * ca
    M = abs(float(x)) + abs(float(y)) + win
    pos = EPS32 * ((win + 3) * M / 2 + 8 * win)
    ix, iy = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    inner = (ix >= 0) & (ix < w - 1) & (iy >= 0) & (iy < h - 1)
    f = img.astype(np.float64)
    cx, cy = np.clip(ix, 0, w - 2), np.clip(iy, 0, h - 2)
    fa, fb = px - ix, py - iy
    p00, p01, p10, p11 = f[cy, cx], f[cy, cx + 1], f[cy + 1, cx], f[cy + 1, cx + 1]
    v = p00 * (1 - fa) * (1 - fb) + p01 * fa * (1 - fb) + p10 * (1 - fa) * fb + p11 * fa * fb
    # slopes over the 4 x 4 pixels around the cell
    pad = np.pad(f, 1, mode="edge")
    gx = np.abs(np.diff(pad, axis=1)); gy = np.abs(np.diff(pad, axis=0))
    Lx = np.zeros_like(v); Ly = np.zeros_like(v)
    for dy in range(4):
        for dx in range(3):
            Lx = np.maximum(Lx, gx[cy + dy, cx + dx])
    for dy in range(3):
        for dx in range(4):
            Ly = np.maximum(Ly, gy[cy + dy, cx + dx])
    ev = pos * (Lx + Ly) + 8 * EPS32 * 255
    nom = np.rint(v)
    lo, hi = np.rint(v - ev), np.rint(v + ev)
    out = ~inner
    rx, ry = np.clip(np.rint(px).astype(np.int64), 0, w - 1), np.clip(np.rint(py).astype(np.int64), 0, h - 1)
    near = f[ry, rx]
    nom = np.where(out, near, nom); lo = np.where(out, near, lo); hi = np.where(out, near, hi)
    edge = ((np.abs(px) <= pos) | (np.abs(px - (w - 1)) <= pos) | (np.abs(py) <= pos) | (np.abs(py - (h - 1)) <= pos)
            | (out & ((np.abs(np.abs(px - np.floor(px)) - 0.5) <= pos) | (np.abs(np.abs(py - np.floor(py)) - 0.5) <= pos))))
    if edge.any():
        p2 = np.pad(f, 1, mode="edge")
        mn = np.minimum.reduce([p2[ry + dy, rx + dx] for dy in range(3) for dx in range(3)])
        mx = np.maximum.reduce([p2[ry + dy, rx + dx] for dy in range(3) for dx in range(3)])
        lo = np.where(edge, np.minimum(lo, mn), lo); hi = np.where(edge, np.maximum(hi, mx), hi)
    lo, hi = np.clip(lo, 0, 255), np.clip(hi, 0, 255)
    assert np.all(lo <= nom) and np.all(nom <= hi)
    if win == PATCH + 1:
        res = (lo, nom, hi)
    elif win % (PATCH + 1) == 0:
        k = win // (PATCH + 1)
        acc = [b.reshape(21, k, 21, k).sum((1, 3)) for b in (lo, nom, hi)]
        if k == 2:
            res = tuple(np.floor((c + 2) / 4) for c in acc)
        else:
            # rint of an exact numerator over k^2; an exact half may go either way
            q = [c / float(k * k) for c in acc]
            half = [np.abs(t - np.floor(t) - 0.5) < 1e-12 for t in q]
            res = (np.where(half[0], np.floor(q[0]), np.rint(q[0])), np.rint(q[1]), np.where(half[2], np.ceil(q[2]), np.rint(q[2])))
            res = (np.minimum(res[0], np.where(half[1], np.floor(q[1]), res[1])), res[1], np.maximum(res[2], np.where(half[1], np.ceil(q[1]), res[2])))
    else:
        Wm = _area_weights(win)
        e = (2 * (win / 21.0 + 2) + 4) * EPS32 * 255
        m = [Wm @ b @ Wm.T for b in (lo, nom, hi)]
        res = (np.rint(m[0] - e), np.rint(m[1]), np.rint(np.minimum(m[2] + e, 255)))
        res = (np.minimum(res[0], np.rint(m[1] - e)), res[1], np.maximum(res[2], np.rint(m[1] + e)))
    return tuple(np.clip(r, 0, 255) for r in res) + (win, tie)


def descriptor(img, x, y, size, angle):
    """the 128 values of an emitted record -> dict(value[128], bound[128], decided, win, loose): over the 20 x 20 samples of the
    patch, dx = (right column - left column of the 2 x 2 bytes) and dy = (lower row - upper row) times the Gaussian weight of
    sigma 3.3; each of the 4 x 4 cells of 5 x 5 samples sums dx and |dx| apart for dy >= 0 and dy < 0, then dy and |dy| apart for
    dx >= 0 and dx < 0; the 128 sums are scaled to unit length.

    Bound.  Where the patch bytes are ranges (patch_of), dx and dy are ranges; a term whose sign bin is the same over the range
    moves its sum by at most the range's half widths, one whose sign bin depends on it by its largest magnitude: b_k per sum.
    Float32: a weight GAUSS_REL, the product u, 25 additions: 30 EPS32 of the cell's sum of magnitudes, added to b.  With n =
    |value| and B = |b|: out_k = v_k / n moves by at most (b_k + |v_k| B / (n - B)) / (n - B) + 4 EPS32.  decided: B < n / 2."""
    lo, nom, hi, win, tie = patch_of(img, x, y, size, angle)

    def grads(p_plus_lo, p_plus_hi, p_minus_lo, p_minus_hi):
        return p_plus_lo - p_minus_hi, p_plus_hi - p_minus_lo
    c = lambda p, di, dj: p[di:di + PATCH, dj:dj + PATCH]
    dxn = (c(nom, 0, 1) - c(nom, 0, 0) + c(nom, 1, 1) - c(nom, 1, 0)) * DESC_W
    dyn = (c(nom, 1, 0) - c(nom, 0, 0) + c(nom, 1, 1) - c(nom, 0, 1)) * DESC_W
    dxl, dxh = grads(c(lo, 0, 1) + c(lo, 1, 1), c(hi, 0, 1) + c(hi, 1, 1), c(lo, 0, 0) + c(lo, 1, 0), c(hi, 0, 0) + c(hi, 1, 0))
    dyl, dyh = grads(c(lo, 1, 0) + c(lo, 1, 1), c(hi, 1, 0) + c(hi, 1, 1), c(lo, 0, 0) + c(lo, 0, 1), c(hi, 0, 0) + c(hi, 0, 1))
    dxl, dxh, dyl, dyh = dxl * DESC_W, dxh * DESC_W, dyl * DESC_W, dyh * DESC_W
    value, bound = np.zeros(128), np.zeros(128)

    def split(t, tl, th, sgn, sl, sh):
        """sums of t and |t| over sgn >= 0 and sgn < 0 with their bounds: [t+, |t|+, t-, |t|-]"""
        dev = np.maximum(th - t, t - tl)
        big = np.maximum(np.abs(tl), np.abs(th))
        sure_p, sure_n = sl >= 0, sh < 0
        vals, bnds = [], []
        for sure, mask in ((sure_p, sgn >= 0), (sure_n, sgn < 0)):
            b = np.where(sure, dev, np.where(sure_p | sure_n, 0.0, big))
            rnd = 30 * EPS32 * np.abs(t * mask).sum()
            vals += [(t * mask).sum(), (np.abs(t) * mask).sum()]
            bnds += [b.sum() + rnd, b.sum() + rnd]
        return vals, bnds
    for ci in range(4):
        for cj in range(4):
            r = (slice(5 * ci, 5 * ci + 5), slice(5 * cj, 5 * cj + 5))
            v1, b1 = split(dxn[r], dxl[r], dxh[r], dyn[r], dyl[r], dyh[r])
            v2, b2 = split(dyn[r], dyl[r], dyh[r], dxn[r], dxl[r], dxh[r])
            k = (ci * 4 + cj) * 8
            value[k:k + 8] = v1 + v2
            bound[k:k + 8] = b1 + b2
    n, B = float(np.sqrt((value * value).sum())), float(np.sqrt((bound * bound).sum()))
    loose = int((lo != hi).sum())
    if n <= 0 or B >= n / 2:
        return dict(value=value, bound=np.full(128, np.inf), decided=False, win=win, loose=loose, tie=tie)
    out = value / n
    bnd = (bound + np.abs(value) * B / (n - B)) / (n - B) + 4 * EPS32
    return dict(value=out, bound=bnd, decided=True, win=win, loose=loose, tie=tie)


# -------------------------------------------------------------------------------------------------------------- final order
def order_key(x, y, size, response, octave):
    """response, size, octave descending, then y descending, then x ascending"""
    return (-response, -size, -octave, -y, x)


def records_of(kp):
    return [dict(x=float(kp["xy"][i, 0]), y=float(kp["xy"][i, 1]), size=float(kp["size"][i]), angle=float(kp["angle"][i]),
                 response=float(kp["response"][i]), octave=int(kp["octave"][i]), laplacian=int(kp["laplacian"][i]))
            for i in range(len(kp["xy"]))]


def check_order(kp, what):
    rec = records_of(kp)
    keys = [order_key(r["x"], r["y"], r["size"], r["response"], r["octave"]) for r in rec]
    for a, b in zip(keys, keys[1:]):
        assert a <= b, (what, a, b)


# ------------------------------------------------------------------------------------------------------------ the checks
_CACHE = {}


def reference(img, thr=THRESHOLD):
    """candidates(img, thr), computed once per frame content and threshold.  Treat as read-only."""
    img = np.ascontiguousarray(img, np.uint8)
    key = (img.shape, img.tobytes(), float(thr))
    if key not in _CACHE:
        H, cand = candidates(img, thr)
        _CACHE[key] = dict(H=H, cand=cand, ii=integral(img))
    return _CACHE[key]


def keypoints(img, thr=THRESHOLD):
    """the restatement's own key points: per candidate whose fit accepts a dict(octave, layer, i, j, x, y, size, response, laplacian,
    decided, fit, deleted, nangle, angle, angle_decided, win, g) with x, y rounded to float32 as a record holds them; computed
    once.  Read-only."""
    ref = reference(img, thr)
    if "kps" not in ref:
        out = []
        shape = np.asarray(img).shape
        for c in ref["cand"]:
            k = c["rec"]
            if k is None:
                continue
            x, y = F32(k["x"]), F32(k["y"])
            o = orientation(ref["ii"], x, y, k["size"])
            _, g, win, _ = scalars(k["size"])
            out.append(dict(octave=c["octave"], layer=c["layer"], i=c["i"], j=c["j"], x=float(x), y=float(y), size=k["size"],
                            response=c["response"], laplacian=c["laplacian"], decided=c["sure"] and c["fit_decided"], fit=k["fit"],
                            deleted=o["deleted"], nangle=o["nangle"], angle=o.get("angle"), angle_decided=o.get("decided", True),
                            win=win, g=g))
        ref["kps"] = out
    return ref["kps"]


def _angle_gap(a, b):
    d = abs(a - b) % 360.0
    return min(d, 360.0 - d)


def _matches(r, c, strict):
    """an emitted record r against a candidate c: the octave, the response within its bar, and the point -- within the fit's
    bars of the fitted one where the fit is decided (strict), within one step of the pattern's centre otherwise"""
    if r["octave"] != c["octave"] or abs(r["response"] - c["response"]) > c["bar_response"] + EPS32 * abs(r["response"]):
        return False
    step, size = 1 << c["octave"], (9 + 6 * c["layer"]) << c["octave"]
    m = (size // 2) // step
    if strict:
        k = c["rec"]
        return (abs(r["x"] - k["x"]) <= k["bar_x"] + EPS32 * abs(r["x"]) and abs(r["y"] - k["y"]) <= k["bar_y"] + EPS32 * abs(r["y"])
                and r["size"] == k["size"])
    ds = 6 << c["octave"]
    return (abs(r["x"] - (step * (c["j"] - m) + (size - 1) * 0.5)) <= step * (1 + 1e-6)
            and abs(r["y"] - (step * (c["i"] - m) + (size - 1) * 0.5)) <= step * (1 + 1e-6) and abs(r["size"] - size) <= ds + 1)


def check_keypoints(img, kp, thr=THRESHOLD, what=""):
    """holds an emitted key-point list to the restatement of `img`:
      * every decided key point (sure candidate, decided and accepted fit) that the deletion test keeps is present: exactly one
        record in its octave with its response within the bar, x, y within the fit's bars, the rounded size, and -- where the trace's
        sign is decided -- its laplacian; where a decided key point has no record, the deletion test on the fitted point must
        delete it;
      * nothing extra: every record is matched by a candidate (sure or within the bars) that the fit may accept, no candidate by two
        records, and the deletion test on the record's own x, y, size keeps it;
      * the angle of every record is the restatement's orientation of its own x, y, size within the tolerance, or one of the
        alternatives where the window argmax is undecided;
      * the final order.
    -> dict(candidates, undecided, present, records, angle_undecided, ties, worst_angle)"""
    ref = reference(img, thr)
    shape = np.asarray(img).shape
    rec = records_of(kp)
    check_order(kp, what)
    cand = ref["cand"]
    used = {}
    und = present = 0
    for c in cand:
        decided = c["sure"] and c["fit_decided"]
        if not decided:
            und += 1
            continue
        if c["rec"] is None:
            continue
        k = c["rec"]
        hits = [i for i, r in enumerate(rec) if _matches(r, c, True)]
        gone = deleted(F32(k["x"]), F32(k["y"]), k["size"], shape)
        if not hits:
            assert gone, "%s: the key point of candidate %s is missing (fitted %r)" % (what, (c["octave"], c["layer"], c["i"], c["j"]), k)
            continue
        assert len(hits) == 1, (what, "two records on one candidate", c, hits)
        i = hits[0]
        assert i not in used, (what, "one record on two candidates", rec[i])
        used[i] = c
        if c["laplacian"] is not None:
            assert rec[i]["laplacian"] == c["laplacian"], (what, rec[i], c["laplacian"])
        present += 1
    for i, r in enumerate(rec):
        if i not in used:
            hits = [c for c in cand if not (c["sure"] and c["fit_decided"]) and _matches(r, c, False) and id(c) not in {id(v) for v in used.values()}]
            assert hits, "%s: the emitted record %r is not in the restatement" % (what, r)
            used[i] = hits[0]
        assert r["size"] > 0 and not deleted(F32(r["x"]), F32(r["y"]), r["size"], shape), "%s: record %r should have been deleted" % (what, r)
    ang_und = ties = 0
    worst = 0.0
    for r in rec:
        o = orientation(ref["ii"], F32(r["x"]), F32(r["y"]), r["size"])
        assert not o["deleted"]
        ties += int(o["ties"] > 0)
        if o["decided"]:
            e = _angle_gap(r["angle"], o["angle"]) / o["tol"]
            assert e <= 1.0, "%s: record %r: angle off by %.3g tolerances (restatement %.4f +- %.4f, %d samples)" % (
                what, r, e, o["angle"], o["tol"], o["nangle"])
            worst = max(worst, e)
        else:
            ang_und += 1
            assert any(_angle_gap(r["angle"], a) <= t for a, t in o["alternatives"]), "%s: record %r: angle is none of %r" % (
                what, r, o["alternatives"])
    return dict(candidates=len(cand), undecided=und, present=present, records=len(rec), angle_undecided=ang_und, ties=ties,
                worst_angle=worst)


def check_descriptors(img, kp, what=""):
    """every emitted descriptor within descriptor()'s bound of its value -> dict(checked, undecided, loose, largest_bound, worst)"""
    n = und = loose = 0
    big = worst = 0.0
    for i, r in enumerate(records_of(kp)):
        d = descriptor(img, F32(r["x"]), F32(r["y"]), r["size"], F32(r["angle"]))
        if not d["decided"]:
            und += 1
            continue
        got = np.asarray(kp["desc"][i], np.float64)
        e = np.abs(got - d["value"]) / d["bound"]
        assert e.max() <= 1.0, "%s: record %d %r: descriptor element %d is %.7g, the restatement %.7g +- %.3g (window %d)" % (
            what, i, r, int(e.argmax()), got[int(e.argmax())], d["value"][int(e.argmax())], d["bound"][int(e.argmax())], d["win"])
        worst = max(worst, float(e.max()))
        big = max(big, float(d["bound"].max()))
        loose += int(d["loose"] > 0)
        n += 1
    return dict(checked=n, undecided=und, loose=loose, largest_bound=big, worst=worst)


def decided_shares(img, thr=THRESHOLD):
    """(undecided candidates, candidates, key points of the restatement alone: sure candidates whose decided fit accepts)"""
    cand = reference(img, thr)["cand"]
    und = sum(1 for c in cand if not (c["sure"] and c["fit_decided"]))
    return und, len(cand), sum(1 for c in cand if c["sure"] and c["fit_decided"] and c["rec"] is not None)
