"""Seeded crafted frames for SIFT's stages after the scale space (k_sift_extrema, k_sift_refine, k_sift_desc and the final order in
evh_sift.hip; find_extrema, adjust_local_extrema, calc_orientation_hist, calc_descriptor in oracle/evz_sift.cpp), driving their
edges on purpose.

  B  blobs          bright and dark Gaussian blobs and discs of every size: extrema of both signs in layers 1, 2, 3 of octaves
                    0 .. 3, candidates on the first and last column and row the 5-pixel border admits and on both sides of the
                    64-column / 4-row tiles of k_sift_extrema
  M  moves          blobs centred between samples and smooth seeded texture: fits that move 1 .. 4 times, leave through the layer
                    range and the border, are used up after 5 steps; a sweep of blob sizes that puts a key point on layer 3 with
                    xi > 0.45 (orientation radius 16, the largest descriptor radius)
  R  rejects        ridges and lines (the edge test: det <= 0 and the ratio) and blobs of falling contrast around 0.04 / 3
  O  orientations   corners, crosses and T-shapes turned through the circle: 2, 3 and 4 peaks per point, peaks in bin 0 and bin 35
                    whose parabola wraps on either side, windows cut by the image border, windows over exactly flat ground
  D  descriptors    key points in every octant of ori, windows leaving the image on every side and, in the top octaves, on all
                    four with the diagonal cap; second and third chunk of k_sift_desc; the 0.2 clip
  T  ties           frames mirrored about the line between two rows (the column filter keeps that symmetry bit for bit): pairs of
                    vertically adjacent candidates with bit-equal D, both admitted by >= (their fits are mirror images, so they
                    never merge), and pairs of blobs at the separation where neighbouring candidates converge on one sample
                    (duplicates the final order drops)
  N  near-flat      the six near-flat noise frames of tools/hygiene_inputs.py (regenerated from their seed; they have no candidate
                    at all) and two frames of the same generator with stronger noise; in for the bit-for-bit leg and the
                    "nothing extra" assertion, exempt from the cap

Blobs and shapes lie over fields of overlapping blobs, not on flat ground: a pixel whose gradient angle is within fastAtan2's
bound of a bin edge may fall on either bin, and on flat ground a blob's few pixels each weigh enough to leave its peaks undecided.

FRAMES maps a name (family letter first) to a gray frame of at most 256 x 192.  info(name) holds what the oracle and the plain
restatement (tests/sift_checks.py) say of a frame, computed once; check_premise(family) asserts on the CPU that the family still
is what its name says.  tests/test_oracle_sift_edges.py and tests/test_gpu_sift_edges.py run them."""
import functools

import numpy as np

import sift_checks as S
from oracle import oracle as O

W, H = 256, 192
WN, HN = 88, 72            # the near-flat noise frames
CAP = 0.9                  # the share of candidates and of key points that has to be decided in every family but N


def _canvas(ground):
    return np.full((H, W), float(ground))


ASPECT = 1.35             # blobs and discs are ellipses: a round one has no orientation to decide


def _uv(img, cx, cy, turn):
    """pixel offsets from (cx, cy) along the long and the short axis of an ellipse turned by `turn` degrees"""
    yy, xx = np.mgrid[0:img.shape[0], 0:img.shape[1]]
    t = np.radians(turn)
    return ((xx - cx) * np.cos(t) + (yy - cy) * np.sin(t)) / ASPECT, (-(xx - cx) * np.sin(t) + (yy - cy) * np.cos(t)) * ASPECT


def _blob(img, cx, cy, s, amp, turn=0.0):
    u, v = _uv(img, cx, cy, turn)
    img += amp * np.exp(-(u * u + v * v) / (2.0 * s * s))


def _disc(img, cx, cy, r, amp, turn=0.0):
    u, v = _uv(img, cx, cy, turn)
    img += amp * np.clip(r + 0.5 - np.hypot(u, v), 0, 1)


def _u8(img):
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------ B
# input coordinates of the octave pixels the border admits first and last: octave 0 (the doubled frame) pixel c is x = c / 2 - 0.25,
# octave 1 pixel c is x = c - 0.25
EDGE_X = (2.25, 4.75, 252.75, 249.75)
EDGE_Y = (2.25, 4.75, 188.75, 185.75)


def _field(seed, count, smin, smax, amp, ground=128.0, shape=(H, W)):
    """`count` seeded elliptical Gaussian blobs of either sign laid over one another, sigma log-uniform in smin .. smax, amplitude
    amp / 2 .. amp: a field of blobs without flat ground, so that no single pixel carries a large part of an orientation
    histogram (on flat ground a blob's few pixels do, and one of them near a bin edge leaves its peaks undecided)"""
    rng = np.random.default_rng(seed)
    img = np.full(shape, float(ground))
    for _ in range(count):
        s = smin * (smax / smin) ** float(rng.random())
        _blob(img, float(rng.uniform(0, shape[1])), float(rng.uniform(0, shape[0])), s,
              float(rng.uniform(amp / 2, amp)) * (1 if rng.random() < 0.5 else -1), float(rng.uniform(0, 180)))
    return img


def _blob_frame(sign, seed):
    """a field of blobs of sigma 0.8 .. 13 and, brighter (sign +1) or darker (-1) than anything in it, blobs of a ladder of sizes
    and small blobs on the border columns and rows"""
    img = _field(seed, 300, 0.8, 14.0, 42.0)
    amp = 110.0 * sign
    for k in range(12):
        _blob(img, 20.0 + 20.0 * k + 0.25 * (k % 4), 40.0 + 27.0 * (k % 5) + 0.25 * (k % 3), 0.8 * 2.0 ** (k / 2.75), amp, 15.0 * k)
    for i, ex in enumerate(EDGE_X):                    # the border columns, rows well inside, and the border rows
        _blob(img, ex, 150.0 + 9 * i, 1.0 + 0.9 * (i % 2), amp, 20.0 + 40 * i)
    for i, ey in enumerate(EDGE_Y):
        _blob(img, 60.0 + 11 * i, ey, 1.0 + 0.9 * (i % 2), amp, 25.0 + 40 * i)
    return _u8(img)


# ------------------------------------------------------------------------------------------------------------------ M
def _texture(seed, cell, lo=30, hi=225):
    """seeded cells of `cell` pixels smoothed by a separable binomial: smooth, contrasted, nowhere flat"""
    rng = np.random.default_rng(seed)
    a = np.kron(rng.integers(lo, hi, (H // cell + 2, W // cell + 2)).astype(np.float64), np.ones((cell, cell)))[:H, :W]
    k = np.array([1, 4, 6, 4, 1], np.float64) / 16
    for _ in range(2):
        a = sum(k[t] * np.roll(a, t - 2, 0) for t in range(5))
        a = sum(k[t] * np.roll(a, t - 2, 1) for t in range(5))
    return a


def _sweep_frame():
    """blobs of sigma 2.6 .. 3.7 in 40 steps (the range over which the extremum passes from layer 3 of octave 1 to layer 1 of
    octave 2), centres a quarter pixel further on each"""
    img = _canvas(30)
    for k in range(40):
        s = 2.6 * (3.7 / 2.6) ** (k / 39.0)
        cx, cy = 18.0 + 31.0 * (k % 8) + 0.25 * (k % 4), 18.0 + 38.0 * (k // 8) + 0.25 * ((k // 4) % 4)
        _blob(img, cx, cy, s, 190.0, 17.0 * k)
    return _u8(img)


# ------------------------------------------------------------------------------------------------------------------ R
def _ridge_frame():
    """rings (curved ridges, 1.2 .. 3 pixels wide) whose brightness swells and fades along the arc -- a straight, even line has a
    Hessian that is singular along it and decides nothing -- bright on 50 and dark on 200 (the two halves), and short plateaus
    (flat tops: extrema whose fitted Hessian is indefinite)"""
    img = _field(33, 150, 2.0, 7.0, 16.0, ground=60.0)
    img[:, W // 2:] += 130
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    for k in range(12):
        cx, cy = 24.0 + 42.0 * (k % 6) + 0.3 * k, 30.0 + 58.0 * (k // 6) + 0.2 * k
        rad, wd = 9.0 + 1.5 * (k % 5), 0.6 + 0.3 * (k % 4)
        d = np.hypot(xx - cx, yy - cy)
        th = np.arctan2(yy - cy, xx - cx)
        amp = 130.0 * (0.7 + 0.3 * np.cos((2 + k % 3) * th + k)) * (1 if cx < W // 2 else -1)
        img += amp * np.exp(-(d - rad) ** 2 / (2 * wd * wd))
    img = np.clip(img, 0, 255)
    for k in range(10):
        x, y = 10 + 25 * k, 150 + 3 * (k % 4)
        img[y:y + 3 + k % 3, x:x + 5 + k % 4] += 120.0 * (1 if x < W // 2 - 8 else -1)
    return _u8(img)


def _contrast_frame():
    """blobs of sigma 2 and 4 whose amplitude falls in steps of one gray level from 40 to 5, over a faint field of blobs"""
    img = _field(34, 250, 1.2, 5.0, 9.0, ground=100.0)
    for k in range(36):
        _blob(img, 16.0 + 28.0 * (k % 9), 20.0 + 44.0 * (k // 9), 2.0, 40.0 - k, 23.0 * k)
        _blob(img, 16.0 + 28.0 * (k % 9), 42.0 + 44.0 * (k // 9), 4.0, -(40.0 - k), 31.0 * k)
    return _u8(img)


# ------------------------------------------------------------------------------------------------------------------ O / D
def _shape(kind, u, v, a, b):
    """indicator of a corner (quadrant), a cross, a T or a bar in the shape's own coordinates; a: half-width of an arm, b: reach"""
    if kind == "corner":
        return (u >= 0) & (v >= 0) & (u < b) & (v < b)
    if kind == "cross":
        return ((np.abs(u) <= a) & (np.abs(v) <= b)) | ((np.abs(v) <= a) & (np.abs(u) <= b))
    if kind == "tee":
        return ((np.abs(u) <= b) & (np.abs(v) <= a)) | ((np.abs(u) <= a) & (v >= 0) & (v <= b))
    if kind == "check":
        return ((u >= 0) == (v >= 0)) & (np.abs(u) < b) & (np.abs(v) < b)
    raise KeyError(kind)


def _shapes_frame(seed, ground, value, first_angle, pitch=42, at_border=False, rough=0.0):
    """corners, crosses, T-shapes and checker junctions, each turned `360 / count` degrees further than the one before; with
    at_border the lattice starts on the frame's edge so that shapes (and the windows of their key points) are cut by it.  The
    shapes carry a smooth seeded texture of 24 gray levels (an even shape has gradients of exactly 45 degrees, which is a bin edge
    of the orientation histogram); the ground stays exactly flat unless `rough` gives it a field of blobs of that amplitude"""
    rng = np.random.default_rng(seed)
    img = _field(seed + 200, 200, 1.5, 8.0, rough, ground=ground) if rough else _canvas(ground)
    tex = _texture(seed + 100, 4, 0, 25) - 12.0
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    kinds = ("corner", "cross", "tee", "check")
    off = 2 if at_border else pitch // 2 + 2
    cells = [(x, y) for y in range(off, H + (pitch // 2 if at_border else -pitch // 2 + 6), pitch) for x in range(off, W + (pitch // 2 if at_border else -pitch // 2 + 6), pitch)]
    for i, (x, y) in enumerate(cells):
        t = np.radians(first_angle + i * 360.0 / len(cells))
        u = (xx - x) * np.cos(t) + (yy - y) * np.sin(t)
        v = -(xx - x) * np.sin(t) + (yy - y) * np.cos(t)
        m = _shape(kinds[i % 4], u, v, 2.0 + (i // 4) % 3, 11.0 + (i % 5))
        img[m] = value + int(rng.integers(-20, 21)) + tex[m]
    return _u8(img)


def _big_frame():
    """one blob of sigma 42: a key point in octave 5, whose 16 x 12 layer is smaller than the descriptor window (all four sides
    cut, the diagonal cap); small blobs in the corners: windows of fewer than 256 and 512 samples"""
    img = _canvas(5)
    _blob(img, 127.75, 95.75, 42.0, 245.0, 30.0)
    for i, (x, y) in enumerate(((2.25, 2.25), (252.75, 2.25), (2.25, 188.75), (252.75, 188.75), (4.75, 4.75), (249.75, 185.75),
                                (2.25, 60.0), (252.75, 130.0), (80.0, 2.25), (170.0, 188.75))):
        _blob(img, x, y, 1.0 + 0.3 * (i % 3), 150.0, 35.0 * i)      # small blobs in the corners and on the sides: windows cut to a quarter
    return _u8(img)


# ------------------------------------------------------------------------------------------------------------------ T
def _mirrored(img):
    """the top half and its mirror image below it: rows r and H - 1 - r are equal"""
    top = img[:H // 2]
    return np.ascontiguousarray(np.concatenate([top, top[::-1]], 0))


def _tie_frame(seed):
    """blobs and discs, some on the mirror line (their two halves meet there: extrema that straddle rows 95 | 96), and flat-topped
    plateaus whose neighbouring candidates converge on one sample"""
    rng = np.random.default_rng(seed)
    img = _field(seed + 300, 160, 1.0, 9.0, 30.0, ground=70.0)
    for k in range(14):
        s = 1.0 * 2.0 ** (k / 4.0)
        _blob(img, 14.0 + 17.5 * k, 95.5 - (k % 3) * 0.5, s, 120.0, 90.0 * (k % 2))      # on, and half a pixel and a pixel above, the line
    for k in range(24):
        cx, cy = 14.0 + 29.0 * (k % 8) + float(rng.integers(0, 2)) / 2, 14.0 + 24.0 * (k // 8) + float(rng.integers(0, 2)) / 2
        if k % 2:
            _disc(img, cx, cy, 2.0 + (k % 5), 110.0, 25.0 * k)
        else:
            img[int(cy) - 1 - k % 3:int(cy) + 2 + k % 3, int(cx) - 2:int(cx) + 3 + k % 2] += 100.0      # small plateaus
    return _mirrored(_u8(img))


# pairs of round blobs (sigma, separation in sigmas, direction in degrees, sub-pixel phase of the centre), found by a sweep of the
# separation from 1.4 to 3 sigma: the two blobs have merged in one layer and not yet in the layer below, the two extrema lie
# two samples apart, and the fit of the one moves onto the sample of the other
PAIRS = tuple((s, 1.4 + 1.6 * k / 47.0, 37.0 * k, 0.25 * (k % 4), 0.25 * (k % 3)) for s, k in ((1.5, 33), (1.5, 40), (1.75, 31), (1.75, 13), (2.5, 16)))


def _pairs_frame():
    """each pair of PAIRS four times, whole pixels apart (a whole-pixel shift changes no bit of a neighbourhood), on flat ground,
    mirrored: neighbouring candidates that converge on one sample, whose records the final order has to drop"""
    img = _canvas(40)
    for n in range(20):
        sig, rel, ang, fx, fy = PAIRS[n % 5]
        sep, t = sig * rel, np.radians(ang)
        cx, cy = 16 + 32 * (n % 8) + fx, 16 + 31 * (n // 8) + fy
        _blob(img, cx - sep / 2 * np.cos(t), cy - sep / 2 * np.sin(t), sig, 150.0, 0.0)
        _blob(img, cx + sep / 2 * np.cos(t), cy + sep / 2 * np.sin(t), sig, 150.0, 0.0)
    return _mirrored(_u8(img))


# ------------------------------------------------------------------------------------------------------------------ N
def _noise_frames():
    """the six frames (127 + integers(-1, 2, (72, 88))) of the hygiene inputs: generator seed 4, drawn after that tool's three
    earlier draws (white noise 120 x 160, binary noise 120 x 160, checker cells 25 x 38)"""
    rng = np.random.default_rng(4)
    rng.integers(0, 256, (120, 160), dtype=np.uint8)
    rng.integers(0, 2, (120, 160))
    rng.integers(0, 2, (25, 38))
    flat = [(127 + rng.integers(-1, 2, (HN, WN))).astype(np.uint8) for _ in range(6)]
    # their differences of Gaussians stay below the threshold of one gray level: no candidate at all.  Two frames of the same
    # kind with noise of +-12 and +-30 gray levels follow, whose candidates do sit on near-singular systems
    return flat + [(127 + rng.integers(-a, a + 1, (HN, WN))).astype(np.uint8) for a in (12, 30)]


def _make_frames():
    f = {}
    f["B_bright"] = _blob_frame(+1, 21)
    f["B_dark"] = _blob_frame(-1, 22)
    f["B_field"] = _u8(_field(35, 340, 0.8, 16.0, 48.0))
    f["M_sweep"] = _sweep_frame()
    f["M_texture_a"] = _u8(_texture(23, 8))
    f["M_texture_b"] = _u8(_texture(24, 11))
    f["M_shapes"] = _shapes_frame(32, 15, 200, 5.0, pitch=34)
    f["R_ridges"] = _ridge_frame()
    f["R_contrast"] = _contrast_frame()
    f["O_shapes_a"] = _shapes_frame(25, 0, 200, 0.0)
    f["O_shapes_b"] = _shapes_frame(26, 200, 60, 7.0, rough=50.0)
    f["O_border"] = _shapes_frame(27, 40, 210, 3.0, pitch=47, at_border=True, rough=50.0)
    f["D_shapes"] = _shapes_frame(28, 45, 190, 11.0, pitch=38, at_border=True, rough=30.0)
    f["D_big"] = _big_frame()
    f["D_mirror"] = _mirrored(_shapes_frame(29, 45, 215, 0.0, pitch=32, rough=30.0))
    f["T_mirror_a"] = _tie_frame(30)
    f["T_mirror_b"] = _tie_frame(31)
    f["T_pairs"] = _pairs_frame()
    f["T_shapes"] = _mirrored(_shapes_frame(51, 45, 200, 56.0, pitch=31, rough=50.0))
    for i, a in enumerate(_noise_frames()):
        f["N_flat_%d" % i if i < 6 else "N_noise_%d" % (i - 6)] = a
    for k, v in f.items():
        assert v.dtype == np.uint8 and v.ndim == 2 and v.shape[0] <= 192 and v.shape[1] <= 256, k
        v.setflags(write=False)
    return f


FRAMES = _make_frames()
FAMILIES = {c: sorted(n for n in FRAMES if n[0] == c) for c in "BMRODTN"}


def by_size():
    """{(w, h): names}: the frames of equal size"""
    out = {}
    for n in sorted(FRAMES):
        out.setdefault(FRAMES[n].shape[::-1], []).append(n)
    return out


# ------------------------------------------------------------------------------------------------- what is known of a frame
@functools.lru_cache(maxsize=None)
def info(name):
    """pyr: the oracle's Gaussian pyramid; kp: O.sift_detect(frame, cap=65536); ref: sift_checks.reference(pyr); desc: per oracle
    record sift_checks.descriptor of it.  Treat all of it as read-only."""
    img = FRAMES[name]
    pyr = O.sift_gauss_pyramid(img)
    kp = O.sift_detect(img, cap=65536)
    ref = S.reference(pyr)
    desc = [S.descriptor(pyr, *t[:4], t[5]) for t in S.records_of(kp)]
    return dict(pyr=pyr, kp=kp, ref=ref, desc=desc)


def shares(fam):
    """(decided candidates, candidates, decided key points, key points) over the family, by the reference alone"""
    t = np.zeros(4, np.int64)
    for n in FAMILIES[fam]:
        t += np.array(S.decided_shares(info(n)["pyr"]))
    return tuple(int(v) for v in t)


def _fits(fam):
    return [(n, f) for n in FAMILIES[fam] for f in info(n)["ref"]["fits"]]


def _kps(fam):
    """(name, fit, orientation) of the reference's key points"""
    out = []
    for n in FAMILIES[fam]:
        r = info(n)["ref"]
        out.extend((n, r["fits"][k], o) for k, o in sorted(r["ori"].items()))
    return out


def check_premise(fam):
    """asserts that the frames of family `fam` are what the family is for; returns a line of figures for the log"""
    problems = []
    fig = _premise(fam, lambda ok, what: ok or problems.append(str(what)))
    assert not problems, "%s: %s -- %s" % (fam, "; ".join(problems), fig)
    return fig


def _premise(fam, need):
    names = FAMILIES[fam]
    need(names, "no frames")
    dc, nc, dk, nk = shares(fam)
    fig = "decided %d/%d candidates (%.1f %%), %d/%d key points (%.1f %%)" % (dc, nc, 100.0 * dc / max(nc, 1), dk, nk, 100.0 * dk / max(nk, 1))
    for n in names:
        need(len(info(n)["kp"]["xy"]) <= 700, (n, len(info(n)["kp"]["xy"])))          # the reference is Python: keep it short
    if fam != "N":
        need(dc >= CAP * nc and dk >= CAP * nk and nk > 0, fig)
    fits, kps = _fits(fam), _kps(fam)
    if fam == "B":
        pairs, signs, cols, rows = set(), set(), set(), set()
        for n, f in fits:
            o, l, r, c = f["cand"]
            h, w = info(n)["pyr"][o].shape[1:]
            d = S.dog(info(n)["pyr"][o])[l, r, c]
            pairs.add((o, l)); signs.add((o, l, bool(d > 0)))
            # k_sift_extrema lays its 64 x 4 tiles behind the border: tile column (c - 5) % 64, tile row (r - 5) % 4; the first
            # column / row of a tile counts from the second tile on (the very first is the border column / row itself)
            tc, tr = c - S.BORDER, r - S.BORDER
            for what, hit in (("first", tc == 0), ("last", c == w - 6), ("tile-", tc % 64 == 63), ("tile+", tc >= 64 and tc % 64 == 0)):
                if hit:
                    cols.add(what)
            for what, hit in (("first", tr == 0), ("last", r == h - 6), ("tile-", tr % 4 == 3), ("tile+", tr >= 4 and tr % 4 == 0)):
                if hit:
                    rows.add(what)
        want = {(o, l) for o in range(4) for l in (1, 2, 3)}
        need(want <= pairs, "no candidate in (octave, layer) %s" % sorted(want - pairs))
        both = {(o, l, s) for o, l in want for s in (True, False)}
        need(both <= signs, "no candidate of (octave, layer, positive) %s" % sorted(both - signs))
        need({"first", "last", "tile-", "tile+"} <= cols and {"first", "last", "tile-", "tile+"} <= rows, (cols, rows))
        return fig + "; (octave, layer) pairs %d, both polarities in each of octaves 0 .. 3; border and tile columns %s rows %s" % (
            len(pairs), sorted(cols), sorted(rows))
    if fam == "M":
        steps = {}
        for n, f in fits:
            if f["decided"]:
                steps[(f["status"], f["steps"])] = steps.get((f["status"], f["steps"]), 0) + 1
        moved = {s for (st, s) in steps if st == "kp"}
        need({1, 2, 3, 4} <= moved, sorted(steps.items()))
        for st in ("layer", "border", "steps"):
            need(any(k[0] == st for k in steps), (st, sorted(steps.items())))
        # the descriptor radius round(3 scl sqrt(2) 2.5); the constants allow scl < 1.6 * 2^(3.5 / 3) = 3.592: radius 38 at the most
        top = [(f["rec"]["xi"], o["radius"], int(np.rint(3 * f["rec"]["scl"] * np.sqrt(2.0) * 2.5)))
               for n, f, o in kps if f["rec"]["layer"] == 3 and f["rec"]["xi"] > 0.45 and f["decided"]]
        need(top and all(t[1] == 16 and t[2] == 38 for t in top), top)
        return fig + "; decided exits by (status, moves) %s; layer 3 with xi > 0.45: %d key points, orientation radius 16, descriptor radius %d" % (
            sorted(steps.items()), len(top), max([t[2] for t in top] or [0]))
    if fam == "R":
        exits = {}
        for n, f in fits:
            if f["decided"]:
                exits[f["status"]] = exits.get(f["status"], 0) + 1
        for st in ("edge_det", "edge_ratio", "contrast", "kp"):
            need(exits.get(st, 0) >= 1, (st, exits))
        # just under and just over: the blobs of R_contrast lose one gray level of amplitude a step and cross the threshold at
        # amplitudes of 10 .. 20, so neighbouring steps differ by 5 .. 10 % in contrast: a decided reject and a decided key point
        # must lie within NEAR = 10 % of 0.04 / 3
        NEAR = 0.10
        t = [abs(f["contr"]) * S.LAYERS / S.CONTRAST for n, f in fits if f["decided"] and f["contr"] is not None and f["status"] in ("contrast", "kp")]
        under, over = [v for v in t if v < 1], [v for v in t if v >= 1]
        need(under and max(under) >= 1 - NEAR, "no decided reject within %g of the contrast threshold" % NEAR)
        need(over and min(over) <= 1 + NEAR, "no decided key point within %g of the contrast threshold" % NEAR)
        return fig + "; decided exits %s; |contr| * 3 / 0.04 closest to 1: %.4f under, %.4f over" % (
            sorted(exits.items()), max(under or [0]), min(over or [0]))
    if fam == "O":
        npk, wraps, cut, zeros, last = {}, {-1: 0, 1: 0}, 0, 0, 0
        for n, f, o in kps:
            if not (f["decided"] and o["decided"] and all(p["sure"] for p in o["peaks"])):
                continue
            npk[len(o["peaks"])] = npk.get(len(o["peaks"]), 0) + 1
            for p in o["peaks"]:
                if p["wrapped"]:
                    wraps[-1 if p["bin"] == 0 else 1] += 1
            cut += int(o["cut"]); zeros += int(o["zeros"] > 0)
            last += sum(1 for p in o["peaks"] if p["bin"] == 35 and p["offset"] > 0)
        need({2, 3, 4} <= set(npk), npk)
        # a strict local maximum keeps the parabola's offset inside (-0.5, 0.5): bin 0 can wrap below 0, bin 35 stays below 35.5 --
        # the operator's branch for bin >= 36 is never taken, so what is asked of bin 35 is a peak with a positive offset
        need(wraps[-1] >= 1 and last >= 1 and cut >= 1 and zeros >= 1, "wraps below 0 %d, peaks in bin 35 with a positive offset %d, windows cut %d, windows with exactly flat samples %d" % (wraps[-1], last, cut, zeros))
        return fig + ("; decided key points by number of peaks %s; parabola wraps below 0: %d; peaks in bin 35 with a positive offset: %d (36 and"
                      " beyond is out of reach: |offset| < 0.5); windows cut by the border: %d; windows holding samples of exactly zero gradient: %d") % (
            sorted(npk.items()), wraps[-1], last, cut, zeros)
    if fam == "D":
        octants, sides, chunks, clip, capped, exact, sat, all4 = set(), [0, 0, 0, 0], [0, 0, 0], 0, 0, 0, 0, 0
        for n in names:
            i = info(n)
            for t, d in zip(S.records_of(i["kp"]), i["desc"]):
                octants.add(int(d["ori"] // 45) % 8)
                for k in range(4):
                    sides[k] += int(d["sides"][k])
                all4 += int(all(d["sides"]))
                chunks[min(2, (d["samples"] - 1) // 256)] += 1
                clip += int(d["clipped"] > 0); capped += int(d["capped"])
                exact += int(t[3] in (0.0, 90.0, 180.0, 270.0)); sat += int(d["value"].max() >= 255.5)
        need(octants == set(range(8)), octants)
        need(min(sides) >= 1 and all4 >= 1 and capped >= 1, (sides, all4, capped))
        need(chunks[1] >= 1 and chunks[2] >= 1 and clip >= 1, (chunks, clip))
        return fig + ("; octants of ori 8; windows leaving left / top / right / bottom %s, all four %d, capped by the diagonal %d; samples"
                      " <= 256 / <= 512 / more: %s; clipped %d; angles of exactly 0 / 90 / 180 / 270: %d (%s); values >= 255.5: %d (%s)") % (
            sides, all4, capped, chunks, clip, exact, "reached" if exact else "not reached", sat, "reached" if sat else "not reached")
    if fam == "T":
        ties = merged = dropped = gone = 0
        for n in names:
            i = info(n)
            cand = {c: f for c, f in zip(i["ref"]["cand"], i["ref"]["fits"])}
            for (o, l, r, c), f in cand.items():
                g = cand.get((o, l, r + 1, c))
                if g is None:
                    continue
                d = S.dog(i["pyr"][o])[l]
                if d[r, c].tobytes() == d[r + 1, c].tobytes():
                    ties += 1
                    a, b = f["rec"], g["rec"]
                    if a is not None and b is not None and (a["r"], a["c"], a["layer"]) == (b["r"], b["c"], b["layer"]):
                        merged += 1
            samples = {}
            for k, f in enumerate(i["ref"]["fits"]):
                if f["rec"] is not None and f["decided"]:
                    samples.setdefault((f["rec"]["o"], f["rec"]["layer"], f["rec"]["r"], f["rec"]["c"]), []).append(k)
            dropped += sum(len(v) - 1 for v in samples.values())
            # the oracle's side of it: on a sample that several decided candidates converge on, with every peak sure, its list
            # holds one record per peak, not one per candidate and peak
            held = {}
            for t in S.records_of(i["kp"]):
                held[S.sample_of(t)] = held.get(S.sample_of(t), 0) + 1
            for s, ks in samples.items():
                o = i["ref"]["ori"][ks[0]]
                if len(ks) > 1 and o["decided"] and all(p["sure"] for p in o["peaks"]):
                    need(held.get(s, 0) == len(o["peaks"]), "%s: sample %s holds %d records for %d peaks of %d candidates" % (
                        n, s, held.get(s, 0), len(o["peaks"]), len(ks)))
                    gone += (len(ks) - 1) * len(o["peaks"])
        need(ties >= 1, "no pair of vertically adjacent candidates with bit-equal D")
        need(dropped >= 10, "only %d duplicates from decided candidates converging on one sample" % dropped)
        need(gone >= 10, "only %d records seen dropped from the oracle's list" % gone)
        return fig + ("; vertically adjacent candidates with bit-equal D: %d pairs, %d of them converging on one sample (mirror images never do);"
                      " decided candidates converging on another's sample: %d; records the oracle's list is shorter by on those samples: %d") % (
            ties, merged, dropped, gone)
    if fam == "N":
        wild = sum(1 for _, f in fits if f["wild"])
        need(nc >= 6, fig)
        return fig + "; %d candidates whose alternatives cannot be enumerated" % wild
    raise KeyError(fam)
