"""Seeded crafted frames for SURF's stages (the seven kernels of evh_surf.hip; oracle/evz_surf.cpp), driving their edges on purpose.

  L  layers         off-centre, slightly elliptic Gaussian blobs of both signs on a ladder of sizes: key points of both laplacian
                    signs in the middle layers of every octave; 288 x 280 frames whose blob of sigma 44 reaches the 216 layer
                    (window side 669, larger than the frame); a perfectly symmetric blob centred on a half pixel, which has no
                    strict maximum and therefore no key point
  W  windows        sweeps of blob sizes around 15 and 30 (windows 42 and 84: the two integer-ratio area averages), 46 and 47
                    (windows 128 and 131, either side of the describe kernel's split) and general ratios on both sides
  B  borders        blobs on the first and last samples the margin admits, in rows and columns, in octaves 0 .. 2; orientation
                    samples partly outside; descriptor windows cut on each side and at a corner
  G  geometry       frames whose height or width is a layer size 27, 33, 42, 54, 108 less one, exact, plus one: a layer just
                    built or just not; the smallest frame with a key point (24 x 24); odd strides
  T  threshold/fit  blobs of falling contrast around the threshold; smoothed noise whose fits have components up to and beyond 1;
                    fitted sizes near a half
  O  orientation    elongated blobs turned through the circle (all four quadrants and the 0 / 360 wrap); O_iso: round blobs
                    whose window argmax is undecided -- counted, exempt from the cap
  R  order          a 64 x 64 tile repeated to 256 x 192: equal response, size and octave, ordered by y and x
  S  saturation     binary 0 / 255 shapes, a frame of 255, near-flat noise (S_flat: exempt from the cap)

FRAMES maps a name (family letter first) to a gray frame.  check_premise(family) asserts on the CPU, from the restatement alone
(tests/surf_checks.py, not the oracle), that the family still is what its name says."""
import numpy as np

import surf_checks as S

W, H = 256, 240
CAP = 0.10                       # the share of candidates / key points that may be undecided in a family
EXEMPT = ("O_iso", "S_flat")     # the near-isotropic and the near-flat frames may exceed it, by name
ASPECT = 1.25


def _blob(img, cx, cy, s, amp, turn=0.0, aspect=ASPECT):
    yy, xx = np.mgrid[0:img.shape[0], 0:img.shape[1]]
    t = np.radians(turn)
    u = ((xx - cx) * np.cos(t) + (yy - cy) * np.sin(t)) / aspect
    v = (-(xx - cx) * np.sin(t) + (yy - cy) * np.cos(t)) * aspect
    img += amp * np.exp(-(u * u + v * v) / (2.0 * s * s))


def _u8(img):
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def _field(seed, shape, count, smin, smax, amp, ground=120.0, aspect=ASPECT):
    """`count` seeded elliptic blobs of either sign, sigma log-uniform in smin .. smax"""
    rng = np.random.default_rng(seed)
    img = np.full(shape, float(ground))
    for _ in range(count):
        s = smin * (smax / smin) ** float(rng.random())
        _blob(img, float(rng.uniform(0, shape[1])), float(rng.uniform(0, shape[0])), s,
              float(rng.uniform(amp / 2, amp)) * (1 if rng.random() < 0.5 else -1), float(rng.uniform(0, 180)), aspect)
    return img


def _ladder(sign, seed, scale=1.0):
    """blobs of sigma 2.6 .. 22 times `scale` (size about 4.7 .. 6 sigma: octaves 0 .. 3) over a faint field, all of one sign"""
    img = _field(seed, (H, W), 40, 3.0, 12.0, 10.0)
    sig = [scale * 2.6 * (22 / 2.6) ** (k / 13.0) for k in range(14)]
    x = 14.0
    for k, s in enumerate(sig[:9]):
        _blob(img, x + 0.3 * (k % 3), 30.0 + 45 * (k % 2) + 0.2 * k, s, 100.0 * sign, 20.0 * k)
        x += 2.2 * s + 10
    _blob(img, 60.3, 150.2, sig[9], 100.0 * sign, 30); _blob(img, 150.6, 160.4, sig[10], 100.0 * sign, 70)
    _blob(img, 215.0, 120.0, sig[11], 90.0 * sign, 110)
    return _u8(img)


def _deep(sign, sigma):
    """one blob of sigma 24 or 30 in the middle of the frame, for layers 1 and 2 of octave 3 (sizes 120 and 168), whose margins
    leave two or three samples a side"""
    img = np.full((H, W), 120.0)
    _blob(img, 126.3, 118.6, sigma, 100.0 * sign, 25)
    return _u8(img)


def _top(sign):
    """the 216 layer has a margin of 17 samples of 8 pixels: at 288 x 280 it admits row 17 and columns 17 and 18 alone; the blob
    sits on the centre of the pattern of sample (17, 17), (139.5, 139.5), a fraction of a pixel off"""
    img = np.full((280, 288), 120.0)
    _blob(img, 139.7, 139.35, 44.0, 100.0 * sign, 25, 1.1)
    return _u8(img)


def _symmetric():
    img = np.full((96, 96), 60.0)
    yy, xx = np.mgrid[0:96, 0:96]
    img += 150.0 * np.exp(-((xx - 47.5) ** 2 + (yy - 47.5) ** 2) / (2 * 5.0 ** 2))
    return _u8(img)


def _sweep(lo, hi, n, seed, amp=100.0):
    """n blobs of sigma lo .. hi on a grid, signs alternating, centres a fraction of a pixel further on each"""
    img = _field(seed, (H, W), 30, 4.0, 12.0, 8.0)
    pitch = max(int(5.5 * hi), 30)
    per = (W - 20) // pitch
    for k in range(n):
        s = lo + (hi - lo) * k / max(n - 1, 1)
        cx, cy = 10 + pitch / 2 + pitch * (k % per) + 0.17 * k, 10 + pitch / 2 + pitch * (k // per) + 0.11 * k
        if cy + pitch / 2 > H:
            break
        _blob(img, cx, cy, s, amp * (1 if k % 2 else -1), 25.0 * k)
    return _u8(img)


def _border(seed):
    """small and middle blobs whose centres walk along the four borders at the distances where the margins of octaves 0 .. 2 admit
    their first and last samples (11, 22 and 45 pixels) and closer"""
    img = _field(seed, (H, W), 30, 4.0, 10.0, 8.0)
    rng = np.random.default_rng(seed + 1)
    for d, s in ((9.0, 2.5), (9.7, 2.6), (10.4, 2.6), (10.7, 2.6), (11.0, 2.6), (11.3, 2.6), (12.0, 2.7), (11.6, 2.7), (12.3, 2.7), (21.5, 5.0), (22.5, 5.1), (23.5, 5.2), (44.0, 10.0), (45.5, 10.2), (47.5, 10.4)):
        for side in range(4):
            t = float(rng.uniform(0.1, 0.9))
            along_w, along_h = 30 + t * (W - 60), 30 + t * (H - 60)
            cx, cy = ((d, along_h), (W - 1 - d, along_h), (along_w, d), (along_w, H - 1 - d))[side]
            _blob(img, cx + 0.1 * side, cy + 0.15 * side, s, 110.0 * (1 if (side + int(d)) % 2 else -1), 40.0 * side + d)
    _blob(img, 12.0, 12.0, 3.2, 110.0, 30)
    _blob(img, W - 13.0, H - 13.0, 3.2, -110.0, 60)
    return _u8(img)


def _geometry(seed, w, h):
    return _u8(_field(seed, (h, w), max(6, w * h // 250), 2.6, 9.0, 80.0))


def _contrast(seed):
    """blobs of sigma about 3.2 whose amplitude falls by 1.5 % a step, the response by 3 %, through the one at which it crosses 400"""
    img = np.full((H, W), 120.0)
    for k in range(48):
        _blob(img, 20.3 + 30 * (k % 8) + 0.07 * k, 20.6 + 36 * (k // 8) + 0.05 * k, 3.2 + 0.02 * (k % 5), (32.0 * 0.985 ** k) * (1 if k % 2 else -1), 15.0 * k)
    return _u8(img)


def _turned(seed, first):
    """elongated blobs turned by 15 degrees a step beside a small offset blob each, so that the dominant direction follows the turn"""
    img = _field(seed, (H, W), 20, 5.0, 12.0, 6.0)
    for k in range(24):
        a = first + 15.0 * k
        cx, cy = 26.0 + 41 * (k % 6) + 0.13 * k, 30.0 + 58 * (k // 6) + 0.09 * k
        _blob(img, cx, cy, 4.2, 100.0, a, 1.5)
        _blob(img, cx + 7 * np.cos(np.radians(a)), cy + 7 * np.sin(np.radians(a)), 2.2, 60.0, a)
    return _u8(img)


def _isotropic():
    img = np.full((H, W), 100.0)
    yy, xx = np.mgrid[0:H, 0:W]
    for k in range(20):
        cx, cy = 28.0 + 48 * (k % 5) + 0.21 * k, 30.0 + 58 * (k // 5) + 0.13 * k
        img += 110.0 * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * (3.0 + 0.15 * k) ** 2))
    return _u8(img)


def _tiled(seed):
    tile = _u8(_field(seed, (64, 64), 14, 2.6, 5.0, 90.0))
    return np.tile(tile, (3, 4))


def _binary(seed):
    rng = np.random.default_rng(seed)
    img = np.zeros((H, W), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for k in range(28):
        cx, cy, r = rng.uniform(10, W - 10), rng.uniform(10, H - 10), rng.uniform(3, 16)
        if k % 3 == 0:                                 # a turned rectangle: an axis-parallel one is mirror symmetric and ties
            t = rng.uniform(0.2, 1.3)
            u, v = (xx - cx) * np.cos(t) + (yy - cy) * np.sin(t), -(xx - cx) * np.sin(t) + (yy - cy) * np.cos(t)
            img[(np.abs(u) <= r) & (np.abs(v) <= r * 0.7)] = 255 if k % 2 else 0
        else:
            img[(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = 255 if k % 2 else 0
    return img


def _rough(seed):
    """strong noise under a 2 x 2 box: a det that is far from quadratic, fits with components up to and beyond 1"""
    rng = np.random.default_rng(seed)
    a = 128 + 90 * rng.standard_normal((160, 192))
    a = (a + np.roll(a, 1, 0) + np.roll(a, 1, 1) + np.roll(np.roll(a, 1, 0), 1, 1)) / 4
    return _u8(a)


def _flat(seed, amp):
    rng = np.random.default_rng(seed)
    return _u8(128 + amp * rng.standard_normal((72, 88)))


GEOMETRY_SIZES = (27, 33, 42, 54, 108)


def _make_frames():
    f = {"L_bright": _ladder(1, 11), "L_dark": _ladder(-1, 12), "L_bright2": _ladder(1, 13, 1.13), "L_dark2": _ladder(-1, 14, 1.13),
         "L_deep24_bright": _deep(1, 24.0), "L_deep24_dark": _deep(-1, 24.0), "L_deep30_bright": _deep(1, 30.0), "L_deep30_dark": _deep(-1, 30.0),
         "L_top_bright": _top(1), "L_top_dark": _top(-1), "L_symmetric": _symmetric(),
         "W_15": _sweep(2.3, 2.8, 56, 21), "W_30": _sweep(4.7, 5.4, 30, 22), "W_46": _sweep(7.4, 8.2, 20, 23), "W_46b": _sweep(7.45, 8.25, 20, 24),
         "B_a": _border(31), "B_b": _border(33),
         "T_contrast": _contrast(41), "T_fit": _sweep(1.3, 2.7, 56, 42), "T_fit2": _sweep(3.6, 4.6, 42, 43), "T_rough": _rough(44),
         "O_a": _turned(51, 0.0), "O_b": _turned(52, 7.0), "O_iso": _isotropic(),
         "R_tiled": _tiled(61), "R_tiled2": _tiled(62),
         "S_binary": _binary(71), "S_binary2": _binary(72), "S_white": np.full((H, W), 255, np.uint8),
         "S_flat": _flat(73, 1.5), "S_flat2": _flat(74, 6.0)}
    k = 0
    for s in GEOMETRY_SIZES:
        for d in (-1, 0, 1):
            f["G_h%03d%+d" % (s, d)] = _geometry(80 + k, 123 + 2 * k, s + d)          # odd widths: strides of every residue
            f["G_w%03d%+d" % (s, d)] = _geometry(100 + k, s + d, 90 + 3 * k)
            k += 1
    tiny = np.full((24, 24), 40.0)
    _blob(tiny, 11.6, 11.4, 2.6, 200.0, 20, 1.1)
    f["G_tiny"] = _u8(tiny)
    for v in f.values():
        v.setflags(write=False)
    return f


FRAMES = _make_frames()
FAMILIES = {c: sorted(n for n in FRAMES if n[0] == c) for c in "LWBGTORS"}
NONE = ("L_symmetric", "S_white")          # frames without a key point on any side


def by_size():
    """{(w, h): names}: the frames of equal size"""
    out = {}
    for n in sorted(FRAMES):
        out.setdefault(FRAMES[n].shape[::-1], []).append(n)
    return out


def shares(fam):
    """(undecided candidates, candidates, key points, key points with an undecided window argmax) of the family's frames that
    count towards the cap, by the restatement alone"""
    t = np.zeros(4, np.int64)
    for n in FAMILIES[fam]:
        if n in EXEMPT:
            continue
        u, c, k = S.decided_shares(FRAMES[n])
        kps = [q for q in S.keypoints(FRAMES[n]) if q["decided"] and not q["deleted"]]
        t += np.array([u, c, k, sum(1 for q in kps if not q["angle_decided"])])
    return tuple(int(v) for v in t)


def _kps(fam):
    return [(n, q) for n in FAMILIES[fam] for q in S.keypoints(FRAMES[n]) if q["decided"] and not q["deleted"]]


def check_premise(fam):
    """asserts that the frames of family `fam` reach what the family is for; returns a line of figures for the log"""
    problems = []
    fig = _premise(fam, lambda ok, what: ok or problems.append(str(what)))
    assert not problems, "%s: %s -- %s" % (fam, "; ".join(problems), fig)
    return fig


def _premise(fam, need):
    u, c, k, au = shares(fam)
    fig = "undecided %d/%d candidates (%.1f %%), window argmax undecided for %d/%d key points (%.1f %%)" % (
        u, c, 100.0 * u / max(c, 1), au, k, 100.0 * au / max(k, 1))
    need(u <= CAP * c and au <= CAP * k, fig)
    kps = _kps(fam)
    for n in FAMILIES[fam]:
        need(len(S.keypoints(FRAMES[n])) <= 400, (n, len(S.keypoints(FRAMES[n]))))
    if fam == "L":
        seen = {(q["octave"], q["layer"], q["laplacian"]) for _, q in kps}
        want = {(o, l, s) for o in range(4) for l in (1, 2, 3) for s in (-1, 1)}
        need(want <= seen, "no key point of (octave, layer, laplacian) %s" % sorted(want - seen))
        top = [q for n, q in kps if n.startswith("L_top") and q["octave"] == 3 and q["layer"] == 3]
        need(top and max(q["win"] for q in top) > 288, [(q["size"], q["win"]) for q in top])
        need(S.reference(FRAMES["L_symmetric"])["cand"] != [] and not [q for q in S.keypoints(FRAMES["L_symmetric"]) if q["decided"]],
             "the symmetric blob should leave tied candidates and no decided key point")
        return fig + "; (octave, layer, laplacian) triples %d of 24; largest size %g, window %d" % (
            len(seen & want), max(q["size"] for _, q in kps), max(q["win"] for _, q in kps))
    if fam == "W":
        wins = {}
        for _, q in kps:
            wins[q["win"]] = wins.get(q["win"], 0) + 1
        for wv in (42, 84, 128, 131):
            need(wins.get(wv, 0) >= 1, "no window of %d (%s)" % (wv, sorted(wins)))
        gen = [v for v in wins if v % 21]
        need(any(v < 128 for v in gen) and any(v > 128 for v in gen), sorted(wins))
        return fig + "; windows %s" % sorted(wins.items())
    if fam == "B":
        first, last = set(), set()
        cut = [0, 0, 0, 0, 0]
        partial = []
        for n, q in kps:
            h, w = FRAMES[n].shape
            step = 1 << q["octave"]
            mg = ((((9 + 6 * (q["layer"] + 1)) << q["octave"]) // 2) // step) + 1
            rows, cols = h // step, w // step
            for axis, v, lim in (("row", q["i"], rows), ("col", q["j"], cols)):
                if v == mg:
                    first.add((q["octave"], axis))
                if v == lim - mg - 1:
                    last.add((q["octave"], axis))
            if 1 <= q["nangle"] < 113:
                partial.append(q["nangle"])
            r = q["win"] * 0.5          # the window's inner circle: cut for every angle
            sides = (q["x"] - r < 0, q["y"] - r < 0, q["x"] + r > w - 1, q["y"] + r > h - 1)
            for s in range(4):
                cut[s] += int(sides[s])
            cut[4] += int((sides[0] or sides[2]) and (sides[1] or sides[3]))
        want = {(o, a) for o in range(3) for a in ("row", "col")}
        need(want <= first and want <= last, "first %s last %s" % (sorted(want - first), sorted(want - last)))
        need(partial and min(partial) < 100 and max(partial) == 112, sorted(partial))
        need(min(cut) >= 1, cut)
        partial = (len(partial), min(partial or [0]), max(partial or [0]))
        return fig + "; margin samples first %s last %s; nangle below 113 (count, least, most): %s; windows cut left / top / right / bottom / corner %s" % (
            sorted(first), sorted(last), partial, cut)
    if fam == "G":
        built = {}
        for n in FAMILIES[fam]:
            h, w = FRAMES[n].shape
            built[n] = sum(1 for L in S.reference(FRAMES[n])["H"] if L["built"])
        for s in GEOMETRY_SIZES:
            for a in "hw":
                b = [built["G_%s%03d%+d" % (a, s, d)] for d in (-1, 0, 1)]
                need(b[0] + 1 == b[1] == b[2], (a, s, b))
        need(len([q for q in S.keypoints(FRAMES["G_tiny"]) if q["decided"] and not q["deleted"]]) >= 1, "no key point in 24 x 24")
        strides = {(FRAMES[n].shape[1] + 1) % 16 for n in FAMILIES[fam]}
        return fig + "; %d frames, %d key points; layers built per frame %d .. %d; (w + 1) %% 16 takes %d values" % (
            len(FAMILIES[fam]), len(kps), min(built.values()), max(built.values()), len(strides))
    if fam == "T":
        low = S.candidates(FRAMES["T_contrast"], 200.0)[1]
        r = sorted(c["response"] / 400.0 for c in low if c["sure"])
        under, over = [v for v in r if v < 1], [v for v in r if v >= 1]
        need(under and max(under) > 0.95 and over and min(over) < 1.05, (under[-3:], over[:3]))
        comp = [float(np.abs(q["fit"]).max()) for _, q in kps]
        need(comp and max(comp) > 0.9, max(comp or [0]))
        half = []
        for _, q in kps:
            v = ((9 + 6 * q["layer"]) << q["octave"]) + q["fit"][2] * (6 << q["octave"])
            half.append(abs(v - np.floor(v) - 0.5))
        need(half and min(half) < 0.02, min(half or [1]))
        cand = [c for n in FAMILIES[fam] for c in S.reference(FRAMES[n])["cand"] if c["sure"] and c["fit_decided"] and c["rec"] is None]
        need(len(cand) >= 1, "no decided reject of the fit")
        return fig + "; responses / 400 closest to 1: %.4f under, %.4f over; largest accepted |x_i| %.4f; decided rejects of the fit %d; fitted size closest to a half: %.4f off" % (
            max(under or [0]), min(over or [0]), max(comp or [0]), len(cand), min(half or [1]))
    if fam == "O":
        quad = {int(q["angle"] // 90) for _, q in kps if q["angle_decided"]}
        wrap = [q["angle"] for _, q in kps if q["angle_decided"] and (q["angle"] < 7.5 or q["angle"] > 352.5)]
        need(quad == {0, 1, 2, 3} and wrap, (quad, wrap))
        iso = [q for q in S.keypoints(FRAMES["O_iso"]) if q["decided"] and not q["deleted"]]
        need(iso and sum(1 for q in iso if not q["angle_decided"]) >= 1, "O_iso has no undecided argmax")
        return fig + "; quadrants %s, %d angles within 7.5 degrees of the wrap; O_iso: %d of %d key points with an undecided argmax" % (
            sorted(quad), len(wrap), sum(1 for q in iso if not q["angle_decided"]), len(iso))
    if fam == "R":
        groups = {}
        for n, q in kps:
            groups.setdefault((n, q["response"], q["size"], q["octave"]), []).append((q["y"], q["x"]))
        big = [v for v in groups.values() if len(v) >= 2]
        need(len(big) >= 5, len(big))
        need(any(len({y for y, _ in v}) < len(v) for v in big) and any(len({y for y, _ in v}) > 1 for v in big), "ties in y and in x")
        return fig + "; %d groups of equal response, size and octave, the largest of %d" % (len(big), max(len(v) for v in big))
    if fam == "S":
        need(len([q for n, q in kps if n.startswith("S_binary")]) >= 20, "few key points on the binary frames")
        need(not S.reference(FRAMES["S_white"])["cand"], "a frame of 255 has a candidate")
        return fig + "; %d key points on binary frames" % len([q for n, q in kps if n.startswith("S_binary")])
    raise KeyError(fam)
