"""Seeded crafted frames for ORB's describe stage (Harris response, intensity-centroid orientation, 7 x 7 fixed-point Gaussian,
steered BRIEF taps: harris_response in evh_detect_select.h, k_describe in evh_detect_describe.h), driving its edges on purpose.

  S  saturation      bright regions whose blurred value reaches 256 / 257 before the saturating store
  A  orientation     moments that are exactly zero, every octant and both branches of fastAtan2, the axes and the diagonals
  P  window phases   every alignment of the staged 45-byte patch rows (cx mod 16, (cx - 22) mod 4) and the 31-pixel border
  H  Harris extremes gradient sums beyond 2^24, responses of both signs, a selection that has to cut
  R  tap rounding    many distinct angles over dense texture

FRAMES maps a name (family letter first) to a gray frame of at most 256 x 192.  info(name) holds what the oracle and the plain
restatement (tests/describe_checks.py) say of a frame, computed once; check_premise(family) asserts on the CPU that the family
still is what its name says.  tests/test_oracle_describe_edges.py and tests/test_gpu_describe_edges.py run them."""
import functools

import numpy as np

import describe_checks as D
from oracle import oracle as O

W, H = 256, 192            # width 256: the level-0 rows are as long as their stride
WS, HS = 224, 160          # the second frame size (its level-0 rows are padded to 256)
BORDER = 31
NLEVELS = 8


# ------------------------------------------------------------------------------------------------------------------ S
def _squares(rng, w, h, n, lo, hi, gap=4):
    """n disjoint squares (x, y, size) with sides lo .. hi, `gap` pixels apart, inside the frame"""
    out = []
    for _ in range(10000):
        s = int(rng.integers(lo, hi + 1))
        x, y = int(rng.integers(8, w - 8 - s)), int(rng.integers(8, h - 8 - s))
        if all(x + s + gap <= a or a + t + gap <= x or y + s + gap <= b or b + t + gap <= y for a, b, t in out):
            out.append((x, y, s))
            if len(out) == n:
                return out
    raise AssertionError("squares do not fit")


def _square_frame(w, h, ground, value, seed=5):
    """ten squares of `value` on `ground`.  A square's corner and its diagonal neighbour score alike at level 0 and suppress each
    other, so the larger squares also carry single pixels of the ground's value: corners with a flat neighbourhood of `value`"""
    img = np.full((h, w), ground, np.uint8)
    for x, y, s in _squares(np.random.default_rng(seed), w, h, 10, 18, 44):
        img[y:y + s, x:x + s] = value
        if s >= 26:
            img[y + s // 2, x + s // 3] = ground
            img[y + s // 3, x + s - 9] = ground
    return img


def _ramp_frame():
    """columns rise from 250 to 255; dark marks of 2 .. 5 pixels, every pixel of a mark another value (no tied scores)"""
    rng = np.random.default_rng(6)
    img = np.tile(np.rint(np.linspace(250, 255, W)).astype(np.uint8), (H, 1))
    for x, y, s in _squares(rng, W, H, 60, 2, 5, gap=9):
        img[y:y + s, x:x + s] = rng.integers(0, 120, (s, s))
    return img


def _marks_frame(seed, shift=(0, 0)):
    """a field of 255 with dark marks of unlike shapes (so that descriptors differ and a pair of such frames matches)"""
    rng = np.random.default_rng(seed)
    img = np.full((H + 16, W + 16), 255, np.uint8)
    for x, y, s in _squares(rng, W + 16, H + 16, 45, 5, 14, gap=6):
        cell = rng.integers(0, 3, (s, s)) > 0
        img[y:y + s, x:x + s] = np.where(cell, rng.integers(0, 90), 255)
    return np.ascontiguousarray(img[8 + shift[1]:8 + shift[1] + H, 8 + shift[0]:8 + shift[0] + W])


# ------------------------------------------------------------------------------------------------------------------ A
def _lattice_frame():
    """single pixels of 255 on 0, 20 apart: no other pixel inside a key point's radius-15 disc, the centre weighs 0"""
    img = np.zeros((H, W), np.uint8)
    img[36:H - 31:20, 38:W - 31:20] = 255
    return img


def _dihedral(stamp):
    return [np.rot90(m, k) for m in (stamp, stamp[:, ::-1]) for k in range(4)]


def _dihedral_frame():
    """one asymmetric blob (seeded, 9 x 9 cells of 0 / 90 .. 255 in a 21 x 21 stamp) in its eight dihedral copies, 56 apart"""
    rng = np.random.default_rng(7)
    stamp = np.zeros((21, 21), np.uint8)
    blob = np.where(rng.integers(0, 2, (9, 9)) > 0, rng.integers(90, 256, (9, 9)), 0)
    blob[4, 4] = 255
    stamp[6:15, 6:15] = blob
    img = np.zeros((H, W), np.uint8)
    for i, m in enumerate(_dihedral(stamp)):
        x, y = 34 + 56 * (i % 4), 40 + 70 * (i // 4)
        img[y:y + 21, x:x + 21] = m
    return img


def _mirror_frame():
    """wedges symmetric about a vertical / horizontal axis with their tip on it (m10 = 0 or m01 = 0, both signs of the other
    moment) and squares whose brightness falls along the diagonal, a corner on it (|m10| = |m01|, all four sign pairs).  The
    brightness falls away from the tip / the corner, so the FAST score has a single maximum there."""
    wedge = np.zeros((25, 25), np.uint8)
    for r in range(10):
        wedge[7 + r, 12 - r // 2:12 + r // 2 + 1] = 255 - 12 * r        # tip at (12, 7), body below: m10 = 0, m01 > 0
    sq = np.zeros((25, 25), np.uint8)
    u, v = np.meshgrid(np.arange(12), np.arange(12))
    sq[8:20, 8:20] = 255 - 8 * (u + v)                                    # corner at (8, 8), symmetric about the diagonal
    img = np.zeros((H, W), np.uint8)
    for i, m in enumerate([np.rot90(wedge, k) for k in range(4)] + [np.rot90(sq, k) for k in range(4)]):
        x, y = 36 + 52 * (i % 4), 40 + 70 * (i // 4)
        img[y:y + 25, x:x + 25] = m
    return img


RIM_DOTS = [(48 + 54 * i, 48 + 48 * j) for j in range(3) for i in range(4)]


def _rim_mask():
    yy, xx = np.mgrid[-20:21, -20:21]
    r2 = xx * xx + yy * yy
    return (r2 >= 10 * 10) & (r2 <= 20 * 20)


def _rim_frame():
    """single pixels of 255, each inside a seeded annulus of radii 10 .. 20 without a zero in it: every pixel on either side
    of the edge of the key point's radius-15 disc carries weight, so the disc has to end exactly where the circle rule says"""
    rng = np.random.default_rng(16)
    img = np.zeros((H, W), np.uint8)
    rim = _rim_mask()
    for x, y in RIM_DOTS:
        patch = img[y - 20:y + 21, x - 20:x + 21]
        patch[rim] = rng.integers(1, 36, int(rim.sum()))
        img[y, x] = 255
    return img


# ------------------------------------------------------------------------------------------------------------------ P
def _phase_dots():
    """(x, y) of the dots: rows 20 apart starting on the border row y = 31, pitch 17 in x, each row starting 5 further right;
    the last row is the border row y = H - 32; dots on the border columns x = 31 and x = W - 32 close every row"""
    pts = set()
    rows = list(range(BORDER, H - BORDER - 10, 20)) + [H - BORDER - 1]
    for j, y in enumerate(rows):
        for x in range(BORDER + 9 + (5 * j) % 17, W - BORDER - 9, 17):
            pts.add((x, y))
        pts.add((BORDER, y)); pts.add((W - BORDER - 1, y))
    return sorted(pts)


def _phase_frame():
    """dots of unlike brightness (160 .. 255) on 0; pitch 17 < 31, so every disc holds neighbours and the angles are general"""
    rng = np.random.default_rng(8)
    img = np.zeros((H, W), np.uint8)
    for x, y in _phase_dots():
        img[y, x] = int(rng.integers(160, 256))
    return img


# ------------------------------------------------------------------------------------------------------------------ H
def _harris_frame(seed):
    """blocks of 0 / 255 stripes (2 pixels wide: every Sobel column sum is +-1020), blocks tiled 8 x 8 and 6 x 6 with upright and level
    stripes in turn (a 7 x 7 window half over each has both gradient sums near 49 * 1020^2 / 2 = 2.5e7 > 2^24), checkers and seeded
    binary cells, on flat ground of 0, 128 and 250; black is 0 .. 8 and white 247 .. 255 (seeded)"""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), 128, np.uint8)
    img[:, :W // 3] = 0
    img[:, 2 * W // 3:] = 250          # the bright ground stays below 253.52: this family's blur never saturates
    yy, xx = np.mgrid[0:40, 0:40]
    up, level = ((xx // 2) % 2) * 255, ((yy // 2) % 2) * 255
    kinds = [up, level, (((xx + yy) // 3) % 2) * 255, ((xx // 2 + yy // 2) % 2) * 255,
             np.where((xx // 8 + yy // 8) % 2 > 0, up, level), np.kron(rng.integers(0, 2, (20, 20)), np.ones((2, 2), int)) * 255,
             up * (yy % 8 < 6), np.where((xx // 6 + yy // 6) % 2 > 0, up, level)]
    order = rng.permutation(len(kinds))
    for i, k in enumerate(order):
        x, y = 12 + 60 * (i % 4), 34 + 76 * (i // 4)
        s = 40 if i % 2 == 0 else 34
        jitter = rng.integers(0, 9, (s, s))           # 0 .. 8 off black / white: no two neighbouring corners score alike
        img[y:y + s, x:x + s] = np.where(kinds[k][:s, :s] > 0, 255 - jitter, jitter)
    return img


# ------------------------------------------------------------------------------------------------------------------ R
def _rotated_texture_frame(seed, first_angle):
    """stamps of one dense seeded texture (3-pixel cells, smoothed once), each turned 1 degree further than the one before"""
    rng = np.random.default_rng(seed)
    cells = rng.integers(0, 256, (40, 40)).astype(np.float64)
    tex = np.kron(cells, np.ones((3, 3)))
    tex = (tex + np.roll(tex, 1, 0) + np.roll(tex, 1, 1) + np.roll(tex, (1, 1), (0, 1))) / 4
    img = np.full((H, W), 20, np.uint8)
    yy, xx = np.mgrid[0:44, 0:44] - 21.5
    for i in range(12):
        t = np.radians(first_angle + i)
        sx = np.rint(60 + xx * np.cos(t) + yy * np.sin(t)).astype(int)
        sy = np.rint(60 - xx * np.sin(t) + yy * np.cos(t)).astype(int)
        x, y = 28 + 50 * (i % 4), 26 + 48 * (i // 4)
        img[y:y + 44, x:x + 44] = tex[sy, sx].astype(np.uint8)
    return img


def _make_frames():
    f = {}
    for v in (255, 254, 253):
        for g in (30, 200):
            f["S_sq%d_bg%d" % (v, g)] = _square_frame(WS, HS, g, v)
    f["S_black_on_255"] = _square_frame(W, H, 255, 0, seed=9)
    f["S_ramp"] = _ramp_frame()
    f["S_marks_a"] = _marks_frame(10)
    f["S_marks_b"] = _marks_frame(10, shift=(5, 3))
    f["A_lattice"] = _lattice_frame()
    f["A_dihedral"] = _dihedral_frame()
    f["A_mirror"] = _mirror_frame()
    f["A_rim"] = _rim_frame()
    f["P_phases"] = _phase_frame()
    f["H_blocks_a"] = _harris_frame(12)
    f["H_blocks_b"] = np.ascontiguousarray(_harris_frame(13)[::-1, ::-1])
    f["R_texture_a"] = _rotated_texture_frame(14, 0)
    f["R_texture_b"] = _rotated_texture_frame(15, 12)
    for k, v in f.items():
        assert v.dtype == np.uint8 and v.ndim == 2 and v.shape[0] <= 192 and v.shape[1] <= 256, k
        v.setflags(write=False)
    return f


FRAMES = _make_frames()
FAMILIES = {c: sorted(n for n in FRAMES if n[0] == c) for c in "SAPHR"}
STREAM_PAIR = ("S_marks_a", "S_marks_b")      # the second is the first moved by (5, 3): one pair for the ordinary pair entry


def by_size():
    """{(w, h): names}: the batches of frames of equal size"""
    out = {}
    for n in sorted(FRAMES):
        out.setdefault(FRAMES[n].shape[::-1], []).append(n)
    return out


# ------------------------------------------------------------------------------------------------- what is known of a frame
@functools.lru_cache(maxsize=None)
def info(name):
    """pyr: the oracle's 8 levels; blur / clipped: blur7_u8 of each; kp: O.orb_detect in the reference order; kp0: the same in
    the canonical order; mom: the plain (m10, m01) of every key point of kp.  Treat all of it as read-only."""
    img = FRAMES[name]
    pyr = O.orb_pyramid(img)
    bc = [D.blur7_u8(p) for p in pyr]
    prev = O.get_orb_order()
    try:
        O.set_orb_order(1); kp = O.orb_detect(img)
        O.set_orb_order(0); kp0 = O.orb_detect(img)
    finally:
        O.set_orb_order(prev)
    mom = [D.moments(pyr[l], x, y) for l, x, y in zip(kp["octave"].tolist(), kp["lx"].tolist(), kp["ly"].tolist())]
    return dict(pyr=pyr, blur=[b for b, _ in bc], clipped=[c for _, c in bc], kp=kp, kp0=kp0, mom=mom)


def clip_near(name):
    """per key point: does a clipped blur pixel lie within the 19-pixel reach of its taps?"""
    i = info(name)
    r = D.TAP_REACH
    return np.array([bool(i["clipped"][l][y - r:y + r + 1, x - r:x + r + 1].any())
                     for l, x, y in zip(i["kp"]["octave"].tolist(), i["kp"]["lx"].tolist(), i["kp"]["ly"].tolist())], bool)


def half_integer_share(name):
    """(taps within 1e-4 of a half-integer in float64, all taps) over the key points of a frame, by the plain restatement alone"""
    i = info(name)
    near = 0
    for l, x, y, a in zip(i["kp"]["octave"].tolist(), i["kp"]["lx"].tolist(), i["kp"]["ly"].tolist(), i["kp"]["angle"]):
        near += int(D.brief_bits(i["blur"][l], x, y, a)[2].sum())
    return near, 256 * len(i["kp"]["lx"])


def candidates_f64(name, level):
    """[(x, y, a, b, response in float64)] of the level's candidates (the corners Harris is computed for)"""
    lv = info(name)["pyr"][level]
    lq = O.orb_layout(FRAMES[name].shape[1], FRAMES[name].shape[0], 500)[3]
    xs, ys, _ = O.orb_level_candidates(lv, int(lq[level]))
    out = []
    for x, y in zip(xs.tolist(), ys.tolist()):
        a, b, _ = D.sobel_sums(lv, x, y)
        out.append((x, y, a, b, D.harris_f64(lv, x, y)))
    return out


OCTANTS = {sx + sy + o for sx in ("+x", "-x") for sy in ("+y", "-y") for o in ("<", ">")}
AXES = {"+x0y>", "-x0y>", "0x+y<", "0x-y<"}
DIAGONALS = {sx + sy + "=" for sx in ("+x", "-x") for sy in ("+y", "-y")}


def check_premise(fam):
    """asserts that the frames of family `fam` are what the family is for; returns a line of figures for the log"""
    names = FAMILIES[fam]
    assert names
    for n in names:
        k = info(n)["kp"]
        assert len(k["lx"]) >= 8, (n, len(k["lx"]))
        # the descriptor stage recovers the centre from the scaled position: it must be the level position itself
        lw, lh, ls, _ = O.orb_layout(FRAMES[n].shape[1], FRAMES[n].shape[0], 500)
        s = ls[k["octave"]].astype(np.float32)
        inv = (np.float32(1) / s).astype(np.float32)
        assert np.array_equal(np.rint(k["xy"][:, 0] * inv).astype(int), k["lx"]) and np.array_equal(np.rint(k["xy"][:, 1] * inv).astype(int), k["ly"]), n
    if fam == "S":
        fig = []
        for n in names:
            near, oc = clip_near(n), info(n)["kp"]["octave"]
            levels = sorted(set(oc[near].tolist()))
            fig.append("%s %d/%d levels %s" % (n, near.sum(), len(near), levels))
            if "253" in n:
                assert not near.any() and not any(c.any() for c in info(n)["clipped"]), n
            elif n == "S_ramp":         # the ramp crosses 253.52: both kinds of key point, a fifth of them each at the least
                assert 5 * near.sum() >= len(near) and 5 * (~near).sum() >= len(near), (n, near.sum(), len(near))
            else:
                assert 2 * near.sum() >= len(near) and len(levels) >= 3, (n, near.sum(), len(near), levels)
        return "; ".join(fig)
    if fam == "A":
        classes = {}
        for n in names:
            i = info(n)
            cl = [D.moment_class(*m) for m in i["mom"]]
            for c in cl:
                classes[c] = classes.get(c, 0) + 1
            if n == "A_lattice":
                at0 = i["kp"]["octave"] == 0
                assert at0.sum() >= 40 and all(c == "zero" for c, z in zip(cl, at0) if z), n
        k, rim = info("A_rim")["kp"], _rim_mask()
        dots = {(x, y) for l, x, y in zip(k["octave"].tolist(), k["lx"].tolist(), k["ly"].tolist()) if l == 0}
        assert set(RIM_DOTS) <= dots, sorted(set(RIM_DOTS) - dots)
        assert all((FRAMES["A_rim"][y - 20:y + 21, x - 20:x + 21][rim] > 0).all() for x, y in RIM_DOTS)
        need = OCTANTS | AXES | DIAGONALS | {"zero"}
        assert need <= set(classes), sorted(need - set(classes))
        return "classes %s" % sorted(classes.items())
    if fam == "P":
        k = info("P_phases")["kp"]
        fig = []
        full = []
        for l in range(NLEVELS):
            x = k["lx"][k["octave"] == l]
            p16, p4 = set((x % 16).tolist()), set(((x - 22) % 4).tolist())
            fig.append("level %d: %d of 16, %d of 4" % (l, len(p16), len(p4)))
            if len(p16) == 16 and len(p4) == 4:
                full.append(l)
        assert 0 in full and len(full) >= 2, fig
        at0 = k["octave"] == 0
        x, y = k["lx"][at0], k["ly"][at0]
        assert x.min() == BORDER and x.max() == W - BORDER - 1 and y.min() == BORDER and y.max() == H - BORDER - 1
        assert FRAMES["P_phases"].shape[1] % 64 == 0          # rows as long as their 64-byte-padded stride
        return "; ".join(fig)
    if fam == "H":
        big = neg = cut = 0
        for n in names:
            i = info(n)
            lq = O.orb_layout(FRAMES[n].shape[1], FRAMES[n].shape[0], 500)[3]
            for l in range(NLEVELS):
                c = candidates_f64(n, l)
                big += sum(1 for _, _, a, b, _ in c if a > 2 ** 24 and b > 2 ** 24)
                cut += int(len(c) > lq[l])
            neg += int((i["kp"]["response"] < 0).sum())
        assert big >= 1 and neg >= 1 and cut >= 1, (big, neg, cut)
        assert not any(c.any() for n in names for c in info(n)["clipped"])
        return "candidates with a, b > 2^24: %d; negative responses kept: %d; levels where the selection cuts: %d" % (big, neg, cut)
    if fam == "R":
        angles = np.concatenate([info(n)["kp"]["angle"] for n in names])
        distinct = len(np.unique(angles))
        assert distinct >= 200 and len(np.unique(np.floor(angles / 10))) == 36, distinct      # every 10-degree sector
        near = [half_integer_share(n) for n in names]
        return "%d distinct angles; taps within 1e-4 of a half-integer: %s" % (distinct, near)
    raise KeyError(fam)
