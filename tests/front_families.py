"""Crafted inputs for the image front end (gray, resize(INTER_AREA), ORB's pyramid), each family with what it must reach.
Everything here is built from numpy and the plain restatement (tests/front_checks.py); the premises are asserted in
tests/test_oracle_front_edges.py, so a case that stops reaching its edge fails on the CPU.

T  ties          integer ratios with block sums placed on exact halves (even and odd floor), on 0 and on 255 * area
A  table shapes  fractional ratios barely above 1, exactly 1.5 and 2.5, very long cells, one output pixel, x integral
E  enlarging     both axes enlarged, one axis enlarged and the other shrunk, sources of one row or column
P  pyramid       saturated patterns, impulses at corners, edges and on the tile seams, the exact-half coefficient
S  seams         small frames whose levels 1 and 2 take the widths and heights around the tile sizes
X  extremes      the largest and the smallest frames"""
import functools

import numpy as np

import front_checks as C

# ------------------------------------------------------------------------------------------------------------- T: ties
T_RATIOS = [(2, 2), (4, 4), (2, 4), (4, 2), (1, 2), (2, 1), (1, 4), (8, 8), (3, 3), (2, 3)]          # (isx, isy)
T_DH = 5


def t_geometry(isx, isy, cn):
    """dw * cn = 258 at cn 3 and 257 at cn 1: one element past 256"""
    dw = 86 if cn == 3 else 257
    return dw * isx, T_DH * isy, dw, T_DH


def t_target_sums(area, n, rng):
    """n block sums.  Element e takes by e % 8: 0 the sum nearest a half from below or on it with an even floor, 1 the same with
    an odd floor (areas that are even have sums ON the half: area * k + area / 2; area 9 has 9 k + 4 below and 9 k + 5 above),
    2 the sum 0, 3 the sum 255 * area, the rest noise."""
    e = np.arange(n)
    k = rng.integers(0, 127, n)
    s = rng.integers(0, 255 * area + 1, n)
    if area % 2 == 0:
        s = np.where(e % 8 == 0, area * (2 * k) + area // 2, s)
        s = np.where(e % 8 == 1, area * (2 * k + 1) + area // 2, s)
    else:
        s = np.where(e % 8 == 0, area * k + area // 2, s)
        s = np.where(e % 8 == 1, area * k + area // 2 + 1, s)
    s = np.where(e % 8 == 2, 0, s)
    s = np.where(e % 8 == 3, 255 * area, s)
    return s


def t_image(isx, isy, cn, seed=0):
    """the source image whose isx x isy blocks carry t_target_sums, the sum spread over the block's pixels at random"""
    sw, sh, dw, dh = t_geometry(isx, isy, cn)
    area = isx * isy
    rng = np.random.default_rng(1000 * isx + 10 * isy + cn + seed)
    n = dh * dw * cn
    s = t_target_sums(area, n, rng)
    # spread: base value everywhere, the remainder as + 1 on a random subset, then moved between random pairs while legal
    px = np.repeat((s // area)[:, None], area, axis=1)
    rem = s % area
    order = np.argsort(rng.random((n, area)), axis=1)
    px[np.arange(n)[:, None], order] += (np.arange(area)[None, :] < rem[:, None])
    if area > 1:
        i, j = order[:, 0], order[:, -1]
        room = np.minimum(255 - px[np.arange(n), i], px[np.arange(n), j])
        d = (rng.random(n) * (room + 1)).astype(np.int64)
        d = np.where(i == j, 0, d)
        px[np.arange(n), i] += d
        px[np.arange(n), j] -= d
    assert px.min() >= 0 and px.max() <= 255 and np.array_equal(px.sum(axis=1), s)
    img = px.reshape(dh, dw, cn, isy, isx).transpose(0, 3, 1, 4, 2).reshape(sh, sw, cn).astype(np.uint8)
    return img[:, :, 0] if cn == 1 else img


def t_cases():
    return [("T_%dx%d_c%d" % (isx, isy, cn), isx, isy, cn) for (isx, isy) in T_RATIOS for cn in (1, 3)]


# -------------------------------------------------------------------------------------------------- A and E: geometries
A_BARELY = [(258, 9, 257, 6), (1001, 3, 1000, 2), (259, 9, 257, 6)]   # the third was added: see `a_entry_counts` in the CPU test
A_GEOMETRIES = A_BARELY + [(300, 200, 200, 80), (4095, 5, 17, 2), (4095, 3, 1, 1), (7, 4095, 3, 1), (640, 361, 320, 100)]
E_GEOMETRIES = [(2, 2, 3, 3), (1, 7, 5, 3), (7, 1, 3, 5), (256, 40, 257, 41), (64, 48, 1000, 750), (100, 60, 150, 40),
                (100, 60, 50, 90), (100, 64, 150, 16)]
E_MIXED = [(100, 60, 150, 40), (100, 60, 50, 90), (100, 64, 150, 16)]
CONTENTS = ("noise", "white", "cells")


def content(kind, sw, sh, dw, dh, cn, seed=0):
    """noise; all 255; 0 / 255 cells whose period is the destination pixel's cell, shifted by half a cell so that every
    cell is half 0 and half 255 and the results sit next to a half.  cn 3: three different channels."""
    if kind == "white":
        g = np.full((sh, sw), 255, np.uint8)
    elif kind == "noise":
        g = np.random.default_rng(sw * 31 + sh * 7 + dw + seed).integers(0, 256, (sh, sw), dtype=np.uint8)
    else:
        cx = np.floor((np.arange(sw) + 0.5) * dw / sw + 0.5).astype(np.int64)
        cy = np.floor((np.arange(sh) + 0.5) * dh / sh + 0.5).astype(np.int64)
        g = (((cx[None, :] + cy[:, None]) & 1) * 255).astype(np.uint8)
    if cn == 1:
        return g
    if kind == "white":
        return np.stack([g, g, g], axis=-1)
    return np.stack([g, np.roll(g, 7, axis=1), 255 - g], axis=-1)


def resize_cases():
    """(name, geometry, cn, content) of families A and E"""
    out = []
    for fam, geos in (("A", A_GEOMETRIES), ("E", E_GEOMETRIES)):
        for g in geos:
            for cn in (1, 3):
                for kind in CONTENTS:
                    out.append(("%s_%dx%d_%dx%d_c%d_%s" % ((fam,) + g + (cn, kind)), g, cn, kind))
    return out


def acceptable_orb_frame(dw, dh):
    """what the fused ingest takes as a working size on a 64 x 64 context and larger: no level may be empty"""
    return min(min(s) for s in C.orb_sizes(dw, dh)) >= 1 and dw < 4096 and dh < 4096


# ------------------------------------------------------------------------------------------------------------ P: pyramid
P_W, P_H = 400, 224
P_SIZES = {"P": (400, 224), "P220": (400, 220), "P120": (120, 120)}
TILE_COLS, TILE_ROWS = (127, 128, 255, 256), (31, 32, 63, 64)


def _feeds(size0, idx, level):
    """the level-0 samples that feed sample `idx` of `level` along one axis of `size0`"""
    sizes = [C.orb_sizes(size0, size0)[l][0] for l in range(level + 1)]
    cur = {idx}
    for l in range(level, 0, -1):
        i0, i1, _, _ = C.linear_taps(sizes[l - 1], sizes[l])
        cur = {int(i0[i]) for i in cur} | {int(i1[i]) for i in cur}
    return sorted(cur)


def seam_points(w=P_W, h=P_H):
    """level-0 columns and rows that feed the seam columns / rows of levels 1 and 2"""
    xs, ys = set(), set()
    for level in (1, 2):
        lw, lh = C.orb_sizes(w, h)[level]
        for c in TILE_COLS:
            if c < lw:
                xs.add(_feeds(w, c, level)[0])
        for r in TILE_ROWS:
            if r < lh:
                ys.add(_feeds(h, r, level)[0])
    return sorted(xs), sorted(ys)


def p_frames(w=P_W, h=P_H, tag="P"):
    """{name: gray frame}"""
    P_W, P_H = w, h
    y, x = np.mgrid[0:P_H, 0:P_W]
    z = np.zeros((P_H, P_W), np.uint8)
    f = {}
    for p in (1, 2, 3):
        f["P_checker%d" % p] = ((((x // p) + (y // p)) & 1) * 255).astype(np.uint8)
    f["P_vstripes"] = ((x & 1) * 255).astype(np.uint8)
    f["P_hstripes"] = ((y & 1) * 255).astype(np.uint8)
    f["P_black"] = z.copy()
    f["P_white"] = np.full((P_H, P_W), 255, np.uint8)
    c = z.copy()
    c[0, 0] = c[0, -1] = c[-1, 0] = c[-1, -1] = 255
    f["P_corners"] = c
    e = z.copy()
    e[-1, 5::37] = 255
    e[7::29, -1] = 255
    f["P_last_row_col"] = e
    s = z.copy()
    xs, ys = seam_points(w, h)
    for xx in xs:
        for yy in ys:
            s[yy, xx] = 255
    f["P_seams"] = s
    return {k.replace("P_", tag + "_"): v for k, v in f.items()}


def p220_frames():
    """400 x 220: the geometry whose level 7 (74 -> 61 rows) takes the 128 x 64 tile kernel; 400 x 224 walks at every level"""
    f = p_frames(400, 220, "P220")
    return {k: f[k] for k in ("P220_checker1", "P220_hstripes", "P220_corners", "P220_seams", "P220_white")}


def p120_frames():
    """120 x 120: level 1 is exactly 1 / 1.2 of it, the right-tap weight is 128 at every column and row v % 5 == 2"""
    y, x = np.mgrid[0:120, 0:120]
    rng = np.random.default_rng(120)
    return {"P120_vstripes": ((x & 1) * 255).astype(np.uint8),
            "P120_checker1": (((x + y) & 1) * 255).astype(np.uint8),
            "P120_low_noise": rng.integers(0, 4, (120, 120), dtype=np.uint8)}


# -------------------------------------------------------------------------------------------------------------- S: seams
SEAM_WIDTHS, SEAM_HEIGHTS = (127, 128, 129, 255, 256, 257), (31, 32, 33, 63, 64, 65)
S_LIMIT = 400


def walks(src, dst):
    """the launcher's condition for the row-walking pyramid kernel (else the 128 x 64 tile kernel): the level shrinks by at
    most 1.21 on both axes and has at least two columns and rows"""
    return src[0] * 100 <= dst[0] * 121 and src[1] * 100 <= dst[1] * 121 and dst[0] >= 2 and dst[1] >= 2


def kernel_of_levels(w, h):
    """per level 1 .. 7: 'walk' or 'down', predicted from the restated sizes"""
    sz = C.orb_sizes(w, h)
    return ["walk" if walks(sz[l - 1], sz[l]) else "down" for l in range(1, C.NLEVELS)]


def staged_residues(w, h):
    """{xofs[x0] & 15} over the tile starts x0 of every level >= 2 of a w x h frame: the first staged column of a tile is
    xofs[x0] & ~15, so this is where the tile's first tap sits in its staged row.  The tile is 256 wide where the level takes
    the walking kernel and 128 where it takes the other."""
    sz = C.orb_sizes(w, h)
    kinds = kernel_of_levels(w, h)
    out = set()
    for l in range(2, C.NLEVELS):
        i0 = C.linear_taps(sz[l - 1][0], sz[l][0])[0]
        out |= {int(i0[x0]) & 15 for x0 in range(0, sz[l][0], 256 if kinds[l - 1] == "walk" else 128)}
    return out


def _first_side(want, limit):
    """the smallest frame side whose level 1 or 2 measures `want`"""
    for v in range(2, limit + 1):
        sz = C.orb_sizes(v, v)
        if want in (sz[1][0], sz[2][0]):
            return v
    raise AssertionError("no frame side up to %d gives a level of %d" % (limit, want))


S_DOWN_HEIGHT = 5          # 5 -> 4 -> 3 rows: level 2 shrinks by 1.33 and takes the 128-wide tiles


def _add_residues(frames, have, widths, heights):
    for w in widths:
        for h in heights:
            add = staged_residues(w, h) - have
            if add:
                frames.append((w, h))
                have |= add
    return have


@functools.lru_cache(maxsize=None)
def s_frames(limit=S_LIMIT):
    """The sweep, by search on the restated level sizes: for every listed width the smallest frame width whose level 1 or 2 has
    it, for every listed height likewise, paired in order; then, from `limit` downwards, every width that adds a residue of the
    staged start, at a height that keeps the walking kernel and at one that does not."""
    ws = [_first_side(v, limit) for v in SEAM_WIDTHS]
    hs = [_first_side(v, limit) for v in SEAM_HEIGHTS]
    frames = list(zip(ws, hs))
    have = set().union(*[staged_residues(w, h) for w, h in frames])
    _add_residues(frames, have, range(limit, 128, -1), (hs[-1], S_DOWN_HEIGHT))
    return tuple(frames)


@functools.lru_cache(maxsize=None)
def s_wide_frames(limit=S_LIMIT):
    """Residues of the staged start that no frame within `limit` reaches need a fourth 128-wide tile column at a level >= 2,
    hence a frame wider than the limit; these few frames supply them, the narrowest first."""
    have = set().union(*[staged_residues(w, h) for w, h in s_frames(limit)])
    frames = []
    for w in range(limit + 1, 2048):
        have = _add_residues(frames, have, (w,), (S_DOWN_HEIGHT,))
        if len(have) == 16:
            break
    return tuple(frames)


# ----------------------------------------------------------------------------------------------------------- X: extremes
X_LARGE = [(4095, 64), (64, 4095)]
X_SMALL = [(2, 2), (5, 9), (17, 40), (63, 63)]
X_REFUSED = [(1, 1), (1, 40), (40, 1)]          # a side of 1 makes a level of size 0


def noise_frames(w, h, n, cn=1, seed=0):
    shape = (n, h, w) if cn == 1 else (n, h, w, cn)
    return np.random.default_rng(w * 4099 + h + seed).integers(0, 256, shape, dtype=np.uint8)
