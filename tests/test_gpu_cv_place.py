"""GPU: the row-major placement of the reference-order selection (k_cv_band_base + k_cv_place, evenvizion_amd/csrc/evh_detect_selcv.h).
Every FAST tile leaves its corners as one burst; the placement puts the bursts of a level into (y, x) order band by band (a band =
one row of 128 x 28 tiles, origin (24, 31)), and KeyPointsFilter::retainBest then permutes that sequence, so with ties one
misplaced corner changes the order of the key points and even the surviving set.  Each frame is compared with the oracle on
order, octave, level coordinates, response bits and descriptors.

Frames are dot lattices (flat background 0, one pixel of value score + 1 per site, sites at least 5 apart, two faint pixels per
dot off every ring that vary the Harris response): level 0 has exactly the dots as corners with exactly those scores.  The shapes
are the smallest at which the placement can go wrong: dots on both sides of every tile and band seam, empty bands, tiles and
frames, one-tile levels, 30 tiles per band, dense noise (tiles that take k_fast_main's dense fall-back), two geometries on one
context."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from evenvizion_amd._lib import Context  # noqa: E402
from oracle import oracle as O  # noqa: E402

OX, OY, TW, TH = 24, 31, 128, 28   # FAST tile grid
QUOTA0 = 109                       # level-0 quota at 500 features


def scores_of(kind, n, rng):
    if kind == "three":
        return rng.choice([60, 61, 200], n)
    if kind == "equal":
        return np.full(n, 137)
    raise ValueError(kind)


def axis(lo, hi, anchors, pitch=5):
    """ascending coordinates in [lo, hi), at least `pitch` apart, that contain every anchor"""
    out, cur = [], lo
    for a in sorted(anchors) + [None]:
        stop = hi - 1 if a is None else a - pitch
        while cur <= stop:
            out.append(cur)
            cur += pitch
        if a is not None:
            out.append(a)
            cur = a + pitch
    return out


def dots(w, h, sites, scores, rng):
    """sites: (x, y) in row-major order; the frame with one dot per site"""
    xs = np.array([s[0] for s in sites], np.int64)
    ys = np.array([s[1] for s in sites], np.int64)
    img = np.zeros((h, w), np.uint8)
    if len(sites):
        img[ys, xs] = np.asarray(scores) + 1
        img[ys + 1, xs + 1] = rng.integers(0, 21, len(sites))
        img[ys - 1, xs + 1] = rng.integers(0, 21, len(sites))
    return img


def grid(xs, ys):
    return [(x, y) for y in ys for x in xs]


def same_keypoints(g, o):
    return (len(g["xy"]) == len(o["xy"]) and all(np.array_equal(g[k], o[k]) for k in ("octave", "lx", "ly"))
            and np.array_equal(g["xy"], o["xy"]) and np.array_equal(g["desc"], o["desc"])
            and np.array_equal(g["response"].view(np.uint32), o["response"].view(np.uint32)))


def check_frames(c, frames, level0=None):
    """one orb_detect_batch over the frames, each against the oracle; level0[f] = the scores level 0 must have, row-major"""
    cap = c.lib.evh_orb_capacity(c.h)
    c.orb_detect_batch(torch.from_numpy(np.ascontiguousarray(frames)).cuda())
    for f, img in enumerate(frames):
        if level0 is not None and level0[f] is not None:
            xs, ys, sc = O.fast_nms(img)
            order = np.lexsort((xs, ys))
            assert np.array_equal(sc[order], np.asarray(level0[f])), f      # exactly the dots, with the chosen scores
        want = O.orb_detect(img)
        assert len(want["xy"]) <= cap, (f, len(want["xy"]), cap)
        assert same_keypoints(c.orb_download(f), want), f


def context(w, h, nframes):
    return Context(device=0, max_w=max(64, w), max_h=max(64, h), max_features=500, max_frames=max(2, nframes))


def seam_sites(w, h, ax, ay):
    """a sparse lattice around the seams of a w x h frame: the column seam - 1 + ax of every tile seam with two columns on
    either side, the row seam - 1 + ay of every band seam likewise, and the first and last admissible column and row"""
    tile_seams = list(range(OX + TW, w - 31, TW))
    band_seams = list(range(OY + TH, h - 31, TH))
    xa = [s - 1 + ax + d for s in tile_seams for d in (-10, -5, 0, 5, 10)] + [31, 90, 215, w - 32 - 2]
    ya = [s - 1 + ay + d for s in band_seams for d in (-5, 0, 5)] + [31, h - 32 - 1]
    return grid(sorted(set(xa)), sorted(set(ya)))


@pytest.mark.parametrize("kind", ["equal", "three"])
def test_dots_on_both_sides_of_every_seam(kind):
    """400 x 224: tile seams at x = 152 and 280, band seams at y = 59, 87, 115, 143, 171.  The four frames put a column on
    x = seam - 1 or seam and a row on y = seam - 1 or seam; the lists are cut to lengths just above 2 * quota = 218."""
    w, h = 400, 224
    rng = np.random.default_rng(31 + len(kind))
    frames, want = [], []
    for ax in (0, 1):
        for ay in (0, 1):
            sites = seam_sites(w, h, ax, ay)
            assert len(sites) > 2 * QUOTA0 + 12
            on_seam = [i for i, (x, y) in enumerate(sites) if (x - OX) % TW in (0, TW - 1) or (y - OY) % TH in (0, TH - 1)]
            free = [i for i in range(len(sites)) if i not in set(on_seam)]
            n = 2 * QUOTA0 + 1 + 2 * ax + 5 * ay                             # 219, 221, 224, 226
            drop = set(rng.choice(free, len(sites) - n, replace=False).tolist())
            sites = [s for i, s in enumerate(sites) if i not in drop]
            for k in range(1, (w - 31 - OX) // TW + 1):                      # both sides of every seam carry dots
                assert any(x == OX + TW * k - 1 + ax for x, _ in sites) and any(x > OX + TW * k for x, _ in sites)
            for k in range(1, (h - 31 - OY) // TH + 1):
                assert any(y == OY + TH * k - 1 + ay for _, y in sites) and any(y > OY + TH * k for _, y in sites)
            s = scores_of(kind, len(sites), rng)
            frames.append(dots(w, h, sites, s, rng))
            want.append(s)
    c = context(w, h, len(frames))
    try:
        check_frames(c, np.stack(frames), want)
    finally:
        c.close()


def test_empty_bands_tiles_levels_and_frames():
    """one batch: bands alternating between empty and full; a band whose only corners lie in its last tile; an all-zero frame
    between busy ones; a level with exactly one corner"""
    w, h = 400, 224
    rng = np.random.default_rng(5)
    xs, ys = list(range(31, w - 31, 5)), list(range(31, h - 31, 5))
    alternating = [(x, y) for x, y in grid(xs, ys) if ((y - OY) // TH) % 2 == 1]
    last_tile = [(x, y) for x, y in grid(xs, ys) if (y - OY) // TH != 2 or x >= OX + 2 * TW]
    one = [(OX + TW + 3, OY + 3 * TH + 1)]
    site_lists = [alternating, [], last_tile, one, grid(xs, ys)]
    assert any((y - OY) // TH == 2 for _, y in last_tile) and len(alternating) > 2 * QUOTA0
    want = [scores_of("three", len(s), rng) for s in site_lists]
    frames = np.stack([dots(w, h, s, sc, rng) for s, sc in zip(site_lists, want)])
    assert not frames[1].any()
    c = context(w, h, len(frames))
    try:
        check_frames(c, frames, want)
    finally:
        c.close()


@pytest.mark.parametrize("w,h", [(2, 2), (183, 90)])
def test_levels_of_one_tile(w, h):
    """level 0 one tile wide and one band high: the smallest frame there is (no pixel far enough from the border to be a corner)
    and the largest one-tile frame, whose tile is filled with dots"""
    rng = np.random.default_rng(w)
    sites = grid(range(31, w - 31, 5), range(31, h - 31, 5))
    assert (len(sites) == 0) == (w == 2)
    s = scores_of("three", len(sites), rng)
    frames = np.stack([dots(w, h, sites, s, rng), dots(w, h, sites[::2], s[::2], rng)])
    c = context(w, h, 2)
    try:
        check_frames(c, frames, [s, s[::2]])
    finally:
        c.close()


def test_widest_band_tables():
    """3840 x 256: 30 tiles per band, seven bands; dots every 5 columns and 10 rows, a column on either side of each seam"""
    w, h = 3840, 256
    rng = np.random.default_rng(38)
    seams = list(range(OX + TW, w - 31, TW))
    assert len(seams) == 29
    sites = grid(axis(31, w - 31, [s - 1 for s in seams[::2]] + [s for s in seams[1::2]]), range(31, h - 31, 10))
    s = scores_of("three", len(sites), rng)
    c = context(w, h, 2)
    try:
        check_frames(c, np.stack([dots(w, h, sites, s, rng), np.zeros((h, w), np.uint8)]), [s, None])
    finally:
        c.close()


@pytest.mark.parametrize("w,h,n", [(400, 224, 4), (1280, 720, 2)])
def test_dense_noise(w, h, n):
    """uniform noise: dense rows, tiles over the queue capacity of k_fast_main (its dense fall-back), long level lists"""
    rng = np.random.default_rng(w + n)
    frames = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    frames[1::2] //= 2                       # another corner density
    c = context(w, h, n)
    try:
        check_frames(c, frames)
    finally:
        c.close()


def test_two_geometries_on_one_context():
    """band bases and totals of an earlier call with another tile grid must not leak into the next"""
    rng = np.random.default_rng(77)
    c = context(640, 360, 3)
    try:
        for w, h in [(640, 360), (400, 224), (183, 90), (640, 360)]:
            sites = grid(range(31, w - 31, 5), range(31, h - 31, 5))
            lists = [sites, sites[len(sites) // 3:], sites[:len(sites) // 2]]
            want = [scores_of("three", len(s), rng) for s in lists]
            check_frames(c, np.stack([dots(w, h, s, sc, rng) for s, sc in zip(lists, want)]), want)
    finally:
        c.close()
