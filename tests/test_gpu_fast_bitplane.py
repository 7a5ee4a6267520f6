"""GPU: the bit-plane segment test of k_fast_main in the reference key-point order (evh_detect_fast.h: fast_plane_scores --
bp_planes_item, bp_segment32 on 32 pixels per word for the 4 groups of a tile, fast_corner_px for the columns x0 - 1 and
x0 + 128, the queue pushed from mask words).

Every case runs the frame and its 180-degree turn as a batch of two and compares, per pyramid level,
  * the candidate list (position and score of every survivor of the 3 x 3 maximum test) with the oracle's,
  * the same list with the one the dense kernel leaves (set_fast_lift(False)),
  * the key points and descriptors in the reference order with the oracle's.

Cases (320 x 160: 3 x 4 tiles with origin x = 24 + 128 tx, y = 31 + 28 ty; 97 x 131: one tile column, an odd width):
  noise        uniform noise, both polarities in every word;
  dense        62 % corners: the full tiles overflow the queue (PQ_CAP) and take the dense fall-back, the edge tiles do not;
  edges_top / edges_bottom   isolated corners of both polarities (255 and 0 on 128) in the group columns 0, 1, 2, 29, 30, 31 of
               every group -- every ring offset dx = +-1 .. +-3 crosses a word boundary, columns 0 and 127 are the tile's own
               edges -- on tile rows 0, 10, 20 / 7, 17, 27;
  halo         pairs of corners side by side across a tile's right edge, its lower edge and its lower right corner, so that one
               of the two lies in the halo column x0 + 128 / x0 - 1 or the halo row y0 + 28 / y0 - 1 of the other's tile: equal
               values (neither survives) and 250 beside 255 in either order (only the 255 survives), both polarities;
  ends         noise of values 0 .. 41 and 214 .. 255: centres below 21 (no darker ring possible: the borrow) and above 234 (the carry);
  empty        no corner.
The frames are checked on the CPU, from the definition of a corner, to be what they are meant to be."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from evenvizion_amd._lib import Context  # noqa: E402
from oracle import oracle as O  # noqa: E402

W, H = 320, 160
OX, OY, TW, TH = 24, 31, 128, 28          # tile grid of k_fast_main
PQ_CAP = 2 * 30 * 34                      # corners a tile's queue holds
GROUP_COLS = (0, 1, 2, 29, 30, 31)
ROW_SLOTS = {"top": (0, 10, 20), "bottom": (7, 17, 27)}

RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0),
        (-3, 1), (-2, 2), (-1, 3)]


def tiles(w, h):
    """(tx, ty, x0, y0) of the level-0 tiles of a w x h frame"""
    nx, ny = max(1, (w - 31 - OX + TW - 1) // TW), max(1, (h - 31 - OY + TH - 1) // TH)
    return [(tx, ty, OX + TW * tx, OY + TH * ty) for ty in range(ny) for tx in range(nx)]


def edge_dots(w, h, which):
    """isolated dots (x, y, value): row slot j of tile (tx, ty) holds, in each of its four groups, a dot in group column
    GROUP_COLS[(tx + 2 ty + j) % 6]; its value alternates between 255 and 0 from group to group.  A dot closer than 8 pixels to one
    placed before it is left out (tile column 127 beside column 0 of the next tile): "top" places the tiles in order and keeps
    column 127, "bottom" places them in reverse order and keeps column 0."""
    pts = []
    order = tiles(w, h)
    for tx, ty, x0, y0 in (order if which == "top" else order[::-1]):
        for j, row in enumerate(ROW_SLOTS[which]):
            for g in range(4):
                x, y = x0 + 32 * g + GROUP_COLS[(tx + 2 * ty + j) % 6], y0 + row
                if 3 <= x < w - 3 and 3 <= y < h - 3 and all(max(abs(x - a), abs(y - b)) >= 8 for a, b, _ in pts):
                    pts.append((x, y, 255 if (g + j + tx + ty) & 1 else 0))
    return pts


def halo_pairs(w, h):
    """((xa, ya, va), (xb, yb, vb)): neighbouring pixels on either side of a tile edge"""
    values = ((255, 255), (250, 255), (255, 250), (0, 0), (5, 0), (0, 5))
    out = []
    k = 0
    for tx, ty, x0, y0 in tiles(w, h):
        xr, yb = x0 + TW - 1, y0 + TH - 1
        for (ax, ay), (bx, by) in (((xr, y0 + 6), (xr + 1, y0 + 6)),          # across the right edge
                                   ((x0 + 40, yb), (x0 + 40, yb + 1)),          # across the lower edge
                                   ((xr, yb), (xr + 1, yb + 1)),                # across the lower right corner
                                   ((xr - 20, yb + 1), (xr - 19, yb))):         # the other diagonal, across the lower edge
            if bx + 4 <= w and by + 4 <= h and ay + 4 <= h and ax + 4 <= w:
                va, vb = values[k % 6]
                out.append(((ax, ay, va), (bx, by, vb)))
                k += 1
    return out


def _make_cases():
    rng = np.random.default_rng(23)
    c = {}
    c["noise"] = rng.integers(0, 256, (H, W), dtype=np.uint8)
    c["noise_97x131"] = rng.integers(0, 256, (131, 97), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    c["dense"] = np.clip(7 * ((xx % 10 - 5) ** 2 + (yy % 10 - 5) ** 2), 0, 255).astype(np.uint8)
    for which in ("top", "bottom"):
        for suffix, (w, h) in (("", (W, H)), ("_97x131", (97, 131))):
            img = np.full((h, w), 128, np.uint8)
            for x, y, v in edge_dots(w, h, which):
                img[y, x] = v
            c["edges_%s%s" % (which, suffix)] = img
    img = np.full((H, W), 128, np.uint8)
    for (xa, ya, va), (xb, yb, vb) in halo_pairs(W, H):
        img[ya, xa], img[yb, xb] = va, vb
    c["halo"] = img
    for name, (w, h) in (("ends", (W, H)), ("ends_97x131", (97, 131))):
        low = rng.integers(0, 42, (h, w))
        c[name] = np.where(rng.integers(0, 2, (h, w)) == 1, 255 - low, low).astype(np.uint8)
    c["empty"] = np.full((H, W), 128, np.uint8)
    c["empty_97x131"] = np.full((131, 97), 128, np.uint8)
    return c


CASES = _make_cases()


def corner_masks(img, T=20):
    """(darker, brighter): the corners of `img` by the definition -- nine contiguous ring pixels all < centre - T / all > centre + T"""
    a = img.astype(np.int32)
    h, w = a.shape
    c = a[3:h - 3, 3:w - 3]
    ring = np.stack([a[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in RING])

    def nine(m):
        m2 = np.concatenate([m, m[:8]])
        return np.any(np.stack([np.all(m2[k:k + 9], axis=0) for k in range(16)]), axis=0)
    out = []
    for m in (nine(ring < c - T), nine(ring > c + T)):
        full = np.zeros((h, w), bool)
        full[3:h - 3, 3:w - 3] = m
        out.append(full)
    return out


def window_counts(corners):
    """corners in the window a tile queues: rows y0 - 1 .. y0 + 28, columns x0 - 1 .. x0 + 128"""
    h, w = corners.shape
    return {(tx, ty): int(corners[max(y0 - 1, 0):y0 + TH + 1, max(x0 - 1, 0):x0 + TW + 1].sum()) for tx, ty, x0, y0 in tiles(w, h)}


def oracle_candidates(level_img):
    ox, oy, os_ = O.fast_nms(level_img, 20)
    lh, lw = level_img.shape
    keep = (ox >= 31) & (ox < lw - 31) & (oy >= 31) & (oy < lh - 31)
    return sorted(zip(oy[keep].tolist(), ox[keep].tolist(), os_[keep].tolist()))


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    """per frame of the batch: (candidates of the eight levels, key points); computed once, shared by the tests"""
    img = CASES[name]
    out = []
    for frame in (img, np.ascontiguousarray(img[::-1, ::-1])):
        pyr = O.orb_pyramid(frame)
        out.append(([oracle_candidates(pyr[l]) for l in range(8)], O.orb_detect(frame)))
    return out


def same_keypoints(g, o):
    return (len(g["xy"]) == len(o["xy"]) and all(np.array_equal(g[k], o[k]) for k in ("octave", "lx", "ly"))
            and np.array_equal(g["xy"], o["xy"]) and np.array_equal(g["desc"], o["desc"])
            and np.array_equal(g["response"].view(np.uint32), o["response"].view(np.uint32)))


@pytest.fixture(scope="module")
def detected():
    """every case once through orb_detect_batch as it is and once with the dense FAST kernel; downloads kept"""
    made, out = {}, {}
    for name, img in CASES.items():
        h, w = img.shape
        if (w, h) not in made:
            made[(w, h)] = Context(device=0, max_w=w, max_h=h, max_frames=2)
        ctx = made[(w, h)]
        batch = torch.from_numpy(np.stack([img, np.ascontiguousarray(img[::-1, ::-1])])).cuda()
        got = {}
        for lift in (True, False):
            ctx.set_fast_lift(lift)
            ctx.orb_detect_batch(batch)
            ctx.synchronize()
            cand = [[ctx.download_candidates(f, l) for l in range(8)] for f in range(2)]
            cand = [[sorted(zip(gy.tolist(), gx.tolist(), gs.tolist())) for gx, gy, gs in per] for per in cand]
            kp = [ctx.orb_download(f) if ctx.lib.evh_orb_count(ctx.h, f) else None for f in range(2)]
            got[lift] = (cand, kp)
        ctx.set_fast_lift(True)
        out[name] = got
    yield out
    for c in made.values():
        c.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_frame_is_what_the_case_says(name):
    """numpy, from the definition of a corner; no device involved"""
    img = CASES[name]
    h, w = img.shape
    darker, brighter = corner_masks(img)
    corners = darker | brighter
    assert not (darker & brighter).any()
    counts = window_counts(corners)
    print("%s: corners ring darker %d, ring brighter %d; per tile window %s" % (name, darker.sum(), brighter.sum(), counts))
    if name.startswith("noise"):
        assert darker.sum() >= 100 and brighter.sum() >= 100
        assert all(0 < n <= PQ_CAP for n in counts.values()), counts          # every tile takes the queue
    elif name == "dense":
        over = [t for t, n in counts.items() if n > PQ_CAP]
        assert (0, 0) in over and (1, 1) in over and len(over) >= 6, counts   # the full tiles overflow the queue,
        assert any(0 < n <= PQ_CAP for n in counts.values()), counts          # the edge tiles do not
    elif name.startswith("edges"):
        which = name.split("_")[1]
        dots = edge_dots(w, h, which)
        ys, xs = np.nonzero(corners)
        assert set(zip(xs.tolist(), ys.tolist())) == {(x, y) for x, y, _ in dots}      # each dot is a corner, nothing else is
        assert all(darker[y, x] == (v == 255) and brighter[y, x] == (v == 0) for x, y, v in dots)
        pts = sorted((x, y) for x, y, _ in dots)
        assert min(max(abs(a[0] - b[0]), abs(a[1] - b[1])) for i, a in enumerate(pts) for b in pts[:i]) >= 8
        if w == W:
            kept = [(x, y, v) for x, y, v in dots if 31 <= x < w - 31 and 31 <= y < h - 31]
            for pol in (255, 0):                                               # both sides in every group-edge column, on the
                for row in (ROW_SLOTS[which][0], ROW_SLOTS[which][-1]):        # first / last slot (tile row 0 / 27 among them)
                    assert {(x - OX) % 32 for x, y, v in kept if v == pol and (y - OY) % TH == row} >= set(GROUP_COLS), (pol, row)
            assert (127 if which == "top" else 0) in {(x - OX) % TW for x, _, _ in kept}      # the tile's own edge column
            want = sorted((y, x, abs(v - 128) - 1) for x, y, v in kept)
            assert oracle_of(name)[0][0][0] == want
    elif name == "halo":
        pairs = halo_pairs(w, h)
        assert len(pairs) >= 24
        ys, xs = np.nonzero(corners)
        assert set(zip(xs.tolist(), ys.tolist())) == {(x, y) for p in pairs for x, y, _ in p}
        # one pixel of every pair lies in the one-pixel halo of the tile that owns the other
        for (xa, ya, _), (xb, yb, _) in pairs:
            assert max(abs(xa - xb), abs(ya - yb)) == 1
            assert ((xa - OX) // TW, (ya - OY) // TH) != ((xb - OX) // TW, (yb - OY) // TH)
        # the oracle keeps the stronger pixel of an unequal pair and neither of an equal one
        want = []
        for (xa, ya, va), (xb, yb, vb) in pairs:
            sa, sb = abs(va - 128), abs(vb - 128)
            if sa != sb:
                x, y, s = (xa, ya, sa) if sa > sb else (xb, yb, sb)
                if 31 <= x < w - 31 and 31 <= y < h - 31:
                    want.append((y, x, s - 1))
        assert len(want) >= 8 and oracle_of(name)[0][0][0] == sorted(want)
    elif name.startswith("ends"):
        centres = img[3:h - 3, 3:w - 3]
        assert darker.sum() >= 100 and brighter.sum() >= 100
        assert not darker[3:h - 3, 3:w - 3][centres < 21].any() and not brighter[3:h - 3, 3:w - 3][centres > 234].any()
        assert brighter[3:h - 3, 3:w - 3][centres < 21].sum() >= 50 and darker[3:h - 3, 3:w - 3][centres > 234].sum() >= 50
        assert all(n <= PQ_CAP for n in counts.values()), counts
    else:
        assert not corners.any()
        assert all(len(c) == 0 for c in oracle_of(name)[0][0]) and len(oracle_of(name)[0][1]["xy"]) == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_candidates_per_level(detected, name):
    cand = detected[name][True][0]
    for f in range(2):
        want = oracle_of(name)[f][0]
        for l in range(8):
            assert cand[f][l] == want[l], "frame %d level %d: %d vs %d candidates" % (f, l, len(cand[f][l]), len(want[l]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_candidates_equal_the_dense_kernels(detected, name):
    lifted, dense = detected[name][True][0], detected[name][False][0]
    for f in range(2):
        for l in range(8):
            assert lifted[f][l] == dense[f][l], "frame %d level %d: %d vs %d candidates" % (f, l, len(lifted[f][l]), len(dense[f][l]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_keypoints_in_reference_order(detected, name):
    kp = detected[name][True][1]
    for f in range(2):
        o = oracle_of(name)[f][1]
        if len(o["xy"]) == 0:
            assert kp[f] is None, f
        else:
            assert kp[f] is not None and same_keypoints(kp[f], o), f
