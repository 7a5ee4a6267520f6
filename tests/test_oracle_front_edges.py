"""CPU: the oracle's image front end (O.bgr2gray, O.resize_area, O.resize_linear_exact, O.orb_pyramid, O.orb_layout) against
the plain restatement (tests/front_checks.py) on the crafted families of tests/front_families.py -- bit for bit against
statement (a), statement (a) within its derived bound of the float64 definition (b) -- and every premise of the families:
that the ties, table shapes, forms, seams and kernels a case is there for are really reached.  The figures the tests print
are the ones in profiles/front_edges.txt.  tests/test_gpu_front_edges.py runs the same families on the device."""
import numpy as np
import pytest

import front_checks as C
import front_families as F
from oracle import oracle as O


def _bound_check(a, true, bound, what):
    d = float(np.abs(a.astype(np.float64) - true).max())
    print("%s: largest |a - b| %.4f, bound %.4f" % (what, d, bound))
    assert d <= bound, what
    return d


# ---------------------------------------------------------------------------------------------------------------- gray
def test_gray():
    rng = np.random.default_rng(1)
    ext = np.array([[b, g, r] for b in (0, 1, 127, 128, 254, 255) for g in (0, 1, 127, 128, 254, 255)
                    for r in (0, 1, 127, 128, 254, 255)], np.uint8).reshape(8, 27, 3)
    for bgr in (ext, rng.integers(0, 256, (37, 131, 3), dtype=np.uint8)):
        a = C.gray(bgr)
        assert np.array_equal(O.bgr2gray(bgr), a)
        _bound_check(a, C.gray_true(bgr), C.GRAY_BOUND, "gray")
    assert C.gray(np.full((1, 1, 3), 255, np.uint8))[0, 0] == 255       # the three weights sum to 2^14


# ------------------------------------------------------------------------------------------------------------- T: ties
@pytest.mark.parametrize("name,isx,isy,cn", F.t_cases(), ids=[c[0] for c in F.t_cases()])
def test_ties(name, isx, isy, cn):
    sw, sh, dw, dh = F.t_geometry(isx, isy, cn)
    img = F.t_image(isx, isy, cn)
    area = isx * isy
    assert img.shape[:2] == (sh, sw) and dw * cn in (257, 258)
    assert C.area_form(sw, sh, dw, dh) == ("int", isx, isy)
    a = C.resize_area(img, dw, dh)
    assert np.array_equal(O.resize_area(img, dw, dh), a)
    _bound_check(a, C.area_true(img, dw, dh), C.area_bound(sw, sh, dw, dh), name)
    # premises
    s = C.block_sums(img, isx, isy, dw, dh).reshape(-1)
    out = a.reshape(-1).astype(np.int64)
    assert (s == 0).sum() >= 8 and (s == 255 * area).sum() >= 8
    assert (out[s == 0] == 0).all() and (out[s == 255 * area] == 255).all()
    if area & (area - 1) == 0:                                        # a power of two: exact halves, both parities of the floor
        half = (2 * s) % (2 * area) == area
        even, odd = half & ((s // area) % 2 == 0), half & ((s // area) % 2 == 1)
        assert even.sum() >= 8 and odd.sum() >= 8
        if (isx, isy) == (2, 2):                                       # (s + 2) >> 2: a half goes up
            assert (out[half] == s[half] // area + 1).all()
        else:                                                          # half to even
            assert (out[even] == s[even] // area).all() and (out[odd] == s[odd] // area + 1).all()
        print("%s: exact halves with an even floor %d, with an odd floor %d" % (name, even.sum(), odd.sum()))
    else:                                                              # 6 and 9: the float32 product on each side of the half
        p = C.area_int_product(s, area).astype(np.float64)
        frac = p - np.floor(p)
        near = np.abs(2 * s - (2 * (s // area) + 1) * area) <= 1       # the sums nearest the half: 6 k + 3, 9 k + 4, 9 k + 5
        below, on, above = near & (frac < 0.5), near & (frac == 0.5), near & (frac > 0.5)
        print("%s: nearest sums with the product below the half %d, on it %d, above %d" % (name, below.sum(), on.sum(), above.sum()))
        fl = s // area
        on_even, on_odd = on & (fl % 2 == 0), on & (fl % 2 == 1)
        # area 9: 9 k + 4 and 9 k + 5 lie on either side.  Area 6: 6 k + 3 is a true half, and float32(1 / 6) is so little above
        # 1 / 6 that the float32 product rounds back ONTO the half for every k: these are ties like those of the powers of two
        if area == 6:
            assert on_even.sum() >= 8 and on_odd.sum() >= 8 and below.sum() == above.sum() == 0
        else:
            assert below.sum() >= 8 and above.sum() >= 8 and on.sum() == 0
        assert (out[below | on_even] == fl[below | on_even]).all() and (out[above | on_odd] == fl[above | on_odd] + 1).all()


# ------------------------------------------------------------------------------------------------------ A and E: resize
@pytest.mark.parametrize("name,geo,cn,kind", F.resize_cases(), ids=[c[0] for c in F.resize_cases()])
def test_resize_cases(name, geo, cn, kind):
    sw, sh, dw, dh = geo
    img = F.content(kind, sw, sh, dw, dh, cn)
    a = C.resize_area(img, dw, dh)
    assert np.array_equal(O.resize_area(img, dw, dh), a)
    if kind == "white":
        assert (a == 255).all()                                       # weights that do not sum to 1 would show here
    if name.startswith("A"):
        _bound_check(a, C.area_true(img, dw, dh), C.area_bound(sw, sh, dw, dh), name)
    if kind == "cells" and name.startswith("A") and min(dw, dh) > 2:
        near = np.abs(a.astype(np.int64) - 127.5) <= 32
        assert near.mean() > 0.25, "the cells no longer put results next to a half"


def a_entry_counts(geos):
    """{entries per cell: cells} over both axes of the geometries"""
    hist = {}
    for sw, sh, dw, dh in geos:
        for s, d in ((sw, dw), (sh, dh)):
            for e in C.area_tab(s, d):
                hist[len(e)] = hist.get(len(e), 0) + 1
    return hist


def test_table_shapes_are_reached():
    # 4095 x 3 -> 1 x 1 is an integer ratio to the operator (one block of 12285 pixels, a sum below 2^24); the cell of 4095
    # table entries is the y axis of 7 x 4095 -> 3 x 1
    for g in F.A_GEOMETRIES:
        assert C.area_form(*g) == (("int", 4095, 3) if g == (4095, 3, 1, 1) else "tables"), g
    assert max(len(e) for e in C.area_tab(4095, 1)) == 4095 and C.area_form(7, 4095, 3, 1) == "tables"
    # Barely above 1.  The two geometries 258 -> 257 and 1001 -> 1000 give cells of 1 and 2 entries only: a cell of 3 (partial,
    # whole, partial) needs two partial pixels wider than 1e-3 that add up to scale - 1, which is 0.001 at 1001 / 1000, and at
    # 258 / 257 the left part is a multiple of 1 / 257 that leaves 0 on the right.  259 -> 257 was added for the cell of 3.
    two = a_entry_counts(F.A_BARELY[:2])
    assert sorted(k for k in two if k <= 3) == [1, 2], two
    hist = a_entry_counts(F.A_BARELY)
    print("entries per cell, barely above 1: %s" % sorted(hist.items()))
    assert all(hist.get(k, 0) > 0 for k in (1, 2, 3)), hist
    # the sliver test on its threshold: 1001 / 1000 - 1 is within 1e-15 of 1e-3
    sliver = 1.0 / (1000.0 / 1001.0) - 1.0
    print("the first right sliver at 1001 -> 1000: %.20f" % sliver)
    assert abs(sliver - 1e-3) < 1e-15
    assert max(len(e) for e in C.area_tab(4095, 17)) in (241, 242)
    for s, d in ((300, 200), (200, 80)):                              # cell edges on integers: no partial pixel is a sliver
        assert all(abs(a - 0.5 / (s / d)) < 1e-6 or abs(a - 1 / (s / d)) < 1e-6 for e in C.area_tab(s, d) for _, a in e)
    assert C._scales(640, 320)[0] == 2.0 and C._scales(361, 100)[0] != round(C._scales(361, 100)[0])


def test_enlarging_cases_are_what_they_say():
    for g in F.E_GEOMETRIES:
        assert C.area_form(*g) == "enlarge", g
    for sw, sh, dw, dh in F.E_MIXED:
        sx, sy = C._scales(sw, dw)[0], C._scales(sh, dh)[0]
        assert sx < 1 <= sy or sy < 1 <= sx, (sx, sy)
    # the substitution past xmax is reached, and so is the row clipping
    for sw, sh, dw, dh in F.E_GEOMETRIES:
        for s, d in ((sw, dw), (sh, dh)):
            if d > s:
                assert C._enlarge_axis(s, d)[3] < d, (s, d)


def test_forms_from_the_geometry():
    assert C.area_form(10, 10, 10, 10) == "copy"
    assert C.area_form(1280, 720, 640, 360) == ("int", 2, 2)
    assert C.area_form(1170, 658, 400, 224) == "tables"
    assert C.area_form(640, 361, 320, 100) == "tables"
    assert C.area_form(100, 64, 150, 16) == "enlarge"


# ------------------------------------------------------------------------------------------------------------ P: pyramid
P_ALL = dict(F.p_frames(), **F.p220_frames(), **F.p120_frames())


def _pyramid_agrees(img, what):
    want = C.orb_pyramid(img)
    got = O.orb_pyramid(img)
    h, w = img.shape
    lw, lh, _, _ = O.orb_layout(w, h)
    assert [(int(a), int(b)) for a, b in zip(lw, lh)] == list(C.orb_sizes(w, h))
    worst = 0.0
    for l in range(C.NLEVELS):
        assert got[l].shape == want[l].shape and np.array_equal(got[l], want[l]), "%s level %d" % (what, l)
        if l:
            assert np.array_equal(O.resize_linear_exact(want[l - 1], want[l].shape[1], want[l].shape[0]), want[l])
            worst = max(worst, float(np.abs(want[l].astype(np.float64) -
                                            C.bilinear_true(want[l - 1], want[l].shape[1], want[l].shape[0])).max()))
    print("%s: largest |a - b| over the levels %.4f, bound %.4f" % (what, worst, C.LINEAR_BOUND))
    assert worst <= C.LINEAR_BOUND
    return want


@pytest.mark.parametrize("name", sorted(P_ALL))
def test_pyramid_content(name):
    pyr = _pyramid_agrees(P_ALL[name], name)
    if name == "P_white":
        assert all((p == 255).all() for p in pyr)
    if name == "P_black":
        assert all((p == 0).all() for p in pyr)


def test_pyramid_premises():
    f = F.p_frames()
    pyr = C.orb_pyramid(f["P_seams"])
    for level in (1, 2):
        lh, lw = pyr[level].shape
        for c in F.TILE_COLS:
            if c < lw:
                assert pyr[level][:, c].any(), "no impulse reaches column %d of level %d" % (c, level)
        for r in F.TILE_ROWS:
            if r < lh:
                assert pyr[level][r].any(), "no impulse reaches row %d of level %d" % (r, level)
    # 400 x 224 walks at every level (75 -> 62 rows at level 7 is 1.2097); 400 x 220 is the one whose level 7 does not
    assert F.kernel_of_levels(F.P_W, F.P_H) == ["walk"] * 7
    assert F.kernel_of_levels(400, 220) == ["walk"] * 6 + ["down"]
    assert C.orb_pyramid(f["P_corners"])[1][[0, 0, -1, -1], [0, -1, 0, -1]].all()
    assert C.orb_pyramid(f["P_last_row_col"])[1][-1].any() and C.orb_pyramid(f["P_last_row_col"])[1][:, -1].any()
    # 120 x 120: level 1 is 100 x 100, the right-tap weight is 128 at v % 5 == 2, and some 16.16 value ends in 0x8000
    assert C.orb_sizes(120, 120)[1] == (100, 100)
    w1 = C.linear_taps(120, 100)[3]
    assert (w1[2::5] == 128).all()
    for name, img in F.p120_frames().items():
        wide = C.linear_exact_wide(img, 100, 100)
        n = int(((wide & 0xFFFF) == 0x8000).sum())
        print("%s: level-1 values with the low half exactly 32768: %d" % (name, n))
        assert n >= 1, name


# -------------------------------------------------------------------------------------------------------------- S: seams
def test_seam_sweep_premises():
    frames = F.s_frames()
    assert max(max(f) for f in frames) <= F.S_LIMIT
    widths, heights, kinds, res = set(), set(), set(), set()
    for w, h in frames:
        sz = C.orb_sizes(w, h)
        widths |= {sz[1][0], sz[2][0]}
        heights |= {sz[1][1], sz[2][1]}
        kinds |= set(F.kernel_of_levels(w, h)[1:])
        res |= F.staged_residues(w, h)
    assert widths >= set(F.SEAM_WIDTHS) and heights >= set(F.SEAM_HEIGHTS)
    assert kinds == {"walk", "down"}
    # Every residue a frame of up to S_LIMIT columns can give, whatever its height (both tile widths at every level >= 2): a
    # level >= 2 of such a frame has at most 278 columns, so its tiles start at 0, 128 and 256 only and the staged start sits
    # at 0, about 153 or about 307.
    reachable = set()
    for w in range(2, F.S_LIMIT + 1):
        sz = [s[0] for s in C.orb_sizes(w, w)]
        for l in range(2, C.NLEVELS):
            i0 = C.linear_taps(sz[l - 1], sz[l])[0]
            reachable |= {int(i0[x]) & 15 for t in (128, 256) for x in range(0, sz[l], t)}
    print("residues of the staged start: within %d px %s" % (F.S_LIMIT, sorted(res)))
    assert res == reachable
    wide = F.s_wide_frames()
    allres = res.union(*[F.staged_residues(w, h) for w, h in wide])
    print("with the wide frames %s: %s" % (wide, sorted(allres)))
    assert len(allres) >= 15
    for w, h in frames + wide:
        print("%4d x %-3d levels 1..7: %s" % (w, h, " ".join(F.kernel_of_levels(w, h))))


@pytest.mark.parametrize("w,h", list(F.s_frames() + F.s_wide_frames()) + F.X_LARGE + F.X_SMALL)
def test_pyramid_on_seam_and_extreme_sizes(w, h):
    for img in F.noise_frames(w, h, 2):
        _pyramid_agrees(img, "%dx%d" % (w, h))


def test_extreme_sizes():
    for w, h in F.X_SMALL:
        sz = C.orb_sizes(w, h)
        assert min(min(s) for s in sz) >= 1 and F.acceptable_orb_frame(w, h)
    assert C.orb_sizes(2, 2)[-1] == (1, 1) and "down" in F.kernel_of_levels(2, 2)
    for w, h in F.X_REFUSED:
        assert min(min(s) for s in C.orb_sizes(w, h)) == 0 and not F.acceptable_orb_frame(w, h)
    assert all(F.acceptable_orb_frame(s, s) for s in range(2, 64))       # a side of 2 is the smallest that leaves no level empty
