"""The numpy restatement of evh_track_points / evh_track_seeds (tests/track_checks.py) checked on its own, on the host: the device
is held to it for equality (test_gpu_track.py), so what it computes has to be a tracker.  Also the crafted families
(tests/track_families.py), the refusals of evenvizion_amd.tracking and the ctypes table."""
import os
import re

import numpy as np
import pytest

import track_checks as T
import track_families as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _texture(seed, w, h, sigma):
    f = F._shifted(F.noise_field(seed, w, h, sigma), 0.0, 0.0)
    return F._to_gray(f, 0, 255, f)


def worst_error(rows, M):
    return float(np.abs(rows[:, 2:].astype(np.float64) - F.apply(M, rows[:, :2])).max())


# ---- positions and levels ------------------------------------------------------------------------------------------------------------------
def test_levels_and_offsets_round_trip_as_stated():
    assert T.down(-16) == -16 and T.down(-17) == -17 and T.down(-15) == -16 and T.down(16) == 0 and T.down(15) == -1
    assert T.down(48) == 16 and T.up(16) == 48 and T.up(0) == 16 and T.up(-16) == -16            # pixel centres map to pixel centres
    for P in range(-200, 200):
        assert T.up(T.down(P)) in (P, P - 1) and T.down(T.up(P)) == P
    g = np.arange(5 * 7, dtype=np.uint8).reshape(5, 7)
    pyr = T.pyramid(g, 4)
    assert [p.shape for p in pyr] == [(5, 7), (2, 3)]                                            # the odd row and column are dropped; 1 x 1 does not exist
    assert pyr[1][0, 0] == (0 + 1 + 7 + 8 + 2) >> 2 and pyr[1][1, 2] == (18 + 19 + 25 + 26 + 2) >> 2
    assert [p.shape for p in T.pyramid(np.zeros((9, 17), np.uint8), 4)] == [(9, 17), (4, 8), (2, 4)]
    # the centre of a 2 x 2 mean: a ramp sampled at a point and at the point one level down agree
    ramp = np.tile((4 * np.arange(32, dtype=np.int64)).astype(np.uint8), (16, 1))
    lv = T.pyramid(ramp, 2)
    P = 32 * 10 + 8
    assert T.sample(lv[0], np.array([P]), np.array([64]))[0] == T.sample(lv[1], np.array([T.down(P)]), np.array([T.down(64)]))[0]


def test_sample_is_the_warps_sum_and_reads_no_tap_of_weight_zero():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (6, 9), dtype=np.uint8)
    X, Y = np.array([32 * 8, 32 * 8, 0, 37]), np.array([32 * 5, 11, 32 * 5, 75])                 # the last column, the last row, both
    s = T.sample(img, X, Y)
    assert s[0] == 1024 * int(img[5, 8]) and s[2] == 1024 * int(img[5, 0])
    assert s[1] == int(img[0, 8]) * 32 * 21 + int(img[1, 8]) * 32 * 11
    I = img.astype(np.int64)
    assert s[3] == I[2, 1] * 27 * 21 + I[2, 2] * 5 * 21 + I[3, 1] * 27 * 11 + I[3, 2] * 5 * 11
    with pytest.raises(AssertionError):
        T.sample(img, np.array([32 * 8 + 1]), np.array([0]))


# ---- the tracker -----------------------------------------------------------------------------------------------------------------------------
def test_identical_pair_returns_the_point_with_zero_steps():
    g = _texture(3, 64, 48, 1.5)
    pyr = T.pyramid(g, 1)
    for A0 in ((32 * 20, 32 * 20), (32 * 30 + 7, 32 * 17 + 29), (32 * 12 + 16, 32 * 24)):
        flag, B, err, steps = T.track_run(pyr, pyr, A0, A0, 5, 20, 0.0)
        assert (flag, B, err, steps) == (T.TRACKED, A0, 0, 0)
    # through three levels the guess goes down and comes up again, up(down(P)) is P or P - 1: the steps take that unit back
    pyr = T.pyramid(g, 3)
    for A0 in ((32 * 30 + 7, 32 * 22 + 29), (32 * 31, 32 * 24)):
        flag, B, err, steps = T.track_run(pyr, pyr, A0, A0, 5, 20, 0.0)
        assert flag == T.TRACKED and max(abs(B[0] - A0[0]), abs(B[1] - A0[1])) <= 1


@pytest.mark.parametrize("dx,dy,levels,sigma", [(3, -2, 1, 2.0), (-4, 1, 2, 2.0), (7, 5, 3, 4.0)])
def test_a_frame_pasted_at_an_integer_offset(dx, dy, levels, sigma):
    """The third case needs its three levels: 8.6 px are out of reach of two (features of sigma 4 are 2 px wide at level 1)."""
    big = _texture(4, 160, 128, sigma)
    cur, prev = big[16:112, 16:144], big[16 - dy:112 - dy, 16 - dx:144 - dx]                      # prev(a + d) = cur(a)
    pts = np.array([(50, 40), (64.5, 48.25), (80, 56)], np.float32)
    rows, counts, flags, err = T.track_points(np.stack([prev, cur]), pts[None], [3], levels=levels, radius=5, iters=20)
    assert counts[0] == 3 and (flags[0] == T.TRACKED).all()
    assert np.abs(rows[0, :3, 2:] - (pts + (dx, dy))).max() <= 2 / 32
    assert np.array_equal(rows[0, :3, :2], pts)


def test_flags_for_border_flat_and_non_finite_points():
    g = _texture(5, 64, 48, 1.5)
    flat = np.full_like(g, 77)
    pts = np.array([(np.nan, 10), (10, np.inf), (-0.25, 10), (63.02, 10), (63, 47), (5.9, 20), (6, 6), (30, 20), (0, 0), (-0.01, 0)], np.float32)
    rows, counts, flags, err = T.track_points(np.stack([g, g]), pts[None], [len(pts)], levels=1, radius=5, iters=5)
    assert flags[0].tolist() == [T.BAD_POINT] * 4 + [T.NO_WINDOW] * 2 + [T.TRACKED] * 2 + [T.NO_WINDOW] * 2
    assert counts[0] == 2 and np.array_equal(rows[0, :2, :2], pts[6:8]) and (err[0, 6:8] == 0).all() and (err[0, :6] == T.NO_ERR).all()
    assert rows[0, 2:].view(np.uint8).min() == 0xFF                                                 # rows past the count are untouched
    rows, counts, flags, err = T.track_points(np.stack([g, flat]), pts[None, 6:8], [2], levels=2, radius=5, iters=5)
    assert flags[0].tolist() == [T.FLAT, T.FLAT] and counts[0] == 0
    # a guess that sends the search window out of the frame
    M = np.array([[1, 0, 40], [0, 1, 0], [0, 0, 1.0]])
    rows, counts, flags, err = T.track_points(np.stack([g, g]), pts[None, 7:8], [1], mats=M.reshape(1, 9), levels=1, radius=5, iters=5)
    assert flags[0].tolist() == [T.LEFT_FRAME]
    for bad in (np.full(9, np.nan), np.zeros(9), np.array([1e308, 1e308, 1e308, 0, 1, 0, 0, 0, 1.0]), np.array([1, 0, 1e9, 0, 1, 0, 0, 0, 1.0])):
        assert T.first_guess((640, 640), bad) == (640, 640)
    assert T.first_guess((640, 640), M) == (640 + 32 * 40, 640)
    # min_eig on the boundary: the bar is lambda itself
    pyr = T.pyramid(g, 1)
    i, j = T._offsets(6)
    Tm = T.sample(pyr[0], 960 + 32 * i, 640 + 32 * j)
    gx, gy = (Tm[1:-1, 2:] - Tm[1:-1, :-2]).reshape(-1), (Tm[2:, 1:-1] - Tm[:-2, 1:-1]).reshape(-1)
    lam = T.min_eigenvalue(int((gx * gx).sum()), int((gx * gy).sum()), int((gy * gy).sum()))
    at = lam / (121 * 4194304.0)
    for me, want in ((at * (1 - 1e-12), T.TRACKED), (at * (1 + 1e-12), T.FLAT)):
        assert T.track_run(pyr, pyr, (960, 640), (960, 640), 5, 5, me)[0] == want


def test_error_bar_and_forward_backward():
    big = _texture(6, 96, 80, 2.0)
    cur, prev = big[16:64, 16:80], big[14:62, 13:77]
    pts = np.array([(24, 20), (40, 28)], np.float32)
    frames = np.stack([prev, cur])
    rows, counts, flags, err = T.track_points(frames, pts[None], [2], levels=2, radius=5, iters=20, fb_max32=16, max_err=255)
    assert counts[0] == 2 and (err[0] < 4 * 121 * 1024).all()
    other = np.stack([_texture(7, 64, 48, 2.0), cur])                                               # nothing to find
    rows, counts, flags, err = T.track_points(other, pts[None], [2], levels=2, radius=5, iters=20, max_err=4)
    assert (flags[0] == T.HIGH_ERROR).all() and (err[0] > 4 * 121 * 1024).all() and (err[0] != T.NO_ERR).all()
    rows, counts, flags, err = T.track_points(other, pts[None], [2], levels=2, radius=5, iters=20, fb_max32=0)
    assert set(flags[0].tolist()) <= {T.FB_FAILED, T.LEFT_FRAME} and counts[0] == 0


def test_counts_are_clamped_and_rows_keep_the_input_order():
    g = _texture(8, 64, 48, 1.5)
    pts = np.array([(30, 20), (np.nan, 0), (20, 30), (1, 1), (40, 22)], np.float32)
    rows, counts, flags, err = T.track_points(np.stack([g, g, g]), np.stack([pts, pts]), [9, -3], levels=1, radius=3, iters=3, row_cap=7)
    assert counts.tolist() == [3, 0] and np.array_equal(rows[0, :3, :2], pts[[0, 2, 4]]) and rows.shape == (2, 7, 4)
    assert flags[1].min() == 0xFF and err.view(np.uint8)[1].min() == 0xFF


# ---- the families ----------------------------------------------------------------------------------------------------------------------------
def test_low_contrast_family_holds_no_corner_and_is_tracked():
    """Gaussian-filtered noise, sigma 2 px, gray 100..120: FAST's test needs a difference above 20.  levels 2, radius 5: the 35 grid
    points of each pair within 0.5 px (the prototype stayed under 0.19 px; this restatement measures 0.13, 0.28, 0.16 px)."""
    from oracle import oracle as O
    for seed, dx, dy in F.LOW_SHIFTS:
        prev, cur, M = F.shift_pair(seed, dx, dy, **F.LOW)
        assert int(cur.max()) - int(cur.min()) <= 20 and int(prev.max()) - int(prev.min()) <= 21
        assert O.pair_gray(cur, prev)[0] == O.NO_DESCRIPTORS
        pts = F.grid_points(F.LOW["w"], F.LOW["h"])
        rows, counts, flags, err = T.track_points(np.stack([prev, cur]), pts[None], [35], levels=2, radius=5, iters=20, fb_max32=16)
        e = worst_error(rows[0, :counts[0]], M)
        print("seed %d shift (%g, %g): %d of 35 kept, worst %.3f px" % (seed, dx, dy, counts[0], e))
        assert counts[0] == 35 and e <= 0.5


def test_full_contrast_family_over_three_levels():
    """sigma 4, shift (9.5, 6.25), levels 3, radius 5 and no guess: what is kept lies within 0.25 px (measured: 0.03 and 0.06 px);
    points whose window leaves the frame on the way, or that do not come back, are dropped."""
    for seed, dx, dy in F.FULL_SHIFTS:
        prev, cur, M = F.shift_pair(seed, dx, dy, **F.FULL)
        pts = F.grid_points(F.FULL["w"], F.FULL["h"])
        rows, counts, flags, err = T.track_points(np.stack([prev, cur]), pts[None], [35], levels=3, radius=5, iters=20, fb_max32=16)
        e = worst_error(rows[0, :counts[0]], M)
        print("seed %d: %d of 35 kept, worst %.3f px, flags %s" % (seed, counts[0], e, np.bincount(flags[0], minlength=7)))
        assert counts[0] >= 18 and e <= 0.25


def test_projective_family_from_a_coarse_guess():
    prev, cur, M, guess = F.projective_pair(31)
    pts = F.grid_points(128, 96)
    rows, counts, flags, err = T.track_points(np.stack([prev, cur]), pts[None], [35], mats=guess.reshape(1, 9), levels=2, radius=7,
                                              iters=20, fb_max32=16)
    e = worst_error(rows[0, :counts[0]], M)
    start = float(np.abs(F.apply(guess, pts) - F.apply(M, pts)).max())
    print("%d of 35 kept, worst %.3f px (the guess: %.2f px)" % (counts[0], e, start))
    assert counts[0] >= 30 and e <= 0.5 < start


# ---- seeds -----------------------------------------------------------------------------------------------------------------------------------
def test_seeds_ties_partial_cells_and_overflow():
    flat = np.full((40, 50), 9, np.uint8)
    pts, npts = T.track_seeds(flat[None], radius=1, cell=16, border=4, min_eig=0.0, pt_cap=16)
    # every lambda is 0: the first pixel of every cell, partial cells at the right (x0 = 36: 10 wide) and at the bottom included
    want = [(x, y) for y in (4, 20) for x in (4, 20, 36)]
    assert npts[0] == 6 and pts[0, :6].tolist() == [list(map(float, p)) for p in want] and pts[0, 6:].view(np.uint8).min() == 0xFF
    assert T.track_seeds(flat[None], 1, 16, 4, 1e-9, 16)[1][0] == 0                                  # nothing reaches a positive bar
    g = _texture(9, 50, 40, 1.5)
    pts, npts = T.track_seeds(np.stack([g, flat]), radius=2, cell=8, border=3, min_eig=0.0, pt_cap=5)
    assert npts.tolist() == [30, 30] and pts.shape == (2, 5, 2)                                      # the full count, five written
    lam = T.seed_field(g, 2)
    x, y = pts[0, 0]
    assert lam[int(y), int(x)] == np.nanmax(lam[3:11, 3:11]) and 3 <= x < 11 and 3 <= y < 11
    assert np.isnan(lam[2, 10]) and not np.isnan(lam[3:-3, 3:-3]).any()
    # an empty rectangle, and one of a single pixel
    assert T.track_seeds(g[None], 1, 8, 25, 0.0, 4)[1][0] == 0
    assert T.track_seeds(g[None, :, :49], 1, 8, 24, 0.0, 4)[1][0] == 0 and T.track_seeds(np.full((1, 49, 49), 9, np.uint8), 1, 8, 24, 0.0, 4)[1][0] == 1
    # one corner in a flat frame: the cells around it see it, and lambda is the hand-computed one
    one = flat.copy()
    one[20:, 25:] = 60
    lam = T.seed_field(one, 1)
    gx = one.astype(np.int64)[19:22, 25:28] - one.astype(np.int64)[19:22, 23:26]
    gy = one.astype(np.int64)[20:23, 24:27] - one.astype(np.int64)[18:21, 24:27]
    assert lam[20, 25] == T.min_eigenvalue(int((gx * gx).sum()), int((gx * gy).sum()), int((gy * gy).sum())) > 0


def test_default_min_eig_seeds_the_low_contrast_family():
    """tracking.MIN_EIG: at least one seed per two cells on the family the tracker is for (measured: 35 of 35 cells)."""
    from evenvizion_amd import tracking
    for seed, dx, dy in F.LOW_SHIFTS:
        _, cur, _ = F.shift_pair(seed, dx, dy, **F.LOW)
        pts, npts = T.track_seeds(cur[None], radius=2, cell=16, border=8, min_eig=tracking.MIN_EIG, pt_cap=64)
        assert 2 * npts[0] >= 7 * 5, (seed, npts[0])


# ---- the driver's refusals and the table -----------------------------------------------------------------------------------------------------
def test_driver_refuses_before_the_capture_is_touched():
    from evenvizion_amd import tracking

    class Untouched:
        def __getattr__(self, name):
            raise AssertionError("the capture was touched: %s" % name)

    good = {"resize_info": {"w": 400, "h": 224}}
    for kw in (dict(levels=0), dict(levels=5), dict(radius=0), dict(radius=11), dict(iters=0), dict(iters=65), dict(cell=7), dict(cell=65),
               dict(seed_radius=4), dict(min_eig=-1.0), dict(min_eig=float("nan")), dict(fb_max=-0.5), dict(fb_max=float("inf")),
               dict(max_err=256), dict(max_err=1.5), dict(levels=True), dict(nfeatures=0), dict(chunk_frames=1), dict(ingest="rgb"),
               dict(features_type_list=["ORB", "SIFT"]), dict(features_type_list=["SIFT"])):
        with pytest.raises(ValueError):
            tracking.recover_homography_dict(Untouched(), good, **kw)
    for bad in (None, {}, {"2": {"H": np.eye(3).tolist()}}):
        with pytest.raises(ValueError):
            tracking.recover_homography_dict(Untouched(), bad)
    with pytest.raises(ValueError):
        tracking.track_rows(Untouched(), good["resize_info"], levels=9)
    tracking.check_track_arguments(fb_max=None, max_err=None)


def test_ctypes_table_matches_the_header():
    from evenvizion_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evhip.h")).read(), flags=re.S)
    for name in ("evh_track_points", "evh_track_points_yuv420", "evh_track_seeds", "evh_track_seeds_yuv420"):
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text).group(1)
        args = [a.strip() for a in decl.split(",")]
        res, sig = _lib.SIGNATURES[name]
        assert res is _lib._i and len(sig) == len(args), name
        for a, s in zip(args, sig):
            want = _lib._vp if "*" in a else _lib._d if a.startswith("double") else _lib._i64 if a.startswith("int64_t") else _lib._i
            assert s is want, (name, a)
    assert len(_lib.TRACK_FLAGS) == 7 == len(T.FLAGS) and tuple(_lib.TRACK_FLAGS) == T.FLAGS
    enum = re.search(r"enum \{ (EVH_TRACK_TRACKED[^}]*) \}", text).group(1)
    assert [e.split("=")[0].strip()[len("EVH_TRACK_"):].lower() for e in enum.split(",")][:7] == list(T.FLAGS)
    assert "EVH_TRACK_GUESS_MAX = 1 << 24" in text and T.GUESS_MAX == 1 << 24
