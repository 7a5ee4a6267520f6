"""evh_track_points / evh_track_seeds (and their _yuv420 forms) on the device, held to the numpy restatement (tests/track_checks.py,
itself checked in test_track_host.py) for EQUALITY: rows, counts, flags and errors byte for byte, what the entry must leave alone
included.  Every call of the entries goes through track() and seeds() below, which hand the outputs over filled with 0xFF bytes."""
import ctypes

import numpy as np
import pytest

import track_checks as T
import track_families as F
import warp_checks as W
from refusal_arena import Arena
from test_gpu_residual import dev, frames_of, strided

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from evenvizion_amd._lib import Context
    c = Context(device=0, max_w=64, max_h=64, max_features=500, max_frames=2)     # the entries do not depend on these sizes
    yield c
    c.close()


def texture(seed, w, h, sigma=1.5, cn=1):
    f = F._shifted(F.noise_field(seed, w, h, sigma), 0.0, 0.0)
    g = F._to_gray(f, 0, 255, f)
    if cn == 1:
        return g
    rng = np.random.default_rng(seed)
    return np.clip(g[..., None].astype(np.int64) + rng.integers(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)


def shifted_stack(seed, n, w, h, cn=1, sigma=1.5):
    """n frames cut from one texture: frame k shows the texture at (2k, k), so a point a of frame k + 1 lies at a + (2, 1) in frame k"""
    big = texture(seed, w + 2 * n, h + n, sigma, cn)
    return np.stack([big[k:k + h, 2 * k:2 * k + w] for k in range(n)])


def scatter(seed, n, w, h):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, 32 * (w - 1) + 1, n), rng.integers(0, 32 * (h - 1) + 1, n)], 1).astype(np.float32) / np.float32(32)


def track(ctx, frames, pts, npts, mats=None, frame_step=1, levels=3, radius=5, iters=20, min_eig=0.0, fb_max32=-1, max_err=-1, row_cap=None,
          src_layout=None, planes=None, size=None, optional=True):
    """Context.track_points[_yuv420] against the restatement -> (rows, counts, flags, err) as numpy arrays.  planes: the source handed
    to the plane form in place of `frames`, which then are the BGR frames they convert to."""
    import torch
    frames = np.asarray(frames)
    pts = np.ascontiguousarray(pts, np.float32)
    npairs, pt_cap = pts.shape[:2]
    row_cap = pt_cap if row_cap is None else row_cap
    _, src, _ = strided(frames.shape, src_layout, frames)
    d_pts, d_npts = dev(pts), dev(np.asarray(npts, np.int32))
    d_M = None if mats is None else dev(np.asarray(mats, np.float64).reshape(-1, 9))
    rows = torch.full((npairs, row_cap, 4), float("nan"), dtype=torch.float32, device="cuda").view(torch.uint8).fill_(0xFF).view(torch.float32)
    counts = torch.full((npairs,), -1, dtype=torch.int32, device="cuda")
    flags = torch.full((npairs, pt_cap), 0xFF, dtype=torch.uint8, device="cuda")
    err = torch.full((npairs, pt_cap), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()                                  # the fills ran on torch's stream, the entry runs on the context's
    kw = dict(levels=levels, radius=radius, iters=iters, min_eig=min_eig, fb_max=None if fb_max32 < 0 else fb_max32 / 32.0,
              max_err=None if max_err < 0 else max_err, rows=rows, counts=counts, flags=flags if optional else None,
              err=err if optional else None, frame_step=frame_step)
    if planes is None:
        got = ctx.track_points(src, d_pts, d_npts, d_M, **kw)
    else:
        got = ctx.track_points_yuv420(planes, d_pts, d_npts, d_M, size=size, **kw)
    assert got[0] is rows and got[1] is counts
    ctx.synchronize()
    out = (rows.cpu().numpy(), counts.cpu().numpy(), flags.cpu().numpy(), err.cpu().numpy().view(np.uint32))
    want = T.track_points(frames, pts, npts, mats, frame_step, levels, radius, iters, min_eig, fb_max32, max_err, row_cap)
    assert np.array_equal(out[1], want[1]), (out[1], want[1])
    if optional:
        assert np.array_equal(out[2], want[2]), np.argwhere(out[2] != want[2])[:8]
        assert np.array_equal(out[3], want[3]), np.argwhere(out[3] != want[3])[:8]
    else:
        assert out[2].min() == 0xFF and out[3].min() == T.NO_ERR
    assert out[0].tobytes() == want[0].tobytes(), np.argwhere(out[0].view(np.uint32) != want[0].view(np.uint32))[:8]
    return out


def seeds(ctx, frames, radius=2, cell=16, border=None, min_eig=0.0, pt_cap=64, src_layout=None, planes=None, size=None):
    import torch
    frames = np.asarray(frames)
    n = len(frames)
    border = radius + 1 if border is None else border
    _, src, _ = strided(frames.shape, src_layout, frames)
    pts = torch.full((n, pt_cap, 2), 0.0, dtype=torch.float32, device="cuda").view(torch.uint8).fill_(0xFF).view(torch.float32)
    npts = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    kw = dict(radius=radius, cell=cell, border=border, min_eig=min_eig, pts=pts, npts=npts)
    got = ctx.track_seeds(src, **kw) if planes is None else ctx.track_seeds_yuv420(planes, size=size, **kw)
    assert got[0] is pts and got[1] is npts
    ctx.synchronize()
    out = pts.cpu().numpy(), npts.cpu().numpy()
    want = T.track_seeds(frames, radius, cell, border, min_eig, pt_cap)
    assert np.array_equal(out[1], want[1]), (out[1], want[1])
    assert out[0].tobytes() == want[0].tobytes(), np.argwhere(out[0].view(np.uint32) != want[0].view(np.uint32))[:8]
    return out


def grid(w, h, nx, ny, margin):
    return F.grid_points(w, h, nx, ny, margin)


# ---- layouts ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("size,frame_step", [((64, 48), 1), ((65, 49), 1), ((65, 49), 2)])
def test_sizes_channels_and_frame_steps(ctx, size, frame_step, cn):
    w, h = size
    frames = shifted_stack(50 + cn, 4, w, h, cn)
    npairs = 3 if frame_step == 1 else 2
    pts = np.stack([np.concatenate([grid(w, h, 5, 4, 7), scatter(60 + p, 12, w, h)]) for p in range(npairs)])
    out = track(ctx, frames, pts, [32] * npairs, frame_step=frame_step, levels=2, radius=5, fb_max32=16)
    assert (out[1] >= 8).all()
    moved = out[0][0, :out[1][0], 2:] - out[0][0, :out[1][0], :2]
    assert np.abs(np.median(moved, 0) - (2.0, 1.0)).max() <= 0.25


@pytest.mark.parametrize("cn", [1, 3])
def test_strided_rows_and_odd_pointers(ctx, cn):
    w, h = 65, 49
    frames = shifted_stack(52, 3, w, h, cn)
    pts = np.stack([grid(w, h, 5, 4, 8)] * 2)
    want = track(ctx, frames, pts, [20, 20], levels=2, radius=5)
    for layout in ((w * cn + 1, (w * cn + 1) * h + 3, 1), (w * cn + 5, (w * cn + 5) * (h + 2), 7)):
        got = track(ctx, frames, pts, [20, 20], levels=2, radius=5, src_layout=layout)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), layout


@pytest.mark.parametrize("size", [(64, 48), (65, 49)])
def test_planes_equal_the_restatement_on_the_converted_frames(ctx, size):
    import torch
    rng = np.random.default_rng(33)
    w, h = size
    cw, ch = (w + 1) // 2, (h + 1) // 2
    luma = shifted_stack(53, 3, w, h, 1)
    planes = [(g, rng.integers(96, 160, (ch, cw), dtype=np.uint8), rng.integers(96, 160, (ch, cw), dtype=np.uint8)) for g in luma]
    bgr = W.planes_to_bgr(planes)
    y, cb, cr = (dev(np.stack([p[i] for p in planes])) for i in range(3))
    uv = torch.stack([cb, cr], dim=-1).contiguous()
    packed = dev(np.stack([np.concatenate([a.reshape(-1) for a in p]) for p in planes]))
    pts = np.stack([grid(w, h, 5, 4, 8)] * 2)
    for name, src, sz in (("i420", (y, cb, cr), None), ("nv12", (y, uv[..., 0], uv[..., 1]), None), ("packed", packed, (w, h))):
        out = track(ctx, bgr, pts, [20, 20], levels=3, radius=3, fb_max32=16, planes=src, size=sz)
        assert (out[1] >= 10).all(), name
        seeds(ctx, bgr, radius=2, cell=16, border=4, min_eig=1.0, planes=src, size=sz)


# ---- levels and radii ------------------------------------------------------------------------------------------------------------------------
def test_a_top_level_too_small_for_the_window_is_skipped(ctx):
    """64 x 48, levels 3, radius 5: level 2 is 16 x 12 and no 13 x 13 template fits it"""
    frames = shifted_stack(54, 2, 64, 48, 1, sigma=2.5)
    pts = grid(64, 48, 5, 4, 14)[None]
    three = track(ctx, frames, pts, [20], levels=3, radius=5)
    two = track(ctx, frames, pts, [20], levels=2, radius=5)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(three, two)) and three[1][0] >= 10


def test_levels_that_do_not_exist(ctx):
    """17 x 9 with levels 4: 8 x 4, 4 x 2, and 2 x 1 does not exist; 3 x 3 and 1 x 1 have level 0 alone and no window"""
    frames = shifted_stack(55, 2, 17, 9, 1)
    pts = np.array([[(8, 4), (8.5, 4.25), (2, 2), (14, 6), (16, 8), (0, 0)]], np.float32)
    out = track(ctx, frames, pts, [6], levels=4, radius=1, iters=8)
    assert out[1][0] >= 2
    for w, h in ((3, 3), (1, 1), (2, 5)):
        out = track(ctx, frames_of(56, 2, w, h, True), np.zeros((1, 2, 2), np.float32), [2], levels=4, radius=1)
        assert out[1][0] == 0 and (out[2][0] == T.NO_WINDOW).all()


@pytest.mark.parametrize("radius", [1, 10])
def test_smallest_and_largest_window(ctx, radius):
    frames = shifted_stack(57, 2, 65, 49, 3, sigma=2.0)
    pts = np.concatenate([grid(65, 49, 6, 4, radius + 1), scatter(58, 8, 65, 49)])[None]
    out = track(ctx, frames, pts, [32], levels=2, radius=radius, iters=64 if radius == 1 else 10, fb_max32=16, max_err=255)
    assert out[1][0] >= 4


# ---- points ----------------------------------------------------------------------------------------------------------------------------------
def test_points_on_and_beside_the_border(ctx):
    """Level 0 alone, identical frames: windows that touch the last column or row, and points one unit to either side of every bound.
    What this holds is the flags and the values.  That the tap of weight 0 beyond the last column is not READ it cannot see: the
    kernel samples the gray pyramid in the context's workspace, where another level or frame follows; the guards in level_sample
    are right by reading."""
    w, h, r = 64, 48, 5
    g = texture(59, w, h)
    frames = np.stack([g, g])
    edge = [(r + 1, r + 1), (w - 2 - r, h - 2 - r), (w - 2 - r, r + 1), (r + 1, h - 2 - r),                 # the template touches the frame's edge
            (r + 1 - 1 / 32, 20), (w - 2 - r + 1 / 32, 20), (20, h - 2 - r + 1 / 32), (r + 1.5, h - 2 - r - 0.5),
            (0, 0), (w - 1, h - 1), (w - 1 + 1 / 64, 5), (w - 1 + 1 / 32, 5), (-1 / 64, 5), (-1 / 32, 5), (5, h - 1 + 1 / 32)]
    pts = np.array([edge], np.float32)
    out = track(ctx, frames, pts, [len(edge)], levels=1, radius=r, iters=4)
    assert out[2][0].tolist() == [0, 0, 0, 0, T.NO_WINDOW, T.NO_WINDOW, T.NO_WINDOW, 0, T.NO_WINDOW, T.NO_WINDOW, T.NO_WINDOW, T.BAD_POINT,
                                  T.NO_WINDOW, T.BAD_POINT, T.BAD_POINT]
    # the search window at the edge while the template is not: a guess that moves the point there
    inner = np.array([[(20, 20), (30, 24)]], np.float32)
    for dx, dy, flag in ((w - 1 - r - 30, 0, None), (w - 1 - r - 30 + 1 / 32, 0, T.LEFT_FRAME), (r - 20, r - 20, None), (r - 20 - 1 / 32, 0, T.LEFT_FRAME)):
        out = track(ctx, frames, inner, [2], mats=W.translation(dx, dy).reshape(1, 9), levels=1, radius=r, iters=1)
        if flag is not None:
            assert flag in out[2][0].tolist(), (dx, dy, out[2])


def test_points_that_are_no_points_and_counts(ctx):
    frames = shifted_stack(60, 4, 64, 48, 1)
    good = grid(64, 48, 3, 2, 12)
    bad = np.array([(np.nan, 5), (5, np.nan), (np.inf, 5), (5, -np.inf), (-3, 5), (5, -0.5), (64, 5), (5, 48), (1e30, 1e30)], np.float32)
    pts = np.stack([np.concatenate([good[:3], bad, good[3:]])] * 3)
    out = track(ctx, frames, pts, [15, 15, 15], levels=2, radius=5)
    assert (out[2][:, 3:12] == T.BAD_POINT).all() and (out[1] == 6).all()
    for npts in ([0, 1, 15], [16, 99, -1], [-2147483648, 2147483647, 7]):                         # counts 0, 1, pt_cap and beyond it
        out = track(ctx, frames, pts, npts, levels=2, radius=5)
    out = track(ctx, frames, pts, [15, 3, 0], levels=2, radius=5, row_cap=21, optional=False)     # d_flags and d_err NULL, wider rows
    assert out[1].tolist() == [6, 3, 0]


def test_three_hundred_points_every_third_lost(ctx):
    """Compaction across waves, across the compaction's rounds of 256 and with a count that is no multiple of either"""
    frames = shifted_stack(61, 3, 65, 49, 1)
    for n in (300, 257, 509):
        pts = np.stack([scatter(62 + p, n, 65, 49) * np.float32(0.5) + np.float32(12) for p in range(2)])       # inside, away from the border
        pts[:, 2::3] = np.nan
        out = track(ctx, frames, pts, [n, n - 1], levels=2, radius=3, iters=10)
        assert out[1][0] == n - n // 3 and (out[2][0, 2::3] == T.BAD_POINT).all()


# ---- content and guesses ---------------------------------------------------------------------------------------------------------------------
def test_flat_frames_and_min_eig_on_the_boundary(ctx):
    g = texture(63, 64, 48)
    flat = np.full_like(g, 90)
    pts = grid(64, 48, 4, 3, 10)[None]
    out = track(ctx, np.stack([g, flat]), pts, [12], levels=2, radius=5)
    assert (out[2][0] == T.FLAT).all()
    out = track(ctx, np.stack([flat, g]), pts, [12], levels=2, radius=5, max_err=255)              # nothing to find, but a template
    # the bar exactly at a point's lambda, and one ulp to either side
    pyr = T.pyramid(g, 1)
    A0 = T.start_point(pts[0, 5, 0], pts[0, 5, 1], 64, 48)
    i, j = T._offsets(6)
    Tm = T.sample(pyr[0], A0[0] + 32 * i, A0[1] + 32 * j)
    gx, gy = (Tm[1:-1, 2:] - Tm[1:-1, :-2]).reshape(-1), (Tm[2:, 1:-1] - Tm[:-2, 1:-1]).reshape(-1)
    lam = T.min_eigenvalue(int((gx * gx).sum()), int((gx * gy).sum()), int((gy * gy).sum()))
    at = float(lam / 4194304.0 / 121.0)
    seen = set()
    for me in (np.nextafter(at, 0), at, np.nextafter(at, 1e9), at * 2, 0.0):
        out = track(ctx, np.stack([g, g]), pts, [12], levels=1, radius=5, min_eig=float(me))
        seen.add(int(out[2][0, 5]))
    assert seen == {T.TRACKED, T.FLAT}


def test_guesses_good_and_hopeless(ctx):
    prev, cur, M, guess = F.projective_pair(31, w=96, h=64)
    pts = grid(96, 64, 5, 3, 14)[None]
    frames = np.stack([prev, cur] * 6)
    nan_one = np.eye(3)
    nan_one[0, 1] = np.nan
    mats = np.stack([guess, np.full((3, 3), np.nan), np.zeros((3, 3)), 1e300 * np.eye(3) + W.translation(1e308, 0), W.translation(1e9, 0), nan_one])
    out = track(ctx, frames, np.repeat(pts, 6, 0), [15] * 6, mats=mats, frame_step=2, levels=2, radius=7, fb_max32=16)
    none = track(ctx, frames[:2], pts, [15], levels=2, radius=7, fb_max32=16)
    for p in (1, 2, 3, 4, 5):                                                                     # no usable guess: as without one
        assert out[1][p] == none[1][0] and out[0][p].tobytes() == none[0][0].tobytes(), p
    e = np.abs(out[0][0, :out[1][0], 2:] - F.apply(M, out[0][0, :out[1][0], :2])).max()
    assert out[1][0] >= 12 and e <= 0.5


@pytest.mark.parametrize("fb_max32,max_err", [(0, -1), (16, 0), (-1, 255), (16, 255), (-1, 3)])
def test_forward_backward_and_the_error_bar(ctx, fb_max32, max_err):
    frames = np.concatenate([shifted_stack(64, 2, 65, 49, 3, sigma=2.0), shifted_stack(65, 1, 65, 49, 3, sigma=2.0)])
    pts = np.stack([np.concatenate([grid(65, 49, 5, 4, 8), scatter(66, 12, 65, 49)])] * 2)
    out = track(ctx, frames, pts, [32, 32], levels=2, radius=5, fb_max32=fb_max32, max_err=max_err)      # pair 1: unrelated frames
    if max_err == 0:
        assert (out[1] == 0).all() or (out[3][out[2] == T.TRACKED] == 0).all()
    if max_err == 3:
        assert T.HIGH_ERROR in out[2][1]


# ---- npairs and repeatability ----------------------------------------------------------------------------------------------------------------
def test_no_pairs_three_pairs_and_the_same_call_twice(ctx):
    import torch
    frames = shifted_stack(67, 4, 64, 48, 3)
    pts = np.stack([grid(64, 48, 5, 4, 8)] * 3)
    a = track(ctx, frames, pts, [20, 7, 0], levels=3, radius=4, fb_max32=8, max_err=40)
    b = track(ctx, frames, pts, [20, 7, 0], levels=3, radius=4, fb_max32=8, max_err=40)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and a[1][2] == 0 and a[1][0] > a[1][1] > 0
    one = track(ctx, frames[1:3], pts[1:2], [7], levels=3, radius=4, fb_max32=8, max_err=40)        # a pair does not depend on its neighbours
    assert one[0][0].tobytes() == a[0][1].tobytes() and one[2][0].tobytes() == a[2][1].tobytes()
    rows, counts = ctx.track_points(dev(frames), dev(pts[:0]), dev(np.zeros(0, np.int32)))
    assert rows.shape == (0, 20, 4) and counts.shape == (0,)
    with pytest.raises(ValueError):
        ctx.track_points(dev(frames[:2]), dev(pts[:2]), dev(np.zeros(2, np.int32)))              # two pairs take three frames
    with pytest.raises(ValueError):
        ctx.track_points(dev(frames), dev(pts), dev(np.zeros(3, np.int32)), rows=torch.zeros((3, 20, 3), device="cuda"))


# ---- seeds -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("size", [(64, 48), (65, 49), (17, 9)])
@pytest.mark.parametrize("radius,cell", [(1, 8), (3, 64), (2, 16)])
def test_seeds_equal_the_restatement(ctx, size, cn, radius, cell):
    w, h = size
    frames = np.stack([texture(70 + cn, w, h, 1.5, cn), np.full((h, w, 3)[:2 if cn == 1 else 3], 50, np.uint8), texture(72, w, h, 3.0, cn)])
    for border, min_eig, pt_cap in ((radius + 1, 0.0, 64), (radius + 2, 4.0, 64), (radius + 1, 0.0, 3), ((min(w, h) + 1) // 2, 0.0, 8)):
        out = seeds(ctx, frames, radius, cell, border, min_eig, pt_cap)
    assert out[1].tolist() == [0, 0, 0]                                                           # the last border empties the rectangle
    w2 = w * cn + 3
    seeds(ctx, frames, radius, cell, radius + 1, 1.0, 16, src_layout=(w2, w2 * h + 5, 1))


def test_seeds_borders_that_empty_the_rectangle_up_to_int_max(ctx):
    """[border, w - 1 - border] holds a pixel iff border <= (w - 1) / 2; 2 * border must not be formed in 32 bits.  Every larger
    border is the empty rectangle of the header: 0 seeds, nothing else written, no launch over the frames."""
    w, h = 65, 49
    frames = np.stack([texture(73, w, h), texture(74, w, h)])
    for border in ((h - 1) // 2 + 1, w, 4096, (1 << 30) - 1, 1 << 30, (1 << 30) + 1, (1 << 31) - 33, (1 << 31) - 1):
        out = seeds(ctx, frames, 2, 16, border, 0.0, 8)
        assert out[1].tolist() == [0, 0], border
    out = seeds(ctx, frames, 2, 16, (h - 1) // 2, 0.0, 8)                                          # the last border that holds a row
    assert (out[1] == (w - 2 * ((h - 1) // 2) + 15) // 16).all()


def test_seeds_feed_the_tracker_on_the_low_contrast_family(ctx):
    from evenvizion_amd import tracking
    seed, dx, dy = F.LOW_SHIFTS[0]
    prev, cur, M = F.shift_pair(seed, dx, dy, **F.LOW)
    pts, npts = seeds(ctx, cur[None], 2, 16, 8, tracking.MIN_EIG, 64)
    assert 2 * npts[0] >= 35
    out = track(ctx, np.stack([prev, cur]), pts, npts, levels=2, radius=5, min_eig=tracking.MIN_EIG, fb_max32=16)
    e = np.abs(out[0][0, :out[1][0], 2:] - F.apply(M, out[0][0, :out[1][0], :2])).max()
    print("%d seeds, %d tracked, worst %.3f px" % (npts[0], out[1][0], e))
    assert out[1][0] >= 18 and e <= 0.5


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(ctx):
    import torch
    from evenvizion_amd._lib import Yuv420
    INVALID, CAPACITY = -1, -3
    n, w, h, cap = 3, 23, 17, 8
    A = Arena(10)
    src = A.put(frames_of(80, n + 1, w, h))
    pts = A.put(np.tile(np.array([(10, 8)], np.float32), (n, cap, 1)))
    npts = A.put(np.full(n, cap, np.int32))
    mats = A.put(np.tile(np.eye(3).reshape(1, 9), (n, 1)))
    rows = A.take((n, cap, 4), torch.float32, 7.0)
    counts = A.take((n,), torch.int32, -1)
    flags = A.take((n, cap), torch.uint8, 9)
    err = A.take((n, cap), torch.int32, -1)
    f, P, N, M, R, C, FL, E = (t.data_ptr() for t in (src, pts, npts, mats, rows, counts, flags, err))
    rs, fs = w * 3, w * h * 3
    good = dict(ctx=ctx.h, frames=f, n=n, step=1, w=w, h=h, cn=3, rs=rs, fs=fs, pts=P, npts=N, cap=cap, M=M, levels=2, radius=2, iters=3,
                eig=0.0, fb=-1, maxerr=-1, rows=R, rcap=cap, counts=C, flags=FL, err=E)

    def call(**kw):
        a = dict(good, **kw)
        return ctx.lib.evh_track_points(a["ctx"], a["frames"], a["n"], a["step"], a["w"], a["h"], a["cn"], a["rs"], a["fs"], a["pts"], a["npts"],
                                        a["cap"], a["M"], a["levels"], a["radius"], a["iters"], a["eig"], a["fb"], a["maxerr"], a["rows"],
                                        a["rcap"], a["counts"], a["flags"], a["err"])

    who, who_yuv = "evh_track_points: ", "evh_track_points_yuv420: "
    NS, NA, CH, STEP = "NULL source", "NULL argument", "channels must be 1 or 3", "frame_step must be 1 or 2"
    EM, PC, RC = "empty frame or negative npairs", "pt_cap must be at least 1", "row_cap smaller than pt_cap"
    LV, RD, IT = "levels must lie in 1..4", "radius must lie in 1..10", "iters must lie in 1..64"
    ME, MX = "min_eig must be finite and not negative", "max_err must be -1 or lie in 0..255"
    BIG, NP, NPT, NF = "w and h stay within 4096", "at most 65535 pairs per call", "at most 65535 points per pair", "at most 65535 frames per call"
    SS = "source stride smaller than a row / frame"

    def refused(rc, code, text, what):
        assert rc == code, what
        assert ctx.lib.evh_last_error_string(ctx.h).decode() == text, what

    assert call(ctx=None) == INVALID
    invalid = [(dict(frames=None), NS), (dict(pts=None), NA), (dict(npts=None), NA), (dict(rows=None), NA), (dict(counts=None), NA),
               (dict(cn=2), CH), (dict(step=0), STEP), (dict(step=3), STEP), (dict(w=0), EM), (dict(h=-1), EM), (dict(n=-1), EM),
               (dict(cap=0, rcap=0), PC), (dict(rcap=cap - 1), RC), (dict(levels=0), LV), (dict(levels=5), LV), (dict(radius=0), RD),
               (dict(radius=11), RD), (dict(iters=0), IT), (dict(iters=65), IT), (dict(eig=-1e-300), ME), (dict(eig=float("nan")), ME),
               (dict(eig=float("inf")), ME), (dict(maxerr=-2), MX), (dict(maxerr=256), MX), (dict(rs=rs - 1), SS), (dict(fs=fs - 1), SS),
               (dict(n=1, fs=fs - 1), SS),
               (dict(rows=f), "d_out_rows overlaps the frames"), (dict(rows=C - n * cap * 16 + 1), "d_out_rows overlaps d_out_counts"),
               (dict(rows=FL), "d_out_rows overlaps d_flags"), (dict(rows=E + 4), "d_out_rows overlaps d_err"),
               (dict(rows=P + 8), "d_out_rows overlaps d_pts"), (dict(rows=N), "d_out_rows overlaps d_npts"), (dict(rows=M + 64), "d_out_rows overlaps d_M"),
               (dict(counts=FL + 3), "d_out_counts overlaps d_flags"), (dict(counts=E), "d_out_counts overlaps d_err"),
               (dict(counts=f + 4), "d_out_counts overlaps the frames"), (dict(flags=E + 1), "d_flags overlaps d_err"),
               (dict(flags=P), "d_flags overlaps d_pts"), (dict(flags=f + (n + 1) * fs - 1), "d_flags overlaps the frames"),
               (dict(err=N + 4), "d_err overlaps d_npts"), (dict(err=M), "d_err overlaps d_M"),
               # two faults: the earlier check of the entry names the refusal
               (dict(frames=None, pts=None), NS), (dict(pts=None, cn=2), NA), (dict(step=0, n=-1), STEP), (dict(levels=9, radius=0), LV),
               (dict(iters=0, eig=-1.0), IT), (dict(maxerr=300, rs=1), MX), (dict(rs=rs - 1, rows=f), SS)]
    for kw, text in invalid:
        refused(call(**kw), INVALID, who + text, kw)
    capacity = [(dict(w=4097, rs=4097 * 3, fs=4097 * 3 * h), BIG), (dict(h=4097, fs=rs * 4097), BIG), (dict(n=65536), NP),
                (dict(cap=65536, rcap=65536), NPT), (dict(w=4097), BIG), (dict(n=65536, fs=fs - 1), NP), (dict(w=4097, n=65536), BIG)]
    for kw, text in capacity:
        refused(call(**kw), CAPACITY, who + text, kw)
    cw, ch = 12, 9
    y = A.take((n + 1, h, w))
    c = A.take((2, n + 1, ch, cw))
    torch.cuda.synchronize()
    yuv = dict(d_y=y.data_ptr(), d_cb=c[0].data_ptr(), d_cr=c[1].data_ptr(), y_stride=w, c_stride=cw, y_frame_stride=w * h,
               c_frame_stride=cw * ch, c_pixel_stride=1)

    def call_yuv(desc, **kw):
        a = dict(good, **kw)
        d = None if desc is None else ctypes.byref(Yuv420(**desc))
        return ctx.lib.evh_track_points_yuv420(a["ctx"], d, a["n"], a["step"], a["w"], a["h"], a["pts"], a["npts"], a["cap"], a["M"], a["levels"],
                                               a["radius"], a["iters"], a["eig"], a["fb"], a["maxerr"], a["rows"], a["rcap"], a["counts"],
                                               a["flags"], a["err"])

    refused(call_yuv(None), INVALID, who_yuv + NS, "no description")
    for bad, text in ((dict(d_y=None), NS), (dict(c_pixel_stride=3), "chroma pixel stride must be 1 or 2"),
                      (dict(y_stride=w - 1), "luma row stride smaller than the width")):
        refused(call_yuv(dict(yuv, **bad)), INVALID, who_yuv + text, bad)
    for kw, text in ((dict(pts=None), NA), (dict(levels=0), LV), (dict(rows=y.data_ptr() + 7), "d_out_rows overlaps the frames"),
                     (dict(flags=c[1].data_ptr()), "d_flags overlaps the frames")):
        refused(call_yuv(yuv, **kw), INVALID, who_yuv + text, kw)
    for kw, text in ((dict(w=4097), BIG), (dict(n=65536), NP), (dict(n=65535), NF)):
        refused(call_yuv(yuv, **kw), CAPACITY, who_yuv + text, kw)

    # the seeds' refusals
    def call_seeds(**kw):
        a = dict(dict(good, radius=2, cell=8, border=3), **kw)
        return ctx.lib.evh_track_seeds(a["ctx"], a["frames"], a["n"], a["w"], a["h"], a["cn"], a["rs"], a["fs"], a["radius"], a["cell"], a["border"],
                                       a["eig"], a["rows"], a["rcap"], a["counts"])

    sw = "evh_track_seeds: "
    for kw, text in ((dict(frames=None), NS), (dict(rows=None), NA), (dict(counts=None), NA), (dict(cn=4), CH), (dict(n=-1), "empty frame or negative nframes"),
                     (dict(rcap=0), PC), (dict(radius=0), "radius must lie in 1..3"), (dict(radius=4, border=9), "radius must lie in 1..3"),
                     (dict(cell=7), "cell must lie in 8..64"), (dict(cell=65), "cell must lie in 8..64"), (dict(border=2), "border must be at least radius + 1"),
                     (dict(eig=-1.0), ME), (dict(rs=rs - 1), SS), (dict(fs=fs - 1), SS), (dict(rows=f + 5), "d_pts overlaps the frames"),
                     (dict(rows=C - 4), "d_pts overlaps d_npts"), (dict(counts=f), "d_npts overlaps the frames")):
        refused(call_seeds(**kw), INVALID, sw + text, kw)
    for kw, text in ((dict(w=4097), BIG), (dict(n=65536), NF), (dict(rcap=65536), "at most 65535 points per frame")):
        refused(call_seeds(**kw), CAPACITY, sw + text, kw)
    assert call_seeds(n=1, fs=0) == 0                                                             # one frame: its stride is not looked at
    ctx.synchronize()
    assert counts[0] >= 0 and (counts[1:] == -1).all()
    counts.fill_(-1)
    rows.fill_(7.0)
    torch.cuda.synchronize()
    # no pairs: success, and nothing is done
    assert call(n=0) == 0 and call_yuv(yuv, n=0) == 0 and call_seeds(n=0) == 0
    ctx.synchronize()
    assert (rows == 7.0).all() and (counts == -1).all() and (flags == 9).all() and (err == -1).all()
    # the same arguments unrefused do write; d_M, d_flags and d_err may be NULL
    assert call() == 0
    ctx.synchronize()
    assert (counts >= 0).all() and (flags < 7).all()
    assert call(M=None, flags=None, err=None, n=1) == 0
    ctx.synchronize()
