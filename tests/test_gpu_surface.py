"""evh_warp_ray_surface / evh_warp_ray_surface_yuv420 on the device, and surface.surface_frames on a rendered pan of 200 degrees.
Every comparison is equality of bytes with the numpy restatement of the header's arithmetic (tests/surface_checks.py, itself
held against warp_checks in test_surface_host.py)."""
import ctypes
import math

import numpy as np
import pytest

import surface_checks as SC
import warp_checks as W
from evenvizion_amd import surface as F

pytestmark = pytest.mark.gpu
SENTINEL = 0xCD


@pytest.fixture(scope="module")
def ctx():
    from evenvizion_amd._lib import Context
    c = Context(device=0, max_w=64, max_h=64, max_features=500, max_frames=2)     # the entry does not depend on these sizes
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(ctx, frames, mats, cols, rows, mode, background=None, src_pad=0, out_pad=0, out_skip=0, bg_skip=None):
    """frames u8[n,sh,sw(,c)] through Context.warp_ray_surface -> the canvases as numpy.  src_pad / out_pad: extra pixels per
    source / output row (views of wider tensors, the padding holds SENTINEL and must survive); out_skip / bg_skip: the output /
    background view starts that many pixels into its rows (an unaligned base; bg_skip defaults to out_skip)."""
    import torch
    frames = np.asarray(frames)
    n, sh, sw = frames.shape[:3]
    tail = frames.shape[3:]
    dw, dh = len(cols), len(rows)
    src = torch.full((n, sh + 1, sw + src_pad) + tail, SENTINEL, dtype=torch.uint8, device="cuda")
    src[:, :sh, :sw] = dev(frames)
    lead = () if mode == "mosaic" else (n,)
    inside = (slice(None),) * len(lead) + (slice(0, dh), slice(out_skip, out_skip + dw))
    full = torch.full(lead + (dh + 1, out_skip + dw + out_pad) + tail, SENTINEL, dtype=torch.uint8, device="cuda")
    bg = None
    if background is not None:
        bg_skip = out_skip if bg_skip is None else bg_skip
        assert bg_skip <= out_skip + out_pad
        bgfull = torch.full((dh + 1, out_skip + dw + out_pad) + tail, SENTINEL, dtype=torch.uint8, device="cuda")
        bg = bgfull[:dh, bg_skip:bg_skip + dw]
        bg.copy_(dev(np.asarray(background, np.uint8).reshape((dh, dw) + tail)))
    ctx.warp_ray_surface(src[:, :sh, :sw], dev(np.asarray(mats, np.float64).reshape(n, 9)), dev(np.asarray(cols, np.float64)),
                         dev(np.asarray(rows, np.float64)), full[inside], mode, background=bg)
    ctx.synchronize()
    got = full.cpu().numpy()
    gaps = np.ones(got.shape, bool)
    gaps[inside] = False
    assert (got[gaps] == SENTINEL).all(), "bytes outside the canvas rows were written"
    return got[inside]


def check(ctx, frames, mats, cols, rows, mode, background=None, **kw):
    want = SC.ray_canvases(frames, mats, cols, rows, mode, background)
    got = run(ctx, frames, mats, cols, rows, mode, background, **kw)
    print("%s %dx%d: differing bytes %d of %d" % (mode, len(cols), len(rows), (got != want).sum(), want.size))
    assert np.array_equal(got, want)
    return got


def frames_of(seed, n, w, h, gray=False):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w) if gray else (n, h, w, 3), dtype=np.uint8)


def rot(pan, tilt=0.0, roll=0.0):
    """Rays of a camera panned, then tilted, then rolled (degrees) -> rays of the fixed system."""
    def c_s(d):
        return math.cos(math.radians(d)), math.sin(math.radians(d))
    (c, s), (ct, st), (cr, sr) = c_s(pan), c_s(tilt), c_s(roll)
    Ry = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float64)
    Rx = np.array([[1, 0, 0], [0, ct, -st], [0, st, ct]], np.float64)
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]], np.float64)
    return np.dot(Ry, np.dot(Rx, Rz))


def camera(R, focal, w, h):
    """d_A of a w x h frame: K . R^T"""
    return F.frame_matrix(R, focal, None, (w, h), (w, h))


# ---- modes and layouts -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("size", [(23, 17, 20.0), (8, 6, 7.0)])
@pytest.mark.parametrize("pads", [(0, 0, 0, None), (3, 1, 0, None), (1, 2, 0, None), (0, 1, 1, None), (0, 1, 0, 1)])
def test_modes_and_layouts(ctx, gray, size, pads):
    """(source pad, output pad, output skip, background skip) in pixels: with gray frames and dw = 43 the output rows are 44 bytes
    apart -- words -- where the pad is 1, and the background of the last case starts one byte into its row -- bytes."""
    w, h, focal = size
    f = frames_of(41, 4, w, h, gray)
    mats = [camera(rot(a, t, r), focal, w, h) for a, t, r in ((0, 0, 0), (25, 8, 0), (-30, -5, 10), (55, 0, -4))]
    dw, dh = 43, 19                                                       # not a multiple of the run of 4
    cols, rows = F.surface_tables("cylinder", focal, -17, -9, dw, dh)
    bg = frames_of(42, 1, dw, dh, gray)[0]
    kw = dict(src_pad=pads[0], out_pad=pads[1], out_skip=pads[2], bg_skip=pads[3])
    covers = [SC.ray_frame(f[k], mats[k], cols, rows)[1] for k in range(4)]
    assert all(c.any() for c in covers) and not np.any(covers, axis=0).all() and (np.sum(covers, axis=0) >= 2).any()
    for mode in ("each", "history", "mosaic"):
        check(ctx, f, mats, cols, rows, mode, bg, **kw)
    check(ctx, f, mats, cols, rows, "each", None, **kw)                  # no background: zeros
    hist = check(ctx, f, mats, cols, rows, "history", None, **kw)
    assert np.array_equal(hist[-1], SC.ray_canvases(f, mats, cols, rows, "mosaic"))


def test_planes_equal_the_bgr_entry_on_the_converted_frames(ctx):
    import torch
    rng = np.random.default_rng(43)
    n, w, h, cw, ch = 3, 23, 17, 12, 9
    planes = [(rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8),
               rng.integers(0, 256, (ch, cw), dtype=np.uint8)) for _ in range(n)]
    bgr = SC.planes_to_bgr(planes)
    mats = np.stack([camera(rot(a, t, r), 20.0, w, h) for a, t, r in ((0, 0, 0), (25, 8, 0), (-30, -5, 10))])
    dw, dh = 45, 19
    cols, rows = F.surface_tables("sphere", 20.0, -20, -9, dw, dh)
    bg = frames_of(44, 1, dw, dh)[0]
    d_m, d_bg, d_c, d_r = dev(mats), dev(bg), dev(cols), dev(rows)
    y, cb, cr = (dev(np.stack([p[i] for p in planes])) for i in range(3))
    uv = torch.stack([cb, cr], dim=-1).contiguous()
    packed = dev(np.stack([np.concatenate([a.reshape(-1) for a in p]) for p in planes]))
    conv = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    ctx.yuv420_to_bgr((y, cb, cr), conv)
    ctx.synchronize()
    assert np.array_equal(conv.cpu().numpy(), bgr)
    for mode in ("each", "history", "mosaic"):
        want = SC.ray_canvases(bgr, mats, cols, rows, mode, bg)
        shape = (dh, dw, 3) if mode == "mosaic" else (n, dh, dw, 3)
        via_bgr = torch.zeros(shape, dtype=torch.uint8, device="cuda")
        ctx.warp_ray_surface(conv, d_m, d_c, d_r, via_bgr, mode, background=d_bg)
        ctx.synchronize()
        assert np.array_equal(via_bgr.cpu().numpy(), want), mode
        for name, src, size in (("i420", (y, cb, cr), None), ("nv12", (y, uv[..., 0], uv[..., 1]), None), ("packed", packed, (w, h))):
            out = torch.full(shape, SENTINEL, dtype=torch.uint8, device="cuda")
            ctx.warp_ray_surface(src, d_m, d_c, d_r, out, mode, background=d_bg, size=size)
            ctx.synchronize()
            assert np.array_equal(out.cpu().numpy(), want), (mode, name)


# ---- the antipode ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, tilt, roll", [("cylinder", 0.0, 0.0), ("sphere", 10.0, 5.0)])
def test_a_frame_lies_on_its_own_half_of_the_surface(ctx, kind, tilt, roll):
    """Eight frames panned in steps of 45 degrees on a surface that closes.  Without tw > 0 every frame would show a second time
    around the antipode of its axis; with it the half of the canvas 90 degrees and more from its axis stays empty."""
    w, h, focal = 23, 17, 20.0
    f = np.maximum(frames_of(45, 8, w, h), 1)                            # no zero byte: what a frame covers is what is not zero
    mats = [camera(rot(45.0 * k, tilt, roll), focal, w, h) for k in range(8)]
    dw, dh, ox = int(round(2 * math.pi * focal)), 24, -63
    assert dw == 126
    cols, rows = F.surface_tables(kind, focal, ox, -12, dw, dh)
    theta = (np.arange(dw) + ox) / focal
    each = check(ctx, f, mats, cols, rows, "each")
    for k in range(8):
        away = np.abs((theta - math.radians(45.0 * k) + math.pi) % (2 * math.pi) - math.pi) >= math.pi / 2
        assert 60 <= away.sum() <= 64                                    # half of the 126 columns
        lit = each[k].any(axis=(0, 2))
        assert lit.any() and not each[k][:, away].any(), k
        assert not (lit & away).any() and lit.sum() >= 18                # 2 atan(11 / 20) * 20 = 20.1 columns, less one at each end
        # the restatement without the sign: the antipode is there, which is what the sign keeps out
        val, cov, tw = SC.ray_frame(f[k], -np.asarray(mats[k]), cols, rows)
        assert cov.any() and cov[:, away].any() and not cov[:, ~away].any()
    mosaic = check(ctx, f, mats, cols, rows, "mosaic")
    assert mosaic.any(axis=(0, 2)).all()                                 # every column is covered
    assert not mosaic.any(axis=(1, 2)).all()                             # not every row: the surface is taller than the frames


# ---- the plane is the special case -----------------------------------------------------------------------------------------------------
def persp(deg, zoom, tx, ty, px, py):
    c, s = zoom * np.cos(np.deg2rad(deg)), zoom * np.sin(np.deg2rad(deg))
    return np.array([[c, -s, tx], [s, c, ty], [px, py, 1.0]], np.float64)


PLANE_MAPS = [np.eye(3), W.translation(4.25, -2.5), persp(17.0, 1.3, 3.5, -2.25, 1e-3, -2e-3), persp(-11.0, 0.8, 14.0, 9.5, -8e-4, 1.5e-3),
              persp(40.0, 0.6, 6.0, 1.0, 5e-3, 4e-3), 7.5 * persp(-3.0, 1.0, -2.0, 3.0, -4e-3, 2e-3)]


@pytest.mark.parametrize("gray", [False, True])
def test_plane_tables_give_the_fixed_plane_entry(ctx, gray):
    import torch
    dw, dh, origin = 37, 29, (-6, -4)
    cols, rows = F.surface_tables("plane", 1.0, origin[0], origin[1], dw, dh)
    assert np.array_equal(cols, SC.plane_tables(dw, dh, origin)[0]) and np.array_equal(rows, SC.plane_tables(dw, dh, origin)[1])
    f = frames_of(46, len(PLANE_MAPS), 23, 17, gray)
    for M in PLANE_MAPS:
        val, cov, tw = SC.ray_frame(f[0], M, cols, rows)
        assert (tw > 0).all() and cov.sum() > 40
    bg = frames_of(47, 1, dw, dh, gray)[0]
    d_f, d_m, d_bg = dev(f), dev(np.stack(PLANE_MAPS).reshape(-1, 9)), dev(bg)
    for mode in ("each", "history", "mosaic"):
        got = check(ctx, f, PLANE_MAPS, cols, rows, mode, bg)
        plane = torch.full(got.shape, SENTINEL, dtype=torch.uint8, device="cuda")
        ctx.warp_fixed_plane(d_f, d_m, plane, mode, origin, background=d_bg, inverse_map=True)
        ctx.synchronize()
        assert np.array_equal(plane.cpu().numpy(), got), mode
    # a horizon inside the canvas: tw = 0.125 X - 0.25 is negative for X < 2, zero at X = 2
    H = np.array([[0.5, 0, 0.25], [0, 0.5, 1.0], [0.125, 0, -0.25]], np.float64)
    val, cov, tw = SC.ray_frame(f[0], H, cols, rows)
    pval, pcov = W.warp_frame(f[0], H, dw, dh, origin, inverse_map=True)
    assert (tw < 0).any() and (tw == 0).any() and (tw > 0).any() and cov.any()
    assert (pcov & ~cov).any() and np.array_equal(pcov & (tw > 0), cov) and not (cov & ~pcov).any()
    got = check(ctx, f[:1], [H], cols, rows, "each", bg)[0]
    plane = torch.zeros((1,) + got.shape, dtype=torch.uint8, device="cuda")
    ctx.warp_fixed_plane(d_f[:1], dev(H.reshape(1, 9)), plane, "each", origin, background=d_bg, inverse_map=True)
    ctx.synchronize()
    plane = plane.cpu().numpy()[0]
    differ = (plane != got) if gray else (plane != got).any(axis=2)
    assert differ.any() and not differ[tw > 0].any()                    # the two differ only behind the horizon
    assert np.array_equal(got[tw <= 0], bg[tw <= 0])                     # and there the sign rules: nothing is covered


# ---- degenerate input ------------------------------------------------------------------------------------------------------------------
GOOD = camera(rot(10, 3, 2), 20.0, 23, 17)
NOTHING = {
    "nan": np.full(9, np.nan),
    "one_nan": np.where(np.arange(9) == 8, np.nan, GOOD),
    "zero": np.zeros(9),
    "inf": np.full(9, np.inf),
    "minus_inf": np.full(9, -np.inf),
    "negative": -GOOD,                                                    # the camera that looks the other way: all of tw <= 0 here
}


@pytest.mark.parametrize("name", sorted(NOTHING))
def test_nothing_covered_nothing_faulted(ctx, name):
    A = NOTHING[name]
    f = frames_of(48, 3, 23, 17)
    cols, rows = F.surface_tables("cylinder", 20.0, -14, -9, 41, 19)       # within 41 degrees of the axis of frame 1
    with np.errstate(all="ignore"):
        assert not SC.ray_frame(f[0], A, cols, rows)[1].any() and SC.ray_frame(f[0], GOOD, cols, rows)[1].sum() > 100
    bg = frames_of(49, 1, 41, 19)[0]
    for mode in ("each", "history", "mosaic"):
        got = check(ctx, f[:2], [A, A], cols, rows, mode, bg)
        assert np.array_equal(got, np.broadcast_to(bg, got.shape))
    check(ctx, f, [A, GOOD, A], cols, rows, "history", bg)               # a good frame between two bad ones is not disturbed
    check(ctx, f, [GOOD, A, GOOD], cols, rows, "mosaic", bg)


def test_nan_in_the_tables_and_tw_of_exactly_zero(ctx):
    f = frames_of(50, 2, 23, 17)
    bg = frames_of(51, 1, 41, 19)[0]
    cols, rows = F.surface_tables("cylinder", 20.0, -14, -9, 41, 19)
    mats = [GOOD, camera(rot(-8, 0, 0), 20.0, 23, 17)]
    whole = SC.ray_canvases(f, mats, cols, rows, "mosaic", bg)
    for what, at in (("a", 13), ("c", 14), ("b", 9)):
        c2, r2 = cols.copy(), rows.copy()
        if what == "b":
            r2[at] = np.nan
        else:
            c2[at, "ac".index(what)] = np.nan
        for mode in ("each", "history", "mosaic"):
            got = check(ctx, f, mats, c2, r2, mode, bg)
        line = (slice(at, at + 1), slice(None)) if what == "b" else (slice(None), slice(at, at + 1))
        assert np.array_equal(got[line], bg[line]) and (whole[line] != bg[line]).any()       # the NaN's line is left to the background
        rest = np.ones((19, 41), bool)
        rest[line] = False
        assert np.array_equal(got[rest], whole[rest])                    # and no other pixel is disturbed
    ct, rt = F.surface_tables("cylinder", 20.0, -14, -9, 41, 19)
    ct[:] = np.nan
    assert np.array_equal(check(ctx, f, mats, ct, rows, "mosaic", bg), bg)
    assert np.array_equal(check(ctx, f, mats, cols, np.full(19, np.nan), "mosaic", bg), bg)
    # tw == 0 exactly, between a side where tw < 0 would pass the range test (tx < 0 too) and the side that is covered
    pc, pr = SC.plane_tables(37, 17, (-12, 0))
    H = np.array([[1, 0, 0], [0, 1, 0], [0.25, 0, -1.0]], np.float64)                         # tw = X / 4 - 1, zero at X = 4
    val, cov, tw = SC.ray_frame(f[0], H, pc, pr)
    assert (tw[:, 16] == 0).all() and cov[:, 17:].any() and not cov[:, :17].any()
    assert W.warp_frame(f[0], H, 37, 17, (-12, 0), inverse_map=True)[1][:, :16].any()           # without the sign: covered
    pbg = frames_of(52, 1, 37, 17)[0]
    got = check(ctx, f[:1], [H], pc, pr, "each", pbg)[0]
    assert np.array_equal(got[:, :17], pbg[:, :17]) and (got[:, 17:] != pbg[:, 17:]).any()


# ---- carry -----------------------------------------------------------------------------------------------------------------------------
def test_mosaic_carried_in_place_over_two_calls(ctx):
    import torch
    w, h, focal = 23, 17, 20.0
    f = frames_of(53, 8, w, h)
    mats = np.stack([camera(rot(20.0 * k - 60, 4.0 * (k % 3) - 4, 3.0), focal, w, h) for k in range(8)])
    cols, rows = F.surface_tables("cylinder", focal, -40, -12, 83, 25)
    bg = frames_of(54, 1, 83, 25)[0]
    whole = check(ctx, f, mats, cols, rows, "mosaic", bg)
    covers = [SC.ray_frame(f[k], mats[k], cols, rows)[1] for k in range(8)]
    assert all(c.any() for c in covers) and (np.sum(covers, axis=0) >= 2).sum() > 100 and not np.any(covers, axis=0).all()
    canvas, d_f, d_m, d_c, d_r = dev(bg), dev(f), dev(mats), dev(cols), dev(rows)
    ctx.warp_ray_surface(d_f[:5], d_m[:5], d_c, d_r, canvas, "mosaic", background=canvas)
    ctx.warp_ray_surface(d_f[5:], d_m[5:], d_c, d_r, canvas, "mosaic", background=canvas)
    ctx.synchronize()
    assert np.array_equal(canvas.cpu().numpy(), whole)
    d_bg, out = dev(bg), torch.zeros((25, 83, 3), dtype=torch.uint8, device="cuda")        # not in place: the background stays
    ctx.warp_ray_surface(d_f, d_m, d_c, d_r, out, "mosaic", background=d_bg)
    ctx.synchronize()
    assert np.array_equal(out.cpu().numpy(), whole) and np.array_equal(d_bg.cpu().numpy(), bg)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_alone(ctx):
    import torch
    from evenvizion_amd._lib import Yuv420
    INVALID, CAPACITY = -1, -3
    n, sw, sh, dw, dh = 2, 23, 17, 31, 22
    src = dev(frames_of(55, n, sw, sh))
    pc, pr = SC.plane_tables(dw, dh)
    mats, cols, rows = dev(np.tile(np.eye(3).reshape(1, 9), (n, 1))), dev(pc), dev(pr)
    out = torch.full((n + 1, dh, dw, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    elsewhere = torch.full((dh, dw, 3), 7, dtype=torch.uint8, device="cuda")
    f, m, o, b = src.data_ptr(), mats.data_ptr(), out.data_ptr(), elsewhere.data_ptr()
    ors, ofs = dw * 3, dw * dh * 3
    good = dict(ctx=ctx.h, frames=f, n=n, sw=sw, sh=sh, cn=3, rs=sw * 3, fs=sw * sh * 3, A=m, col=cols.data_ptr(), row=rows.data_ptr(),
                mode=0, bg=b, out=o, dw=dw, dh=dh, ors=ors, ofs=ofs)

    def call(**kw):
        a = dict(good, **kw)
        return ctx.lib.evh_warp_ray_surface(a["ctx"], a["frames"], a["n"], a["sw"], a["sh"], a["cn"], a["rs"], a["fs"], a["A"], a["col"],
                                            a["row"], a["mode"], a["bg"], a["out"], a["dw"], a["dh"], a["ors"], a["ofs"])

    who, who_yuv = "evh_warp_ray_surface: ", "evh_warp_ray_surface_yuv420: "
    NS, NA, CH, EM, MODE = "NULL source", "NULL argument", "channels must be 1 or 3", "empty frame or canvas", "unknown mode"
    BIG, AREA = "source sizes stay below 2^26 (positions are held in 1/32 pixels)", "dw * dh above INT_MAX"
    NF, OS, SS = "at most 65535 frames per call", "output stride smaller than a row / canvas", "source stride smaller than a row / frame"
    OV = "d_background overlaps d_out"

    def refused(rc, code, text, what):
        assert rc == code, what
        assert ctx.lib.evh_last_error_string(ctx.h).decode() == text, what

    assert call(ctx=None) == INVALID
    invalid = [(dict(frames=None), NS), (dict(A=None), NA), (dict(col=None), NA), (dict(row=None), NA), (dict(out=None), NA),
               (dict(cn=2), CH), (dict(cn=0), CH), (dict(cn=4), CH),
               (dict(sw=0), EM), (dict(sh=0), EM), (dict(dw=0), EM), (dict(dh=-1), EM), (dict(n=-1), EM), (dict(rs=sw * 3 - 1), SS),
               (dict(fs=sw * sh * 3 - 1), SS), (dict(ors=ors - 1), OS), (dict(ofs=ofs - 1), OS), (dict(mode=1, ofs=ofs - 1), OS),
               (dict(mode=3), MODE), (dict(mode=-1), MODE),
               (dict(bg=o), OV), (dict(mode=1, bg=o), OV), (dict(bg=o + ofs), OV), (dict(bg=o + ofs + ors), OV), (dict(bg=o - ors), OV),
               (dict(mode=2, bg=o + 3), OV), (dict(mode=2, bg=o + ors), OV), (dict(mode=2, bg=o - ors), OV),      # mosaic: only bg == out
               (dict(frames=None, col=None), NS), (dict(col=None, cn=2), NA), (dict(row=None, mode=9), NA), (dict(cn=2, sw=0), CH)]
    for kw, text in invalid:
        refused(call(**kw), INVALID, who + text, kw)
    big = 1 << 26
    capacity = [(dict(sw=big, rs=big * 3, fs=big * 3 * sh), BIG), (dict(sh=big, fs=sw * 3 * big), BIG),
                (dict(dw=65536, dh=32768, ors=65536 * 3, ofs=1 << 40), AREA), (dict(n=65536), NF), (dict(n=65536, ors=ors - 1), NF)]
    for kw, text in capacity:
        refused(call(**kw), CAPACITY, who + text, kw)
    y = torch.zeros((n, sh, sw), dtype=torch.uint8, device="cuda")
    c = torch.zeros((2, n, 9, 12), dtype=torch.uint8, device="cuda")
    yuv = dict(d_y=y.data_ptr(), d_cb=c[0].data_ptr(), d_cr=c[1].data_ptr(), y_stride=sw, c_stride=12, y_frame_stride=sw * sh,
               c_frame_stride=12 * 9, c_pixel_stride=1)

    def call_yuv(desc, **kw):
        a = dict(good, **kw)
        d = None if desc is None else ctypes.byref(Yuv420(**desc))
        return ctx.lib.evh_warp_ray_surface_yuv420(a["ctx"], d, a["n"], a["sw"], a["sh"], a["A"], a["col"], a["row"], a["mode"], a["bg"],
                                                   a["out"], a["dw"], a["dh"], a["ors"], a["ofs"])

    refused(call_yuv(None), INVALID, who_yuv + NS, "no description")
    for bad, text in ((dict(d_cb=None), NS), (dict(c_pixel_stride=3), "chroma pixel stride must be 1 or 2"),
                      (dict(y_stride=sw - 1), "luma row stride smaller than the width")):
        refused(call_yuv(dict(yuv, **bad)), INVALID, who_yuv + text, bad)
    for kw, text in ((dict(A=None), NA), (dict(col=None), NA), (dict(row=None), NA), (dict(out=None), NA), (dict(dw=0), EM),
                     (dict(mode=7), MODE), (dict(ors=ors - 1), OS), (dict(bg=o), OV)):
        refused(call_yuv(yuv, **kw), INVALID, who_yuv + text, kw)
    for kw, text in ((dict(sw=big), BIG), (dict(n=65536), NF), (dict(dw=65536, dh=32768, ors=65536 * 3, ofs=1 << 40), AREA)):
        refused(call_yuv(yuv, **kw), CAPACITY, who_yuv + text, kw)
    # no frames: success, and nothing is done
    assert call(n=0) == 0 and call(n=0, mode=2, bg=o) == 0 and call_yuv(yuv, n=0) == 0
    ctx.synchronize()
    assert (out == SENTINEL).all() and (elsewhere == 7).all()
    # and the same arguments unrefused do write
    assert call() == 0 and call_yuv(yuv, mode=2, out=o + 2 * ofs, bg=None) == 0
    ctx.synchronize()
    assert np.array_equal(out[:n, :sh, :sw].cpu().numpy(), src.cpu().numpy()) and (out[0, sh:] == 7).all()
    assert (out[2] != SENTINEL).any()
    # the Python wrapper: tables of the wrong shape never reach the library
    for kw in (dict(cols=cols[:-1]), dict(rows=rows[:-1]), dict(cols=cols.float()), dict(rows=rows.cpu())):
        with pytest.raises(ValueError):
            ctx.warp_ray_surface(src, mats, kw.get("cols", cols), kw.get("rows", rows), out[:n], "each")


# ---- the driver: a pan of 200 degrees --------------------------------------------------------------------------------------------------
BLOCK, MARGIN, FOCAL, FRAME = 16, 2.0, 48.0, (64, 36)
THETA0 = math.radians(-60.0)                 # where the texture's columns start: outside everything a frame of the pan sees


def block_colour(theta, v, table):
    """The world: a cylinder of radius FOCAL pixels textured with constant BLOCK x BLOCK blocks of random colours.  -> (colours
    u8[..., 3], how many pixels the point lies inside its block: the distance to the block's nearest side)"""
    s = ((theta - THETA0) % (2 * math.pi)) * FOCAL
    t = v * FOCAL + 10 * BLOCK
    i, j = np.floor(s / BLOCK).astype(np.int64), np.floor(t / BLOCK).astype(np.int64)
    inside = np.minimum(np.minimum(s - i * BLOCK, (i + 1) * BLOCK - s), np.minimum(t - j * BLOCK, (j + 1) * BLOCK - t))
    return table[j % table.shape[0], i % table.shape[1]], inside


class Frames:
    """A capture over frames held in memory."""

    def __init__(self, frames):
        self.frames, self.at = frames, 0

    def read(self):
        if self.at >= len(self.frames):
            return False, None
        self.at += 1
        return True, self.frames[self.at - 1]


@pytest.fixture(scope="module")
def pan():
    """41 frames of 64 x 36 rendered from the world at pan steps of 5 degrees, and their dictionary: S_k = H_k . S_{k-1} divided by
    its [2][2], the reference's composition, from the exact H_k = K . R_k . R_{k-1}^T . K^-1."""
    w, h = FRAME
    table = np.random.default_rng(56).integers(1, 256, (24, 32, 3), dtype=np.uint8)          # no zero byte: covered is not zero
    centre = F._centre(FRAME, None)
    K = F.camera_matrix(FOCAL, centre)
    Rs = [rot(5.0 * k) for k in range(41)]
    px, py = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    frames = []
    for R in Rs:
        rays = np.einsum("ij,hwj->hwi", R, np.stack([(px - centre[0]) / FOCAL, (py - centre[1]) / FOCAL, np.ones_like(px)], axis=-1))
        frames.append(block_colour(np.arctan2(rays[..., 0], rays[..., 2]), rays[..., 1] / np.hypot(rays[..., 0], rays[..., 2]), table)[0])
    sup = {1: np.eye(3)}
    for k in range(1, 41):
        H = np.dot(np.dot(K, np.dot(Rs[k], Rs[k - 1].T)), np.linalg.inv(K))
        S = np.dot(H, sup[k])
        sup[k + 1] = S / S[2][2]
    return np.stack(frames), sup, {"w": w, "h": h}, table, Rs


@pytest.mark.parametrize("focal", [FOCAL, None])
def test_surface_frames_over_a_pan_the_plane_cannot_hold(pan, focal):
    """The mosaic of the pan on the cylinder.  A canvas pixel MARGIN = 2 or more pixels inside a block of the world must carry that
    block's colour exactly: its four taps are frame pixels at most one frame pixel away, a frame pixel is at most one canvas
    pixel wide on the cylinder (scale 1: equality at the frame's centre column), and v moves by less than 0.3 pixels per frame
    pixel along a row, so every tap lies inside the block, and bilinear weights over one colour give that colour.  Blocks are 16
    pixels wide: with 2 pixels off every side (12 / 16)^2 = 56 % of a block qualifies, which keeps the share asked for -- at
    least half of the covered area -- within reach; blocks of 8 would leave (4 / 8)^2 = 25 %."""
    from evenvizion_amd.stabilization import fixed_plane_bounds
    frames, sup, ri, table, Rs = pan
    with pytest.raises(ValueError):
        fixed_plane_bounds(sup, ri)                                      # past a quarter turn the plane has no canvas
    model = F.surface_model(sup, ri, "cylinder", focal=focal)
    print("focal %s: model focal %.6f, median fit residual %.3e, canvas %s" % (focal, model.focal, F.surface_report(model)["fit_residual_median"],
                                                                             model.bounds))
    assert abs(model.focal - FOCAL) <= 0.02 * FOCAL and model.estimated == (focal is None)
    ox, oy, dw, dh, scale_px = model.bounds
    assert dw > math.radians(200.0) * FOCAL and dw < int(round(2 * math.pi * scale_px))      # more than the pan, less than the turn
    got = list(F.surface_frames(Frames(frames), sup, ri, surface="cylinder", focal=focal, mode="mosaic", chunk_frames=16))
    assert len(got) == 1 and got[0][0] == 41 and got[0][1].shape == (dh, dw, 3)
    canvas = got[0][1]
    # the restatement of the whole run: the same tables and matrices through surface_checks
    cols, rows = F.surface_tables("cylinder", scale_px, ox, oy, dw, dh)
    mats = [F.frame_matrix(model.rotations[k + 1], model.focal, model.centre, FRAME, FRAME) for k in range(41)]
    assert np.array_equal(canvas, SC.ray_canvases(frames, mats, cols, rows, "mosaic"))
    covered = np.any([SC.ray_frame(frames[k], mats[k], cols, rows)[1] for k in range(41)], axis=0)
    assert np.array_equal(covered, canvas.any(axis=2)) and covered.mean() > 0.6
    theta = ((np.arange(dw) + ox) / scale_px)[None, :] + np.zeros((dh, 1))
    v = ((np.arange(dh) + oy) / scale_px)[:, None] + np.zeros((1, dw))
    colour, inside = block_colour(theta, v, table)
    sure = covered & (inside >= MARGIN)
    share = sure.sum() / covered.sum()
    wrong = (canvas[sure] != colour[sure]).any(axis=1).sum()
    print("covered %d of %d pixels, %d of them %g or more inside a block (share %.3f), %d of those wrong" %
          (covered.sum(), covered.size, sure.sum(), MARGIN, share, wrong))
    assert share >= 0.5
    assert wrong == 0
    # and the last frame lies where it was taken: 200 degrees from the first
    assert abs(F.surface_coordinates([model.centre], 41, model.rotations, model.focal, model.centre, "cylinder")[0][0]
               - math.radians(200.0) * model.focal) < 1e-6 * FOCAL


def test_surface_frames_history_and_each_follow_the_mosaic(pan):
    frames, sup, ri, table, Rs = pan
    n = 12
    sub = {k: sup[k] for k in range(1, n + 1)}
    model = F.surface_model(sub, ri, "sphere", focal=FOCAL)
    ox, oy, dw, dh, scale_px = model.bounds
    cols, rows = F.surface_tables("sphere", scale_px, ox, oy, dw, dh)
    mats = [F.frame_matrix(model.rotations[k + 1], FOCAL, model.centre, FRAME, FRAME) for k in range(n)]
    for mode in ("history", "each"):
        got = list(F.surface_frames(Frames(frames[:n]), sub, ri, surface="sphere", focal=FOCAL, mode=mode, chunk_frames=5))
        assert [g[0] for g in got] == list(range(1, n + 1))
        assert np.array_equal(np.stack([g[1] for g in got]), SC.ray_canvases(frames[:n], mats, cols, rows, mode)), mode
    # frames beyond the dictionary have no rotation and leave the canvas alone
    got = list(F.surface_frames(Frames(frames[:n + 2]), sub, ri, surface="sphere", focal=FOCAL, mode="history", chunk_frames=5))
    assert len(got) == n + 2 and np.array_equal(got[n][1], got[n - 1][1]) and np.array_equal(got[n + 1][1], got[n - 1][1])
