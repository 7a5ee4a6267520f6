"""evh_plate_fixed_plane / evh_plate_fixed_plane_yuv420 on the device.  Every assertion is equality of bytes with the numpy
restatement of the header's contract (tests/plate_checks.py, itself checked against a literal loop in test_plate_host.py), on
buffers padded with a sentinel that must survive."""
import ctypes
import os

import numpy as np
import pytest

import plate_checks as P
import warp_checks as W
from refusal_arena import Arena
from test_gpu_warp import NOTHING, rot_zoom_persp

pytestmark = pytest.mark.gpu
SENTINEL = 0xCD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MP4 = os.path.join(ROOT, "tests", "golden", "ref_test_video.mp4")
GOLD = os.path.join(ROOT, "tests", "golden", "ref_dict_with_homography_matrix.json")
PADS = [(0, 0, 0), (3, 1, 0), (1, 2, 0), (0, 1, 1)]          # (source, output, skipped) pixels per row, as in test_gpu_warp.py


@pytest.fixture(scope="module")
def ctx():
    from evenvizion_amd._lib import Context
    c = Context(device=0, max_w=64, max_h=64, max_features=500, max_frames=2)     # the entry does not depend on these sizes
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(ctx, frames, mats, dw, dh, origin=(0, 0), background=None, inverse_map=False, min_cover=1, threshold=16, count=True,
        masks=True, src_pad=0, out_pad=0, out_skip=0):
    """frames u8[n,sh,sw(,3)] through Context.plate_fixed_plane -> (plate, count or None, masks or None) as numpy.  All three
    outputs are views of wider, taller tensors filled with SENTINEL (out_pad extra pixels per row, starting out_skip pixels into
    their rows); everything outside the views -- and an output that was not asked for -- must still hold it afterwards."""
    import torch
    frames = np.asarray(frames)
    n, sh, sw = frames.shape[:3]
    tail = frames.shape[3:]
    src = torch.full((n, sh + 1, sw + src_pad) + tail, SENTINEL, dtype=torch.uint8, device="cuda")
    src[:, :sh, :sw] = dev(frames)
    wide = out_skip + dw + out_pad
    inside = (slice(0, dh), slice(out_skip, out_skip + dw))
    full = {"plate": torch.full((dh + 1, wide) + tail, SENTINEL, dtype=torch.uint8, device="cuda"),
            "count": torch.full((dh + 1, wide), SENTINEL, dtype=torch.uint8, device="cuda"),
            "masks": torch.full((n, dh + 1, wide), SENTINEL, dtype=torch.uint8, device="cuda")}
    where = {"plate": inside, "count": inside, "masks": (slice(None),) + inside}
    asked = {"plate": True, "count": count, "masks": masks}
    bg = None
    if background is not None:
        bgfull = torch.full((dh + 1, wide) + tail, SENTINEL, dtype=torch.uint8, device="cuda")
        bg = bgfull[inside]
        bg.copy_(dev(np.asarray(background, np.uint8).reshape((dh, dw) + tail)))
    ctx.plate_fixed_plane(src[:, :sh, :sw], dev(np.asarray(mats, np.float64).reshape(n, 9)), full["plate"][inside], origin,
                          background=bg, count=full["count"][inside] if count else None,
                          masks=full["masks"][where["masks"]] if masks else None, threshold=threshold, min_cover=min_cover,
                          inverse_map=inverse_map)
    ctx.synchronize()
    out = []
    for name in ("plate", "count", "masks"):
        got = full[name].cpu().numpy()
        gaps = np.ones(got.shape, bool)
        if asked[name]:
            gaps[where[name]] = False
        assert (got[gaps] == SENTINEL).all(), "bytes outside the rows of %s were written" % name
        out.append(got[where[name]] if asked[name] else None)
    if background is not None:
        assert np.array_equal(bg.cpu().numpy(), np.asarray(background, np.uint8).reshape((dh, dw) + tail))
    return tuple(out)


def check(ctx, frames, mats, dw, dh, origin=(0, 0), background=None, inverse_map=False, min_cover=1, threshold=16, want=None, **kw):
    """-> the expected (plate, count, masks), for further assertions and for reuse as `want`"""
    if want is None:
        want = P.plate(frames, mats, dw, dh, origin, background, inverse_map, min_cover, threshold)
    got = run(ctx, frames, mats, dw, dh, origin, background, inverse_map, min_cover, threshold, **kw)
    for g, w, name in zip(got, want, ("plate", "count", "masks")):
        if g is not None:
            print("%s %dx%d n=%d: differing bytes %d of %d" % (name, dw, dh, len(frames), (g != w).sum(), w.size))
    for g, w, name in zip(got, want, ("plate", "count", "masks")):
        assert g is None or np.array_equal(g, w), name
    return want


def frames_of(seed, n, w, h, gray=False):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w) if gray else (n, h, w, 3), dtype=np.uint8)


# ---- staggered pastes: every number of covering frames from 0 to nframes ---------------------------------------------------------
@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 63, 64, 65, 255])
def test_staggered_frames(ctx, n, gray):
    """12 x 9 frames pasted at (k % 4, (k // 4) % 3) + (2, 1) on a 23 x 17 canvas: the pixels under every frame, under some and
    under none.  dw is no multiple of 4 and the canvas takes more than one workgroup."""
    f = frames_of(40 + n, n, 12, 9, gray)
    mats = [W.translation(2 + k % 4, 1 + (k // 4) % 3) for k in range(n)]
    bg = frames_of(41, 1, 23, 17, gray)[0]
    want = None
    for pads in PADS:
        want = check(ctx, f, mats, 23, 17, (0, 0), bg, want=want, src_pad=pads[0], out_pad=pads[1], out_skip=pads[2])
    assert want[1].max() == n and want[1].min() == 0 and len(np.unique(want[1])) >= min(n, 4)
    check(ctx, f, mats, 23, 17, (-3, 2), None, min_cover=min(n, 2), threshold=0)


# ---- the order of the samples must not matter, ties and single bits must ---------------------------------------------------------
def constant_frames(values):
    """values [n] or [n,3] -> frames of 8 x 6 that hold one value (per channel) each"""
    v = np.asarray(values, np.uint8)
    return np.broadcast_to(v.reshape((len(v), 1, 1) + v.shape[1:]), (len(v), 6, 8) + v.shape[1:]).copy()


def orders(n):
    up = np.linspace(0, 255, n).astype(np.uint8)
    rng = np.random.default_rng(n)
    yield "ascending", up
    yield "descending", up[::-1]
    yield "alternating", np.where(np.arange(n) % 2 == 0, 0, 255)
    yield "alternating from 255", np.where(np.arange(n) % 2 == 0, 255, 0)
    yield "all 0", np.zeros(n)
    yield "all 255", np.full(n, 255)
    yield "bit 0 only", 100 + rng.integers(0, 2, n)
    yield "bit 7 only", 0x2A + 128 * rng.integers(0, 2, n)
    yield "bit 0 only, the odd value first", 100 + (np.arange(n) % 2 == 0)
    yield "one permutation per channel", np.stack([rng.permutation(up), rng.permutation(up), rng.permutation(up)], axis=1)
    yield "random", rng.integers(0, 256, (n, 3))


@pytest.mark.parametrize("n", [2, 5, 6, 64, 255])
def test_adversarial_sample_orders(ctx, n):
    eye = [np.eye(3)] * n
    for name, values in orders(n):
        f = constant_frames(values)
        plate, count, _ = check(ctx, f, eye, 8, 6, threshold=0)
        assert (count == n).all(), name
        expect = np.sort(np.asarray(values, np.int64), axis=0)[(n - 1) >> 1]          # the lower of the two middle values
        assert (plate == np.asarray(expect, np.uint8)).all(), name
    up = np.linspace(0, 255, n).astype(np.uint8)
    rng = np.random.default_rng(n + 1)
    values = np.stack([rng.permutation(up), rng.permutation(up), rng.permutation(up)], axis=1)
    if n >= 5:                                                                         # the three medians come from three frames
        mid = np.sort(up)[(n - 1) >> 1]
        assert len({int(np.flatnonzero(values[:, c] == mid)[0]) for c in range(3)}) > 1
    check(ctx, constant_frames(values), eye, 8, 6)
    check(ctx, frames_of(50 + n, n, 8, 6), eye, 8, 6, threshold=3)                     # and every pixel its own samples
    check(ctx, frames_of(51 + n, n, 8, 6, gray=True), eye, 8, 6, threshold=3)


# ---- projective matrices, fractional taps ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("inverse_map", [False, True])
@pytest.mark.parametrize("fill", [0, 255])
def test_projective(ctx, gray, inverse_map, fill):
    f = frames_of(60, 5, 37, 29, gray)
    mats = [rot_zoom_persp(17.0, 1.3, 3.5, -2.25, 1e-3, -2e-3), rot_zoom_persp(12, 1.2, 8, 3, 5e-4, -3e-4), W.translation(6.25, 2.75),
            rot_zoom_persp(-20, 0.9, 14, 10, 0, 1e-3), np.eye(3)]
    if inverse_map:
        mats = [rot_zoom_persp(-11.0, 0.8, 14.0, 9.5, -8e-4, 1.5e-3), rot_zoom_persp(6, 0.7, 11, 6, 0, 0), W.translation(16.25, 7.75),
                rot_zoom_persp(-4, 1.1, 20, 12, 2e-4, 0), W.translation(20, 10)]
    bg = np.full((48, 64) + f.shape[3:], fill, np.uint8)
    want = check(ctx, f, mats, 64, 48, (-20, -10), bg, inverse_map, min_cover=2, out_pad=1)
    count = want[1]
    assert count.max() >= 3 and (count == 0).sum() > 100 and (count == 1).sum() > 100       # the background shows through
    check(ctx, f, mats, 64, 48, (-20, -10), None, inverse_map, min_cover=1, threshold=40)


# ---- matrices that cover nothing, between frames that do -------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(NOTHING))
def test_nothing_covered_nothing_faulted(ctx, name):
    M, inverse_map = NOTHING[name]
    f = frames_of(61, 5, 37, 29)
    good = [W.translation(-18, -8), W.translation(3.5, 2.25), W.translation(-30, -20)]
    if inverse_map:
        good = [W.translation(18, 8), W.translation(-3.5, -2.25), W.translation(30, 20)]
    bg = frames_of(62, 1, 64, 48)[0]
    with np.errstate(all="ignore"):
        want = check(ctx, f, [good[0], M, good[1], M, good[2]], 64, 48, (-20, -10), bg, inverse_map, threshold=8)
        alone = P.plate(f[::2], good, 64, 48, (-20, -10), bg, inverse_map, 1, 8)
        only = check(ctx, f[:2], [M, M], 64, 48, (-20, -10), bg, inverse_map)
    assert np.array_equal(want[0], alone[0]) and np.array_equal(want[1], alone[1]) and np.array_equal(want[2][::2], alone[2])
    assert not want[2][1::2].any() and want[1].max() == 3
    assert np.array_equal(only[0], bg) and not only[1].any() and not only[2].any()


# ---- min_cover -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_cover", [1, 2, 7, 255])
def test_min_cover_lets_the_background_through(ctx, min_cover):
    n = 7
    f = frames_of(63, n, 12, 9)
    mats = [W.translation(2 + k % 4, 1 + (k // 4) % 3) for k in range(n)]
    bg = frames_of(64, 1, 23, 17)[0]
    plate, count, masks = check(ctx, f, mats, 23, 17, (0, 0), bg, min_cover=min_cover, threshold=0)
    assert count.max() == n
    below = count < min_cover
    assert below.any() and np.array_equal(plate[below], bg[below]) and not masks[:, below].any()
    assert below.all() == (min_cover == 255)                           # the count is reported whatever min_cover is
    check(ctx, f, mats, 23, 17, (0, 0), None, min_cover=min_cover)


# ---- outputs given or not ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [False, True])
@pytest.mark.parametrize("masks", [False, True])
def test_optional_outputs_and_thresholds(ctx, count, masks):
    f = frames_of(65, 6, 12, 9)
    mats = [W.translation(2 + k % 4, 1.5 * (k // 4)) for k in range(6)]
    bg = frames_of(66, 1, 23, 17)[0]
    for threshold in (0, 16, 255):
        want = check(ctx, f, mats, 23, 17, (0, 0), bg, threshold=threshold, count=count, masks=masks, out_pad=1)
        assert not want[2].any() if threshold == 255 else want[2].any()


# ---- what the plate is for -------------------------------------------------------------------------------------------------------------
def test_panning_scene_loses_its_moving_object(ctx):
    import torch

    def plate_of(f, m, dw, dh, **kw):
        return run(ctx, f, m, dw, dh, **kw)

    def mosaic_of(f, m, dw, dh):
        out = torch.full((dh, dw, 3), SENTINEL, dtype=torch.uint8, device="cuda")
        ctx.warp_fixed_plane(dev(f), dev(np.asarray(m, np.float64).reshape(len(f), 9)), out, "mosaic", (0, 0))
        ctx.synchronize()
        return out.cpu().numpy()
    P.check_panning_scene(plate_of, mosaic_of)


# ---- planes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(23, 17), (8, 6)])
def test_planes_equal_the_bgr_entry_on_the_converted_frames(ctx, w, h):
    import torch
    rng = np.random.default_rng(67)
    n, cw, ch = 4, (w + 1) // 2, (h + 1) // 2
    planes = [(rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8),
               rng.integers(0, 256, (ch, cw), dtype=np.uint8)) for _ in range(n)]
    bgr = W.planes_to_bgr(planes)
    mats = np.stack([np.eye(3), rot_zoom_persp(12, 1.2, 8, 3, 5e-4, -3e-4), W.translation(6.25, 2.75), W.translation(-2, 3)])
    dw, dh, origin = 44, 30, (-5, -4)
    bg = frames_of(68, 1, dw, dh)[0]
    want = P.plate(bgr, mats, dw, dh, origin, bg, False, 2, 10)
    d_m, d_bg = dev(mats.reshape(n, 9)), dev(bg)
    y, cb, cr = (dev(np.stack([p[i] for p in planes])) for i in range(3))
    uv = torch.stack([cb, cr], dim=-1).contiguous()
    packed = dev(np.stack([np.concatenate([a.reshape(-1) for a in p]) for p in planes]))
    conv = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    ctx.yuv420_to_bgr((y, cb, cr), conv)
    ctx.synchronize()
    assert np.array_equal(conv.cpu().numpy(), bgr)
    for name, src, size in (("bgr", conv, None), ("i420", (y, cb, cr), None), ("nv12", (y, uv[..., 0], uv[..., 1]), None),
                            ("packed", packed, (w, h))):
        plate = torch.full((dh, dw, 3), SENTINEL, dtype=torch.uint8, device="cuda")
        count = torch.full((dh, dw), SENTINEL, dtype=torch.uint8, device="cuda")
        masks = torch.full((n, dh, dw), SENTINEL, dtype=torch.uint8, device="cuda")
        ctx.plate_fixed_plane(src, d_m, plate, origin, background=d_bg, count=count, masks=masks, threshold=10, min_cover=2, size=size)
        ctx.synchronize()
        for got, w_ in zip((plate, count, masks), want):
            assert np.array_equal(got.cpu().numpy(), w_), name


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(ctx):
    import torch
    from evenvizion_amd._lib import Yuv420
    INVALID, CAPACITY = -1, -3
    n, sw, sh, dw, dh = 2, 23, 17, 31, 22
    A = Arena(8)            # every buffer a fixed distance from the others: which ranges meet is the test's to say
    src = A.put(frames_of(69, n, sw, sh))
    mats = A.put(np.tile(np.eye(3).reshape(1, 9), (n, 1)))
    plate = A.take((dh, dw, 3), fill=SENTINEL)
    count = A.take((dh, dw), fill=SENTINEL)
    masks = A.take((n, dh, dw), fill=SENTINEL)
    elsewhere = A.take((dh, dw, 3), fill=7)
    f, m, p, c, k, b = (t.data_ptr() for t in (src, mats, plate, count, masks, elsewhere))
    rs, fs, prs, mfs = sw * 3, sw * sh * 3, dw * 3, dw * dh
    good = dict(ctx=ctx.h, frames=f, n=n, sw=sw, sh=sh, cn=3, rs=rs, fs=fs, M=m, inv=0, mc=1, bg=b, plate=p, prs=prs, count=c,
                crs=dw, mask=k, thr=16, mrs=dw, mfs=mfs, dw=dw, dh=dh, ox=0, oy=0)
    tail = ("M", "inv", "mc", "bg", "plate", "prs", "count", "crs", "mask", "thr", "mrs", "mfs", "dw", "dh", "ox", "oy")

    def call(**kw):
        a = dict(good, **kw)
        return ctx.lib.evh_plate_fixed_plane(a["ctx"], a["frames"], a["n"], a["sw"], a["sh"], a["cn"], a["rs"], a["fs"],
                                             *[a[t] for t in tail])

    who, who_yuv = "evh_plate_fixed_plane: ", "evh_plate_fixed_plane_yuv420: "
    NS, NA, CH, EM = "NULL source", "NULL argument", "channels must be 1 or 3", "empty frame or canvas"
    MC, TH = "min_cover must lie in 1..255", "threshold must lie in 0..255"
    PLN, BIG = "at most EVH_PLATE_MAX_FRAMES = 255 frames per call", "source sizes stay below 2^26 (positions are held in 1/32 pixels)"
    AREA, SS = "dw * dh above INT_MAX", "source stride smaller than a row / frame"
    PS, CTS, MS = "plate stride smaller than a row", "count stride smaller than a row", "mask stride smaller than a row / picture"

    def over(a, b):
        return "%s overlaps %s" % (a, b)
    PL, CO, MA, BG, FR = "d_plate", "d_count", "d_mask", "d_background", "the frames"

    def refused(rc, code, text, what):
        assert rc == code, what
        assert ctx.lib.evh_last_error_string(ctx.h).decode() == text, what

    assert call(ctx=None) == INVALID
    invalid = [(dict(frames=None), NS), (dict(M=None), NA), (dict(plate=None), NA), (dict(cn=2), CH), (dict(cn=0), CH), (dict(cn=4), CH),
               (dict(sw=0), EM), (dict(sh=0), EM), (dict(dw=0), EM), (dict(dh=-1), EM), (dict(n=-1), EM), (dict(mc=0), MC),
               (dict(mc=256), MC), (dict(mc=-1), MC), (dict(thr=-1), TH), (dict(thr=256), TH), (dict(rs=rs - 1), SS), (dict(fs=fs - 1), SS),
               (dict(prs=prs - 1), PS), (dict(crs=dw - 1), CTS), (dict(mrs=dw - 1), MS), (dict(mfs=mfs - 1), MS),
               # an output over another output, the frames or the background
               (dict(count=p), over(PL, CO)), (dict(count=p + prs * dh - 1), over(PL, CO)), (dict(mask=p), over(PL, MA)),
               (dict(mask=c), over(CO, MA)), (dict(mask=c - mfs), over(CO, MA)), (dict(count=k + mfs), over(CO, MA)),
               (dict(plate=f), over(PL, FR)), (dict(plate=f + 2 * fs - 1), over(PL, FR)), (dict(count=f), over(CO, FR)),
               (dict(mask=f + fs), over(MA, FR)), (dict(bg=p), over(PL, BG)), (dict(bg=p + prs), over(PL, BG)),
               (dict(bg=p - prs), over(PL, BG)), (dict(bg=c), over(CO, BG)), (dict(bg=k + mfs), over(MA, BG)),
               # two faults: the earlier check of the entry names the refusal
               (dict(frames=None, plate=None), NS), (dict(M=None, cn=2), NA), (dict(n=256, mc=0), MC), (dict(prs=prs - 1, rs=rs - 1), PS),
               (dict(count=p, crs=dw - 1), CTS), (dict(count=p, mask=p), over(PL, CO)), (dict(mask=f, bg=c), over(CO, BG))]
    for kw, text in invalid:
        refused(call(**kw), INVALID, who + text, kw)
    big = 1 << 26
    capacity = [(dict(n=256), PLN), (dict(n=65536), PLN), (dict(sw=big, rs=big * 3, fs=big * 3 * sh), BIG), (dict(sh=big, fs=sw * 3 * big), BIG),
                (dict(dw=65536, dh=32768, prs=65536 * 3, crs=65536, mrs=65536, mfs=1 << 40), AREA),
                # two faults: a capacity refusal precedes the strides and the overlaps
                (dict(sw=big, rs=big * 3 - 1, fs=big * 3 * sh), BIG), (dict(n=256, sw=big), PLN), (dict(sh=big, count=p), BIG),
                (dict(n=256, prs=prs - 1), PLN)]
    for kw, text in capacity:
        refused(call(**kw), CAPACITY, who + text, kw)
    refused(call(n=255, fs=fs - 1), INVALID, who + SS, "at the limit")                                # there the ordinary checks apply
    refused(call(sw=big - 1, rs=(big - 1) * 3 - 1), INVALID, who + SS, "below the limit")
    # the plane form: its own description, then the same checks
    y = A.take((n, sh, sw))
    cc = A.take((2, n, 9, 12))
    yuv = dict(d_y=y.data_ptr(), d_cb=cc[0].data_ptr(), d_cr=cc[1].data_ptr(), y_stride=sw, c_stride=12, y_frame_stride=sw * sh,
               c_frame_stride=12 * 9, c_pixel_stride=1)

    def call_yuv(desc, **kw):
        a = dict(good, **kw)
        d = None if desc is None else ctypes.byref(Yuv420(**desc))
        return ctx.lib.evh_plate_fixed_plane_yuv420(a["ctx"], d, a["n"], a["sw"], a["sh"], *[a[t] for t in tail])

    refused(call_yuv(None), INVALID, who_yuv + NS, "no description")
    CPS, PLANE = "chroma pixel stride must be 1 or 2", "frame stride smaller than a plane"
    for bad, text in ((dict(d_y=None), NS), (dict(d_cb=None), NS), (dict(d_cr=None), NS), (dict(c_pixel_stride=3), CPS),
                      (dict(y_stride=sw - 1), "luma row stride smaller than the width"),
                      (dict(c_stride=11), "chroma row stride smaller than a chroma row"),
                      (dict(y_frame_stride=sw * sh - 1), PLANE), (dict(c_frame_stride=12 * 9 - 1), PLANE)):
        refused(call_yuv(dict(yuv, **bad)), INVALID, who_yuv + text, bad)
    for kw, text in ((dict(M=None), NA), (dict(plate=None), NA), (dict(dw=0), EM), (dict(mc=0), MC), (dict(thr=256), TH),
                     (dict(prs=prs - 1), PS), (dict(bg=p), over(PL, BG)), (dict(count=p), over(PL, CO)),
                     (dict(plate=y.data_ptr()), over(PL, FR)), (dict(mask=cc[1].data_ptr()), over(MA, FR)),
                     (dict(count=cc[0].data_ptr()), over(CO, FR))):                                    # the last: over the Cb plane
        refused(call_yuv(yuv, **kw), INVALID, who_yuv + text, kw)
    # two faults, one of them in the description: a NULL plane first, the strides before the planes, the planes before the overlaps
    refused(call_yuv(dict(yuv, d_cr=None), plate=None), INVALID, who_yuv + NS, "NULL plane before NULL argument")
    refused(call_yuv(dict(yuv, y_stride=sw - 1), prs=prs - 1), INVALID, who_yuv + PS, "strides before the description")
    refused(call_yuv(dict(yuv, c_pixel_stride=3), count=p), INVALID, who_yuv + CPS, "the description before the overlaps")
    refused(call_yuv(dict(yuv, c_pixel_stride=3), n=256), CAPACITY, who_yuv + PLN, "capacity before the description")
    for kw, text in ((dict(n=256), PLN), (dict(sw=big), BIG), (dict(dw=65536, dh=32768, prs=65536 * 3, crs=65536, mrs=65536, mfs=1 << 40), AREA)):
        refused(call_yuv(yuv, **kw), CAPACITY, who_yuv + text, kw)
    ctx.synchronize()
    assert (plate == SENTINEL).all() and (count == SENTINEL).all() and (masks == SENTINEL).all() and (elsewhere == 7).all()
    # no frames: every pixel takes the background, the count is 0, no mask is written
    assert call(n=0) == 0
    ctx.synchronize()
    assert (plate == 7).all() and (count == 0).all() and (masks == SENTINEL).all()
    plate.fill_(SENTINEL)
    assert call_yuv(yuv, n=0, bg=None, count=None) == 0
    ctx.synchronize()
    assert (plate == 0).all() and (masks == SENTINEL).all()
    # a threshold outside 0..255 is nobody's business without masks; and the same arguments unrefused do write
    assert call(thr=256, mask=None) == 0 and call_yuv(yuv, bg=None, count=None, mask=None) == 0 and call() == 0
    ctx.synchronize()
    lower = np.minimum(src[0].cpu().numpy(), src[1].cpu().numpy())       # two frames at the same place: the lower value of each byte
    assert np.array_equal(plate[:sh, :sw].cpu().numpy(), lower) and (plate[sh:] == 7).all() and (plate[:, sw:] == 7).all()
    assert (count[:sh, :sw] == 2).all() and (count[sh:] == 0).all() and (masks[:, sh:] == 0).all() and (masks[:, :sh, :sw] != 0).any()


# ---- the driver on the reference video ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recorded_plate():
    """background_plate over the recorded dictionary from BGR frames, and what plate_checks makes of the same frames."""
    import torch
    from evenvizion_amd import capture, runtime
    from evenvizion_amd import stabilization as S
    from evenvizion_amd.processing.utils import read_homography_dict, superposition_dict
    hd, ri = read_homography_dict(GOLD)
    sup = superposition_dict(hd)
    got = S.background_plate(capture.VideoCapture(MP4), sup, ri, placement="translate", max_frames=16, masks=True, ingest="bgr")
    w, h = ri["w"], ri["h"]
    nos = S.plate_frame_numbers(max(k for k in sup if k != "resize_info"), 16)
    cap = capture.VideoCapture(MP4)
    frames = []
    for k in range(1, nos[-1] + 1):
        ok, frame = cap.read()
        assert ok
        if k in nos:
            frames.append(frame)
    small = torch.zeros((len(nos), h, w, 3), dtype=torch.uint8, device="cuda")
    ctx = runtime.get_context(64, 64)
    ctx.resize_area(torch.from_numpy(np.stack(frames)).cuda(), small)
    ctx.synchronize()
    corner = S.get_reference_system(sup)
    dh, dw = S.panorama_shape(corner, (h, w))
    origin = (-abs(corner["min_x"]), -abs(corner["min_y"]))
    mats = [W.translation(*S.translate_offset(sup[k])) for k in nos]
    return sup, ri, nos, got, P.plate(small.cpu().numpy(), mats, dw, dh, origin, None, False, 1, 16), origin


def test_background_plate_on_the_reference_video(recorded_plate):
    sup, ri, nos, got, want, origin = recorded_plate
    assert got.frame_nos == nos and len(nos) == 16 and nos[0] == 1 and got.origin == origin
    assert got.plate.dtype == got.count.dtype == got.masks.dtype == np.uint8
    for g, w_, name in zip((got.plate, got.count, got.masks), want, ("plate", "count", "masks")):
        print("%s: differing bytes %d of %d" % (name, (g != w_).sum(), w_.size))
        assert g.shape == w_.shape and np.array_equal(g, w_), name
    assert got.count.max() >= 2 and got.plate.any() and got.masks.any()


def test_background_plate_from_planes_equals_the_bgr_one(recorded_plate):
    from evenvizion_amd import capture
    from evenvizion_amd import stabilization as S
    sup, ri, nos, got, _, _ = recorded_plate
    planes = S.background_plate(capture.VideoCapture(MP4), sup, ri, placement="translate", max_frames=16, masks=True, ingest="yuv420")
    assert planes.frame_nos == nos and planes.origin == got.origin
    assert np.array_equal(planes.plate, got.plate) and np.array_equal(planes.count, got.count) and np.array_equal(planes.masks, got.masks)


def test_stabilize_plate_writes_its_files(recorded_plate, tmp_path, monkeypatch):
    from evenvizion_amd import stabilization as S
    from evenvizion_amd import stabilize
    sup, ri, _, got, _, _ = recorded_plate
    monkeypatch.chdir(tmp_path)
    folder = stabilize.main(["--path_to_homography_dict", GOLD, "--path_to_video", MP4, "--experiment_name", "run", "--plate", "1",
                             "--plate_frames", "8", "--plate_min_cover", "2", "--plate_masks", "1", "--plate_threshold", "20"])
    nos = S.plate_frame_numbers(121, 8)
    assert len(nos) == 8 and folder.startswith(str(tmp_path))
    assert sorted(os.listdir(folder)) == sorted(["plate.ppm", "plate_count.png"] + ["mask_%06d.png" % k for k in nos])
    data = open(os.path.join(folder, "plate.ppm"), "rb").read()
    dh, dw = got.plate.shape[:2]
    head = b"P6\n%d %d\n255\n" % (dw, dh)
    assert data.startswith(head) and len(data) == len(head) + dw * dh * 3 and any(data[len(head):])
