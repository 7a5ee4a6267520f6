"""evh_pair_residual / evh_pair_residual_yuv420 and evenvizion_amd.registration on the device.  Every assertion is equality of
integers and bytes with the numpy restatement of the header's arithmetic (tests/residual_checks.py, itself checked against plain
differences in test_residual_host.py)."""
import ctypes
import json
import os

import numpy as np
import pytest

import residual_checks as R
import warp_checks as W
from refusal_arena import Arena

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MP4 = os.path.join(ROOT, "tests", "golden", "ref_test_video.mp4")
GOLD = os.path.join(ROOT, "tests", "golden", "ref_dict_with_homography_matrix.json")
SENTINEL = 0xCD
NAN = np.full((3, 3), np.nan)


@pytest.fixture(scope="module")
def ctx():
    from evenvizion_amd._lib import Context
    c = Context(device=0, max_w=64, max_h=64, max_features=500, max_frames=2)     # the entry does not depend on these sizes
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def frames_of(seed, n, w, h, gray=False):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w) if gray else (n, h, w, 3), dtype=np.uint8)


def rot_zoom_persp(deg, zoom, tx, ty, px, py):
    c, s = zoom * np.cos(np.deg2rad(deg)), zoom * np.sin(np.deg2rad(deg))
    return np.array([[c, -s, tx], [s, c, ty], [px, py, 1.0]], np.float64)


def strided(shape, layout, content=None):
    """A [n,h,w(,c)] uint8 view with byte strides layout = (row stride, frame stride, offset) into a buffer of SENTINEL; None =
    tight.  -> (buffer, view, the buffer positions of the view's bytes)"""
    import torch
    n, h, w = shape[:3]
    cn = shape[3] if len(shape) == 4 else 1
    rs, fs, off = layout or (w * cn, w * cn * h, 0)
    at = (off + np.arange(n, dtype=np.int64)[:, None, None] * fs + np.arange(h, dtype=np.int64)[None, :, None] * rs
          + np.arange(cn * w, dtype=np.int64)[None, None, :])
    buf = torch.full((int(at.max()) + 9 if at.size else 9,), SENTINEL, dtype=torch.uint8, device="cuda")
    view = buf.as_strided(tuple(shape), (fs, rs, cn, 1) if len(shape) == 4 else (fs, rs, 1), off)
    if content is not None:
        view.copy_(dev(content))
    return buf, view, at.reshape(-1)


def run(ctx, frames, mats, threshold=16, kind="abs", frame_step=1, src_layout=None, out_layout=None, picture=True):
    """Context.pair_residual -> (stats int64[npairs,6], picture u8[npairs,h,w] or None).  The stats tensor goes in filled with
    0xFF bytes; bytes of the picture buffer outside the rows must come back as SENTINEL."""
    import torch
    frames = np.asarray(frames)
    mats = np.asarray(mats, np.float64).reshape(-1, 9)
    npairs, (h, w) = len(mats), frames.shape[1:3]
    _, src, _ = strided(frames.shape, src_layout, frames)
    stats = torch.full((npairs, 6), -1, dtype=torch.int64, device="cuda")
    buf = out = at = None
    if picture:
        buf, out, at = strided((npairs, h, w), out_layout)
    d_mats = dev(mats)
    torch.cuda.synchronize()                                  # the fills above ran on torch's stream, the entry runs on the context's
    got = ctx.pair_residual(src, d_mats, stats=stats, out=out, threshold=threshold, kind=kind, frame_step=frame_step)
    ctx.synchronize()
    assert got is stats
    if not picture:
        return stats.cpu().numpy(), None
    whole = buf.cpu().numpy()
    gaps = np.ones(whole.shape, bool)
    gaps[at] = False
    assert (whole[gaps] == SENTINEL).all(), "bytes outside the picture rows were written"
    return stats.cpu().numpy(), out.cpu().numpy()


def check(ctx, frames, mats, threshold=16, frame_step=1, **kw):
    """Both kinds and the call without a picture against residual_checks -> (stats, abs picture)"""
    want, want_abs, want_mask = R.residual_pairs(frames, mats, threshold, frame_step)
    got, got_abs = run(ctx, frames, mats, threshold, "abs", frame_step, **kw)
    got_m, got_mask = run(ctx, frames, mats, threshold, "mask", frame_step, **kw)
    got_n, _ = run(ctx, frames, mats, threshold, "abs", frame_step, picture=False, **{k: v for k, v in kw.items() if k == "src_layout"})
    print("%s pairs %d threshold %d: stats differing %d, abs bytes %d, mask bytes %d" % (
        np.asarray(frames).shape, len(want), threshold, (got != want).sum(), (got_abs != want_abs).sum(), (got_mask != want_mask).sum()))
    assert np.array_equal(got, want) and np.array_equal(got_m, want) and np.array_equal(got_n, want)
    assert np.array_equal(got_abs, want_abs) and np.array_equal(got_mask, want_mask)
    return got, got_abs


# ---- matrices ----------------------------------------------------------------------------------------------------------------------
def matrices(w, h):
    return {
        "identity": np.eye(3),
        "shift": W.translation(2, -1),
        "shift_far": W.translation(-(w - 1), h - 1),                       # one pixel of overlap
        "fraction": W.translation(1.25, 0.5),
        "fraction_ties": W.translation(1 / 64, -1 / 64),                   # halves of 1/32: ties to even
        "projective": rot_zoom_persp(7.0, 1.05, 0.75, -0.5, 4e-4, -6e-4),
        "projective_wide": rot_zoom_persp(-15.0, 0.8, 0.2 * w, 0.1 * h, -1e-3, 2e-3),
        # tw = 0.1 x - 0.45 changes sign between x = 4 and x = 5: left of it ty / tw < 0, further right (x >= 7 at width 37) the
        # position comes back inside the frame
        "horizon": np.array([[1, 0, 0], [0, 0.5, 1], [0.1, 0, -0.45]], np.float64),
        # tw = 0.25 x - 1 is exactly 0 at x = 4
        "horizon_zero": np.array([[1, 0, 0], [0, 1, 0], [0.25, 0, -1]], np.float64),
        "one_point": np.outer([1.0, 2.0, 0.5], [3.0, -1.0, 2.0]),          # singular, every pixel -> (2, 4)
    }


NOTHING = {
    "nan": NAN,
    "one_nan": np.array([[1, 0, 0], [0, 1, 0], [0, 0, np.nan]]),
    "zero": np.zeros((3, 3)),
    "singular": np.array([[1, 2, 3], [2, 4, 6], [0, 0, 0]], np.float64),   # rank 1 with tw = 0 everywhere
    "inf": np.array([[np.inf, 0, 0], [0, 1, 0], [0, 0, 1]]),
    "overflow": np.array([[1e308, 1e308, 1e308], [0, 1, 0], [1e308, 1e308, -1e308]]),     # inf / inf, or a position far outside
    "away": W.translation(1e6, 0),
}


@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("size", [(9, 7), (13, 11), (37, 29)])
def test_matrices(ctx, size, gray):
    w, h = size
    ms = matrices(w, h)
    f = frames_of(71, len(ms) + 1, w, h, gray)
    stats, pics = check(ctx, f, list(ms.values()))
    by = dict(zip(ms, stats))
    assert by["identity"][R.COVERED] == w * h and by["identity"][R.SAD] == by["identity"][R.SAD0]
    assert by["identity"][R.SSD] == by["identity"][R.SSD0] > 0
    assert by["shift"][R.COVERED] == (w - 2) * (h - 1) and by["shift_far"][R.COVERED] == 1
    assert 0 < by["fraction"][R.COVERED] < w * h
    if size == (37, 29):
        assert 0 < by["projective"][R.COVERED] < w * h and 0 < by["projective_wide"][R.COVERED] < w * h
        hz = list(ms).index("horizon")
        assert 0 < by["horizon"][R.COVERED] < w * h and not pics[hz][:, :5].any() and pics[hz][:, 6:].any()
        assert by["one_point"][R.COVERED] > 0


@pytest.mark.parametrize("name", sorted(NOTHING))
def test_nothing_covered_six_zeros_and_a_black_picture(ctx, name):
    f = frames_of(72, 2, 37, 29)
    with np.errstate(all="ignore"):
        stats, pic = check(ctx, f, [NOTHING[name]])
    assert not stats.any() and not pic.any()
    _, mask = run(ctx, f, [NOTHING[name]], kind="mask", threshold=0)
    assert not mask.any()


# ---- geometry ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("frame_step", [1, 2])
@pytest.mark.parametrize("size", [(1, 1), (2, 1), (3, 1), (5, 1), (1, 5), (5, 3)])
def test_small_frames_channels_and_frame_step(ctx, size, frame_step, gray):
    w, h = size
    mats = [np.eye(3), W.translation(1, 0), W.translation(0.5, 0), W.translation(-0.25, 0.75)]
    f = frames_of(73, (len(mats) - 1) * frame_step + 2, w, h, gray)
    stats, _ = check(ctx, f, mats, frame_step=frame_step)
    assert stats[0][R.COVERED] == w * h and stats[1][R.COVERED] == (w - 1) * h


def test_frame_step_picks_other_frames(ctx):
    f = frames_of(74, 6, 13, 11)
    mats = [np.eye(3)] * 3
    one, _ = check(ctx, f[:4], mats, frame_step=1)
    two, _ = check(ctx, f, mats, frame_step=2)
    assert not np.array_equal(one[1], two[1]) and np.array_equal(one[0], two[0])


# ---- pairs do not leak into each other --------------------------------------------------------------------------------------------------
def test_good_nan_good(ctx):
    f = frames_of(75, 6, 37, 29)
    M = rot_zoom_persp(3.0, 1.02, 1.5, -0.75, 1e-4, 2e-4)
    stats, pics = check(ctx, f, [M, NAN, M, np.zeros((3, 3)), np.eye(3)])
    assert not stats[1].any() and not stats[3].any() and not pics[1].any() and not pics[3].any()
    for p in (0, 2, 4):                                                   # each pair alone gives the same
        alone, pic = check(ctx, f[p:p + 2], [[M, NAN, M, NAN, np.eye(3)][p]])
        assert np.array_equal(alone[0], stats[p]) and np.array_equal(pic[0], pics[p])


# ---- pointers: the bytes path against the words path -----------------------------------------------------------------------------------
@pytest.mark.parametrize("gray", [False, True])
def test_odd_pointers_and_strides(ctx, gray):
    """Rows of 23 pixels: 69 (BGR) or 23 (gray) bytes, so a tight layout already goes bytewise.  The first layout of each list has
    its base and both strides at multiples of 4 -- the words path, with the last run of a row cut by the edge -- and the others
    break one of the three, or are tight."""
    w, h, n = 23, 9, 4
    cn = 1 if gray else 3
    f = frames_of(76, n, w, h, gray)
    mats = [np.eye(3), rot_zoom_persp(5.0, 1.1, 1.0, 0.5, 2e-4, -3e-4), W.translation(3.5, -1.25)]
    rs, ors = w * cn + (-w * cn) % 4 + 4, w + (-w) % 4 + 4
    assert rs % 4 == 0 and ors % 4 == 0
    src_layouts = [(rs, rs * h + 8, 4), (rs + 1, (rs + 1) * h, 0), (rs, rs * h + 8, 1), (rs, rs * h + 2, 0), None]
    out_layouts = [(ors, ors * h + 4, 8), (ors + 1, (ors + 1) * h, 0), (ors, ors * h + 4, 3), (ors, ors * h + 1, 0), None]
    words, words_pic = check(ctx, f, mats, src_layout=src_layouts[0], out_layout=out_layouts[0])
    for sl in src_layouts:
        for ol in out_layouts:
            stats, pic = check(ctx, f, mats, src_layout=sl, out_layout=ol)
            assert np.array_equal(stats, words) and np.array_equal(pic, words_pic), (sl, ol)


# ---- kinds and thresholds -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threshold", [0, 16, 254, 255])
def test_thresholds(ctx, threshold):
    w, h = 37, 29
    f = frames_of(77, 2, w, h, gray=True)
    f[1, 0, :4] = (0, 255, 255, 0)                                            # differences of 255 and of 0 exist
    f[0, 0, :4] = (255, 0, 255, 0)
    stats, pic = check(ctx, f, [np.eye(3)], threshold=threshold)
    _, mask = run(ctx, f, [np.eye(3)], threshold=threshold, kind="mask")
    assert pic.max() == 255 and pic.min() == 0
    assert stats[0][R.MOVING] == (pic > threshold).sum() == (mask == 255).sum()
    assert set(np.unique(mask)) <= {0, 255}
    if threshold == 255:
        assert stats[0][R.MOVING] == 0 and not mask.any()
    else:
        assert stats[0][R.MOVING] > 0
    if threshold == 0:
        assert stats[0][R.MOVING] == (pic != 0).sum() < w * h


# ---- the stats buffer --------------------------------------------------------------------------------------------------------------------
def test_stats_are_overwritten_and_repeatable(ctx):
    import torch
    f = dev(frames_of(78, 3, 37, 29))
    mats = dev(np.stack([rot_zoom_persp(4.0, 0.97, -1.0, 2.0, 0, 1e-4), NAN]).reshape(2, 9))
    stats = torch.full((2, 6), -1, dtype=torch.int64, device="cuda")            # 0xFF in every byte
    torch.cuda.synchronize()
    ctx.pair_residual(f, mats, stats=stats)
    ctx.synchronize()
    first = stats.cpu().numpy().copy()
    assert (first[0] > 0).all() and not first[1].any()                          # the uncovered pair's row was zeroed too
    ctx.pair_residual(f, mats, stats=stats)                                      # onto its own result: not accumulated
    ctx.synchronize()
    assert np.array_equal(stats.cpu().numpy(), first)
    fresh = ctx.pair_residual(f, mats)
    ctx.synchronize()
    assert fresh.dtype == torch.int64 and tuple(fresh.shape) == (2, 6) and np.array_equal(fresh.cpu().numpy(), first)


# ---- extreme values ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gray", [False, True])
def test_white_against_black(ctx, gray):
    w = h = 64
    f = np.zeros((2, h, w) if gray else (2, h, w, 3), np.uint8)
    f[1] = 255
    stats, pic = check(ctx, f, [np.eye(3)])
    assert stats[0].tolist() == [w * h, w * h * 255, w * h * 65025, w * h * 255, w * h * 65025, w * h] and (pic == 255).all()


def test_sums_beyond_32_bits_in_one_launch(ctx):
    """One 2048 x 2048 pair, white against black: SSD = 4 194 304 * 65025 = 272 734 617 600 > 2^32, summed from 4096 workgroups."""
    import torch
    side = 2048
    f = torch.zeros((2, side, side, 3), dtype=torch.uint8, device="cuda")
    f[1] = 255
    mats = dev(np.eye(3).reshape(1, 9))
    out = torch.zeros((1, side, side), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for kw in (dict(out=out), dict()):
        stats = ctx.pair_residual(f, mats, threshold=254, **kw)
        ctx.synchronize()
        n = side * side
        assert n * 65025 > 2 ** 32
        assert stats.cpu().numpy()[0].tolist() == [n, n * 255, n * 65025, n * 255, n * 65025, n]
    assert int((out == 255).sum()) == side * side
    # half a pixel to the right: the last column is not covered, every other pixel samples black between two black taps
    stats = ctx.pair_residual(f, dev(W.translation(0.5, 0).reshape(1, 9)))
    ctx.synchronize()
    n = (side - 1) * side
    assert stats.cpu().numpy()[0].tolist() == [n, n * 255, n * 65025, n * 255, n * 65025, n]


# ---- planes --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(23, 17), (8, 6)])
def test_planes_equal_the_bgr_entry_on_the_converted_frames(ctx, size):
    import torch
    rng = np.random.default_rng(79)
    w, h = size
    n, cw, ch = 4, (w + 1) // 2, (h + 1) // 2
    planes = [(rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8),
               rng.integers(0, 256, (ch, cw), dtype=np.uint8)) for _ in range(n)]
    bgr = W.planes_to_bgr(planes)
    mats = np.stack([np.eye(3), rot_zoom_persp(6.0, 1.1, 1.5, -0.5, 3e-4, -2e-4), W.translation(2.25, 1.75)])
    d_m = dev(mats.reshape(3, 9))
    y, cb, cr = (dev(np.stack([p[i] for p in planes])) for i in range(3))
    uv = torch.stack([cb, cr], dim=-1).contiguous()
    packed = dev(np.stack([np.concatenate([a.reshape(-1) for a in p]) for p in planes]))
    conv = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.yuv420_to_bgr((y, cb, cr), conv)
    ctx.synchronize()
    assert np.array_equal(conv.cpu().numpy(), bgr)
    for kind in ("abs", "mask"):
        want, want_abs, want_mask = R.residual_pairs(bgr, mats, 16)
        want_pic = want_abs if kind == "abs" else want_mask
        via = torch.zeros((3, h, w), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        via_stats = ctx.pair_residual(conv, d_m, out=via, kind=kind)
        ctx.synchronize()
        assert np.array_equal(via_stats.cpu().numpy(), want) and np.array_equal(via.cpu().numpy(), want_pic)
        for name, src, sz in (("i420", (y, cb, cr), None), ("nv12", (y, uv[..., 0], uv[..., 1]), None), ("packed", packed, (w, h))):
            out = torch.full((3, h, w), SENTINEL, dtype=torch.uint8, device="cuda")
            stats = torch.full((3, 6), -1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            ctx.pair_residual_yuv420(src, d_m, stats=stats, out=out, kind=kind, size=sz)
            ctx.synchronize()
            assert np.array_equal(stats.cpu().numpy(), want), (kind, name)
            assert np.array_equal(out.cpu().numpy(), want_pic), (kind, name)
            bare = ctx.pair_residual_yuv420(src, d_m, size=sz)
            ctx.synchronize()
            assert np.array_equal(bare.cpu().numpy(), want), (kind, name)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(ctx):
    import torch
    from evenvizion_amd._lib import Yuv420
    INVALID, CAPACITY = -1, -3
    n, w, h = 3, 23, 17
    A = Arena(6)            # every buffer a fixed distance from the others: which ranges meet is the test's to say
    src = A.put(frames_of(80, n + 1, w, h))
    mats = A.put(np.tile(np.eye(3).reshape(1, 9), (n, 1)))
    stats = A.take((n + 1, 6), torch.int64, -1)
    out = A.take((n + 1, h, w), fill=SENTINEL)
    f, m, s, o = src.data_ptr(), mats.data_ptr(), stats.data_ptr(), out.data_ptr()
    rs, fs, ors, ofs = w * 3, w * h * 3, w, w * h
    good = dict(ctx=ctx.h, frames=f, n=n, step=1, w=w, h=h, cn=3, rs=rs, fs=fs, M=m, thr=16, stats=s, out=o, kind=0, ors=ors, ofs=ofs)

    def call(**kw):
        a = dict(good, **kw)
        return ctx.lib.evh_pair_residual(a["ctx"], a["frames"], a["n"], a["step"], a["w"], a["h"], a["cn"], a["rs"], a["fs"], a["M"],
                                         a["thr"], a["stats"], a["out"], a["kind"], a["ors"], a["ofs"])

    who, who_yuv = "evh_pair_residual: ", "evh_pair_residual_yuv420: "
    NS, NA, CH, STEP = "NULL source", "NULL argument", "channels must be 1 or 3", "frame_step must be 1 or 2"
    EM, TH, KIND = "empty frame or negative npairs", "threshold must lie in 0..255", "unknown kind"
    BIG, AREA = "frame sizes stay below 2^26 (positions are held in 1/32 pixels)", "w * h above INT_MAX"
    NP, NF = "at most 65535 pairs per call", "at most 65535 frames per call"
    SS, OS = "source stride smaller than a row / frame", "output stride smaller than a row / picture"
    OST, OFR = "d_out overlaps d_stats", "d_out overlaps the frames"

    def refused(rc, code, text, what):
        assert rc == code, what
        assert ctx.lib.evh_last_error_string(ctx.h).decode() == text, what

    assert call(ctx=None) == INVALID
    invalid = [(dict(frames=None), NS), (dict(M=None), NA), (dict(stats=None), NA), (dict(cn=2), CH), (dict(cn=0), CH), (dict(cn=4), CH),
               (dict(step=0), STEP), (dict(step=3), STEP), (dict(w=0), EM), (dict(h=0), EM), (dict(h=-1), EM), (dict(n=-1), EM),
               (dict(thr=-1), TH), (dict(thr=256), TH), (dict(kind=2), KIND), (dict(kind=-1), KIND), (dict(rs=rs - 1), SS),
               (dict(fs=fs - 1), SS), (dict(n=1, fs=fs - 1), SS), (dict(ors=ors - 1), OS), (dict(ofs=ofs - 1), OS),
               (dict(out=f), OFR), (dict(out=f + (n + 1) * fs - 1), OFR), (dict(out=f - n * ofs + 1), OFR), (dict(frames=o + 5), OFR),
               (dict(out=s), OST), (dict(out=s + n * 48 - 1), OST), (dict(stats=o + n * ofs - 8), OST), (dict(stats=o), OST),
               # two faults: the earlier check of the entry names the refusal
               (dict(frames=None, stats=None), NS), (dict(M=None, cn=2), NA), (dict(step=0, n=-1), STEP), (dict(rs=rs - 1, ors=ors - 1), SS),
               (dict(out=s, ors=ors - 1), OS), (dict(out=f, stats=f), OST)]
    for kw, text in invalid:
        refused(call(**kw), INVALID, who + text, kw)
    big = 1 << 26
    capacity = [(dict(w=big, rs=big * 3, fs=big * 3 * h), BIG), (dict(h=big, fs=rs * big), BIG),
                (dict(w=65536, h=32768, rs=65536 * 3, fs=1 << 40, ors=65536, ofs=1 << 40), AREA), (dict(n=65536), NP),
                # two faults: a capacity refusal precedes the strides and the overlaps
                (dict(w=big, rs=big * 3 - 1, fs=big * 3 * h), BIG), (dict(n=65536, fs=fs - 1), NP), (dict(h=big, out=s), BIG),
                (dict(w=big, n=65536), BIG)]
    for kw, text in capacity:
        refused(call(**kw), CAPACITY, who + text, kw)
    refused(call(w=big - 1, rs=(big - 1) * 3 - 1), INVALID, who + SS, "below the limit")      # there the ordinary checks apply
    # the plane form: its own description, then the same checks
    cw, ch = 12, 9
    y = A.take((n + 1, h, w))
    c = A.take((2, n + 1, ch, cw))
    torch.cuda.synchronize()
    yuv = dict(d_y=y.data_ptr(), d_cb=c[0].data_ptr(), d_cr=c[1].data_ptr(), y_stride=w, c_stride=cw, y_frame_stride=w * h,
               c_frame_stride=cw * ch, c_pixel_stride=1)

    def call_yuv(desc, **kw):
        a = dict(good, **kw)
        d = None if desc is None else ctypes.byref(Yuv420(**desc))
        return ctx.lib.evh_pair_residual_yuv420(a["ctx"], d, a["n"], a["step"], a["w"], a["h"], a["M"], a["thr"], a["stats"], a["out"],
                                                a["kind"], a["ors"], a["ofs"])

    refused(call_yuv(None), INVALID, who_yuv + NS, "no description")
    CPS, PLANE = "chroma pixel stride must be 1 or 2", "frame stride smaller than a plane"
    for bad, text in ((dict(d_y=None), NS), (dict(d_cb=None), NS), (dict(d_cr=None), NS), (dict(c_pixel_stride=3), CPS),
                      (dict(y_stride=w - 1), "luma row stride smaller than the width"),
                      (dict(c_stride=cw - 1), "chroma row stride smaller than a chroma row"),
                      (dict(y_frame_stride=w * h - 1), PLANE), (dict(c_frame_stride=cw * ch - 1), PLANE)):
        refused(call_yuv(dict(yuv, **bad)), INVALID, who_yuv + text, bad)
    for kw, text in ((dict(M=None), NA), (dict(stats=None), NA), (dict(w=0), EM), (dict(step=3), STEP), (dict(thr=256), TH), (dict(kind=5), KIND),
                     (dict(ors=ors - 1), OS), (dict(out=y.data_ptr() + 7), OFR), (dict(out=c[1].data_ptr()), OFR), (dict(out=s), OST),
                     (dict(out=c[0].data_ptr()), OFR)):                                                # the last: over the Cb plane
        refused(call_yuv(yuv, **kw), INVALID, who_yuv + text, kw)
    # two faults, one of them in the description: a NULL plane first, the strides before the planes, the planes before the overlaps
    refused(call_yuv(dict(yuv, d_y=None), stats=None), INVALID, who_yuv + NS, "NULL plane before NULL argument")
    refused(call_yuv(dict(yuv, y_stride=w - 1), ors=ors - 1), INVALID, who_yuv + OS, "strides before the description")
    refused(call_yuv(dict(yuv, c_pixel_stride=3), out=s), INVALID, who_yuv + CPS, "the description before the overlaps")
    refused(call_yuv(dict(yuv, c_pixel_stride=3), n=65535, step=2), CAPACITY, who_yuv + NF, "the frames' capacity before the description")
    for kw, text in ((dict(w=big), BIG), (dict(n=65536), NP), (dict(w=65536, h=32768, ors=65536, ofs=1 << 40), AREA), (dict(n=65535), NF)):
        refused(call_yuv(yuv, **kw), CAPACITY, who_yuv + text, kw)
    # no pairs: success, and nothing is done, not even the zeroing
    assert call(n=0) == 0 and call_yuv(yuv, n=0) == 0
    ctx.synchronize()
    assert (out == SENTINEL).all() and (stats == -1).all()
    # and the same arguments unrefused do write; without a picture its strides and place do not count
    assert call() == 0 and call(out=None, ors=0, ofs=0, stats=s + 48 * n, n=1) == 0
    ctx.synchronize()
    got = stats.cpu().numpy()
    want = R.residual_pairs(src.cpu().numpy(), np.tile(np.eye(3).reshape(1, 9), (n, 1)))
    assert np.array_equal(got[:n], want[0]) and np.array_equal(got[n], want[0][0])
    assert np.array_equal(out[:n].cpu().numpy(), want[1]) and (out[n] == SENTINEL).all()
    assert call_yuv(yuv) == 0
    ctx.synchronize()
    assert stats[:n, 0].tolist() == [w * h] * n and not stats[:n, 1:].any() and not out[:n].any()      # black planes: no difference


def test_python_layer_refuses_what_does_not_fit(ctx):
    import torch
    f = dev(frames_of(81, 3, 9, 7))
    m = dev(np.tile(np.eye(3).reshape(1, 9), (2, 1)))
    for kw in (dict(frames=f[:2]), dict(mats=m.float()), dict(mats=m.cpu()), dict(stats=torch.zeros((2, 6), dtype=torch.int32, device="cuda")),
               dict(stats=torch.zeros((3, 6), dtype=torch.int64, device="cuda")), dict(out=torch.zeros((2, 7, 8), dtype=torch.uint8, device="cuda")),
               dict(out=torch.zeros((1, 7, 9), dtype=torch.uint8, device="cuda")), dict(frame_step=3), dict(frame_step=2)):
        a = dict(dict(frames=f, mats=m), **kw)
        with pytest.raises(ValueError):
            ctx.pair_residual(a.pop("frames"), a.pop("mats"), **a)
    with pytest.raises(KeyError):
        ctx.pair_residual(f, m, kind="sum")
    from evenvizion_amd._lib import EvhError
    with pytest.raises(EvhError):
        ctx.pair_residual(f, m, threshold=256)
    none = ctx.pair_residual(f, m[:0])
    assert tuple(none.shape) == (0, 6)


# ---- the reference video --------------------------------------------------------------------------------------------------------------------
class Recording:
    """A capture read as BGR frames that keeps a copy of the frames whose numbers it is given."""

    def __init__(self, cap, numbers):
        self.cap, self.numbers, self.count, self.kept = cap, set(numbers), 0, {}

    def read(self):
        ok, frame = self.cap.read()
        if ok:
            self.count += 1
            if self.count in self.numbers:
                self.kept[self.count] = np.array(frame)
        return ok, frame


@pytest.fixture(scope="module")
def video(ctx):
    """The recorded superposition of the reference video, registration_report over the whole video from BGR frames in chunks of 32
    (one decoding pass, which also keeps frames 1, 2, 99, 100, 120 and 121), and those frames resized on the device."""
    import torch
    from evenvizion_amd import capture, registration
    from evenvizion_amd.processing.utils import read_homography_dict, superposition_dict
    hd, ri = read_homography_dict(GOLD)
    sup = superposition_dict(hd)
    rec = Recording(capture.VideoCapture(MP4), (1, 2, 99, 100, 120, 121))
    report = registration.registration_report(rec, sup, ri, chunk_frames=32, ingest="bgr")
    nos = sorted(rec.kept)
    assert nos == [1, 2, 99, 100, 120, 121]
    small = torch.zeros((len(nos), ri["h"], ri["w"], 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.resize_area(torch.from_numpy(np.stack([rec.kept[k] for k in nos])).cuda(), small)
    ctx.synchronize()
    small = small.cpu().numpy()
    return hd, sup, ri, {no: small[i] for i, no in enumerate(nos)}, report


def test_report_over_the_reference_video(video):
    """Pairs 2, 100 and 121 are residual_checks' on the device-resized frames; registered SSD below unregistered on at least 114 of
    120 pairs (the issue's bound; measured on subsampled frames on the host: 120 of 120)."""
    from evenvizion_amd import registration
    hd, sup, ri, small, report = video
    maps = registration.pair_maps(sup)
    assert list(report["frames"]) == list(range(2, 122)) == list(maps)
    assert (ri["w"], ri["h"]) == (400, 224)
    for no in (2, 100, 121):
        want = R.residual(small[no - 1], small[no], maps[no], 16)[0]
        e = report["frames"][no]
        got = tuple(e[k] for k in registration.STAT_NAMES)
        print("pair %d: device %s restatement %s" % (no, got, want))
        assert got == want, no
        assert e["psnr"] == registration.psnr(want[0], want[2]) and e["psnr_unregistered"] == registration.psnr(want[0], want[4])
    better = sum(e["ssd"] < e["ssd_unregistered"] for e in report["frames"].values())
    ratios = {no: e["ssd"] / e["ssd_unregistered"] for no, e in report["frames"].items()}
    worst = max(ratios, key=ratios.get)
    print("registered below unregistered on %d of 120 pairs; worst ratio %.3f at frame %d; itf %.2f dB against %.2f dB; least gain %s"
          % (better, ratios[worst], worst, report["itf"], report["itf_unregistered"], report["worst"][:3]))
    assert better >= 114
    assert sorted(report["worst"]) == list(range(2, 122))
    gains = [report["frames"][no]["psnr"] - report["frames"][no]["psnr_unregistered"] for no in report["worst"]]
    assert gains == sorted(gains)
    finite = [e["psnr"] for e in report["frames"].values()]
    assert abs(report["itf"] - float(np.mean(finite))) < 1e-12


def test_chunks_and_planes_give_the_same_report(video):
    from evenvizion_amd import capture, registration
    _, sup, ri, _, report = video
    fives = registration.registration_report(capture.VideoCapture(MP4), sup, ri, chunk_frames=5, ingest="bgr")
    assert fives == report
    planes = registration.registration_report(capture.VideoCapture(MP4), sup, ri, ingest="auto")            # 4:2:0 planes, chunks of 32
    assert planes == report


def test_residual_frames_and_short_captures(ctx, video):
    from evenvizion_amd import capture, registration
    _, sup, ri, small, report = video

    class Three:
        def __init__(self):
            self.cap, self.left = capture.VideoCapture(MP4), 3
            self.width, self.height, self.bgr_mode = self.cap.width, self.cap.height, self.cap.bgr_mode

        def read(self):
            self.left -= 1
            return self.cap.read() if self.left >= 0 else (False, None)

    maps = registration.pair_maps(sup)
    want = R.residual(small[1], small[2], maps[2], 16)
    for kind, pic in (("abs", want[1]), ("mask", want[2])):
        got = list(registration.residual_frames(Three(), sup, ri, ingest="bgr", kind=kind, chunk_frames=2))
        assert [k for k, _ in got] == [2, 3]
        assert got[0][1].shape == (224, 400) and got[0][1].dtype == np.uint8 and np.array_equal(got[0][1], pic)
    short = registration.registration_report(Three(), sup, ri, ingest="bgr")
    assert list(short["frames"]) == [2, 3] and short["frames"][2] == report["frames"][2]
    assert list(registration.residual_frames(capture.VideoCapture(MP4), {1: np.eye(3)}, ri)) == []
    # an entry without a matrix scores nothing on both pairs it takes part in
    odd = {1: sup[1], 2: None, 3: sup[3], 4: sup[4]}
    rep = registration.registration_report(capture.VideoCapture(MP4), odd, ri, ingest="bgr")
    assert rep["frames"][2]["covered"] == 0 == rep["frames"][3]["covered"] and rep["frames"][2]["psnr"] is None
    assert rep["frames"][4]["covered"] > 0 and rep["worst"][:2] == [2, 3]


# ---- python -m evenvizion_amd.component --registration_report / --residual_pictures ------------------------------------------------------
def test_component_writes_report_and_pictures_only_on_request(tmp_path, monkeypatch):
    from evenvizion_amd import component, registration
    from evenvizion_amd.processing.utils import read_homography_dict, superposition_dict
    monkeypatch.chdir(tmp_path)
    spec = "synthetic:4:400x224:3"
    base = ["--path_to_video", spec, "--features", "ORB"]
    plain = component.main(base + ["--experiment_name", "plain"])
    assert sorted(os.listdir(plain)) == ["dict_with_homography_matrix.json", "metrics_file.txt"]
    folder = component.main(base + ["--experiment_name", "scored", "--registration_report", "1", "--residual_pictures", "1"])
    assert sorted(os.listdir(folder)) == ["dict_with_homography_matrix.json", "metrics_file.txt", "registration_report.json",
                                          "registration_visualization"]
    hd, ri = read_homography_dict(os.path.join(folder, "dict_with_homography_matrix.json"))
    sup = superposition_dict(hd)
    want = registration.registration_report(component.open_capture(spec)[0], sup, ri)
    with open(os.path.join(folder, "registration_report.json")) as f:
        got = json.load(f)
    assert list(got["frames"]) == [str(k) for k in want["frames"]] == ["2", "3", "4"]
    for k, e in want["frames"].items():
        assert got["frames"][str(k)] == e
    assert got["itf"] == want["itf"] and got["itf_unregistered"] == want["itf_unregistered"] and got["worst"] == want["worst"]
    names = sorted(os.listdir(os.path.join(folder, "registration_visualization")))
    assert names == ["res%06d.ppm" % k for k in want["frames"]]
    pics = dict(registration.residual_frames(component.open_capture(spec)[0], sup, ri))
    for k in want["frames"]:
        with open(os.path.join(folder, "registration_visualization", "res%06d.ppm" % k), "rb") as f:
            data = f.read()
        head = b"P6\n%d %d\n255\n" % (ri["w"], ri["h"])
        assert data.startswith(head) and len(data) == len(head) + 3 * ri["w"] * ri["h"]
        rgb = np.frombuffer(data[len(head):], np.uint8).reshape(ri["h"], ri["w"], 3)
        assert np.array_equal(rgb, np.repeat(pics[k][:, :, None], 3, axis=2))
