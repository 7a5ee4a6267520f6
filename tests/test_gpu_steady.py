"""evh_steady_frames / evh_steady_frames_yuv420 on the device.  Every assertion is equality of bytes, tap_of and counts with
the numpy restatement of the header's arithmetic (tests/steady_checks.py, itself checked against plain statements in
test_steady_host.py)."""
import ctypes

import numpy as np
import pytest

import steady_checks as S
import warp_checks as W

pytestmark = pytest.mark.gpu
SENTINEL = 0xCD
SIZES = [(13, 9), (37, 21)]


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


def maps_of(seed, nout, ntaps, sw, sh):
    """Seeded maps output pixel -> frame pixel: rotations, zooms, shifts of up to a third of the frame, some perspective."""
    rng = np.random.default_rng(seed)
    out = np.empty((nout, ntaps, 3, 3))
    for j in range(nout):
        for t in range(ntaps):
            out[j, t] = rot_zoom_persp(rng.uniform(-12, 12), rng.uniform(0.7, 1.3), rng.uniform(-sw / 3, sw / 3),
                                       rng.uniform(-sh / 3, sh / 3), rng.uniform(-2e-3, 2e-3), rng.uniform(-2e-3, 2e-3))
    return out.reshape(nout, ntaps, 9)


def run(ctx, frames, tap_frame, tap_M, dw, dh, feather=0, background=None, src_pad=0, out_pad=0, out_skip=0, tap_of=True,
        counts=True, launches=1):
    """frames u8[n,sh,sw(,c)] through Context.steady_frames -> (pictures, tap_of or None, counts or None) as numpy.  src_pad /
    out_pad: extra pixels per source / output row (views of wider tensors; the padding holds SENTINEL and must survive);
    out_skip: the output views start that many pixels into their rows (an unaligned base)."""
    import torch
    frames = np.asarray(frames)
    n, sh, sw = frames.shape[:3]
    tail = frames.shape[3:]
    tap_frame = np.asarray(tap_frame, np.int32)
    nout, ntaps = tap_frame.shape
    src = torch.full((n, sh + 1, sw + src_pad) + tail, SENTINEL, dtype=torch.uint8, device="cuda")
    src[:, :sh, :sw] = dev(frames)
    inside = (slice(None), slice(0, dh), slice(out_skip, out_skip + dw))
    full = torch.full((nout, dh + 1, out_skip + dw + out_pad) + tail, SENTINEL, dtype=torch.uint8, device="cuda")
    of_full = torch.full((nout, dh + 1, out_skip + dw + out_pad), SENTINEL, dtype=torch.uint8, device="cuda") if tap_of else None
    d_counts = torch.full((nout, ntaps + 1), 0x5A5A5A5A, dtype=torch.int32, device="cuda") if counts else None
    bg = None
    if background is not None:
        bgfull = torch.full((dh + 1, out_skip + dw + out_pad) + tail, SENTINEL, dtype=torch.uint8, device="cuda")
        bg = bgfull[:dh, out_skip:out_skip + dw]
        bg.copy_(dev(np.asarray(background, np.uint8).reshape((dh, dw) + tail)))
    for _ in range(launches):
        ctx.steady_frames(src[:, :sh, :sw], dev(tap_frame), dev(np.asarray(tap_M, np.float64).reshape(nout, ntaps, 9)), full[inside],
                          feather=feather, background=bg, tap_of=of_full[inside] if tap_of else None, counts=d_counts)
    ctx.synchronize()
    assert np.array_equal(src[:, :sh, :sw].cpu().numpy(), frames)
    outs = []
    for t in (full, of_full):
        if t is None:
            outs.append(None)
            continue
        got = t.cpu().numpy()
        gaps = np.ones(got.shape, bool)
        gaps[inside] = False
        assert (got[gaps] == SENTINEL).all(), "bytes outside the picture rows were written"
        outs.append(got[inside])
    return outs[0], outs[1], None if d_counts is None else d_counts.cpu().numpy().astype(np.int64)


def check(ctx, frames, tap_frame, tap_M, dw, dh, feather=0, background=None, **kw):
    want = S.steady_frames(frames, tap_frame, tap_M, dw, dh, feather, background)
    got = run(ctx, frames, tap_frame, tap_M, dw, dh, feather, background, **kw)
    print("%dx%d taps %s feather %d: differing bytes %d of %d" % (dw, dh, np.asarray(tap_frame).shape, feather,
                                                                   (got[0] != want[0]).sum(), want[0].size))
    assert np.array_equal(got[0], want[0])
    if got[1] is not None:
        assert np.array_equal(got[1], want[1])
    if got[2] is not None:
        assert np.array_equal(got[2], want[2])
        assert (got[2].sum(axis=1) == dw * dh).all()
    return want


# ---- one tap per picture is EVH_WARP_EACH --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("size", SIZES)
def test_one_tap_equals_warp_each_with_inverse_map(ctx, gray, size):
    import torch
    sw, sh = size
    n = 3
    f = frames_of(41, n, sw, sh, gray)
    d_f = dev(f)
    for dw in (1, 3, 4, 5, 37):
        for dh in (1, 9):
            mats = maps_of(42 + dw + dh, n, 1, sw, sh)
            mats[0, 0] = np.eye(3).reshape(9)
            bg = frames_of(43, 1, dw, dh, gray)[0]
            shape = (n, dh, dw) + f.shape[3:]
            a = torch.full(shape, SENTINEL, dtype=torch.uint8, device="cuda")
            b = torch.full(shape, SENTINEL, dtype=torch.uint8, device="cuda")
            d_m, d_bg = dev(mats), dev(bg)
            ctx.warp_fixed_plane(d_f, d_m.reshape(n, 9), a, "each", (0, 0), background=d_bg, inverse_map=True)
            ctx.steady_frames(d_f, dev(np.arange(n, dtype=np.int32).reshape(n, 1)), d_m, b, feather=0, background=d_bg)
            ctx.synchronize()
            assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()), (dw, dh)
            want = check(ctx, f, np.arange(n).reshape(n, 1), mats, dw, dh, 0, bg)
            assert np.array_equal(b.cpu().numpy(), want[0])
            if dw <= sw and dh <= sh:
                assert np.array_equal(want[0][0], f[0][:dh, :dw])      # the identity tap copies the frame


# ---- seeded rotations, zooms and perspective maps over every tap count and feather ----------------------------------------------------
@pytest.mark.parametrize("ntaps", [1, 2, 5, 16])
@pytest.mark.parametrize("feather", [0, 1, 33, 256, 8160])
def test_seeded_maps(ctx, ntaps, feather):
    seen_mix = False
    for case, (gray, (sw, sh), dw, dh, nout, nframes, with_bg, pads) in enumerate([
            (False, SIZES[1], 37, 9, 3, 6, True, (0, 0, 0)), (True, SIZES[1], 37, 9, 3, 4, False, (3, 1, 0)),
            (False, SIZES[0], 5, 9, 1, 1, True, (1, 2, 0)), (True, SIZES[0], 4, 1, 3, 2, True, (0, 0, 0)),
            (False, SIZES[0], 3, 9, 1, 3, False, (0, 1, 1)), (True, SIZES[1], 1, 1, 1, 5, True, (0, 0, 0)),
            (True, SIZES[1], 37, 9, 1, 6, True, (0, 3, 1)), (False, SIZES[1], 37, 9, 3, 6, False, (0, 1, 1))]):
        seed = 1000 * ntaps + 10 * feather + case
        f = frames_of(seed, nframes, sw, sh, gray)
        tap_frame = np.random.default_rng(seed + 1).integers(0, nframes, (nout, ntaps))
        mats = maps_of(seed + 2, nout, ntaps, sw, sh)
        bg = frames_of(seed + 3, 1, dw, dh, gray)[0] if with_bg else None
        want = check(ctx, f, tap_frame, mats, dw, dh, feather, bg, src_pad=pads[0], out_pad=pads[1], out_skip=pads[2])
        plain = S.steady_frames(f, tap_frame, mats, dw, dh, 0, bg)
        assert np.array_equal(plain[1], want[1]) and np.array_equal(plain[2], want[2])      # the feather moves no pixel's owner
        seen_mix = seen_mix or not np.array_equal(plain[0], want[0])
    if feather == 0 or ntaps == 1:
        assert not seen_mix                               # no second tap, no band: nothing is mixed
    elif feather >= 33:
        assert seen_mix                                   # the cases do reach the mixing (at feather 1 it needs d == 0 exactly)


# ---- taps that are no frame, matrices that cover nothing ---------------------------------------------------------------------------------
BAD = {
    "nan": np.full(9, np.nan), "zero": np.zeros(9), "one_nan": np.array([1, 0, 0, 0, 1, 0, 0, 0, np.nan]),
    "singular_rank1": np.outer([100.0, 2.0, 0.5], [3.0, -1.0, 2.0]).reshape(9),      # every pixel -> (200, 4), beside the frame
    "inf": np.array([np.inf, 0, 0, 0, 1, 0, 0, 0, 1]),
    # tw = 0.05 X - 1 changes sign at X = 20 inside the picture; tx = 1e6 keeps both sides outside the frame
    "horizon": np.array([0, 0, 1e6, 0, 1, 0, 0.05, 0, -1], np.float64),
    "far": W.translation(1e4, 0).reshape(9),
}


@pytest.mark.parametrize("gray", [False, True])
def test_dead_taps_cover_nothing_and_read_nothing(ctx, gray):
    sw, sh = SIZES[1]
    f = frames_of(51, 2, sw, sh, gray)
    bg = frames_of(52, 1, 37, 9, gray)[0]
    eye = np.eye(3).reshape(9)
    for dead in (-1, 2, 3, 65536, 2 ** 31 - 1, -2 ** 31):
        tap_frame = [[dead, dead], [dead, 1], [0, dead]]
        mats = np.tile(eye, (3, 2, 1))
        want = check(ctx, f, tap_frame, mats, 37, 9, 64, bg)
        assert np.array_equal(want[0][0], bg) and (want[1][0] == 0).all() and list(want[2][0]) == [37 * 9, 0, 0]
        assert np.array_equal(want[0][1], f[1][:9]) and (want[1][1] == 2).all()
        assert np.array_equal(want[0][2], f[0][:9]) and (want[1][2] == 1).all()          # a band without a second tap stays v0
    check(ctx, f, [[-1]], [eye], 37, 9, 0, None)


@pytest.mark.parametrize("name", sorted(BAD))
def test_bad_matrices_cover_nothing(ctx, name):
    sw, sh = SIZES[1]
    f = frames_of(53, 3, sw, sh)
    bg = frames_of(54, 1, 37, 9)[0]
    M, eye = BAD[name], np.eye(3).reshape(9)
    with np.errstate(all="ignore"):
        assert not W.warp_frame(f[0], M, 37, 9, (0, 0), True)[1].any()
    for feather in (0, 256):
        # a first tap covering nothing, alone and in front of a good one; bad taps between tap 0 and its second tap
        want = check(ctx, f, [[0, 1, 2]], [[M, M, M]], 37, 9, feather, bg)
        assert np.array_equal(want[0][0], bg) and list(want[2][0]) == [37 * 9, 0, 0, 0]
        want = check(ctx, f, [[0, 1, 2]], [[M, eye, M]], 37, 9, feather, bg)
        assert np.array_equal(want[0][0], f[1][:9]) and (want[1] == 2).all()
        check(ctx, f, [[0, 1, 2], [2, 1, 0]], [[W.translation(3, 2).reshape(9), M, eye], [eye, M, M]], 37, 9, feather, bg)


# ---- the feather band ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("feather", [1, 33, 256, 8160])
def test_feather_band_with_and_without_a_second_tap(ctx, gray, feather):
    sw, sh = SIZES[1]
    f = frames_of(55, 4, sw, sh, gray)
    eye = np.eye(3).reshape(9)
    shift = W.translation(-4.25, -2.5).reshape(9)                   # tap 0 covers the picture from (5, 3) on: an L-shaped wedge is open
    far = BAD["far"]
    dw, dh = 37, 21
    bg = frames_of(56, 1, dw, dh, gray)[0]
    # picture 0: the second tap right behind; 1: found behind a dead tap, a NaN map and one that covers nothing; 2: none covers
    tap_frame = [[0, 1, 2, 3, 1], [0, -1, 2, 3, 1], [0, 7, 2, 3, -1]]
    mats = [[shift, eye, eye, eye, eye], [shift, eye, BAD["nan"], far, eye], [shift, eye, BAD["nan"], far, eye]]
    want = check(ctx, f, tap_frame, mats, dw, dh, feather, bg, out_pad=1)
    plain = S.steady_frames(f, tap_frame, mats, dw, dh, 0, bg)[0]
    d = S.edge_distance(shift, sw, sh, dw, dh)
    own = want[1] == 1
    assert own[0].any() and (want[1][0][~own[0]] == 2).all() and (want[1][1][~own[1]] == 5).all() and (want[1][2][~own[2]] == 0).all()
    assert np.array_equal(want[0][2], plain[2])                       # nothing is feathered into the background
    assert np.array_equal(want[0][2][~own[2]], bg[~own[2]])
    edge = own[0] & (d == 0)                                          # integer rows of a shift by halves: d == 0 does not occur...
    inner = own[0] & (d >= feather)
    assert np.array_equal(want[0][0][inner], plain[0][inner]) and np.array_equal(want[0][1][inner], plain[1][inner])
    band = own[0] & (d < feather)
    assert band.any() == (feather > 16)                               # the nearest samples of tap 0 lie 16/32 and 24/32 inside
    assert not band.any() or not np.array_equal(want[0][0][band], plain[0][band])
    assert not edge.any()
    # ... so paste tap 0 at whole pixels as well: on its first row and column d == 0, and the byte is wholly the second tap's
    whole = W.translation(-5, -3).reshape(9)
    want = check(ctx, f, [[0, 3, 1]], [[whole, far, eye]], dw, dh, feather, bg, out_skip=1)
    d = S.edge_distance(whole, sw, sh, dw, dh)
    edge = (want[1][0] == 1) & (d == 0)
    assert edge.sum() == (dw - 5) + (dh - 3) - 1 and np.array_equal(want[0][0][edge], f[1][:dh, :dw][edge])


# ---- counts, the optional outputs, alignment ----------------------------------------------------------------------------------------------
def test_counts_repeat_and_optional_outputs(ctx):
    sw, sh = SIZES[1]
    f = frames_of(57, 6, sw, sh)
    tap_frame = np.random.default_rng(58).integers(-1, 7, (3, 5))
    mats = maps_of(59, 3, 5, sw, sh)
    base = run(ctx, f, tap_frame, mats, 37, 9, 33)
    want = S.steady_frames(f, tap_frame, mats, 37, 9, 33)
    assert all(np.array_equal(g, w) for g, w in zip(base, want))
    again = run(ctx, f, tap_frame, mats, 37, 9, 33, launches=2)          # the entry zeroes the counts itself, every time
    assert np.array_equal(again[2], want[2]) and (again[2].sum(axis=1) == 37 * 9).all()
    for tap_of, counts in ((False, True), (True, False), (False, False)):
        got = run(ctx, f, tap_frame, mats, 37, 9, 33, tap_of=tap_of, counts=counts)
        assert np.array_equal(got[0], want[0])
        assert got[1] is None or np.array_equal(got[1], want[1])
        assert got[2] is None or np.array_equal(got[2], want[2])


@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("dw", [36, 37])
def test_word_and_byte_paths(ctx, gray, dw):
    """An aligned base with strides that are multiples of 4 stores words; a base one pixel in, or a row pitch that is no multiple
    of 4, goes bytewise; both must give the same bytes and leave the padding alone."""
    sw, sh = SIZES[1]
    f = frames_of(60, 3, sw, sh, gray)
    tap_frame = [[0, 1, 2], [1, 2, 0], [2, -1, 1]]
    mats = maps_of(61, 3, 3, sw, sh)
    bg = frames_of(62, 1, dw, 9, gray)[0]
    for out_pad, out_skip in ((0, 0), (4, 0), (3, 1), (1, 0), (0, 4), (2, 2)):
        check(ctx, f, tap_frame, mats, dw, 9, 33, bg, out_pad=out_pad, out_skip=out_skip)
        check(ctx, f, tap_frame, mats, dw, 9, 33, None, out_pad=out_pad, out_skip=out_skip)


# ---- planes --------------------------------------------------------------------------------------------------------------------------------
def test_planes_equal_the_bgr_entry_on_the_converted_frames(ctx):
    import torch
    rng = np.random.default_rng(63)
    n, w, h, cw, ch = 3, 37, 21, 19, 11
    planes = [(rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8),
               rng.integers(0, 256, (ch, cw), dtype=np.uint8)) for _ in range(n)]
    bgr = W.planes_to_bgr(planes)
    nout, ntaps, dw, dh, feather = 3, 3, 37, 9, 64
    tap_frame = np.array([[0, 1, 2], [1, 0, -1], [2, 2, 0]], np.int32)
    mats = maps_of(64, nout, ntaps, w, h)
    bg = frames_of(65, 1, dw, dh)[0]
    want = S.steady_frames(bgr, tap_frame, mats, dw, dh, feather, bg)
    d_t, d_m, d_bg = dev(tap_frame), dev(mats), dev(bg)
    y, cb, cr = (dev(np.stack([p[i] for p in planes])) for i in range(3))
    uv = torch.stack([cb, cr], dim=-1).contiguous()
    packed = dev(np.stack([np.concatenate([a.reshape(-1) for a in p]) for p in planes]))
    conv = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    ctx.yuv420_to_bgr((y, cb, cr), conv)
    for name, src, size in (("bgr", conv, None), ("i420", (y, cb, cr), None), ("nv12", (y, uv[..., 0], uv[..., 1]), None),
                            ("packed", packed, (w, h))):
        out = torch.full((nout, dh, dw, 3), SENTINEL, dtype=torch.uint8, device="cuda")
        of = torch.full((nout, dh, dw), SENTINEL, dtype=torch.uint8, device="cuda")
        counts = torch.zeros((nout, ntaps + 1), dtype=torch.int32, device="cuda")
        ctx.steady_frames(src, d_t, d_m, out, feather=feather, background=d_bg, tap_of=of, counts=counts, size=size)
        ctx.synchronize()
        assert np.array_equal(out.cpu().numpy(), want[0]), name
        assert np.array_equal(of.cpu().numpy(), want[1]) and np.array_equal(counts.cpu().numpy(), want[2]), name


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(ctx):
    import torch
    from evenvizion_amd._lib import Yuv420
    INVALID, CAPACITY = -1, -3
    n, sw, sh, dw, dh, nout, ntaps = 2, 23, 17, 31, 22, 2, 3
    src = dev(frames_of(66, n, sw, sh))
    tap_frame = dev(np.array([[0, -1, -1], [1, -1, -1]], np.int32))
    mats = dev(np.tile(np.eye(3).reshape(1, 1, 9), (nout, ntaps, 1)))
    out = torch.full((nout + 1, dh, dw, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    of = torch.full((nout + 1, dh, dw), SENTINEL, dtype=torch.uint8, device="cuda")
    counts = torch.full((nout + 1, ntaps + 1), 77, dtype=torch.int32, device="cuda")
    elsewhere = torch.full((dh, dw, 3), 7, dtype=torch.uint8, device="cuda")
    o, ors, ofs = out.data_ptr(), dw * 3, dw * dh * 3
    good = dict(ctx=ctx.h, frames=src.data_ptr(), n=n, sw=sw, sh=sh, cn=3, rs=sw * 3, fs=sw * sh * 3, tf=tap_frame.data_ptr(),
                tm=mats.data_ptr(), nout=nout, ntaps=ntaps, feather=64, bg=elsewhere.data_ptr(), out=o, dw=dw, dh=dh, ors=ors,
                ofs=ofs, of=of.data_ptr(), trs=dw, tfs=dw * dh, counts=counts.data_ptr())
    tail = ("tf", "tm", "nout", "ntaps", "feather", "bg", "out", "dw", "dh", "ors", "ofs", "of", "trs", "tfs", "counts")

    def call(**kw):
        a = dict(good, **kw)
        return ctx.lib.evh_steady_frames(a["ctx"], a["frames"], a["n"], a["sw"], a["sh"], a["cn"], a["rs"], a["fs"], *[a[k] for k in tail])

    who, who_yuv = "evh_steady_frames: ", "evh_steady_frames_yuv420: "
    NS, NA, CH, EM = "NULL source", "NULL argument", "channels must be 1 or 3", "empty frame or canvas"
    NT, FE, NO = "ntaps must lie in 1..16", "feather must lie in 0..8160", "negative nout"
    BIG, AREA = "source sizes stay below 2^26 (positions are held in 1/32 pixels)", "dw * dh above INT_MAX"
    NP, OS, TS = "at most 65535 pictures per call", "output stride smaller than a row / picture", "d_tap_of stride smaller than a row / picture"
    SS = "source stride smaller than a row / frame"

    def refused(rc, code, text, what):
        assert rc == code, what
        assert ctx.lib.evh_last_error_string(ctx.h).decode() == text, what

    assert call(ctx=None) == INVALID
    invalid = [(dict(frames=None), NS), (dict(tf=None), NA), (dict(tm=None), NA), (dict(out=None), NA), (dict(cn=2), CH), (dict(cn=0), CH),
               (dict(sw=0), EM), (dict(sh=0), EM), (dict(dw=0), EM), (dict(dh=-1), EM), (dict(n=-1), EM), (dict(nout=-1), NO),
               (dict(ntaps=0), NT), (dict(ntaps=17), NT), (dict(feather=-1), FE), (dict(feather=8161), FE),
               (dict(rs=sw * 3 - 1), SS), (dict(fs=sw * sh * 3 - 1), SS), (dict(ors=ors - 1), OS), (dict(ofs=ofs - 1), OS),
               (dict(trs=dw - 1), TS), (dict(tfs=dw * dh - 1), TS),
               (dict(bg=o), "d_out overlaps d_background"), (dict(bg=o + ofs + ors), "d_out overlaps d_background"),
               (dict(bg=o - ors), "d_out overlaps d_background"), (dict(of=o + 5), "d_out overlaps d_tap_of"),
               (dict(counts=o + 2 * ofs - 4), "d_out overlaps d_counts"), (dict(of=counts.data_ptr()), "d_tap_of overlaps d_counts"),
               # two faults: the earlier check of the entry names the refusal
               (dict(frames=None, tf=None), NS), (dict(tm=None, cn=2), NA), (dict(cn=2, sw=0), CH), (dict(ntaps=0, feather=-1), NT),
               (dict(bg=o, ors=ors - 1), OS), (dict(feather=9000, nout=65536), FE)]
    for kw, text in invalid:
        refused(call(**kw), INVALID, who + text, kw)
    big = 1 << 26
    capacity = [(dict(sw=big, rs=big * 3, fs=big * 3 * sh), BIG), (dict(sh=big, fs=sw * 3 * big), BIG),
                (dict(dw=65536, dh=32768, ors=65536 * 3, ofs=1 << 40, trs=65536, tfs=1 << 40), AREA), (dict(nout=65536), NP),
                (dict(nout=65536, ors=ors - 1), NP), (dict(sh=big, bg=o), BIG)]
    for kw, text in capacity:
        refused(call(**kw), CAPACITY, who + text, kw)
    # the plane form: its own description, then the same checks
    y = torch.zeros((n, sh, sw), dtype=torch.uint8, device="cuda")
    c = torch.zeros((2, n, 9, 12), dtype=torch.uint8, device="cuda")
    yuv = dict(d_y=y.data_ptr(), d_cb=c[0].data_ptr(), d_cr=c[1].data_ptr(), y_stride=sw, c_stride=12, y_frame_stride=sw * sh,
               c_frame_stride=12 * 9, c_pixel_stride=1)

    def call_yuv(desc, **kw):
        a = dict(good, **kw)
        d = None if desc is None else ctypes.byref(Yuv420(**desc))
        return ctx.lib.evh_steady_frames_yuv420(a["ctx"], d, a["n"], a["sw"], a["sh"], *[a[k] for k in tail])

    refused(call_yuv(None), INVALID, who_yuv + NS, "no description")
    for bad, text in ((dict(d_y=None), NS), (dict(c_pixel_stride=3), "chroma pixel stride must be 1 or 2"),
                      (dict(y_stride=sw - 1), "luma row stride smaller than the width")):
        refused(call_yuv(dict(yuv, **bad)), INVALID, who_yuv + text, bad)
    for kw, text in ((dict(tm=None), NA), (dict(dw=0), EM), (dict(ntaps=17), NT), (dict(feather=8161), FE), (dict(ors=ors - 1), OS),
                     (dict(bg=o), "d_out overlaps d_background")):
        refused(call_yuv(yuv, **kw), INVALID, who_yuv + text, kw)
    refused(call_yuv(yuv, nout=65536), CAPACITY, who_yuv + NP, "capacity")
    # no pictures: success, and nothing is done
    assert call(nout=0) == 0 and call_yuv(yuv, nout=0) == 0
    ctx.synchronize()
    assert (out == SENTINEL).all() and (of == SENTINEL).all() and (counts == 77).all() and (elsewhere == 7).all()
    # and the same arguments unrefused do write
    assert call() == 0
    ctx.synchronize()
    assert np.array_equal(out[:nout, :sh, :sw].cpu().numpy(), src.cpu().numpy()) and (out[0, sh:] == 7).all()
    assert (out[nout] == SENTINEL).all() and (of[:nout, :sh, :sw] == 1).all() and (of[:nout, sh:] == 0).all()
    assert counts[:nout].cpu().numpy().tolist() == [[dw * dh - sw * sh, sw * sh, 0, 0]] * nout and (counts[nout] == 77).all()
