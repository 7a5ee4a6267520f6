"""evh_trail_fixed_plane / evh_trail_fixed_plane_yuv420 on the device, and the pictures built on them.  Every assertion is
equality of bytes with the numpy restatement of the header's arithmetic (tests/trail_checks.py, itself checked in
test_trail_host.py)."""
import ctypes
import itertools
import json
import os

import numpy as np
import pytest

import trail_checks as T
import warp_checks as W
from refusal_arena import Arena

pytestmark = pytest.mark.gpu
SENTINEL = 0xCD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MP4 = os.path.join(ROOT, "tests", "golden", "ref_test_video.mp4")
GOLD = os.path.join(ROOT, "tests", "golden", "ref_dict_with_homography_matrix.json")


@pytest.fixture(scope="module")
def ctx():
    from evenvizion_amd._lib import Context
    c = Context(device=0, max_w=64, max_h=64, max_features=500, max_frames=2)     # the entry does not depend on these sizes
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def strided(shape, row_pad, skip):
    """A SENTINEL-filled flat buffer and a view [*shape] into it whose rows are row_pad bytes longer than their pixels (pictures
    lie a spare row apart) and which starts skip bytes in.  Rows of a multiple of 4 bytes from skip 0 take the kernel's word
    path, anything else its bytewise one."""
    import torch
    *lead, dh, dw, _ = shape
    rs = dw * 3 + row_pad
    fs = rs * (dh + 1)
    flat = torch.full((skip + fs * (lead[0] if lead else 1) + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    strides = ((fs,) if lead else ()) + (rs, 3, 1)
    return flat, flat.as_strided(tuple(shape), strides, skip)


def untouched_outside(flat, view):
    """The bytes of the buffer that the view does not name still hold SENTINEL."""
    before = flat.clone()
    view.fill_(SENTINEL)
    same = bool((flat == SENTINEL).all())
    flat.copy_(before)
    return same


class Canvas:
    """A carried canvas on the device (row padding of SENTINEL) and calls of Context.trail_fixed_plane on it.  The default
    paddings give rows of 116 (canvas) and 112 (pictures) bytes for the 37-pixel canvas: words."""

    def __init__(self, ctx, canvas, origin=(0, 0), row_pad=5, skip=0):
        self.ctx, self.origin, self.row_pad, self.skip = ctx, origin, row_pad, skip
        self.flat, self.view = strided(canvas.shape, row_pad, skip)
        self.view.copy_(dev(canvas))

    def advance(self, frames, mats, rects=None, pictures=True, inverse_map=False, size=None, out_pad=1, out_skip=0):
        n = len(mats)
        out_flat = out = None
        if pictures:
            out_flat, out = strided((n,) + tuple(self.view.shape), out_pad, out_skip)
        src = frames if not isinstance(frames, np.ndarray) else dev(frames)
        self.ctx.trail_fixed_plane(src, dev(np.asarray(mats, np.float64).reshape(n, 9)), self.view, self.origin, out=out,
                                   rects=None if rects is None else dev(np.asarray(rects, np.int32).reshape(n, 4)),
                                   inverse_map=inverse_map, size=size)
        self.ctx.synchronize()
        assert untouched_outside(self.flat, self.view), "bytes between the canvas rows were written"
        if not pictures:
            return None
        assert untouched_outside(out_flat, out), "bytes between the picture rows were written"
        return out.cpu().numpy()

    def numpy(self):
        return self.view.cpu().numpy()


# ---- every colour ------------------------------------------------------------------------------------------------------------------
def test_every_colour_through_show_and_keep(ctx):
    import torch
    frame, kept, shown, _ = T.every_colour()
    canvas = torch.zeros((4096, 4096, 3), dtype=torch.uint8, device="cuda")
    out = torch.full((1, 4096, 4096, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    ctx.trail_fixed_plane(dev(np.array(frame)[None]), dev(np.eye(3).reshape(1, 9)), canvas, (0, 0), out=out)
    ctx.synchronize()
    got_show, got_keep = out[0].cpu().numpy(), canvas.cpu().numpy()
    print("show: %d colours differ; keep: %d colours differ" % ((got_show != shown).any(axis=-1).sum(),
                                                               (got_keep != kept).any(axis=-1).sum()))
    assert np.array_equal(got_show, shown)
    assert np.array_equal(got_keep, kept)


# ---- a long sequence, cut and aligned in four ways -----------------------------------------------------------------------------------
N, DW, DH = 140, 37, 29


def sequence(sw, sh):
    rng = np.random.default_rng(43)
    frames = rng.integers(0, 256, (N, sh, sw, 3), dtype=np.uint8)
    frames[:, 0, 0] = 255                                              # pure white
    frames[:, 1, 1] = rng.integers(0, 2, (N, 3))                       # V < 2
    frames[:, 2, 2] = 0
    frames[3] = 255
    k = np.arange(N)
    dx = np.rint(17 + 22 * np.cos(2 * np.pi * k / 70)).astype(int)     # -5 .. 39: off the canvas on the left and the right
    dy = np.rint(11 + 17 * np.sin(2 * np.pi * k / 70)).astype(int)     # -6 .. 28: off it above and below
    assert dx.min() < 0 and dx.max() + sw > DW and dy.min() < 0 and dy.max() + sh > DH
    mats = np.stack([W.translation(x, y) for x, y in zip(dx, dy)])
    mats[20] = np.nan
    mats[21] = 0
    rects = np.stack([dx, dy, dx + sw, dy + sh], axis=1).astype(np.int32)      # inside the canvas or clipped by it
    rects[7] = (5, 6, 4, 9)                                            # absent: x1 < x0
    rects[8] = (5, 6, 9, 5)                                            # absent: y1 < y0
    rects[9] = (12, 13, 12, 13)                                        # degenerate: one pixel
    rects[10] = (3, 20, 30, 20)                                        # degenerate: one row
    rects[11] = (-50, -50, 90, 90)                                     # around the canvas: nothing of it inside
    rects[12] = (0, 0, DW - 1, DH - 1)                                 # the canvas's own edge
    canvas = rng.integers(0, 256, (DH, DW, 3), dtype=np.uint8)
    return frames, mats, rects, canvas


@pytest.fixture(scope="module")
def expected_sequence():
    frames, mats, rects, canvas = sequence(9, 7)
    pictures, after = T.trail(frames, mats, canvas, (0, 0), rects)
    # more than 128 frames: the first canvas and frames 0 .. 12 have faded out altogether
    late = T.trail(frames[13:], mats[13:], np.zeros_like(canvas), (0, 0), rects[13:])
    assert np.array_equal(late[1], after) and np.array_equal(late[0][-1], pictures[-1])
    assert (pictures[11] != pictures[10]).any() and (pictures == 253).any() and (pictures == np.array(T.DARK, np.uint8)).all(-1).any()
    return frames, mats, rects, canvas, pictures, after


def test_sequence_as_one_call(ctx, expected_sequence):
    frames, mats, rects, canvas, want, want_canvas = expected_sequence
    c = Canvas(ctx, canvas)
    got = c.advance(frames, mats, rects)
    print("pictures: %d bytes differ; canvas: %d bytes differ" % ((got != want).sum(), (c.numpy() != want_canvas).sum()))
    assert np.array_equal(got, want) and np.array_equal(c.numpy(), want_canvas)


def test_sequence_in_two_calls_carries_the_canvas(ctx, expected_sequence):
    frames, mats, rects, canvas, want, want_canvas = expected_sequence
    c = Canvas(ctx, canvas)
    got = np.concatenate([c.advance(frames[:5], mats[:5], rects[:5]), c.advance(frames[5:], mats[5:], rects[5:])])
    assert np.array_equal(got, want) and np.array_equal(c.numpy(), want_canvas)


def test_sequence_without_pictures_only_advances_the_canvas(ctx, expected_sequence):
    frames, mats, rects, canvas, want, want_canvas = expected_sequence
    c = Canvas(ctx, canvas)
    assert c.advance(frames[:5], mats[:5], rects[:5], pictures=False) is None
    assert np.array_equal(c.numpy(), T.trail(frames[:5], mats[:5], canvas, (0, 0), rects[:5])[1])
    got = c.advance(frames[5:], mats[5:], rects[5:])
    assert np.array_equal(got, want[5:]) and np.array_equal(c.numpy(), want_canvas)


def test_sequence_through_odd_pointers_and_strides(ctx, expected_sequence):
    frames, mats, rects, canvas, want, want_canvas = expected_sequence
    c = Canvas(ctx, canvas, row_pad=2, skip=1)                         # rows of 113 bytes from an odd address
    got = c.advance(frames, mats, rects, out_pad=2, out_skip=1)
    assert c.view.data_ptr() % 2 == 1 and c.view.stride(0) % 2 == 1
    assert np.array_equal(got, want) and np.array_equal(c.numpy(), want_canvas)
    # words for the canvas and bytes for the pictures, and the other way round
    for (cp, cs), (op, os_) in (((5, 0), (2, 1)), ((2, 1), (1, 0))):
        c = Canvas(ctx, canvas, row_pad=cp, skip=cs)
        got = c.advance(frames[:12], mats[:12], rects[:12], out_pad=op, out_skip=os_)
        assert np.array_equal(got, want[:12])


def test_planes_equal_the_bgr_entry_on_the_converted_frames(ctx):
    import torch
    _, mats, rects, canvas = sequence(10, 8)
    rng = np.random.default_rng(44)
    sw, sh, cw, ch = 10, 8, 5, 4
    planes = [(rng.integers(0, 256, (sh, sw), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8),
               rng.integers(0, 256, (ch, cw), dtype=np.uint8)) for _ in range(N)]
    y, cb, cr = (dev(np.stack([p[i] for p in planes])) for i in range(3))
    packed = dev(np.stack([np.concatenate([a.reshape(-1) for a in p]) for p in planes]))
    conv = torch.zeros((N, sh, sw, 3), dtype=torch.uint8, device="cuda")
    ctx.yuv420_to_bgr((y, cb, cr), conv)
    ctx.synchronize()
    bgr = conv.cpu().numpy()
    assert np.array_equal(bgr, W.planes_to_bgr(planes))
    want, want_canvas = T.trail(bgr, mats, canvas, (0, 0), rects)
    via_bgr = Canvas(ctx, canvas)
    assert np.array_equal(via_bgr.advance(conv, mats, rects), want) and np.array_equal(via_bgr.numpy(), want_canvas)
    for name, src, size in (("i420", (y, cb, cr), None), ("packed", packed, (sw, sh))):
        c = Canvas(ctx, canvas)
        got = c.advance(src, mats, rects, size=size)
        assert np.array_equal(got, want) and np.array_equal(c.numpy(), want_canvas), name


# ---- projective matrices --------------------------------------------------------------------------------------------------------
def test_projective_frames_with_and_without_inverse_map(ctx):
    rng = np.random.default_rng(45)
    n, sw, sh, dw, dh, origin = 6, 16, 12, 41, 27, (-6, -4)
    frames = rng.integers(0, 256, (n, sh, sw, 3), dtype=np.uint8)
    mats = []
    for k in range(n):
        th = np.deg2rad(-10 + 5 * k)
        c, s = (0.9 + 0.1 * k) * np.cos(th), (0.9 + 0.1 * k) * np.sin(th)
        mats.append([[c, -s, 2 + 3 * k], [s, c, 1 + 2 * k], [4e-4 * k, -3e-4 * k, 1.0]])
    mats = np.array(mats)
    canvas = rng.integers(0, 256, (dh, dw, 3), dtype=np.uint8)
    for inverse_map, m in ((False, mats), (True, np.linalg.inv(mats))):
        want, want_canvas = T.trail(frames, m, canvas, origin, None, inverse_map)
        assert (want != T.trail(frames[:0], m[:0], canvas, origin)[1]).any()
        c = Canvas(ctx, canvas, origin)
        got = c.advance(frames, m, None, inverse_map=inverse_map)
        print("inverse_map %s: %d bytes differ" % (inverse_map, (got != want).sum()))
        assert np.array_equal(got, want) and np.array_equal(c.numpy(), want_canvas)


# ---- no frame covers anything ------------------------------------------------------------------------------------------------------
def test_canvas_alone_fades_to_black(ctx):
    rng = np.random.default_rng(46)
    n = 130
    canvas = rng.integers(0, 256, (8, 8, 3), dtype=np.uint8)
    canvas[0, 0] = 255
    frames, mats = np.zeros((n, 3, 3, 3), np.uint8), np.full((n, 9), np.nan)
    want, want_canvas = T.trail(frames, mats, canvas)
    c = Canvas(ctx, canvas)
    got = c.advance(frames, mats)
    assert np.array_equal(got, want) and np.array_equal(c.numpy(), want_canvas)
    assert not c.numpy().any() and (got[-1] == np.array(T.DARK, np.uint8)).all()
    assert (got[0, 0, 0] == 253).all() and (got[110, 0, 0] == 33).all() and (got[126, 0, 0] == 1).all()      # white, step by step


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(ctx):
    import torch
    from evenvizion_amd._lib import Yuv420
    INVALID, CAPACITY = -1, -3
    n, sw, sh, dw, dh = 2, 10, 8, 31, 22
    rng = np.random.default_rng(47)
    A = Arena(6)            # every buffer a fixed distance from the others: which ranges meet is the test's to say
    src = A.put(rng.integers(1, 256, (n + 1, sh, sw, 3), dtype=np.uint8))
    mats = A.put(np.tile(np.eye(3).reshape(1, 9), (n, 1)))
    out = A.take((n + 1, dh, dw, 3), fill=SENTINEL)
    canvas = A.take((dh + 1, dw, 3), fill=7)
    f, m, o, cv = src.data_ptr(), mats.data_ptr(), out.data_ptr(), canvas.data_ptr()
    rs, fs, ors, ofs = sw * 3, sw * sh * 3, dw * 3, dw * dh * 3
    good = dict(ctx=ctx.h, frames=f, n=n, sw=sw, sh=sh, rs=rs, fs=fs, M=m, inv=0, rect=None, canvas=cv, crs=ors, out=o, ors=ors,
                ofs=ofs, dw=dw, dh=dh, ox=0, oy=0)

    def call(**kw):
        a = dict(good, **kw)
        return ctx.lib.evh_trail_fixed_plane(a["ctx"], a["frames"], a["n"], a["sw"], a["sh"], a["rs"], a["fs"], a["M"], a["inv"],
                                             a["rect"], a["canvas"], a["crs"], a["out"], a["ors"], a["ofs"], a["dw"], a["dh"],
                                             a["ox"], a["oy"])

    who, who_yuv = "evh_trail_fixed_plane: ", "evh_trail_fixed_plane_yuv420: "
    NS, NA, EM = "NULL source", "NULL argument", "empty frame or canvas"
    BIG, AREA = "source sizes stay below 2^26 (positions are held in 1/32 pixels)", "dw * dh above INT_MAX"
    NF, SS = "at most 65535 frames per call", "source stride smaller than a row / frame"
    CS = "canvas or output stride smaller than a row / picture"
    OC, OF, CF = "d_out overlaps d_canvas", "d_out overlaps the frames", "d_canvas overlaps the frames"

    def refused(rc, code, text, what):
        assert rc == code, what
        assert ctx.lib.evh_last_error_string(ctx.h).decode() == text, what

    assert call(ctx=None) == INVALID
    invalid = [(dict(frames=None), NS), (dict(M=None), NA), (dict(canvas=None), NA), (dict(sw=0), EM), (dict(sh=0), EM), (dict(dw=0), EM),
               (dict(dh=-1), EM), (dict(n=-1), EM), (dict(rs=rs - 1), SS), (dict(fs=fs - 1), SS), (dict(crs=ors - 1), CS),
               (dict(ors=ors - 1), CS), (dict(ofs=ofs - 1), CS),
               (dict(out=cv), OC), (dict(out=cv + ors), OC), (dict(out=cv - ofs), OC), (dict(canvas=o + ofs + ors), OC),
               (dict(out=f), OF), (dict(out=f + fs + rs), OF), (dict(out=f - ofs - ors), OF),
               (dict(canvas=f), CF), (dict(canvas=f + 2 * fs - 1), CF), (dict(canvas=f - ofs + 1), CF),
               (dict(out=None, canvas=f + fs), CF),
               # two faults: the earlier check of the entry names the refusal
               (dict(frames=None, canvas=None), NS), (dict(M=None, sw=0), NA), (dict(out=cv, crs=ors - 1), CS),
               (dict(ors=ors - 1, rs=rs - 1), CS), (dict(rs=rs - 1, out=cv), SS), (dict(out=f, canvas=f), OC)]
    for kw, text in invalid:
        refused(call(**kw), INVALID, who + text, kw)
    big = 1 << 26
    capacity = [(dict(sw=big, rs=big * 3, fs=big * 3 * sh), BIG), (dict(sh=big, fs=sw * 3 * big), BIG),
                (dict(dw=65536, dh=32768, crs=65536 * 3, ors=65536 * 3, ofs=1 << 40), AREA), (dict(n=65536), NF),
                # two faults: a capacity refusal precedes the strides and the overlaps
                (dict(sw=big, rs=big * 3 - 1, fs=big * 3 * sh), BIG), (dict(n=65536, crs=ors - 1), NF), (dict(sh=big, out=cv), BIG),
                (dict(sw=big, n=65536), BIG)]
    for kw, text in capacity:
        refused(call(**kw), CAPACITY, who + text, kw)
    refused(call(sw=big - 1, rs=(big - 1) * 3 - 1), INVALID, who + SS, "below the limit")     # there the ordinary checks apply
    # what touches nothing is accepted: the buffers may lie side by side, and without pictures their strides do not count
    assert call(n=0) == 0 and call(n=0, out=None, ors=0, ofs=0) == 0
    # the plane form: its own description, then the same checks
    y = A.take((n, sh, sw), fill=200)
    c = A.take((2, n, 4, 5), fill=128)
    yuv = dict(d_y=y.data_ptr(), d_cb=c[0].data_ptr(), d_cr=c[1].data_ptr(), y_stride=sw, c_stride=5, y_frame_stride=sw * sh,
               c_frame_stride=20, c_pixel_stride=1)

    def call_yuv(desc, **kw):
        a = dict(good, **kw)
        d = None if desc is None else ctypes.byref(Yuv420(**desc))
        return ctx.lib.evh_trail_fixed_plane_yuv420(a["ctx"], d, a["n"], a["sw"], a["sh"], a["M"], a["inv"], a["rect"], a["canvas"],
                                                    a["crs"], a["out"], a["ors"], a["ofs"], a["dw"], a["dh"], a["ox"], a["oy"])

    refused(call_yuv(None), INVALID, who_yuv + NS, "no description")
    CPS, PLANE = "chroma pixel stride must be 1 or 2", "frame stride smaller than a plane"
    for bad, text in ((dict(d_y=None), NS), (dict(d_cb=None), NS), (dict(d_cr=None), NS), (dict(c_pixel_stride=3), CPS),
                      (dict(y_stride=sw - 1), "luma row stride smaller than the width"),
                      (dict(c_stride=4), "chroma row stride smaller than a chroma row"),
                      (dict(y_frame_stride=sw * sh - 1), PLANE), (dict(c_frame_stride=19), PLANE)):
        refused(call_yuv(dict(yuv, **bad)), INVALID, who_yuv + text, bad)
    for kw, text in ((dict(M=None), NA), (dict(canvas=None), NA), (dict(dw=0), EM), (dict(crs=ors - 1), CS), (dict(ors=ors - 1), CS),
                     (dict(out=cv), OC), (dict(out=y.data_ptr()), OF), (dict(canvas=c[1].data_ptr() + 39), CF),
                     (dict(out=c[0].data_ptr() - ofs - ors + 1), OF), (dict(out=c[0].data_ptr()), OF)):       # the last: over the Cb plane
        refused(call_yuv(yuv, **kw), INVALID, who_yuv + text, kw)
    # two faults, one of them in the description: a NULL plane first, the strides before the planes, the planes before the overlaps
    refused(call_yuv(dict(yuv, d_cb=None), M=None), INVALID, who_yuv + NS, "NULL plane before NULL argument")
    refused(call_yuv(dict(yuv, y_stride=sw - 1), crs=ors - 1), INVALID, who_yuv + CS, "strides before the description")
    refused(call_yuv(dict(yuv, c_pixel_stride=3), out=cv), INVALID, who_yuv + CPS, "the description before the overlaps")
    refused(call_yuv(dict(yuv, c_pixel_stride=3), n=65536), CAPACITY, who_yuv + NF, "capacity before the description")
    for kw, text in ((dict(sw=big), BIG), (dict(n=65536), NF), (dict(dw=65536, dh=32768, crs=65536 * 3, ors=65536 * 3, ofs=1 << 40), AREA)):
        refused(call_yuv(yuv, **kw), CAPACITY, who_yuv + text, kw)
    assert call_yuv(yuv, n=0) == 0
    ctx.synchronize()
    assert (out == SENTINEL).all() and (canvas == 7).all() and (y == 200).all() and (c == 128).all()
    # and the same arguments unrefused do write: both pictures, the canvas rows of the call and nothing after them
    assert call() == 0
    ctx.synchronize()
    frames = src.cpu().numpy()[:n]
    want, want_canvas = T.trail(frames, np.tile(np.eye(3), (n, 1, 1)), np.full((dh, dw, 3), 7, np.uint8))
    assert np.array_equal(out[:n].cpu().numpy(), want) and (out[n] == SENTINEL).all()
    assert np.array_equal(canvas[:dh].cpu().numpy(), want_canvas) and (canvas[dh] == 7).all()
    assert call_yuv(yuv, out=None) == 0
    ctx.synchronize()
    assert (canvas[0, 0] != torch.from_numpy(want_canvas[0, 0]).cuda()).any() and (canvas[dh] == 7).all()


# ---- the pictures of the reference video -----------------------------------------------------------------------------------------
class First:
    """The first n frames of a capture, with whatever ways of reading it offers."""

    def __init__(self, cap, n):
        self.cap, self.left = cap, n
        self.width, self.height, self.bgr_mode = cap.width, cap.height, cap.bgr_mode

    def read(self):
        if self.left == 0:
            return False, None
        self.left -= 1
        return self.cap.read()

    def read_yuv420_into(self, y, cb, cr):
        if self.left == 0:
            return False
        self.left -= 1
        return self.cap.read_yuv420_into(y, cb, cr)


@pytest.fixture(scope="module")
def video():
    """The first 12 frames, full size and resized on the device, the recorded dictionary, and the numpy trail over them."""
    import torch
    from evenvizion_amd import capture, runtime
    from evenvizion_amd import stabilization as S
    from evenvizion_amd.processing.utils import read_homography_dict, superposition_dict
    hd, ri = read_homography_dict(GOLD)
    sup = superposition_dict(hd)
    n, w, h = 12, ri["w"], ri["h"]
    cap = capture.VideoCapture(MP4)
    frames = np.stack([cap.read()[1] for _ in range(n)])
    small = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    ctx = runtime.get_context(64, 64)
    d_frames = torch.from_numpy(frames).cuda()
    ctx.resize_area(d_frames, small)
    ctx.synchronize()
    small = small.cpu().numpy()
    with open(os.path.join(ROOT, "tests", "golden", "stabilization_goldens.json")) as f:
        case = [c for c in json.load(f)["cases"] if c["name"] == "all"][0]
    shape = [s["panorama_shape"] for s in case["shapes"] if s["width"] == w][0]
    corner = case["corner_dict"]
    ax, ay = abs(corner["min_x"]), abs(corner["min_y"])
    canvas = np.zeros(tuple(shape) + (3,), np.uint8)
    canvas[ay:ay + h, ax:ax + w] = small[0]                              # initialize_background (stabilization.py:245-249)
    offsets = [S.translate_offset(sup[k]) for k in range(1, n + 1)]
    mats = np.stack([W.translation(x, y) for x, y in offsets])
    rects = np.array([[ax + x, ay + y, ax + x + w, ay + y + h] for x, y in offsets], np.int32)
    want = {True: T.trail(small, mats, canvas, (-ax, -ay), rects)[0], False: T.trail(small, mats, canvas, (-ax, -ay), None)[0]}
    assert (want[True] != want[False]).any()
    return dict(sup=sup, ri=ri, n=n, frames=frames, want=want, open=lambda: First(capture.VideoCapture(MP4), n))


def test_translate_trail_is_the_reference_picture(video):
    from evenvizion_amd import stabilization as S
    runs = {}
    for chunk, ingest in ((5, "auto"), (32, "auto"), (5, "bgr")):
        got = list(S.stabilized_frames(video["open"](), video["sup"], video["ri"], mode="history", placement="translate",
                                       chunk_frames=chunk, ingest=ingest, trail=True))
        assert [k for k, _ in got] == list(range(1, video["n"] + 1))
        runs[chunk, ingest] = np.stack([p for _, p in got])
    first = runs[5, "auto"]
    print("differing bytes: %d of %d" % ((first != video["want"][True]).sum(), first.size))
    assert np.array_equal(first, video["want"][True])
    assert np.array_equal(runs[32, "auto"], first) and np.array_equal(runs[5, "bgr"], first)
    plain = list(itertools.islice(S.stabilized_frames(video["open"](), video["sup"], video["ri"], mode="history",
                                                      placement="translate", chunk_frames=5, trail=True, border=False), 7))
    assert np.array_equal(np.stack([p for _, p in plain]), video["want"][False][:7])


def test_comparison_pictures(video):
    import torch
    from evenvizion_amd import runtime
    from evenvizion_amd import stabilization as S
    n, frames, trail = video["n"], video["frames"], video["want"][True]
    got = list(S.comparison_frames(video["open"](), video["sup"], video["ri"], chunk_frames=5))
    assert [k for k, _ in got] == list(range(1, n + 1))
    h0, w0 = frames.shape[1:3]
    dh, dw = trail.shape[1:3]
    wa, wb = int(w0 * 300 / h0), int(dw * 300 / dh)
    assert S.comparison_size(w0, h0, dw, dh) == ((wa, wb), 300)
    ctx = runtime.get_context(64, 64)
    left = torch.zeros((n, 300, wa, 3), dtype=torch.uint8, device="cuda")
    right = torch.zeros((n, 300, wb, 3), dtype=torch.uint8, device="cuda")
    d_frames, d_trail = torch.from_numpy(frames).cuda(), torch.from_numpy(trail).cuda()      # both alive until the context is done
    ctx.resize_area(d_frames, left)
    ctx.resize_area(d_trail, right)
    ctx.synchronize()
    left, right = left.cpu().numpy(), right.cpu().numpy()
    right[:, 0, :] = right[:, -1, :] = right[:, :, 0] = right[:, :, -1] = (0, 0, 248)      # create_border (stabilization.py:188-190)
    for (k, picture), a, b in zip(got, left, right):
        assert picture.shape == (300, wa + wb, 3) and picture.dtype == np.uint8
        assert np.array_equal(picture[:, :wa], a), k
        assert np.array_equal(picture[:, wa:], b), k
    planes = list(S.comparison_frames(video["open"](), video["sup"], video["ri"], chunk_frames=32, ingest="bgr"))
    assert all(np.array_equal(p, q) for (_, p), (_, q) in zip(got, planes))
