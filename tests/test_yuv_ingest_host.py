"""Decoded 4:2:0 planes as the source of the hot path, the parts that need no GPU: the numpy statement of the BGR conversion
against libevcap's own (which the reference's recorded run pins, tests/test_capture_golden.py), the C ABI surface, and the
stream driver's plane path on the CPU with a scripted context (in the manner of tests/test_host_glue.py)."""
import os
import re

import numpy as np
import pytest

from evenvizion_amd import capture, runtime, synthetic
from evenvizion_amd.processing import video_processing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MP4 = os.path.join(ROOT, "tests", "golden", "ref_test_video.mp4")
NEW_ENTRIES = ["evh_yuv420_to_bgr", "evh_orb_detect_batch_yuv420", "evh_stream_homography_batch_yuv420",
               "evh_stream_homography_batch_types_yuv420"]


def test_numpy_statement_equals_capture_read_on_the_reference_video():
    """yuv420_to_bgr_host(planes of one capture) == read() of a second capture of the same file, all 121 presented frames."""
    capture.build()
    bgr, yuv = capture.VideoCapture(MP4), capture.VideoCapture(MP4)
    assert bgr.isOpened() and yuv.isOpened() and yuv.bgr_mode == capture.BGR_SWSCALE_X86
    h, w = yuv.height, yuv.width
    y = np.empty((h, w), np.uint8)
    cb = np.empty(((h + 1) // 2, (w + 1) // 2), np.uint8)
    cr = np.empty_like(cb)
    frames = differing = 0
    while True:
        ok, f = bgr.read()
        assert yuv.read_yuv420_into(y, cb, cr) == ok
        if not ok:
            break
        frames += 1
        differing += int((synthetic.yuv420_to_bgr_host(y, cb, cr) != f).sum())
    print("frames %d, differing bytes %d" % (frames, differing))
    assert frames == 121 and differing == 0
    assert capture.VideoCapture(MP4, bgr_mode=capture.BGR_SWSCALE_C).bgr_mode == capture.BGR_SWSCALE_C


def test_read_yuv420_into_writes_strided_planes_in_place():
    capture.build()
    a, b = capture.VideoCapture(MP4), capture.VideoCapture(MP4)
    h, w = a.height, a.width
    ch, cw = (h + 1) // 2, (w + 1) // 2
    ok, (y, cb, cr) = a.read_yuv420()
    assert ok
    big_y = np.full((h, w + 7), 0xA5, np.uint8)
    big_c = np.full((2, ch, cw + 5), 0x5A, np.uint8)
    assert b.read_yuv420_into(big_y[:, :w], big_c[0, :, :cw], big_c[1, :, :cw]) is True
    assert np.array_equal(big_y[:, :w], y) and np.array_equal(big_c[0, :, :cw], cb) and np.array_equal(big_c[1, :, :cw], cr)
    assert (big_y[:, w:] == 0xA5).all() and (big_c[:, :, cw:] == 0x5A).all()
    with pytest.raises(ValueError):
        b.read_yuv420_into(big_y[:, :w - 1], cb, cr)


def test_new_entries_are_declared_exported_and_bound():
    from evenvizion_amd import _lib
    _lib.build()
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evhip.h")).read(), flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), "%s is not declared in include/evhip.h" % name
        assert hasattr(lib, name), "libevhip.so does not export %s" % name
        assert name in _lib.SIGNATURES
    for method in ("yuv420_to_bgr", "orb_detect_batch_yuv420", "stream_homography_batch_yuv420",
                   "stream_homography_batch_types_yuv420"):
        assert callable(getattr(_lib.Context, method))
    assert lib.evh_version() == 100
    assert "for tests" not in open(os.path.join(ROOT, "include", "evcap.h")).read()


def test_plane_description_of_tensors():
    """Context._yuv420: packed I420, separate strided planes and NV12 views all describe the same samples."""
    import ctypes
    import torch
    from evenvizion_amd._lib import Context, yuv420_size, yuv420_views
    n, w, h = 2, 7, 5
    fb, cw, ch = yuv420_size(w, h)
    assert (fb, cw, ch) == (35 + 2 * 12, 4, 3)
    packed = torch.arange(n * fb, dtype=torch.int64).to(torch.uint8).reshape(n, fb)

    def sample(d, plane, f, r, c):          # the byte the description addresses, read back through the host pointer
        base = {"y": d.d_y, "cb": d.d_cb, "cr": d.d_cr}[plane]
        if plane == "y":
            off = f * d.y_frame_stride + r * d.y_stride + c
        else:
            off = f * d.c_frame_stride + r * d.c_stride + c * d.c_pixel_stride
        return ctypes.cast(base + off, ctypes.POINTER(ctypes.c_uint8))[0]

    y, cb, cr = yuv420_views(packed, w, h)
    assert y.data_ptr() == packed.data_ptr() and cb.data_ptr() == packed.data_ptr() + w * h      # views, not copies
    nv = torch.stack([cb, cr], dim=-1).contiguous()                                                # [n,ch,cw,2]
    descs = [Context._yuv420(packed, (w, h)), Context._yuv420((y, cb, cr), None), Context._yuv420((y, nv[..., 0], nv[..., 1]), None)]
    assert [d[0].c_pixel_stride for d in descs] == [1, 1, 2] and all(d[1:] == (n, w, h) for d in descs)
    for d, _, _, _ in descs:
        for f in range(n):
            assert sample(d, "y", f, h - 1, w - 1) == int(y[f, h - 1, w - 1])
            assert sample(d, "cb", f, ch - 1, cw - 1) == int(cb[f, ch - 1, cw - 1])
            assert sample(d, "cr", f, 1, 2) == int(cr[f, 1, 2])
    with pytest.raises(ValueError):
        Context._yuv420(packed, None)
    with pytest.raises(ValueError):
        Context._yuv420((y, cb, cr[:, :, :cw - 1]), None)


class _PlaneCap:
    """Planes whose every byte names the frame (and the plane), so that staged bytes can be checked; counts its reads."""
    bgr_mode = capture.BGR_SWSCALE_X86

    def __init__(self, n, w, h, refuse=False):
        self.n, self.i, self.width, self.height, self.refuse = n, 0, w, h, refuse
        self.bgr_reads, self.plane_reads = [], []

    def _planes(self, i):
        ch, cw = (self.height + 1) // 2, (self.width + 1) // 2
        return (np.full((self.height, self.width), i, np.uint8), np.full((ch, cw), 100 + i, np.uint8),
                np.full((ch, cw), 200 + i, np.uint8))

    def read(self):
        if self.i >= self.n:
            return False, None
        self.bgr_reads.append(self.i)
        f = synthetic.yuv420_to_bgr_host(*self._planes(self.i))
        f[0, 0, 0] = self.i                     # the scripted context identifies a BGR frame by this byte
        self.i += 1
        return True, f

    def read_yuv420_into(self, y, cb, cr):
        if self.refuse:
            raise capture.CaptureError("libevcap: odd crop offset")       # before a frame is consumed
        if self.i >= self.n:
            return False
        self.plane_reads.append(self.i)
        py, pcb, pcr = self._planes(self.i)
        y[...] = py; cb[...] = pcb; cr[...] = pcr
        self.i += 1
        return True


class _BgrOnlyCap:
    def __init__(self, inner):
        self.inner = inner

    def read(self):
        return self.inner.read()


class _FakeCtx:
    """Scripted context with the device kernel's stream semantics (tests/test_host_glue.py), both sources."""

    def __init__(self, plan, w, h):
        self.plan, self.prev, self.w, self.h = plan, None, w, h
        self.bgr_calls, self.yuv_calls, self.types_calls, self.staged = [], [], 0, []

    def _play(self, ids, H, st):
        import torch
        for k in range(1, len(ids)):
            r = self.plan[str(ids[k])]
            if isinstance(r, str):
                st[k - 1] = 2
                H[k - 1] = float("nan") if self.prev is None else self.prev
            else:
                st[k - 1] = 0
                self.prev = torch.tensor(r, dtype=torch.float64).reshape(9)
                H[k - 1] = self.prev

    def stream_homography_batch(self, frames, H, st, state_in=None, **kw):
        ids = frames[:, 0, 0, 0].tolist()
        self.bgr_calls.append((ids, state_in is not None))
        self._play(ids, H, st)

    def stream_homography_batch_types(self, frames, H, st, features, **kw):
        self.types_calls += 1
        self.stream_homography_batch(frames, H, st, **kw)

    def stream_homography_batch_yuv420(self, planes, size, H, st, state_in=None, resize_to=None, **kw):
        from evenvizion_amd._lib import yuv420_size
        assert tuple(size) == (self.w, self.h) and planes.shape[1] == yuv420_size(self.w, self.h)[0]
        ids = planes[:, 0].tolist()
        self.yuv_calls.append((ids, state_in is not None))
        self.staged.append(planes.clone().numpy())
        self._play(ids, H, st)

    def stream_homography_batch_types_yuv420(self, planes, size, H, st, features, **kw):
        self.types_calls += 1
        self.stream_homography_batch_yuv420(planes, size, H, st, **kw)

    def synchronize(self):
        pass


def _plan(n):
    rng = np.random.default_rng(5)
    plan = {}
    for i in range(1, n):
        plan[str(i)] = "nomatch" if i in (4, 9) else (np.eye(3) + rng.normal(0, 1e-2, (3, 3))).tolist()
    return plan


@pytest.mark.parametrize("chunk", [2, 3, 5, 64])
@pytest.mark.parametrize("size", [(13, 7), (12, 6)])
def test_driver_plane_path(monkeypatch, chunk, size):
    import torch
    from evenvizion_amd._lib import yuv420_size
    w, h = size
    n = 11
    fb, cw, ch = yuv420_size(w, h)
    assert fb == w * h + 2 * cw * ch
    monkeypatch.setattr(runtime, "device", lambda: torch.device("cpu"))
    plan = _plan(n)

    def run(cap, **kw):
        runtime.release_staging()
        fake = _FakeCtx(plan, w, h)
        monkeypatch.setattr(runtime, "get_context", lambda *a, **k: fake)
        res = video_processing.get_homography_dict(cap, resize_width=w, chunk_frames=chunk, **kw)
        return res, fake

    want, f_bgr = run(_PlaneCap(n, w, h), features_type_list=["ORB"], ingest="bgr")
    assert f_bgr.bgr_calls and not f_bgr.yuv_calls
    assert sorted(k for k in want if k != "resize_info") == list(range(2, n + 1)) and want["resize_info"] == {"h": h, "w": w}

    cap = _PlaneCap(n, w, h)
    got, fake = run(cap, features_type_list=["ORB"], ingest="auto")
    assert fake.yuv_calls and not fake.bgr_calls and fake.types_calls == 0
    assert cap.plane_reads == list(range(n)) and cap.bgr_reads == []
    assert list(got.keys()) == list(want.keys()) and got == want     # the same dictionary, key for key
    assert [s for _, s in fake.yuv_calls] == [False] + [True] * (len(fake.yuv_calls) - 1)
    # every staged frame holds w*h + 2*cw*ch bytes: Y, then Cb, then Cr of the frame its first byte names
    for (ids, _), staged in zip(fake.yuv_calls, fake.staged):
        assert staged.shape == (len(ids), fb)
        for row, i in zip(staged, ids):
            assert (row[:w * h] == i).all() and (row[w * h:w * h + cw * ch] == 100 + i).all() and (row[w * h + cw * ch:] == 200 + i).all()
    # the last frame of a chunk is the first of the next, byte for byte; together the chunks hold every frame once more
    for a, b in zip(fake.staged, fake.staged[1:]):
        assert np.array_equal(a[-1], b[0])
    assert [i for ids, _ in fake.yuv_calls for i in ids[1:]] == list(range(1, n))

    got, fake = run(_PlaneCap(n, w, h), features_type_list=["ORB"], ingest="yuv420")
    assert fake.yuv_calls and got == want
    got, fake = run(_PlaneCap(n, w, h), ingest="auto")               # the default three-detector list
    assert fake.types_calls == len(fake.yuv_calls) >= 1 and not fake.bgr_calls and got == want

    # captures that cannot (or must not) deliver planes take today's path and read every frame exactly once
    for make in (lambda: _BgrOnlyCap(_PlaneCap(n, w, h)), lambda: _PlaneCap(n, w, h, refuse=True),
                 lambda: _c_tables(_PlaneCap(n, w, h))):
        cap = make()
        got, fake = run(cap, features_type_list=["ORB"], ingest="auto")
        inner = getattr(cap, "inner", cap)
        assert fake.bgr_calls and not fake.yuv_calls and got == want
        assert inner.bgr_reads == list(range(n)) and inner.plane_reads == []
    for make in (lambda: _BgrOnlyCap(_PlaneCap(n, w, h)), lambda: _PlaneCap(n, w, h, refuse=True),
                 lambda: _c_tables(_PlaneCap(n, w, h))):
        with pytest.raises(ValueError):
            run(make(), features_type_list=["ORB"], ingest="yuv420")
    cap = _PlaneCap(n, w, h)                                         # without the keyword: today's path
    got, fake = run(cap, features_type_list=["ORB"])
    assert fake.bgr_calls and not fake.yuv_calls and got == want and cap.plane_reads == []
    with pytest.raises(ValueError):
        run(_PlaneCap(n, w, h), ingest="nv12")
    with pytest.raises(ValueError):
        run(_PlaneCap(0, w, h), features_type_list=["ORB"])          # no first frame
    runtime.release_staging()


def _c_tables(cap):
    cap.bgr_mode = capture.BGR_SWSCALE_C
    return cap


def test_synthetic_yuv_capture_reads_both_ways():
    rng = np.random.default_rng(3)
    gray, _ = synthetic.make_stream(4, 3, 66, 35)
    planes = [(g,) + synthetic.chroma_for(rng, g) for g in gray]
    assert planes[0][1].shape == (18, 33) and len(np.unique(planes[0][1])) > 1
    a, b = synthetic.SyntheticYuvCapture(planes), synthetic.SyntheticYuvCapture(planes)
    assert (a.width, a.height, a.bgr_mode) == (66, 35, capture.BGR_SWSCALE_X86)
    y = np.empty((35, 66), np.uint8); cb = np.empty((18, 33), np.uint8); cr = np.empty_like(cb)
    for k in range(3):
        ok, f = a.read()
        assert ok and b.read_yuv420_into(y, cb, cr) is True
        assert np.array_equal(f, synthetic.yuv420_to_bgr_host(y, cb, cr)) and np.array_equal(y, gray[k])
    assert a.read() == (False, None) and b.read_yuv420_into(y, cb, cr) is False
    # the statement itself at the corners of the input cube (values worked out by hand from the integer form)
    one = lambda yy, u, v: synthetic.yuv420_to_bgr_host(np.full((1, 1), yy, np.uint8), np.full((1, 1), u, np.uint8),
                                                         np.full((1, 1), v, np.uint8))[0, 0].tolist()
    assert one(16, 128, 128) == [0, 0, 0] and one(235, 128, 128) == [255, 255, 255]
    assert one(0, 0, 0) == [0, 135, 0] and one(255, 255, 255) == [255, 124, 255]
