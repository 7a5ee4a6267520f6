"""Decoded 4:2:0 planes as the source of the device path.  Every assertion is equality of bytes: the BGR bytes are a pure
per-pixel function of (Y, Cb, Cr), so the new code is pinned by the numpy statement (synthetic.yuv420_to_bgr_host, itself
pinned to libevcap's read() in tests/test_yuv_ingest_host.py) and by the existing BGR device path on the same frames."""
import ctypes
import json
import os

import numpy as np
import pytest

from evenvizion_amd import capture, synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MP4 = os.path.join(ROOT, "tests", "golden", "ref_test_video.mp4")
GOLD = os.path.join(ROOT, "tests", "golden", "ref_dict_with_homography_matrix.json")


@pytest.fixture(scope="module")
def ctx():
    from evenvizion_amd._lib import Context
    c = Context(device=0, max_w=1280, max_h=720, max_features=500, max_frames=2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def video():
    """(planes [121] of (y, cb, cr), BGR frames [121]) of the reference video, from two captures of the file."""
    a, b = capture.VideoCapture(MP4), capture.VideoCapture(MP4)
    planes, frames = [], []
    while True:
        ok, f = a.read()
        ok2, p = b.read_yuv420()
        assert ok == ok2
        if not ok:
            break
        frames.append(f); planes.append(p)
    assert len(frames) == 121
    return planes, frames


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pack(planes):
    """list of (y, cb, cr) -> uint8 [n, w*h + 2*cw*ch] packed I420"""
    return np.stack([np.concatenate([p.reshape(-1) for p in t]) for t in planes])


def nv12(cb, cr):
    """CUDA chroma planes [n,ch,cw] -> the (Cb, Cr) views of one interleaved [n,ch,cw,2] tensor"""
    import torch
    uv = torch.stack([cb, cr], dim=-1).contiguous()
    return uv[..., 0], uv[..., 1]


def test_converter_on_the_whole_input_cube(ctx):
    """All 256^3 (y, u, v) triples: chroma sample s of a 2048 x 2048 plane holds pair s // 64, and the four luma pixels of
    sample s take the luma values 4 * (s % 64) .. + 3.  I420 and NV12 presentations give the same bytes."""
    import torch
    s = np.arange(2048 * 2048, dtype=np.int64).reshape(2048, 2048)
    cb = (s // 64 >> 8).astype(np.uint8)
    cr = (s // 64 & 255).astype(np.uint8)
    y = np.empty((4096, 4096), np.uint8)
    k4 = (s % 64 * 4).astype(np.uint8)
    y[0::2, 0::2] = k4; y[0::2, 1::2] = k4 + 1; y[1::2, 0::2] = k4 + 2; y[1::2, 1::2] = k4 + 3
    # every triple occurs: 65 536 pairs x 256 luma values, counted
    code = (np.repeat(np.repeat(cb, 2, 0), 2, 1).astype(np.int64) << 16) | (np.repeat(np.repeat(cr, 2, 0), 2, 1).astype(np.int64) << 8) | y
    assert len(np.unique(code)) == 1 << 24
    want = synthetic.yuv420_to_bgr_host(y, cb, cr)
    dy, dcb, dcr = dev(y[None]), dev(cb[None]), dev(cr[None])
    out = torch.zeros((1, 4096, 4096, 3), dtype=torch.uint8, device="cuda")
    ctx.yuv420_to_bgr((dy, dcb, dcr), out)
    ctx.synchronize()
    got = out.cpu().numpy()[0]
    print("cube, I420: differing bytes %d of %d" % ((got != want).sum(), want.size))
    assert np.array_equal(got, want)
    out.zero_()
    ctx.yuv420_to_bgr((dy,) + nv12(dcb, dcr), out)
    ctx.synchronize()
    assert np.array_equal(out.cpu().numpy()[0], want)
    out.zero_()
    vu = nv12(dcr, dcb)                                    # NV21: Cr first
    ctx.yuv420_to_bgr((dy, vu[1], vu[0]), out)
    ctx.synchronize()
    assert np.array_equal(out.cpu().numpy()[0], want)


def test_converter_on_the_reference_video(ctx, video):
    import torch
    planes, frames = video
    h, w = frames[0].shape[:2]
    out = torch.zeros((len(frames), h, w, 3), dtype=torch.uint8, device="cuda")
    ctx.yuv420_to_bgr(dev(pack(planes)), out, size=(w, h))
    ctx.synchronize()
    got = out.cpu().numpy()
    differing = int(sum((got[i] != frames[i]).sum() for i in range(len(frames))))
    print("video: frames %d, differing bytes %d" % (len(frames), differing))
    assert differing == 0


@pytest.mark.parametrize("w,h", [(333, 217), (1, 1), (1, 6), (6, 1), (2, 2), (16, 2), (17, 3), (48, 5), (64, 4)])
@pytest.mark.parametrize("pad", [(16, 8, 16), (13, 7, 5)])      # (luma, chroma, output-pixel) padding: aligned and not
def test_converter_odd_sizes_and_padded_rows(ctx, w, h, pad):
    """Row strides larger than the width, non-zero bytes in the padding: the padding is not read into the result, and the
    output's own padding is not written."""
    import torch
    rng = np.random.default_rng(1000 * w + h)
    n, cw, ch = 3, (w + 1) // 2, (h + 1) // 2
    # strides: a multiple of 16 (8) that holds the row, or the row plus an odd pad
    ys = -(-w // 16) * 16 + 16 if pad[0] == 16 else w + pad[0]
    cs = -(-cw // 8) * 8 + 8 if pad[1] == 8 else cw + pad[1]
    ow = -(-w // 16) * 16 + 16 if pad[2] == 16 else w + pad[2]
    Y = rng.integers(0, 256, (n, h + 1, ys), dtype=np.uint8)
    CB = rng.integers(0, 256, (n, ch + 1, cs), dtype=np.uint8)
    CR = rng.integers(0, 256, (n, ch + 1, cs), dtype=np.uint8)
    dY, dCB, dCR = dev(Y), dev(CB), dev(CR)
    out = torch.full((n, h + 1, ow, 3), 0xCD, dtype=torch.uint8, device="cuda")
    for present in ("planar", "nv12"):
        out.fill_(0xCD)
        cbv, crv = dCB[:, :ch, :cw], dCR[:, :ch, :cw]
        if present == "nv12":
            uv = torch.stack([dCB, dCR], dim=-1).contiguous()           # padded interleaved rows
            cbv, crv = uv[:, :ch, :cw, 0], uv[:, :ch, :cw, 1]
        ctx.yuv420_to_bgr((dY[:, :h, :w], cbv, crv), out[:, :h, :w])
        ctx.synchronize()
        got = out.cpu().numpy()
        for i in range(n):
            want = synthetic.yuv420_to_bgr_host(Y[i, :h, :w], CB[i, :ch, :cw], CR[i, :ch, :cw])
            assert np.array_equal(got[i, :h, :w], want), (present, i)
        assert (got[:, :h, w:] == 0xCD).all() and (got[:, h:] == 0xCD).all(), present


def random_planes(seed, n, w, h):
    """Textured luma (a synthetic stream) with chroma drawn per sample: any error in the chroma indexing shows."""
    rng = np.random.default_rng(seed)
    gray, _ = synthetic.make_stream(seed, n, w, h)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    return [(gray[i], rng.integers(0, 256, (ch, cw), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8))
            for i in range(n)]


def detect_results(ctx, n):
    ctx.synchronize()
    return [(ctx.download_level(f, 0), ctx.download_level(f, 1), ctx.orb_download(f)) for f in range(n)]


GEOMETRIES = [("video", (1170, 658), (400, 224)),        # the reference's geometry: float tables
              ("random", (1280, 720), (640, 360)),       # integer ratio 2: the (sum + 2) >> 2 case
              ("random", (1280, 720), (320, 180)),       # integer ratio 4
              ("random", (1280, 720), (1280, 720)),      # no resize
              ("random", (320, 180), (400, 225)),        # enlargement
              ("random", (1171, 659), (400, 225)),       # odd source size
              ("random", (333, 217), (333, 217))]        # odd size, no resize (bytewise rows of the converter)


@pytest.mark.parametrize("kind,src,dst", GEOMETRIES)
@pytest.mark.parametrize("present", ["i420", "nv12"])
def test_fused_ingest_equals_the_bgr_ingest(ctx, video, kind, src, dst, present):
    """Levels 0 and 1 and the key points, responses, angles and descriptors, in order, after orb_detect_batch_yuv420 ==
    after orb_detect_batch(resize_to=) on the BGR frames capture.read() / yuv420_to_bgr_host gives for the same planes."""
    n = 2
    (w, h), (dw, dh) = src, dst
    from evenvizion_amd.processing.video_processing import resized_shape
    assert resized_shape((h, w), dw) == (dw, dh)
    if kind == "video":
        planes, frames = video[0][40:40 + n], video[1][40:40 + n]
        assert len(np.unique(planes[0][1])) > 8           # real chroma
    else:
        planes = random_planes(7 * w + dw, n, w, h)
        frames = [synthetic.yuv420_to_bgr_host(*p) for p in planes]
    ctx.orb_detect_batch(dev(np.stack(frames)), resize_to=(dw, dh))
    want = detect_results(ctx, n)
    assert all(len(r[2]["xy"]) > 50 for r in want)
    # The plane call must not find its answer already in the context: detect other frames of the same geometry (the same
    # frames with every byte inverted) in between, so that a pixel, key point or descriptor it fails to write stays wrong.
    ctx.orb_detect_batch(dev(255 - np.stack(frames)), resize_to=(dw, dh))
    dirty = detect_results(ctx, n)
    assert all((dirty[f][0] != want[f][0]).mean() > 0.5 and (dirty[f][1] != want[f][1]).mean() > 0.5 for f in range(n))
    if present == "i420":
        ctx.orb_detect_batch_yuv420(dev(pack(planes)), size=(w, h), resize_to=(dw, dh))
    else:
        y, cb, cr = (dev(np.stack([p[k] for p in planes])) for k in range(3))
        ctx.orb_detect_batch_yuv420((y,) + nv12(cb, cr), resize_to=(dw, dh))
    got = detect_results(ctx, n)
    for f in range(n):
        assert np.array_equal(got[f][0], want[f][0]), "level 0 of frame %d" % f
        assert np.array_equal(got[f][1], want[f][1]), "level 1 of frame %d" % f
        assert sorted(got[f][2]) == sorted(want[f][2])
        for key in want[f][2]:
            assert np.array_equal(got[f][2][key], want[f][2][key]), (f, key)


@pytest.mark.parametrize("features", [["ORB"], None])
def test_streams_equal_the_bgr_path_and_the_reference(monkeypatch, features):
    """get_homography_dict on the reference video through planes == through BGR frames, exactly, with chunk boundaries inside
    the video; with the reference's default detector list also == its recorded JSON under the bounds of
    tests/test_gpu_order.py::test_reference_video_end_to_end.  The plane entry is counted: a silent fall-back cannot pass."""
    from evenvizion_amd import _lib
    from evenvizion_amd.processing import get_homography_dict
    calls = {"yuv": 0, "types_yuv": 0}
    for key, name in (("yuv", "stream_homography_batch_yuv420"), ("types_yuv", "stream_homography_batch_types_yuv420")):
        inner = getattr(_lib.Context, name)

        def counted(self, *a, _inner=inner, _key=key, **kw):
            calls[_key] += 1
            return _inner(self, *a, **kw)
        monkeypatch.setattr(_lib.Context, name, counted)
    kw = dict(resize_width=400, chunk_frames=17, features_type_list=features)
    via_bgr = get_homography_dict(capture.VideoCapture(MP4), ingest="bgr", **kw)
    assert calls == {"yuv": 0, "types_yuv": 0}
    via_yuv = get_homography_dict(capture.VideoCapture(MP4), ingest="yuv420", **kw)
    assert calls["yuv" if features == ["ORB"] else "types_yuv"] == 8 and sum(calls.values()) == 8       # ceil(120 / 16) chunks
    assert list(via_yuv.keys()) == list(via_bgr.keys()) == list(range(2, 122)) + ["resize_info"]
    assert via_yuv["resize_info"] == via_bgr["resize_info"] == {"h": 224, "w": 400}
    Hy = np.array([via_yuv[k]["H"] for k in range(2, 122)])
    Hb = np.array([via_bgr[k]["H"] for k in range(2, 122)])
    assert np.array_equal(Hy.view(np.uint64), Hb.view(np.uint64))            # bit for bit
    via_auto = get_homography_dict(capture.VideoCapture(MP4), ingest="auto", **kw)
    assert sum(calls.values()) == 16 and via_auto == via_yuv
    if features is None:
        gold = json.load(open(GOLD))
        G = np.array([gold[str(k)]["H"] for k in range(2, 122)])
        tau = np.array([[1e-3, 1e-3, 1.0], [1e-3, 1e-3, 1.0], [1e-6, 1e-6, 1.0]])
        rel = np.array([(np.abs(Hy[k] - G[k]) / np.maximum(np.abs(G[k]), tau)).max() for k in range(120)])
        exact = int((np.abs(Hy - G).reshape(120, -1).max(1) == 0).sum())
        print("planes vs the reference's recorded run: max rel %.2e, pairs equal to the last digit %d of 120" % (rel.max(), exact))
        assert rel.max() <= 1e-3 and rel.max() <= 1e-6 and exact >= 100


def test_refusals_leave_the_context_usable(ctx):
    """Bad descriptions are refused on the host side of the ABI with a status and a message; nothing is launched on them."""
    import torch
    from evenvizion_amd._lib import Yuv420, EvhError
    w, h = 64, 32
    planes = random_planes(3, 1, w, h)
    packed = dev(pack(planes))
    out = torch.zeros((1, h, w, 3), dtype=torch.uint8, device="cuda")
    good, n, _, _ = ctx._yuv420(packed, (w, h))

    def variant(**kw):
        d = Yuv420.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    lib = ctx.lib
    H = torch.zeros((1, 9), dtype=torch.float64, device="cuda"); st = torch.zeros(1, dtype=torch.int32, device="cuda")
    for bad, word in ((variant(c_pixel_stride=3), "pixel stride"), (variant(d_cr=None), "NULL"), (variant(d_y=None), "NULL"),
                      (variant(c_stride=w // 2 - 1), "chroma row stride"), (variant(y_stride=w - 1), "luma row stride"),
                      (variant(c_pixel_stride=0), "pixel stride")):
        for rc in (lib.evh_yuv420_to_bgr(ctx.h, ctypes.byref(bad), 1, w, h, out.data_ptr(), 3 * w, 3 * w * h),
                   lib.evh_orb_detect_batch_yuv420(ctx.h, ctypes.byref(bad), 1, w, h, w, h, 500),
                   lib.evh_stream_homography_batch_yuv420(ctx.h, ctypes.byref(bad), 2, w, h, w, h, 500, 3.0, 2000, 0.995, 0, None,
                                                          None, H.data_ptr(), st.data_ptr())):
            assert rc < 0
            assert word in lib.evh_last_error_string(ctx.h).decode(), lib.evh_last_error_string(ctx.h)
    assert lib.evh_yuv420_to_bgr(ctx.h, None, 1, w, h, out.data_ptr(), 3 * w, 3 * w * h) < 0
    assert lib.evh_yuv420_to_bgr(ctx.h, ctypes.byref(good), 1, w, h, None, 3 * w, 3 * w * h) < 0
    assert lib.evh_yuv420_to_bgr(ctx.h, ctypes.byref(good), 1, w, h, out.data_ptr(), 3 * w - 1, 3 * w * h) < 0
    with pytest.raises(EvhError):
        ctx._check(lib.evh_yuv420_to_bgr(ctx.h, ctypes.byref(variant(c_pixel_stride=3)), 1, w, h, out.data_ptr(), 3 * w, 3 * w * h))
    # a valid call right after
    ctx.yuv420_to_bgr(packed, out, size=(w, h))
    ctx.synchronize()
    assert np.array_equal(out.cpu().numpy()[0], synthetic.yuv420_to_bgr_host(*planes[0]))
