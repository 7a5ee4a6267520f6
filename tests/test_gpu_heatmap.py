"""evh_heatmap_render and heatmap.heatmap_frames on the device.  Every assertion is equality of bytes with the numpy restatement
of the header's arithmetic (tests/heatmap_checks.py, itself checked against the reference's expression in test_heatmap_host.py);
the fields it starts from are the reference-captured ones of plane_goldens.json or the CPU oracle's."""
import json
import os

import numpy as np
import pytest

import heatmap_checks as HC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MP4 = os.path.join(ROOT, "tests", "golden", "ref_test_video.mp4")
GOLD = os.path.join(ROOT, "tests", "golden", "ref_dict_with_homography_matrix.json")
SENTINEL = 0xCD
GRIDS = [(1, 1), (1, 37), (37, 1), (17, 9), (65, 5)]


@pytest.fixture(scope="module")
def ctx():
    from evenvizion_amd._lib import Context
    c = Context(device=0, max_w=64, max_h=64, max_features=500, max_frames=2)     # the entry does not depend on these sizes
    yield c
    c.close()


@pytest.fixture(scope="module")
def plane():
    with open(os.path.join(ROOT, "tests", "golden", "plane_goldens.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def jet():
    from evenvizion_amd.heatmap import jet_lut
    return jet_lut()


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
    """The recorded superposition of the reference video, heatmap_frames over the whole video from BGR frames (one decoding pass,
    which also keeps frames 1, 2, 3, 61 and 121), and those frames resized to the working size on the device."""
    import torch
    from evenvizion_amd import capture, heatmap
    from evenvizion_amd.processing.utils import read_homography_dict, superposition_dict
    hd, ri = read_homography_dict(GOLD)
    sup = superposition_dict(hd)
    rec = Recording(capture.VideoCapture(MP4), (1, 2, 3, 61, 121))
    pictures = list(heatmap.heatmap_frames(rec, sup, ri, chunk_frames=50, ingest="bgr"))
    nos = sorted(rec.kept)
    assert nos == [1, 2, 3, 61, 121]
    small = torch.zeros((len(nos), ri["h"], ri["w"], 3), dtype=torch.uint8, device="cuda")
    ctx.resize_area(torch.from_numpy(np.stack([rec.kept[k] for k in nos])).cuda(), small)
    ctx.synchronize()
    small = small.cpu().numpy()
    return sup, ri, {no: small[i] for i, no in enumerate(nos)}, pictures


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def strided(n, h, w, row_stride, frame_stride, offset, content=None):
    """A [n,h,w,3] view with the given byte strides, `offset` bytes into a buffer of SENTINEL -> (buffer, view, the buffer
    positions of the view's bytes)."""
    import torch
    at = (offset + np.arange(n, dtype=np.int64)[:, None, None] * frame_stride + np.arange(h, dtype=np.int64)[None, :, None] * row_stride
          + np.arange(3 * w, dtype=np.int64)[None, None, :])
    buf = torch.full((int(at.max()) + 9,), SENTINEL, dtype=torch.uint8, device="cuda")
    view = buf.as_strided((n, h, w, 3), (frame_stride, row_stride, 3, 1), offset)
    if content is not None:
        view.copy_(dev(content))
    return buf, view, at.reshape(-1)


def run(ctx, Hs, w, h, lut, frames=None, out_layout=None, frame_layout=None, **kw):
    """Context.heatmap_render -> u8[n,h,w,3]; a layout is (row stride, frame stride, offset) in bytes, default tight.  Bytes of
    the output buffer outside the pictures' rows must keep SENTINEL."""
    Hs = np.asarray(Hs, np.float64).reshape(-1, 9)
    n = len(Hs)
    tight = (3 * w, 3 * w * h, 0)
    buf, out, at = strided(n, h, w, *(out_layout or tight))
    src = None
    if frames is not None:
        _, src, _ = strided(n, h, w, *(frame_layout or tight), content=frames)
    ctx.heatmap_render(dev(Hs), out, dev(lut), frames=src, **kw)
    ctx.synchronize()
    got = buf.cpu().numpy()
    gaps = np.ones(got.shape, bool)
    gaps[at] = False
    assert (got[gaps] == SENTINEL).all(), "bytes outside the picture rows were written"
    return got[at].reshape(n, h, w, 3)


def check(ctx, field, Hs, lut, frames=None, out_layout=None, frame_layout=None, **kw):
    field = np.asarray(field, np.float64)
    h, w = field.shape[-3:-1]
    want = HC.render(field, lut, frames, kw.get("heatmap_constant", 1000.0), kw.get("alpha", 0.8), kw.get("saturate", False))
    got = run(ctx, Hs, w, h, lut, frames, out_layout, frame_layout, **kw)
    print("%dx%d x%d %s: differing bytes %d of %d" % (w, h, len(want), kw, (got != want).sum(), want.size))
    assert np.array_equal(got, want)
    return got


def grid_cases(plane, w, h):
    cases = [c for c in plane["grids"] if (c["w"], c["h"]) == (w, h)]
    assert len(cases) == 9
    return np.array([c["H"] for c in cases]), np.array([c["field"] for c in cases]).reshape(9, h, w, 2)


def up4(v):
    return (v + 3) // 4 * 4


# ---- the reference-captured grids: all nine matrices of a grid in one call, over frames of random bytes ---------------------------
@pytest.mark.parametrize("w,h", GRIDS)
def test_golden_grids(ctx, plane, jet, w, h):
    Hs, field = grid_cases(plane, w, h)
    rng = np.random.default_rng(41 + w)
    frames = rng.integers(0, 256, (9, h, w, 3), dtype=np.uint8)
    other = rng.integers(0, 256, (256, 3), dtype=np.uint8)                    # a table that is not jet
    with np.errstate(all="ignore"):
        t = 255.0 * (np.sqrt(field[..., 0] ** 2 + field[..., 1] ** 2) / 1000.0)
    assert np.isnan(t).any() and np.isinf(t).any()
    if h > 1:
        assert (np.isfinite(t) & (t > 255)).any()                             # the wrap, and with saturate the hold at 255
    rs = up4(3 * w)
    word = (rs, rs * h, 0)                                                    # rows and frames on 4-byte boundaries
    for lut in (jet, other):
        for constant in (1000.0, 37.5):
            for saturate in (False, True):
                kw = dict(heatmap_constant=constant, saturate=saturate)
                check(ctx, field, Hs, lut, frames, **kw)                                          # alpha 0.8: the integer blend
                check(ctx, field, Hs, lut, frames, out_layout=word, frame_layout=word, **kw)      # stored and loaded as words
    for alpha in (0.0, 0.5, 1.0, 2.5, 0.8000000000000002, 1e300):                                 # the float64 blend
        check(ctx, field, Hs, other, frames, alpha=alpha)
        check(ctx, field, Hs, other, frames, out_layout=word, alpha=alpha)
        check(ctx, field, Hs, other, None, alpha=alpha)                                           # no frames: the scaled table
    check(ctx, field, Hs, jet, None, out_layout=word, saturate=True)


def test_saturate_differs_from_the_wrap_where_t_exceeds_255(ctx, plane, jet):
    Hs, field = grid_cases(plane, 65, 5)
    wrap = check(ctx, field, Hs, jet, None, alpha=1.0, saturate=False)
    sat = check(ctx, field, Hs, jet, None, alpha=1.0, saturate=True)
    with np.errstate(all="ignore"):
        t = 255.0 * (np.sqrt(field[..., 0] ** 2 + field[..., 1] ** 2) / 1000.0)
    over = t >= 255
    assert over.any() and (sat[over] == jet[255]).all() and (sat[~over] == wrap[~over]).all()
    assert (wrap[over] != sat[over]).any()


# ---- rows on odd strides from an odd address: every store bytewise; nothing between the rows is touched --------------------------
@pytest.mark.parametrize("w,h", [(17, 9), (65, 5), (8, 4)])
def test_odd_strides_and_an_odd_base(ctx, plane, jet, w, h):
    if (w, h) == (8, 4):
        Hs = np.array([[1, 0.25, 3, -0.5, 1, 2, 1e-3, 2e-3, 1], [40, 0, 0, 0, 40, 0, 0, 0, 1]], np.float64)
        field = HC.oracle_field(Hs, w, h)
    else:
        Hs, field = grid_cases(plane, w, h)
    n = len(Hs)
    frames = np.random.default_rng(43).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    rs = 3 * w + 2 if (3 * w) % 2 else 3 * w + 1
    assert rs % 2 == 1
    fs = rs * h + 5
    check(ctx, field, Hs, jet, frames, out_layout=(rs, fs, 1), frame_layout=(rs + 2, (rs + 2) * h + 1, 3))
    check(ctx, field, Hs, jet, frames, out_layout=(rs, fs, 1), alpha=0.5)
    check(ctx, field, Hs, jet, frames, out_layout=(up4(3 * w), up4(3 * w) * h, 2))        # aligned strides, unaligned base
    check(ctx, field, Hs, jet, frames, frame_layout=(up4(3 * w), up4(3 * w) * h, 1), out_layout=(up4(3 * w), up4(3 * w) * h, 0))


# ---- the reference video's working size ------------------------------------------------------------------------------------------------
def test_three_matrices_of_the_reference_video(ctx, plane, jet, video):
    _, ri, small, _ = video
    w, h = ri["w"], ri["h"]
    assert (w, h) == (400, 224)
    fr = plane["video"]["frames"]
    assert [fr[k]["frame"] for k in (0, 59, 120)] == [1, 60, 121]
    Hs = np.array([fr[k]["H"] for k in (0, 59, 120)], np.float64).reshape(3, 9)
    field = HC.oracle_field(Hs, w, h)
    frames = np.stack([small[1], small[2], small[3]])
    got = check(ctx, field, Hs, jet, frames)
    assert len(np.unique(HC.color_index(field))) > 100                        # the pictures are not one colour
    check(ctx, field, Hs, jet, frames, alpha=0.7)
    check(ctx, field, Hs, jet, frames, saturate=True, heatmap_constant=37.5)
    # no frames and alpha = 1: the table itself
    bare = check(ctx, field, Hs, jet, None, alpha=1.0)
    assert np.array_equal(bare, jet[HC.color_index(field)])
    assert not np.array_equal(bare, got)


# ---- offsets beyond 2^31 ---------------------------------------------------------------------------------------------------------------
def test_frame_strides_beyond_two_gib(ctx, jet):
    import torch
    n, w, h = 2, 8, 4
    stride = 2 ** 31 + 4
    Hs = np.array([[1, 0.25, 3, -0.5, 1, 2, 1e-3, 2e-3, 1], [40, 0, 0, 0, 40, 0, 0, 0, 1]], np.float64)
    field = HC.oracle_field(Hs, w, h)
    frames = np.random.default_rng(44).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    want = HC.render(field, jet, frames)
    assert len(np.unique(HC.color_index(field)[1])) > 4
    src = torch.zeros(stride + 3 * w * h, dtype=torch.uint8, device="cuda")
    out = torch.full((stride + 3 * w * h,), SENTINEL, dtype=torch.uint8, device="cuda")
    shape, strides = (n, h, w, 3), (stride, 3 * w, 3, 1)
    src.as_strided(shape, strides).copy_(dev(frames))
    ctx.heatmap_render(dev(Hs), out.as_strided(shape, strides), dev(jet), frames=src.as_strided(shape, strides))
    ctx.synchronize()
    assert np.array_equal(out.as_strided(shape, strides).cpu().numpy(), want)
    assert (out[3 * w * h:3 * w * h + 4096] == SENTINEL).all() and (out[stride - 4096:stride] == SENTINEL).all()
    assert int((out != SENTINEL).sum()) == int((want != SENTINEL).sum())      # nothing else was written
    del src, out
    torch.cuda.empty_cache()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_alone(ctx, jet):
    import torch
    INVALID, CAPACITY = -1, -3
    n, w, h = 2, 23, 17
    rs, fs = 3 * w, 3 * w * h
    src = dev(np.random.default_rng(45).integers(0, 256, (n, h, w, 3), dtype=np.uint8))
    mats = dev(np.tile(np.eye(3).reshape(1, 9), (n, 1)))
    lut = dev(jet)
    out = torch.full((n + 1, h, w, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    f, m, t, o = src.data_ptr(), mats.data_ptr(), lut.data_ptr(), out.data_ptr()
    good = dict(ctx=ctx.h, H=m, n=n, w=w, h=h, frames=f, rs=rs, fs=fs, lut=t, const=1000.0, alpha=0.8, sat=0, out=o, ors=rs, ofs=fs)

    def call(**kw):
        a = dict(good, **kw)
        return ctx.lib.evh_heatmap_render(a["ctx"], a["H"], a["n"], a["w"], a["h"], a["frames"], a["rs"], a["fs"], a["lut"], a["const"],
                                          a["alpha"], a["sat"], a["out"], a["ors"], a["ofs"])

    nan, inf = float("nan"), float("inf")
    who = "evh_heatmap_render: "
    NA, EM, SR, SF = "NULL argument", "empty grid or negative n", "stride smaller than a row", "stride smaller than a frame"
    HCON, AL = "heatmap_constant must be finite and positive", "alpha must be finite and not negative"
    NM, AREA, OV = "at most 65535 matrices per call", "w * h above INT_MAX", "d_frames overlaps d_out"

    def refused(rc, code, text, what):
        assert rc == code, what
        assert ctx.lib.evh_last_error_string(ctx.h).decode() == text, what

    assert call(ctx=None) == INVALID
    invalid = [(dict(H=None), NA), (dict(lut=None), NA), (dict(out=None), NA), (dict(w=0), EM), (dict(h=0), EM), (dict(w=-3), EM),
               (dict(n=-1), EM), (dict(rs=rs - 1), SR), (dict(fs=fs - 1), SF), (dict(ors=rs - 1), SR), (dict(ofs=fs - 1), SF),
               (dict(frames=None, ors=rs - 1), SR), (dict(const=0.0), HCON), (dict(const=-1.0), HCON), (dict(const=nan), HCON),
               (dict(const=inf), HCON), (dict(const=-inf), HCON), (dict(alpha=-0.5), AL), (dict(alpha=nan), AL), (dict(alpha=inf), AL),
               (dict(alpha=-inf), AL), (dict(frames=o), OV), (dict(frames=o + fs), OV), (dict(frames=o + 2 * fs - 1), OV),
               (dict(frames=o - 2 * fs + 1), OV), (dict(n=1, frames=o + fs - 1), OV),
               # two faults: the earlier check of the entry names the refusal
               (dict(H=None, w=0), NA), (dict(w=-3, alpha=nan), EM), (dict(const=0.0, n=65536), HCON), (dict(rs=rs - 1, fs=fs - 1), SR),
               (dict(frames=o, ofs=fs - 1), SF), (dict(frames=o, ors=rs - 1), SR)]
    for kw, text in invalid:
        refused(call(**kw), INVALID, who + text, kw)
    capacity = [(dict(n=65536), NM), (dict(w=65536, h=32768, rs=65536 * 3, ors=65536 * 3, fs=1 << 40, ofs=1 << 40), AREA),
                # two faults: a capacity refusal precedes the strides and the overlap, the matrices come before the grid
                (dict(n=65536, rs=rs - 1), NM), (dict(n=65536, frames=o), NM), (dict(n=65536, w=65536, h=32768), NM),
                (dict(w=65536, h=32768), AREA)]
    for kw, text in capacity:
        refused(call(**kw), CAPACITY, who + text, kw)
    assert call(n=0) == 0 and call(n=0, frames=None) == 0                    # no matrices: success, and nothing is done
    ctx.synchronize()
    assert (out == SENTINEL).all()
    # frames that end where the output begins do not overlap it, and the same arguments unrefused do write
    assert call(n=1, frames=o + fs, out=o) == 0 and call(n=1, frames=None, rs=0, fs=0, out=o + 2 * fs) == 0
    ctx.synchronize()
    assert (out[1] == SENTINEL).all()
    assert (out[0] != SENTINEL).any(dim=-1).all() and (out[2] != SENTINEL).any(dim=-1).all()


def test_wrapper_checks_its_tensors(ctx, jet):
    import torch
    out = torch.zeros((2, 4, 8, 3), dtype=torch.uint8, device="cuda")
    H = dev(np.tile(np.eye(3).reshape(1, 9), (2, 1)))
    with pytest.raises(ValueError):
        ctx.heatmap_render(H[:1], out, dev(jet))
    with pytest.raises(ValueError):
        ctx.heatmap_render(H.float(), out, dev(jet))
    with pytest.raises(ValueError):
        ctx.heatmap_render(H, out, dev(jet[:255]))
    with pytest.raises(ValueError):
        ctx.heatmap_render(H, out, dev(jet), frames=out[:, :, :4])
    with pytest.raises(ValueError):
        ctx.heatmap_render(H, out.cpu(), dev(jet))


# ---- heatmap_frames over the reference video -----------------------------------------------------------------------------------------
def test_heatmap_frames_over_the_reference_video(video, jet):
    from evenvizion_amd import capture, heatmap
    sup, ri, small, bgr = video
    auto = list(heatmap.heatmap_frames(capture.VideoCapture(MP4), sup, ri, ingest="auto"))        # planes, chunks of 32
    assert [k for k, _ in auto] == list(sup.keys()) == list(range(1, 122)) == [k for k, _ in bgr]
    for (_, a), (_, b) in zip(auto, bgr):
        assert a.shape == (ri["h"], ri["w"], 3) and a.dtype == np.uint8 and np.array_equal(a, b)
    for no in (1, 61, 121):
        field = HC.oracle_field(np.asarray(sup[no], np.float64), ri["w"], ri["h"])
        want = HC.render(field, jet, small[no][None])[0]
        print("picture %d: differing bytes %d" % (no, (auto[no - 1][1] != want).sum()))
        assert np.array_equal(auto[no - 1][1], want), no


def test_heatmap_frames_pairs_in_dictionary_order_and_ends_with_the_shorter(video, jet):
    from evenvizion_amd import capture, heatmap
    sup, ri, small, _ = video
    other = np.random.default_rng(46).integers(0, 256, (256, 3), dtype=np.uint8)
    # three entries in an order of their own, one without a matrix, one not finite: the first three frames go under them
    odd = {61: sup[61], 7: None, 5: np.full((3, 3), np.nan)}
    got = list(heatmap.heatmap_frames(capture.VideoCapture(MP4), odd, ri, lut=other, alpha=0.5, chunk_frames=2))
    assert [k for k, _ in got] == [61, 7, 5]
    field = HC.oracle_field(np.asarray(sup[61], np.float64), ri["w"], ri["h"])
    assert np.array_equal(got[0][1], HC.render(field, other, small[1][None], alpha=0.5)[0])
    for i, no in ((1, 2), (2, 3)):                                            # index 0 everywhere: the frame plus alpha * entry 0
        assert np.array_equal(got[i][1], HC.blend(np.broadcast_to(other[0], small[no].shape), small[no], 0.5))

    class Two:
        def __init__(self):
            self.cap, self.left = capture.VideoCapture(MP4), 2
            self.width, self.height, self.bgr_mode = self.cap.width, self.cap.height, self.cap.bgr_mode

        def read(self):
            self.left -= 1
            return self.cap.read() if self.left >= 0 else (False, None)

    assert [k for k, _ in heatmap.heatmap_frames(Two(), sup, ri, ingest="bgr")] == [1, 2]
    assert list(heatmap.heatmap_frames(capture.VideoCapture(MP4), {}, ri)) == []


# ---- python -m evenvizion_amd.component --heatmap_pictures ---------------------------------------------------------------------------
def test_component_writes_the_pictures_only_on_request(tmp_path, monkeypatch, jet):
    from evenvizion_amd import capture, component, heatmap, synthetic
    from evenvizion_amd.processing.utils import read_homography_dict, superposition_dict
    monkeypatch.chdir(tmp_path)
    spec = "synthetic:4:400x224:3"
    base = ["--path_to_video", spec, "--features", "ORB"]
    plain = component.main(base + ["--experiment_name", "plain"])
    assert sorted(os.listdir(plain)) == ["dict_with_homography_matrix.json", "metrics_file.txt"]
    folder = component.main(base + ["--experiment_name", "pictures", "--heatmap_pictures", "1"])
    assert sorted(os.listdir(folder)) == ["dict_with_homography_matrix.json", "heatmap_visualization", "metrics_file.txt"]
    hd, ri = read_homography_dict(os.path.join(folder, "dict_with_homography_matrix.json"))
    sup = superposition_dict(hd)
    names = sorted(os.listdir(os.path.join(folder, "heatmap_visualization")))
    assert names == ["img%06d.ppm" % k for k in sup] and len(names) == 4
    want = dict(heatmap.heatmap_frames(component.open_capture(spec)[0], sup, ri))
    for k in sup:
        with open(os.path.join(folder, "heatmap_visualization", "img%06d.ppm" % k), "rb") as f:
            data = f.read()
        head = b"P6\n%d %d\n255\n" % (ri["w"], ri["h"])
        assert data.startswith(head) and len(data) == len(head) + 3 * ri["w"] * ri["h"]
        rgb = np.frombuffer(data[len(head):], np.uint8).reshape(ri["h"], ri["w"], 3)
        assert np.array_equal(rgb[:, :, ::-1], want[k])
