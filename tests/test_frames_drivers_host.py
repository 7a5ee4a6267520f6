"""The host loops of the second-pass drivers against a recording context, no GPU: which frames every product call receives, in
which order, with which size=, with which matrices, and whether evh_yuv420_to_bgr, evh_resize_area_u8 and the gray expansion
ran.  Only public functions are driven, so the file passes on any layout of the loops behind them."""
import numpy as np
import pytest

import frames_checks as F
from evenvizion_amd import heatmap, moving, registration, runtime, stabilization
from evenvizion_amd.processing import video_processing

FULL, SMALL, PACKED = (F.H0, F.W0, 3), (4, 8, 3), (F.W0 * F.H0 * 3 // 2,)
FORMS = ("bgr", "planes")
WORK = ((F.W0, F.H0), (8, 4))          # the working size: the frames' own, and smaller


def _ids(frames):
    while frames.dim() > 1:
        frames = frames[:, 0]
    return [int(v) for v in frames]


def _shift(mats):
    return [float(v) for v in mats.reshape(-1, 9)[:, 2]]


class Recorder:
    """Stands in for libevhip: every call is noted as (name, frame positions, shape of a frame, ...) and leaves the position
    of each frame in the first byte of what it writes."""
    CAP = 100

    def __init__(self):
        self.calls, self.batch = [], None

    def of(self, *names):
        return [c for c in self.calls if c[0] in names]

    def order_torch_after(self):
        pass

    def synchronize(self):
        pass

    def yuv420_to_bgr(self, planes, out, size=None):
        self.calls.append(("yuv", _ids(planes), tuple(planes.shape[1:]), tuple(out.shape[1:]), tuple(size)))
        out.zero_()
        out[:, 0, 0, 0] = planes[:, 0]

    def resize_area(self, src, dst):
        self.calls.append(("resize", _ids(src), tuple(src.shape[1:]), tuple(dst.shape[1:])))
        dst.zero_()
        dst[:, 0, 0, 0] = src[:, 0, 0, 0]

    def warp_fixed_plane(self, frames, mats, out, mode, origin, background=None, size=None):
        import torch
        ids = _ids(frames)
        self.calls.append(("warp", ids, tuple(frames.shape[1:]), size, _shift(mats), mode))
        if out.dim() == 4:
            out.zero_()
            out[:, 0, 0, 0] = torch.tensor(ids, dtype=torch.uint8)
        else:
            out[0, 0, 0] = ids[-1]

    def trail_fixed_plane(self, frames, mats, canvas, origin, out=None, rects=None, size=None):
        import torch
        ids = _ids(frames)
        self.calls.append(("trail", ids, tuple(frames.shape[1:]), size, _shift(mats), rects is not None))
        out.zero_()
        out[:, 0, 0, 0] = torch.tensor(ids, dtype=torch.uint8)

    def plate_fixed_plane(self, frames, mats, plate, origin, count=None, masks=None, threshold=16, min_cover=1, size=None):
        self.calls.append(("plate", _ids(frames), tuple(frames.shape[1:]), size, _shift(mats)))
        plate.zero_()
        count.zero_()
        if masks is not None:
            masks.zero_()

    def heatmap_render(self, mats, out, lut, frames=None, heatmap_constant=1000.0, alpha=0.8, saturate=False):
        import torch
        ids = _ids(frames)
        self.calls.append(("heatmap", ids, tuple(frames.shape[1:]), None, _shift(mats)))
        out.zero_()
        out[:, 0, 0, 0] = torch.tensor(ids, dtype=torch.uint8)

    def pair_residual(self, frames, mats, stats=None, out=None, threshold=16, kind="abs"):
        import torch
        ids = _ids(frames)
        self.calls.append(("residual", ids, tuple(frames.shape[1:]), None))
        assert mats.shape == (len(ids) - 1, 9)
        stats.zero_()
        stats[:, 0] = torch.tensor(ids[1:], dtype=torch.int64)
        if out is not None:
            out.zero_()
            out[:, 0, 0] = torch.tensor(ids[1:], dtype=torch.uint8)

    def _batch(self, frames, size, H, st):
        self.batch = _ids(frames)
        self.calls.append(("batch", self.batch, tuple(frames.shape[1:]), size))
        H[:len(self.batch) - 1] = 0
        st[:len(self.batch) - 1] = 0

    def stream_homography_batch(self, frames, H, st, state_in=None, state_out=None, nfeatures=500, resize_to=None):
        self._batch(frames, None, H, st)

    def stream_homography_batch_yuv420(self, planes, size, H, st, state_in=None, state_out=None, nfeatures=500, resize_to=None):
        self._batch(planes, tuple(size), H, st)

    def batch_static_info(self):
        return len(self.batch) - 1, self.CAP

    def batch_static_rows(self, first_pair=0, npairs=None, rows=None, counts=None, status=None):
        import torch
        assert first_pair == 0 and npairs == len(self.batch) - 1
        if rows is None:
            rows, counts = torch.zeros((npairs, self.CAP, 4)), torch.zeros(npairs, dtype=torch.int32)
            status = torch.zeros(npairs, dtype=torch.int32)
        counts[:npairs] = torch.tensor(self.batch[1:], dtype=torch.int32) + 1        # the 1-based number of the pair's newer frame
        status[:npairs] = 0
        return rows, counts, status

    def rows_moving_filter(self, frames, mats, plate, count, origin, rows, counts, status1, out_rows, out_counts, moving, *,
                           threshold, min_cover, radius, min_hits, row_scale, frame_step, min_keep, size):
        ids = _ids(frames)
        assert ids == self.batch, "the filter judges other frames than the batch entry matched"
        self.calls.append(("filter", ids, tuple(frames.shape[1:]), size, _shift(mats), tuple(row_scale)))
        out_counts.copy_(counts)
        moving.zero_()

    def stream_scan(self, rows, counts, status1, state_in=None, state_out=None):
        import torch
        H = torch.eye(3, dtype=torch.float64).reshape(1, 9) * counts.to(torch.float64)[:, None]
        return H, torch.zeros(len(counts), dtype=torch.int32)

    def draw_matches(self, frames, rows, counts, out, status=None, frame_step=1, points="reference", color=(0, 255, 0)):
        import torch
        ids = _ids(frames)
        self.calls.append(("draw", ids, tuple(frames.shape[1:]), None))
        out.zero_()
        out[:, 0, 0, 0] = torch.tensor(ids[1:], dtype=torch.uint8)


@pytest.fixture
def rec(monkeypatch):
    import torch
    fake = Recorder()
    monkeypatch.setattr(runtime, "device", lambda: torch.device("cpu"))
    monkeypatch.setattr(runtime, "get_context", lambda *a, **k: fake)
    runtime.release_staging()
    yield fake
    runtime.release_staging()


def taken(pictures):
    """What a generator yields, each picture copied as it comes: on the CPU the arrays are views of the chunk's buffer."""
    return [(no, picture.copy()) for no, picture in pictures]


def translation(dx, dy=0):
    return [[1.0, 0.0, float(dx)], [0.0, 1.0, float(dy)], [0.0, 0.0, 1.0]]


def superposition(n, work):
    """Frame f of n sits f pixels to the right: the matrix names its frame."""
    d = {f: translation(f) for f in range(1, n + 1)}
    return d, {"w": work[0], "h": work[1]}


def ladder(rec, form, total, size, overlap, resize, convert, product, extra=lambda ids: ()):
    """What the ladder of a driver must have done for `total` frames: per chunk the conversion of the planes (when `convert`), the
    resize to SMALL (when `resize`), and `product` on the chunk's frames, in the form the ladder leaves them in.
    -> (shape of a frame handed to the product, its size=)"""
    convert = convert and form == "planes"
    shape = SMALL if resize else FULL if (convert or form != "planes") else PACKED
    size_kw = (F.W0, F.H0) if shape == PACKED else None
    chunks = [list(range(a, a + n)) for a, n in F.spans(total, size, overlap)]
    assert rec.of("yuv") == ([("yuv", ids, PACKED, FULL, (F.W0, F.H0)) for ids in chunks] if convert else [])
    assert [c for c in rec.of("resize") if c[3] == SMALL] == ([("resize", ids, FULL, SMALL) for ids in chunks] if resize else [])
    assert [c for c in rec.of(product)] == [(product, ids, shape, size_kw) + tuple(extra(ids)) for ids in chunks]
    return shape, size_kw


# ---- stabilized_frames in its three modes, the trail, comparison_frames --------------------------------------------------------------
@pytest.mark.parametrize("chunk", [2, 3])
@pytest.mark.parametrize("n", [6, 7])
@pytest.mark.parametrize("work", WORK)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("placement", ["warp", "translate"])
@pytest.mark.parametrize("mode", ["each", "history", "mosaic"])
def test_stabilized_frames(rec, mode, placement, form, work, n, chunk):
    cap, ingest = F.make(form, n)
    sup, info = superposition(n, work)
    got = taken(stabilization.stabilized_frames(cap, sup, info, mode=mode, placement=placement, chunk_frames=chunk, ingest=ingest))
    resize = placement == "translate" and work != (F.W0, F.H0)
    ladder(rec, form, n, chunk, 0, resize, resize, "warp", lambda ids: ([float(i + 1) for i in ids], mode))
    if mode == "mosaic":
        assert [f for f, _ in got] == [n] and got[0][1][0, 0, 0] == n - 1
    else:
        assert [f for f, _ in got] == list(range(1, n + 1))
        assert [int(p[0, 0, 0]) for _, p in got] == list(range(n))


@pytest.mark.parametrize("chunk", [2, 3])
@pytest.mark.parametrize("n", [6, 7])
@pytest.mark.parametrize("work", WORK)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("placement", ["warp", "translate"])
def test_trail(rec, placement, form, work, n, chunk):
    cap, ingest = F.make(form, n)
    sup, info = superposition(n, work)
    got = taken(stabilization.stabilized_frames(cap, sup, info, placement=placement, chunk_frames=chunk, ingest=ingest, trail=True))
    resize = placement == "translate" and work != (F.W0, F.H0)
    shape, size = ladder(rec, form, n, chunk, 0, resize, resize, "trail",
                         lambda ids: ([float(i + 1) for i in ids], placement == "translate"))
    # initialize_background: frame 1 alone, before the first trail call, in the form the chunk's frames have
    first = [("warp", [0], shape, size, [0.0], "mosaic")] if placement == "translate" else []
    assert rec.of("warp") == first and (not first or rec.calls.index(first[0]) < rec.calls.index(rec.of("trail")[0]))
    assert [f for f, _ in got] == list(range(1, n + 1)) and [int(p[0, 0, 0]) for _, p in got] == list(range(n))


@pytest.mark.parametrize("chunk", [2, 3])
@pytest.mark.parametrize("n", [6, 7])
@pytest.mark.parametrize("work", WORK)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("placement", ["warp", "translate"])
def test_comparison_frames(rec, placement, form, work, n, chunk):
    cap, ingest = F.make(form, n)
    sup, info = superposition(n, work)
    got = taken(stabilization.comparison_frames(cap, sup, info, placement=placement, height=3, chunk_frames=chunk, ingest=ingest))
    resize = placement == "translate" and work != (F.W0, F.H0)
    ladder(rec, form, n, chunk, 0, resize, True, "trail", lambda ids: ([float(i + 1) for i in ids], placement == "translate"))
    # the left half is the chunk's full-size BGR frames taken to `height` rows, whatever the trail was fed
    chunks = [list(range(a, k + a)) for a, k in F.spans(n, chunk, 0)]
    assert [c[:3] for c in rec.of("resize") if c[3] == (3, 6, 3)] == [("resize", ids, FULL) for ids in chunks]
    assert [f for f, _ in got] == list(range(1, n + 1)) and [int(p[0, 0, 0]) for _, p in got] == list(range(n))
    assert all(p.shape[0] == 3 and p.shape[1] > 6 for _, p in got)


# ---- background_plate ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_frames,frames,kept", [(64, 7, [1, 2, 3, 4, 5, 6, 7]), (3, 7, [1, 4, 7]), (3, 9, [1, 4, 7]), (3, 6, [1, 4]),
                                                    (3, 4, [1, 4]), (3, 3, [1]), (2, 1, [1])])
@pytest.mark.parametrize("work", WORK)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("placement", ["warp", "translate"])
def test_background_plate(rec, placement, form, work, max_frames, frames, kept):
    cap, ingest = F.make(form, frames)
    sup, info = superposition(7, work)
    plate = stabilization.background_plate(cap, sup, info, placement=placement, max_frames=max_frames, masks=True, ingest=ingest)
    assert plate.frame_nos == kept and plate.masks.shape[0] == len(kept)
    resize = placement == "translate" and work != (F.W0, F.H0)
    convert = resize and form == "planes"
    shape = SMALL if resize else PACKED if form == "planes" else FULL
    ids = [f - 1 for f in kept]
    assert rec.of("yuv") == ([("yuv", ids, PACKED, FULL, (F.W0, F.H0))] if convert else [])
    assert rec.of("resize") == ([("resize", ids, FULL, SMALL)] if resize else [])
    assert rec.of("plate") == [("plate", ids, shape, (F.W0, F.H0) if shape == PACKED else None, [float(f) for f in kept])]
    assert cap.i == min(frames, stabilization.plate_frame_numbers(7, max_frames)[-1])      # read once, and no further than needed


# ---- heatmap_frames -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [2, 3])
@pytest.mark.parametrize("frames,entries", [(6, 6), (7, 7), (9, 6), (5, 7), (1, 4), (4, 1)])
@pytest.mark.parametrize("work", WORK)
@pytest.mark.parametrize("form", FORMS + ("gray",))
def test_heatmap_frames(rec, form, work, frames, entries, chunk):
    cap, ingest = F.make(form, frames)
    keys = [10 + 3 * k for k in range(entries)]
    d = {key: translation(k) for k, key in enumerate(keys)}
    got = taken(heatmap.heatmap_frames(cap, d, {"w": work[0], "h": work[1]}, chunk_frames=chunk, ingest=ingest))
    total, resize = min(frames, entries), work != (F.W0, F.H0)
    chunks = [list(range(a, a + n)) for a, n in F.spans(total, min(chunk, entries), 0)]
    assert rec.of("yuv") == ([("yuv", ids, PACKED, FULL, (F.W0, F.H0)) for ids in chunks] if form == "planes" else [])
    # gray frames are B = G = R before anything else sees them
    assert rec.of("resize") == ([("resize", ids, FULL, SMALL) for ids in chunks] if resize else [])
    assert rec.of("heatmap") == [("heatmap", ids, SMALL if resize else FULL, None, [float(i) for i in ids]) for ids in chunks]
    assert [k for k, _ in got] == keys[:total] and [int(p[0, 0, 0]) for _, p in got] == list(range(total))
    assert cap.i == total


# ---- registration_report, residual_frames -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [2, 3, 4])
@pytest.mark.parametrize("frames,entries", [(6, 6), (7, 7), (9, 6), (5, 7), (1, 4), (2, 5), (4, 1)])
@pytest.mark.parametrize("work", WORK)
@pytest.mark.parametrize("form", FORMS + ("gray",))
def test_registration_report_and_residual_frames(rec, form, work, frames, entries, chunk):
    keys = [10 + 3 * k for k in range(entries)]
    d = {key: translation(k) for k, key in enumerate(keys)}
    total, resize = (min(frames, entries) if entries >= 2 else 0), work != (F.W0, F.H0)
    chunks = [list(range(a, a + n)) for a, n in F.spans(total, min(max(chunk, 2), max(entries, 2)), 1)]
    for pictures in (False, True):
        del rec.calls[:]
        cap, ingest = F.make(form, frames)
        if pictures:
            got = taken(registration.residual_frames(cap, d, {"w": work[0], "h": work[1]}, chunk_frames=chunk, ingest=ingest))
            assert [k for k, _ in got] == keys[1:total] and [int(p[0, 0]) for _, p in got] == list(range(1, total))
            assert all(p.shape == ((4, 8) if resize else (F.H0, F.W0)) for _, p in got)
        else:
            report = registration.registration_report(cap, d, {"w": work[0], "h": work[1]}, chunk_frames=chunk, ingest=ingest)
            assert list(report["frames"]) == keys[1:total]
            assert [e["covered"] for e in report["frames"].values()] == list(range(1, total))
        assert rec.of("yuv") == ([("yuv", ids, PACKED, FULL, (F.W0, F.H0)) for ids in chunks] if form == "planes" else [])
        assert rec.of("resize") == ([("resize", ids, FULL, SMALL) for ids in chunks] if resize else [])
        assert rec.of("residual") == [("residual", ids, SMALL if resize else FULL, None) for ids in chunks]
        assert cap.i == (total if entries >= 2 else 0)


# ---- refine_homography_dict ---------------------------------------------------------------------------------------------------------
def host_superposition(per_frame):
    sup, S = {1: np.eye(3).tolist()}, np.eye(3)
    for k, v in per_frame.items():
        S = np.dot(np.asarray(v["H"], np.float64), S)
        sup[k] = S.tolist()
    return sup


@pytest.mark.parametrize("chunk", [2, 3, 4])
@pytest.mark.parametrize("n", [1, 2, 6, 7])
@pytest.mark.parametrize("work", WORK)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("placement", ["warp", "translate"])
def test_refine_homography_dict(rec, monkeypatch, placement, form, work, n, chunk):
    monkeypatch.setattr(moving, "superposition_dict", host_superposition)
    first = {f: {"H": translation(1)} for f in range(2, 8)}               # frame f sits f - 1 pixels to the right
    first["resize_info"] = {"w": work[0], "h": work[1]}
    ox, oy, dw, dh, _ = stabilization._placement(host_superposition({k: v for k, v in first.items() if k != "resize_info"}),
                                                 first["resize_info"], placement, 1.0, F.W0, F.H0, stabilization.MAX_PIXELS)
    plate = stabilization.BackgroundPlate(np.zeros((dh, dw, 3), np.uint8), np.zeros((dh, dw), np.uint8), (ox, oy), [1], None)
    cap, ingest = F.make(form, n)
    refined, stats = moving.refine_homography_dict(cap, first, plate, placement=placement, chunk_frames=chunk, ingest=ingest)
    translate = placement == "translate"
    resize = translate and work != (F.W0, F.H0)
    chunks = [list(range(a, a + k)) for a, k in F.spans(n, chunk, 1)]
    # the batch entry always runs on the chunk as it was uploaded
    assert rec.of("batch") == [("batch", ids, PACKED if form == "planes" else FULL, (F.W0, F.H0) if form == "planes" else None)
                               for ids in chunks]
    scale = (1.0, 1.0) if translate else (F.W0 / work[0], F.H0 / work[1])
    ladder(rec, form, n, chunk, 1, resize, resize, "filter", lambda ids: ([float(i) for i in ids], scale))
    assert list(refined) == list(range(2, n + 1)) + ["resize_info"] and refined["resize_info"] == {"h": work[1], "w": work[0]}
    assert all(refined[f]["H"] == (np.eye(3) * f).tolist() for f in range(2, n + 1))
    assert stats == {f: (f, 0, f) for f in range(2, n + 1)}
    assert cap.i == n


# ---- the matching pictures of get_homography_dict -----------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [2, 3])
@pytest.mark.parametrize("n", [6, 7])
@pytest.mark.parametrize("work", WORK)
@pytest.mark.parametrize("form", FORMS)
def test_matching_pictures(rec, form, work, n, chunk):
    cap, ingest = F.make(form, n)
    got = []
    res = video_processing.get_homography_dict(cap, resize_width=work[0], chunk_frames=chunk, features_type_list=["ORB"],
                                               ingest=ingest, matching_sink=lambda f, pic: got.append((f, pic)))
    resize = work != (F.W0, F.H0)
    shape, _ = ladder(rec, form, n, chunk, 1, resize, True, "draw")
    assert [f for f, _ in got] == list(range(2, n + 1)) == [k for k in res if k != "resize_info"]
    assert [int(p[0, 0, 0]) for _, p in got] == list(range(1, n)) and all(p.shape == (shape[0], 2 * shape[1], 3) for _, p in got)
