"""The matching pictures without a GPU: the line rule of evh_draw_matches as tests/draw_checks.py restates it (known answers,
the closed form against the literal loop), Python's int() on coordinates, write_png, and the sink logic of get_homography_dict
through a scripted context."""
import struct
import zlib

import numpy as np
import pytest

import draw_checks as DC
from evenvizion_amd import runtime
from evenvizion_amd.processing import video_processing


# ---- the line rule ------------------------------------------------------------------------------------------------------------------
def test_known_answers():
    want = [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (5, 2)]
    assert DC.line_pixels((0, 0), (5, 2)) == want and DC.line_pixels((5, 2), (0, 0)) == want
    assert DC.line_pixels((0, 0), (2, 1)) == [(0, 0), (1, 0), (2, 1)]
    assert DC.line_pixels((0, 1), (2, 0)) == [(0, 1), (1, 1), (2, 0)]
    assert DC.line_pixels((3, 4), (3, 1)) == [(3, 4), (3, 3), (3, 2), (3, 1)]          # dx == 0: walked from pt1
    assert DC.line_pixels((2, 0), (0, 5)) == [(0, 5), (0, 4), (1, 3), (1, 2), (2, 1), (2, 0)]
    assert DC.line_pixels((4, 4), (4, 4)) == [(4, 4)]


def test_closed_form_equals_the_loop_for_every_pair_of_a_box():
    pts = [(x, y) for x in range(9) for y in range(7)]
    for a in pts:
        for b in pts:
            walk = DC.line_pixels(a, b)
            assert len(walk) == max(abs(a[0] - b[0]), abs(a[1] - b[1])) + 1
            assert a in (walk[0], walk[-1]) and b in (walk[0], walk[-1])
            assert DC.closed_form(a, b) == walk, (a, b)


def test_closed_form_on_long_and_shifted_lines():
    rng = np.random.default_rng(5)
    for _ in range(200):
        a = tuple(int(v) for v in rng.integers(-40000, 40000, 2))
        b = tuple(int(v) for v in rng.integers(-40000, 40000, 2))
        if max(abs(a[0] - b[0]), abs(a[1] - b[1])) > 3000:
            b = (a[0] + int(rng.integers(-3000, 3000)), a[1] + int(rng.integers(-3000, 3000)))
        assert DC.closed_form(a, b) == DC.line_pixels(a, b)
    assert DC.closed_form((-32768, -32768), (32767 + 16383, 32767)) == DC.line_pixels((-32768, -32768), (32767 + 16383, 32767))


def test_coordinates_truncate_toward_zero_and_bad_rows_are_skipped():
    assert int(-0.5) == 0 and int(3.99) == 3
    assert DC.ends(np.float32([-0.5, 3.99, -1.5, 2.0]), 10, DC.REFERENCE) == ((0, 3), (9, 2))
    assert DC.ends(np.float32([-0.5, 3.99, -1.5, 2.0]), 10, DC.OWN_FRAME) == ((-1, 2), (10, 3))
    for bad in (np.nan, np.inf, -np.inf, 1e9, 32768.0, -32769.0):
        for at in range(4):
            row = np.float32([1, 2, 3, 4])
            row[at] = bad
            assert DC.ends(row, 10, DC.REFERENCE) is None
    assert DC.ends(np.float32([32767.9, -32768.9, 0, 0]), 10, DC.REFERENCE) == ((32767, -32768), (10, 0))


def test_picture_pastes_and_clips():
    prev = np.full((3, 4, 3), 10, np.uint8)
    cur = np.full((3, 4, 3), 20, np.uint8)
    got = DC.picture(prev, cur, np.float32([[1, 1, 2, 1], [-3, 0, 50, 0], [np.nan, 0, 0, 0]]), color=(1, 2, 3))
    want = np.concatenate([prev, cur], axis=1)
    want[1, 1:7] = (1, 2, 3)
    want[0, :] = (1, 2, 3)                      # from x = -3 to 54: the part inside the picture
    assert np.array_equal(got, want)
    own = DC.picture(prev, cur, np.float32([[1, 1, 2, 1]]), points=DC.OWN_FRAME, color=(1, 2, 3))
    want = np.concatenate([prev, cur], axis=1)
    want[1, 2:6] = (1, 2, 3)
    assert np.array_equal(own, want)


# ---- write_png ----------------------------------------------------------------------------------------------------------------------
def test_write_png_round_trip(tmp_path):
    from evenvizion_amd.matching_pictures import write_png
    rng = np.random.default_rng(3)
    bgr = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    path = tmp_path / "p.png"
    write_png(str(path), bgr)
    data = path.read_bytes()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        n, tag = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        chunks.append((tag, body))
        at += 12 + n
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    assert struct.unpack(">IIBBBBB", chunks[0][1]) == (7, 5, 8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(5, 1 + 21)
    assert (raw[:, 0] == 0).all()                                               # filter 0 on every row
    assert np.array_equal(raw[:, 1:].reshape(5, 7, 3)[:, :, ::-1], bgr)
    with pytest.raises(ValueError):
        write_png(str(path), bgr[..., 0])


# ---- the ABI and the refusals that stay ---------------------------------------------------------------------------------------------
def test_the_three_symbols_are_declared_and_bound():
    from evenvizion_amd import _lib
    for name in ("evh_batch_static_info", "evh_batch_static_rows", "evh_draw_matches"):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["evh_draw_matches"][1]) == 17
    for method in ("batch_static_info", "batch_static_rows", "draw_matches"):
        assert callable(getattr(_lib.Context, method))


def test_the_reference_names_still_raise_and_name_the_new_ones():
    from evenvizion_amd import component
    with pytest.raises(NotImplementedError, match="matching_sink"):
        video_processing.get_homography_dict(_Cap(3), matching_path="/tmp/x")
    with pytest.raises(NotImplementedError, match="--matching_pictures"):
        component.main(["--show_matching_visualization", "True"])
    with pytest.raises(ValueError):
        component.main(["--path_to_videos", "a.npy", "b.npy", "--matching_pictures", "1"])


# ---- the sink logic of get_homography_dict through a scripted context -------------------------------------------------------------
class _Cap:
    """Frames of one value each: frame number f (1-based) is filled with f - 1."""

    def __init__(self, n, shape=(6, 12, 3)):
        self.n, self.i, self.shape = n, 0, shape

    def read(self):
        if self.i >= self.n:
            return False, None
        f = np.full(self.shape, self.i, np.uint8)
        self.i += 1
        return True, f


class _Scripted:
    """Stands in for libevhip: plays a per-frame plan ("nomatch": the front fails with status 2; "lowratio": matching
    succeeds, compute_homography fails with status 4; else H) with the stream semantics of the device entry, and records every
    call of the matching-picture methods."""
    CAP = 5

    def __init__(self, plan):
        self.plan, self.prev, self.touched, self.front, self.points = plan, None, [], None, set()

    def stream_homography_batch(self, frames, H, st, state_in=None, state_out=None, nfeatures=500, **kw):
        import torch
        ids = frames[:, 0, 0, 0].tolist()
        self.front = []
        for k in range(1, len(ids)):
            r = self.plan.get(str(ids[k]), np.eye(3).tolist())
            if isinstance(r, str):
                st[k - 1] = 2 if r == "nomatch" else 4
                self.front.append(2 if r == "nomatch" else 0)
                H[k - 1] = float("nan") if self.prev is None else self.prev
            else:
                st[k - 1] = 0
                self.front.append(0)
                self.prev = torch.tensor(r, dtype=torch.float64).reshape(9)
                H[k - 1] = self.prev

    def resize_area(self, src, dst):
        self.touched.append("resize")
        dst.copy_(src[:, :dst.shape[1], :dst.shape[2]])

    def batch_static_info(self):
        self.touched.append("info")
        return len(self.front), self.CAP

    def batch_static_rows(self, first_pair, npairs, rows, counts, status):
        import torch
        self.touched.append("rows")
        assert first_pair == 0 and npairs == len(self.front) and rows.shape[1:] == (self.CAP, 4)
        status[:npairs] = torch.tensor(self.front, dtype=torch.int32)
        counts[:npairs] = 1

    def draw_matches(self, frames, rows, counts, out, status=None, frame_step=1, points="reference", color=(0, 255, 0)):
        self.touched.append("draw")
        self.points.add(points)
        w = frames.shape[2]
        assert frame_step == 1 and status is not None and out.shape[0] == frames.shape[0] - 1 and out.shape[2] == 2 * w
        out[:, :, :w] = frames[:-1]
        out[:, :, w:] = frames[1:]

    def synchronize(self):
        pass


@pytest.fixture
def scripted(monkeypatch):
    import torch
    monkeypatch.setattr(runtime, "device", lambda: torch.device("cpu"))
    monkeypatch.setattr(video_processing, "resized_shape", lambda shape, width: (width, shape[0]))     # a crop stands in

    def install(plan):
        fake = _Scripted(plan)
        monkeypatch.setattr(runtime, "get_context", lambda *a, **k: fake)
        return fake
    yield install
    runtime.release_staging()


def _run(nframes, chunk, sink, **kw):
    return video_processing.get_homography_dict(_Cap(nframes), resize_width=8, chunk_frames=chunk, features_type_list=["ORB"],
                                                matching_sink=sink, **kw)


@pytest.mark.parametrize("chunk", [2, 3, 64])
def test_sink_numbering_order_and_pictures(scripted, chunk):
    fake = scripted({})
    got = []
    res = _run(7, chunk, lambda f, pic: got.append((f, pic)))
    assert [f for f, _ in got] == [2, 3, 4, 5, 6, 7] == [k for k in res if k != "resize_info"]
    for f, pic in got:
        assert pic.shape == (6, 16, 3) and pic.dtype == np.uint8
        assert (pic[:, :8] == f - 2).all() and (pic[:, 8:] == f - 1).all()       # the previous frame | the current frame
    assert fake.points == {"reference"} and {"info", "rows", "draw", "resize"} <= set(fake.touched)
    first = got[0][1]
    first[:] = 255                                                                # the array is the sink's own
    fake = scripted({})
    _run(7, chunk, lambda f, pic: None, matching_points="own_frame")
    assert fake.points == {"own_frame"}
    with pytest.raises(ValueError):
        _run(3, chunk, lambda f, pic: None, matching_points="neither")


@pytest.mark.parametrize("chunk", [2, 3, 64])
def test_sink_leaves_out_pairs_whose_matching_failed(scripted, chunk):
    scripted({"3": "nomatch", "5": "lowratio"})        # frame numbers 4 and 6
    got = []
    res = _run(8, chunk, lambda f, pic: got.append(f))
    assert got == [2, 3, 5, 6, 7, 8]                    # no picture after NoMatchesException, one before HomographyException
    assert [k for k in res if k != "resize_info"] == [2, 3, 4, 5, 6, 7, 8]


@pytest.mark.parametrize("chunk", [2, 3, 64])
def test_pictures_are_delivered_before_the_call_raises(scripted, chunk):
    scripted({"4": "lowratio"})                         # frame number 5: matched, then no homography
    got = []
    with pytest.raises(AttributeError):
        _run(8, chunk, lambda f, pic: got.append(f), none_H_processing=False)
    assert got == [2, 3, 4, 5]
    scripted({"4": "nomatch"})
    got = []
    with pytest.raises(AttributeError):
        _run(8, chunk, lambda f, pic: got.append(f), none_H_processing=False)
    assert got == [2, 3, 4]
    scripted({"1": "nomatch"})                          # a failing first pair raises with none_H_processing too
    got = []
    with pytest.raises(AttributeError):
        _run(4, chunk, lambda f, pic: got.append(f))
    assert got == []


def test_gray_frames_are_refused_with_a_sink_only(scripted):
    fake = scripted({})
    cap = _Cap(4, shape=(6, 12))
    with pytest.raises(ValueError, match="gray"):
        video_processing.get_homography_dict(cap, resize_width=8, features_type_list=["ORB"], matching_sink=lambda f, pic: None)
    assert fake.touched == [] and fake.front is None          # refused before any work


def test_picture_buffers_are_kept_with_the_staging_set(scripted):
    scripted({})
    _run(5, 3, lambda f, pic: None)
    B = runtime.staging((3, 6, 12, 3), runtime.device())
    kept = B[("pictures", 8, 6)]
    got = []
    _run(5, 3, lambda f, pic: got.append((f, pic)))             # a second video of the same size: the same buffers
    assert B is runtime.staging((3, 6, 12, 3), runtime.device()) and B[("pictures", 8, 6)] is kept
    assert [f for f, _ in got] == [2, 3, 4, 5]
    for f, pic in got:
        assert (pic[:, :8] == f - 2).all() and (pic[:, 8:] == f - 1).all()


@pytest.mark.parametrize("chunk", [2, 64])
def test_without_a_sink_nothing_new_is_called(scripted, chunk):
    fake = scripted({"3": "nomatch"})
    res = _run(6, chunk, None)
    assert fake.touched == [] and [k for k in res if k != "resize_info"] == [2, 3, 4, 5, 6]
