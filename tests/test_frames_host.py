"""evenvizion_amd.frames off the device: the chunk reader over scripted captures whose frames carry their position (every
chunk size, overlap, capture length around the chunk boundaries and limit), the shape-mismatch error, planes and the fall-back
from them, the dictionary-entry helper and the ladder's rule against a recording context."""
import numpy as np
import pytest

import frames_checks as F
from evenvizion_amd import frames


def lengths(size, overlap):
    return sorted({n for n in (1, 2, size - 1, size, size + 1, 2 * size - overlap - 1, 2 * size - overlap, 2 * size - overlap + 1)
                   if n >= 1})


CASES = [(size, overlap, n) for overlap, sizes in ((0, (1, 2, 3, 4)), (1, (2, 3, 4))) for size in sizes for n in lengths(size, overlap)]


@pytest.mark.parametrize("form", ["bgr", "gray", "planes"])
@pytest.mark.parametrize("size,overlap,length", CASES)
def test_chunks_cover_the_capture_once_in_order(size, overlap, length, form):
    for limit in (None, max(1, length - 1), length, length + 2):
        cap, ingest = F.make(form, length)
        reader = frames.FrameReader(cap, ingest)
        assert reader.planes == (form == "planes") and (reader.w0, reader.h0) == (F.W0, F.H0)
        total = length if limit is None else min(length, limit)
        seen, last = [], None
        for start, chunk in reader.chunks(size, overlap, limit):
            ids = [int(f.reshape(-1)[0]) for f in chunk]
            assert ids == list(range(start, start + len(ids))) and overlap + 1 <= len(ids) <= size
            if seen:
                assert ids[:overlap] == [last] * overlap, "the shared frame is not the chunk before's last"
            new = ids[overlap if seen else 0:]
            assert new, "a chunk without a new frame"
            seen += new
            last = ids[-1]
        # a capture of one frame has no pair to give
        assert seen == (list(range(total)) if total > overlap else [])
        assert reader.consumed == cap.i == total
        assert cap.failed <= 1 and cap.calls == total + cap.failed
        if limit is not None:
            assert cap.calls <= limit
        assert reader.exhausted == bool(cap.failed)


@pytest.mark.parametrize("size,overlap", [(1, 0), (3, 0), (2, 1), (3, 1)])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_a_frame_of_another_shape_is_named_by_its_number(size, overlap, k):
    reader = frames.FrameReader(F.Cap(7, odd={k: (F.H0 + 2, F.W0, 3)}), "auto")
    with pytest.raises(ValueError, match=r"^frame %d has shape \(8, 12, 3\), the first frame \(6, 12, 3\)$" % (k + 1)):
        for _ in reader.chunks(size, overlap):
            pass
    reader = frames.FrameReader(F.Cap(7, odd={k: (F.H0, F.W0)}), "bgr")
    slot = np.empty((F.H0, F.W0, 3), np.uint8)
    assert all(reader.read_into(slot) for _ in range(k - 1))
    with pytest.raises(ValueError, match="^frame %d has shape" % (k + 1)):
        reader.read_into(slot)


def test_read_into_counts_and_asks_a_dry_capture_once():
    cap = F.Cap(3)
    reader = frames.FrameReader(cap, "bgr")
    host = reader.buffer(4)
    assert host.shape == (4, F.H0, F.W0, 3) and host[0, 0, 0, 0] == 0 and reader.consumed == 1
    assert reader.read_into(host[1]) and reader.read_into(host[2]) and reader.consumed == 3 and not reader.exhausted
    assert [int(f[0, 0, 0]) for f in host[:3]] == [0, 1, 2]
    assert not reader.read_into(host[3]) and not reader.read_into(host[3])
    assert reader.exhausted and reader.consumed == 3 and cap.failed == 1


def test_planes_are_taken_refused_or_demanded():
    cap = F.PlaneCap(3)
    first, planes, w0, h0 = frames.open_capture(cap, "auto")
    assert planes and first.shape == (F.W0 * F.H0 * 3 // 2,) and (w0, h0) == (F.W0, F.H0) and first[0] == 0
    slot = np.empty_like(first)
    assert frames.read_frame(cap, True, slot, w0, h0, 2) and slot[0] == 1 and (slot[F.W0 * F.H0:] == 128).all()
    assert frames.open_capture(F.PlaneCap(3), "bgr")[1] is False          # the same capture read as BGR when asked to
    # a capture that refuses planes does so before it consumes a frame: "auto" starts from the same first frame as BGR
    cap = F.PlaneCap(3, refuse=True)
    reader = frames.FrameReader(cap, "auto")
    assert not reader.planes and reader.first.shape == (F.H0, F.W0, 3) and reader.first[0, 0, 0] == 0 and cap.i == 1
    assert [int(f[0, 0, 0]) for _, c in reader.chunks(2, 0) for f in c] == [0, 1, 2]
    with pytest.raises(ValueError, match="refused to deliver planes"):
        frames.FrameReader(F.PlaneCap(3, refuse=True), "yuv420")
    with pytest.raises(ValueError, match="does not deliver 4:2:0 planes"):
        frames.FrameReader(F.Cap(3), "yuv420")
    for empty in (F.Cap(0), F.PlaneCap(0)):
        with pytest.raises(ValueError, match="Can't read first frame"):
            frames.FrameReader(empty, "auto")


def test_check_ingest_and_entry_matrix():
    for ok in ("auto", "bgr", "yuv420"):
        frames.check_ingest(ok)
    for bad in ("nv12", None, 0, "BGR"):
        with pytest.raises(ValueError, match="^ingest must be 'auto', 'bgr' or 'yuv420'$"):
            frames.check_ingest(bad)
    m = frames.entry_matrix(list(range(9)))
    assert m.dtype == np.float64 and m.shape == (3, 3) and m.reshape(9).tolist() == list(range(9))
    assert frames.entry_matrix(np.eye(3, dtype=np.float32)).dtype == np.float64
    for bad in (None, [1, 2, 3], np.zeros((4, 4)), []):
        m = frames.entry_matrix(bad)
        assert m.shape == (3, 3) and np.isnan(m).all()
    assert np.isinf(frames.entry_matrix([[np.inf] * 3] * 3)).all()          # what is not finite is the caller's to judge


class Steps:
    def __init__(self):
        self.calls = []

    def yuv420_to_bgr(self, planes, out, size=None):
        self.calls.append(("yuv", tuple(out.shape), size))

    def resize_area(self, src, dst):
        self.calls.append(("resize", tuple(src.shape), tuple(dst.shape)))


# (no driver resizes gray frames that it has not expanded: the resize takes BGR)
LADDERS = [(form, work, bgr, gray3) for form in ("bgr", "gray", "planes") for work in (None, (F.W0, F.H0), (8, 4))
           for bgr in (False, True) for gray3 in (False, True) if not (form == "gray" and work == (8, 4) and not gray3)]


@pytest.mark.parametrize("form,work,bgr,gray3", LADDERS)
def test_ladder_rule_and_buffers(form, work, bgr, gray3):
    import torch
    planes, resize = form == "planes", work == (8, 4)
    ladder = frames.DeviceLadder(torch.device("cpu"), 3, planes, (F.W0, F.H0), work, bgr=bgr, gray3=gray3)
    convert = planes and (resize or bgr)
    assert (ladder.bgr is not None) == convert and (ladder.small is not None) == resize
    shape = {"bgr": (2, F.H0, F.W0, 3), "gray": (2, F.H0, F.W0), "planes": (2, F.W0 * F.H0 * 3 // 2)}[form]
    ctx, up = Steps(), torch.zeros(shape, dtype=torch.uint8)
    full, src, size = ladder(ctx, up)
    three = (2, F.H0, F.W0, 3)
    assert ctx.calls == ([("yuv", three, (F.W0, F.H0))] if convert else []) + ([("resize", three, (2, 4, 8, 3))] if resize else [])
    expanded = form == "gray" and gray3
    assert tuple(full.shape) == (three if convert or expanded else shape)
    assert tuple(src.shape) == ((2, 4, 8, 3) if resize else tuple(full.shape))
    assert size == ((F.W0, F.H0) if planes and not convert else None)
    if not (convert or expanded):
        assert full is up
    if convert:
        assert full.data_ptr() == ladder.bgr.data_ptr()
    if resize:
        assert src.data_ptr() == ladder.small.data_ptr()
