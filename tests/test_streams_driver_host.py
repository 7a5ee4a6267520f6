"""Host loop of get_homography_dicts (several captures per GPU call) against a scripted context, no GPU: the segment
tables round by round, the replacement of an ended capture, the frame numbering of every dictionary, the two error modes and
the grouping by geometry.  The fake keeps the device's stream semantics (a failed pair repeats the previous H, a failing first
pair gives NaNs) and carries H_prev through the state rows it is handed, so a state that went to the wrong place shows."""
import json

import numpy as np
import pytest

from evenvizion_amd import _lib, runtime
from evenvizion_amd.processing import video_processing


class _Cap:
    """Capture `cid` with n frames; frame i carries (cid, i) in its first two pixels."""

    def __init__(self, cid, n, shape=(6, 12, 3)):
        self.cid, self.n, self.i, self.shape = cid, n, 0, shape

    def read(self):
        if self.i >= self.n:
            return False, None
        f = np.zeros(self.shape, np.uint8)
        f[0, 0, 0], f[0, 1, 0] = self.cid, self.i
        self.i += 1
        return True, f


def _H(cid, i):
    return (np.eye(3) * (100.0 * cid + i + 0.5)).reshape(9)


class _FakeCtx:
    """Plays evh_streams_homography_batch: pair (cid, i) fails when it is in `bad`, else gives _H(cid, i)."""

    def __init__(self, bad=()):
        self.bad, self.tables, self.shapes = set(bad), [], []

    def streams_homography_batch(self, frames, segments, H, st, features=None, state_in=None, state_out=None, **kw):
        import torch
        self.tables.append([(a, n, bool(s)) for a, n, s in segments])
        self.shapes.append(tuple(frames.shape[1:]))
        self.features = list(features)
        assert segments[0][0] == 0 and all(segments[k][0] == segments[k - 1][0] + segments[k - 1][1] for k in range(1, len(segments)))
        assert state_in.shape == (len(segments), 18) and state_out.shape == (len(segments), 18)
        H[:] = -7.0                                     # rows at segment ends must never be read
        st[:] = -9
        for s, (a, n, start) in enumerate(segments):
            cid = int(frames[a, 0, 0, 0])
            assert all(int(frames[a + k, 0, 0, 0]) == cid for k in range(n)), "a segment mixes two captures"
            ids = [int(frames[a + k, 0, 1, 0]) for k in range(n)]
            assert ids == list(range(ids[0], ids[0] + n)), "the frames of a segment are not consecutive"
            prev = None
            if not start:
                assert state_in[s, 0] == cid + 1, "the state of another capture"     # row tag written below
                prev = state_in[s, 9:18].clone() if state_in[s, 1] else None
            dead = False
            for k in range(1, n):
                if dead or (cid, ids[k]) in self.bad:
                    st[a + k - 1] = 2
                    if prev is None:
                        dead = True
                        H[a + k - 1] = float("nan")
                    else:
                        H[a + k - 1] = prev
                else:
                    st[a + k - 1] = 0
                    prev = torch.tensor(_H(cid, ids[k]), dtype=torch.float64)
                    H[a + k - 1] = prev
            state_out[s] = 0
            state_out[s, 0] = cid + 1
            if prev is not None:
                state_out[s, 1] = 1
                state_out[s, 9:18] = prev

    def synchronize(self):
        pass


def _want(cid, n, bad=()):
    """What get_homography_dict returns for _Cap(cid, n) behind the same fake: resize_width 8 of 12 x 6 frames."""
    out, prev = {}, None
    for i in range(1, n):
        if (cid, i) in bad:
            assert prev is not None
        else:
            prev = _H(cid, i)
        out[i + 1] = {"H": prev.reshape(3, 3).tolist()}
    out["resize_info"] = {"h": 4, "w": 8}
    return out


@pytest.fixture
def on_cpu(monkeypatch):
    import torch
    monkeypatch.setattr(runtime, "device", lambda: torch.device("cpu"))
    runtime.release_staging()

    def use(fake):
        monkeypatch.setattr(runtime, "get_context", lambda *a, **k: (fake.__dict__.setdefault("asked", []).append((a, k)), fake)[1])
        return fake
    yield use
    runtime.release_staging()


def test_symbols_of_the_ragged_entries_are_declared():
    for name in ("evh_streams_homography_batch", "evh_streams_homography_batch_yuv420"):
        assert name in _lib.SIGNATURES
    assert [f[0] for f in _lib.StreamSeg._fields_] == ["first_frame", "nframes", "start", "reserved"]
    import ctypes
    assert ctypes.sizeof(_lib.StreamSeg) == 16


def test_rounds_tables_and_numbering(on_cpu):
    lengths = [9, 3, 1, 6, 4]
    bad = {(0, 4), (3, 3)}            # (0, 4): the first pair of capture 0's second round -- H_prev must come from the state
    fake = on_cpu(_FakeCtx(bad))
    res = video_processing.get_homography_dicts([_Cap(i, n) for i, n in enumerate(lengths)], resize_width=8, chunk_frames=4,
                                                max_streams=2, features_type_list=["ORB"], decode_threads=3)
    assert fake.features == ["ORB"]
    # round 0: captures 0 and 1 start; 1 ends (3 frames).  round 1: capture 0 goes on; capture 2 took 1's place, has one
    # frame only and leaves the table.  round 2: capture 0's last two pairs; capture 3 starts in the free place.  round 3: capture 4
    # starts in capture 0's place, capture 3 ends.  Nothing is left for a round 4.
    assert fake.tables == [[(0, 4, True), (4, 3, True)], [(0, 4, False)], [(0, 3, False), (3, 4, True)],
                           [(0, 4, True), (4, 3, False)]]
    assert len(res) == len(lengths)
    for i, n in enumerate(lengths):
        want = _want(i, n, bad)
        assert list(res[i].keys()) == list(want.keys()), i            # 2..n, then "resize_info" last
        assert res[i] == want, i
        assert json.loads(json.dumps(res[i])) == json.loads(json.dumps(want))
    assert res[2] == {"resize_info": {"h": 4, "w": 8}}


@pytest.mark.parametrize("max_streams,chunk", [(1, 2), (3, 3), (8, 64), (2, 5)])
def test_any_schedule_gives_the_same_dictionaries(on_cpu, max_streams, chunk):
    lengths = [5, 2, 7, 1, 3, 6]
    bad = {(2, 3), (2, 4), (5, 5)}
    fake = on_cpu(_FakeCtx(bad))
    res = video_processing.get_homography_dicts([_Cap(i, n) for i, n in enumerate(lengths)], resize_width=8, chunk_frames=chunk,
                                                max_streams=max_streams, features_type_list=["ORB"])
    assert res == [_want(i, n, bad) for i, n in enumerate(lengths)]
    assert all(len(t) <= max_streams and sum(n for _, n, _ in t) <= max_streams * chunk for t in fake.tables)
    # every capture with a pair enters exactly once with start set
    assert sum(s for t in fake.tables for _, _, s in t) == sum(1 for n in lengths if n >= 2)
    # the default list is the reference's three detectors
    fake = on_cpu(_FakeCtx())
    video_processing.get_homography_dicts([_Cap(0, 3)], resize_width=8, chunk_frames=chunk, max_streams=max_streams)
    assert fake.features == ["SURF", "SIFT", "ORB"]


def test_error_modes(on_cpu):
    def caps():
        return [_Cap(0, 4), _Cap(1, 3), _Cap(2, 0), _Cap(3, 5), _Cap(4, 3)]
    bad = {(1, 1)}                     # capture 1: its FIRST pair fails -> AttributeError, as the reference's None.tolist()
    on_cpu(_FakeCtx(bad))
    res = video_processing.get_homography_dicts(caps(), resize_width=8, chunk_frames=3, max_streams=2,
                                                features_type_list=["ORB"], return_exceptions=True)
    assert isinstance(res[1], AttributeError) and isinstance(res[2], ValueError)
    for i, n in ((0, 4), (3, 5), (4, 3)):
        assert res[i] == _want(i, n)
    # return_exceptions=False: the exception of the LOWEST failing index, whatever was found first (capture 2 fails at once,
    # capture 1 only when its first round is collected)
    on_cpu(_FakeCtx(bad))
    with pytest.raises(AttributeError):
        video_processing.get_homography_dicts(caps(), resize_width=8, chunk_frames=3, max_streams=2, features_type_list=["ORB"])
    fake = on_cpu(_FakeCtx())
    with pytest.raises(ValueError):
        video_processing.get_homography_dicts(caps(), resize_width=8, chunk_frames=3, max_streams=2, features_type_list=["ORB"])
    # captures behind the failing one are not run
    assert all(shape == (6, 12, 3) for shape in fake.shapes) and sum(s for t in fake.tables for _, _, s in t) == 2
    # none_H_processing=False: any failed pair raises
    on_cpu(_FakeCtx({(0, 2)}))
    res = video_processing.get_homography_dicts([_Cap(0, 4), _Cap(1, 3)], resize_width=8, chunk_frames=3, max_streams=2,
                                                features_type_list=["ORB"], none_H_processing=False, return_exceptions=True)
    assert isinstance(res[0], AttributeError) and res[1] == _want(1, 3)
    with pytest.raises(ValueError):
        video_processing.get_homography_dicts([_Cap(0, 3)], features_type_list=["BRISK"])
    with pytest.raises(ValueError):
        video_processing.get_homography_dicts([_Cap(0, 3)], ingest="nv12")
    assert video_processing.get_homography_dicts([]) == []


def test_two_geometries_run_as_two_groups(on_cpu):
    small, large = (6, 12, 3), (8, 16, 3)
    fake = on_cpu(_FakeCtx())
    caps = [_Cap(0, 4, small), _Cap(1, 3, large), _Cap(2, 5, small), _Cap(3, 4, large)]
    res = video_processing.get_homography_dicts(caps, resize_width=8, chunk_frames=4, max_streams=4, features_type_list=["ORB"])
    assert len(fake.asked) == 2                                        # one context request per group
    # no call mixes the two sizes, and the groups run one after the other
    assert fake.shapes == sorted(fake.shapes, key=lambda s: s != small) and set(fake.shapes) == {small, large}
    for i, c in enumerate(caps):
        want = _want(i, c.n)
        want["resize_info"] = {"h": 4, "w": 8}                         # both sizes are 2:1
        assert res[i] == want


def test_round_with_an_overflowing_frame_is_rerun_as_a_whole(on_cpu, monkeypatch):
    """A pair of round 1 reports EVH_PAIR_CAPACITY: the whole round runs again on a context with larger frame slots, from the
    states the round was entered with (the gathered copy, not what the overflowing run left), with the same segment table --
    a segment that starts still starts -- and only the re-run's states go back to their places."""
    import torch

    class Overflowing(_FakeCtx):
        max_features = 500

        def streams_homography_batch(self, frames, segments, H, st, state_in=None, state_out=None, **kw):
            super().streams_homography_batch(frames, segments, H, st, state_in=state_in, state_out=state_out, **kw)
            if len(self.tables) == 2:                   # round 1: capture 0 goes on, capture 2 starts
                self.entered = state_in.clone()
                st[segments[1][0]] = _lib.PAIR_CAPACITY
                state_out[:] = float("nan")             # what this run leaves must not be used

    bigs = []

    class Big(_FakeCtx):
        def __init__(self, device=0, max_w=0, max_h=0, max_features=0, max_frames=0):
            super().__init__(bad)
            self.made = dict(max_features=max_features, max_frames=max_frames)
            self.closed = False
            bigs.append(self)

        def streams_homography_batch(self, frames, segments, H, st, state_in=None, state_out=None, **kw):
            self.entered = state_in.clone()
            super().streams_homography_batch(frames, segments, H, st, state_in=state_in, state_out=state_out, **kw)

        def close(self):
            self.closed = True

    bad = {(0, 3), (0, 5)}            # the first pairs of capture 0's rounds 1 and 2: H_prev comes from the carried state
    lengths = [7, 2, 4]
    small = on_cpu(Overflowing(bad))
    monkeypatch.setattr(_lib, "Context", Big)
    res = video_processing.get_homography_dicts([_Cap(i, n) for i, n in enumerate(lengths)], resize_width=8, chunk_frames=3,
                                                max_streams=2, features_type_list=["ORB"])
    assert res == [_want(i, n, bad) for i, n in enumerate(lengths)]
    assert len(bigs) == 1 and bigs[0].closed and bigs[0].made == dict(max_features=1000, max_frames=6)
    assert small.tables[1] == [(0, 3, False), (3, 3, True)] and bigs[0].tables == [small.tables[1]]
    assert torch.equal(bigs[0].entered, small.entered)
    assert len(small.tables) == 3                       # round 2 ran on the first context again


def test_captures_are_opened_only_when_a_place_is_free(on_cpu):
    """What is held scales with max_streams, not with the list: when a round is launched, no capture beyond the places of
    that round and the next (whose reads overlap it) has been touched."""
    caps = [_Cap(i, 3) for i in range(9)]
    opened = []

    class Watching(_FakeCtx):
        def streams_homography_batch(self, *a, **k):
            opened.append(sum(1 for c in caps if c.i > 0))
            super().streams_homography_batch(*a, **k)

    on_cpu(Watching())
    res = video_processing.get_homography_dicts(caps, resize_width=8, chunk_frames=4, max_streams=2, features_type_list=["ORB"])
    assert res == [_want(i, 3) for i in range(9)]
    assert opened[0] == 2 and all(n <= 2 * (r + 1) for r, n in enumerate(opened)) and opened[-1] == 9
