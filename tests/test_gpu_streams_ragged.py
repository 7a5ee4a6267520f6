"""GPU: evh_streams_homography_batch[_yuv420] -- ragged batches of several streams -- and get_homography_dicts over them.

Every comparison is equality: per stream the ragged batch must give the bits of that stream alone through the single-stream
entry in the same chunks, rows that belong to no stream must keep the sentinel the outputs were filled with, and the driver's
dictionaries must be == those of get_homography_dict."""
import os

import numpy as np
import pytest
import torch

from evenvizion_amd import synthetic as S
from evenvizion_amd._lib import Context, EvhError, ORDER_CANONICAL, ORDER_OPENCV

pytestmark = pytest.mark.gpu

W, H = 400, 224
HS, SS = -7.25, -9          # sentinels of H and status rows
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIDEO = os.path.join(ROOT, "tests", "golden", "ref_test_video.mp4")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def outputs(n):
    return (torch.full((n, 9), HS, dtype=torch.float64, device="cuda"), torch.full((n,), SS, dtype=torch.int32, device="cuda"))


def alone(c, chunks, single, **kw):
    """One stream through the single-stream entry `single`, chunk by chunk with carried state -> ([(H, status)], state)."""
    state = torch.zeros(18, dtype=torch.float64, device="cuda")
    out = []
    for k, fr in enumerate(chunks):
        Hk, sk = outputs(len(fr) - 1)
        single(dev(fr), Hk, sk, state_in=state if k else None, state_out=state, **kw)
        c.synchronize()
        out.append((Hk.clone(), sk.clone()))
    return out, state.clone()


def ragged(c, segs, state, **kw):
    """segs: [(frames, start)] -> (H, status) of the whole batch; state f64[len(segs), 18] is read and written in place."""
    table, at = [], 0
    for fr, start in segs:
        table.append((at, len(fr), start))
        at += len(fr)
    Hb, sb = outputs(at - 1)
    c.streams_homography_batch(dev(np.concatenate([fr for fr, _ in segs])), table, Hb, sb, state_in=state, state_out=state, **kw)
    c.synchronize()
    return table, Hb, sb


def check(table, Hb, sb, want):
    """Every segment's rows equal want[segment] = (H, status); the row at every segment's last frame holds the sentinel."""
    for (a, n, _), (Hw, sw) in zip(table, want):
        assert torch.equal(sb[a:a + n - 1], sw), (a, sb[a:a + n - 1], sw)
        assert torch.equal(Hb[a:a + n - 1].view(torch.int64), Hw.view(torch.int64)), a     # bits: NaN rows compare too
        if a + n - 1 < len(sb):
            assert int(sb[a + n - 1]) == SS and bool((Hb[a + n - 1] == HS).all()), "a row between two streams was written"


def four_streams(flat_first):
    """A (5 frames: 2 + 4 with one carried), B (5, with a flat frame: inside, or first), C (5: 3 + 3), D (2)."""
    A, B, Cs, D = (S.make_stream(70 + i, n, W, H)[0] for i, n in enumerate((5, 5, 5, 2)))
    B[0 if flat_first else 2] = 128
    return A, B, Cs, D


@pytest.fixture(scope="module")
def ctx():
    c = Context(device=0, max_w=W, max_h=H, max_features=500, max_frames=12)
    yield c
    c.close()


@pytest.mark.parametrize("order", [ORDER_OPENCV, ORDER_CANONICAL])
@pytest.mark.parametrize("flat_first", [False, True])
def test_ragged_orb_with_carried_state(ctx, flat_first, order):
    """Call 1: A, B, C with 2, 5, 3 frames, all starting; call 2: A goes on with 4 frames, a new stream D takes B's place,
    C goes on with 3.  B's flat frame fails two pairs (inside) or, as its first frame, the first pair: NaNs and the status for
    the whole segment.  ORDER_CANONICAL runs FAST with threshold lifting, whose share groups cross the segment borders."""
    c = ctx
    c.set_keypoint_order(order)
    try:
        A, B, Cs, D = four_streams(flat_first)
        refA, stA = alone(c, (A[:2], A[1:]), c.stream_homography_batch)
        refB, stB = alone(c, (B,), c.stream_homography_batch)
        refC, stC = alone(c, (Cs[:3], Cs[2:]), c.stream_homography_batch)
        refD, stD = alone(c, (D,), c.stream_homography_batch)
        if flat_first:
            assert refB[0][1].tolist() == [1, 1, 1, 1] and bool(torch.isnan(refB[0][0]).all())
        else:
            assert refB[0][1].tolist() == [0, 1, 1, 0]
        state = torch.zeros(3, 18, dtype=torch.float64, device="cuda")
        table, Hb, sb = ragged(c, [(A[:2], 1), (B, 1), (Cs[:3], 1)], state)
        assert [t[:2] for t in table] == [(0, 2), (2, 5), (7, 3)]
        check(table, Hb, sb, [refA[0], refB[0], refC[0]])
        assert torch.equal(state[1], stB)
        # B's row of the state belongs to D now: D starts, so what the row holds must not matter
        state[1] = float("nan")
        table, Hb, sb = ragged(c, [(A[1:], 0), (D, 1), (Cs[2:], 0)], state)
        check(table, Hb, sb, [refA[1], refD[0], refC[1]])
        assert torch.equal(state[0], stA) and torch.equal(state[1], stD) and torch.equal(state[2], stC)
    finally:
        c.set_keypoint_order(ORDER_OPENCV)


def test_forced_iterations_streams_of_unequal_length(ctx):
    """force_max_iters: the per-pair launches (k_scan_hyp / k_scan_finish) run up to the longest stream, the stream of 2
    frames leaves after the first; then both go on from the carried state, the other one shorter."""
    c = ctx
    a, b = (S.make_stream(60 + i, 6, W, H)[0] for i in range(2))
    refa, sta = alone(c, (a[:2], a[1:]), c.stream_homography_batch, force_max_iters=True)
    refb, stb = alone(c, (b[:4], b[3:5]), c.stream_homography_batch, force_max_iters=True)
    state = torch.zeros(2, 18, dtype=torch.float64, device="cuda")
    table, Hb, sb = ragged(c, [(a[:2], 1), (b[:4], 1)], state, force_max_iters=True)
    check(table, Hb, sb, [refa[0], refb[0]])
    table, Hb, sb = ragged(c, [(a[1:], 0), (b[3:5], 0)], state, force_max_iters=True)
    check(table, Hb, sb, [refa[1], refb[1]])
    assert torch.equal(state[0], sta) and torch.equal(state[1], stb)
    assert int(refa[1][1].abs().sum()) == 0 and int(refb[0][1].abs().sum()) == 0


def test_default_detector_list_and_orb_through_the_type_list():
    """["SURF", "SIFT", "ORB"] on segments of 3 and 2 frames == evh_stream_homography_batch_types per stream; the list
    ["ORB"] == the fused ORB entry."""
    a, b = S.make_stream(81, 3, W, H)[0], S.make_stream(82, 2, W, H)[0]
    c = Context(device=0, max_w=W, max_h=H, max_features=500, max_frames=5)
    try:
        c.sift_enable(4096)
        c.surf_enable(2048)
        feats = ["SURF", "SIFT", "ORB"]

        def single(fr, Hk, sk, **kw):
            c.stream_homography_batch_types(fr, Hk, sk, feats, **kw)

        refa, sta = alone(c, (a,), single)
        refb, stb = alone(c, (b,), single)
        state = torch.zeros(2, 18, dtype=torch.float64, device="cuda")
        table, Hb, sb = ragged(c, [(a, 1), (b, 1)], state, features=feats)
        check(table, Hb, sb, [refa[0], refb[0]])
        assert torch.equal(state[0], sta) and torch.equal(state[1], stb)
        assert refa[0][1].tolist() == [0, 0] and refb[0][1].tolist() == [0]
        orba, _ = alone(c, (a,), c.stream_homography_batch)
        orbb, _ = alone(c, (b,), c.stream_homography_batch)
        table, Hb, sb = ragged(c, [(a, 1), (b, 1)], state, features=["ORB"])
        check(table, Hb, sb, [orba[0], orbb[0]])
        assert not torch.equal(orba[0][0], refa[0][0])          # the two lists are different computations
    finally:
        c.close()


@pytest.mark.parametrize("sw,sh", [(500, 280), (800, 448)])
def test_resize_and_planes(sw, sh):
    """Full-size frames, 500x280 (float tables) and 800x448 (integer ratio), shrunk to 400x224 inside the ingest: the BGR form
    == evh_stream_homography_batch_resized per stream; the plane form (packed I420, and NV12 through strides) == the BGR
    form on the frames the planes convert to."""
    rng = np.random.default_rng(5)
    lens = (3, 2, 4)
    planes = [[(g,) + S.chroma_for(rng, g) for g in S.make_stream(90 + i, n, sw, sh)[0]] for i, n in enumerate(lens)]
    bgr = [np.stack([S.yuv420_to_bgr_host(*p) for p in st]) for st in planes]
    c = Context(device=0, max_w=W, max_h=H, max_features=500, max_frames=sum(lens))
    try:
        refs = [alone(c, (fr,), c.stream_homography_batch, resize_to=(W, H)) for fr in bgr]
        state = torch.zeros(3, 18, dtype=torch.float64, device="cuda")
        table, Hb, sb = ragged(c, [(fr, 1) for fr in bgr], state, resize_to=(W, H))
        check(table, Hb, sb, [r[0][0] for r in refs])
        assert all(torch.equal(state[i], refs[i][1]) for i in range(3))
        assert all(r[0][0][1].tolist() == [0] * (n - 1) for r, n in zip(refs, lens))
        flat = [p for st in planes for p in st]
        packed = dev(np.stack([np.concatenate([a.reshape(-1) for a in p]) for p in flat]))
        y = dev(np.stack([p[0] for p in flat]))
        uv = dev(np.stack([np.stack([p[1], p[2]], axis=-1) for p in flat]))            # NV12: interleaved chroma
        for frames, size in ((packed, (sw, sh)), ((y, uv[..., 0], uv[..., 1]), None)):
            Hp, sp = outputs(len(flat) - 1)
            st2 = torch.zeros(3, 18, dtype=torch.float64, device="cuda")
            c.streams_homography_batch(frames, table, Hp, sp, state_in=None, state_out=st2, resize_to=(W, H), size=size)
            c.synchronize()
            assert torch.equal(sp, sb) and torch.equal(Hp.view(torch.int64), Hb.view(torch.int64)) and torch.equal(st2, state)
    finally:
        c.close()


def test_uniform_segments_equal_multi_stream(ctx):
    c = ctx
    Sn, F = 3, 4
    streams = np.stack([S.make_stream(40 + i, F, W, H)[0] for i in range(Sn)])
    Hm = torch.zeros(Sn, F - 1, 9, dtype=torch.float64, device="cuda")
    sm = torch.full((Sn, F - 1), -1, dtype=torch.int32, device="cuda")
    stm = torch.zeros(Sn, 18, dtype=torch.float64, device="cuda")
    c.multi_stream_homography_batch(dev(streams), Hm, sm, state_out=stm)
    c.synchronize()
    state = torch.zeros(Sn, 18, dtype=torch.float64, device="cuda")
    table, Hb, sb = ragged(c, [(fr, 1) for fr in streams], state)
    check(table, Hb, sb, [(Hm[i], sm[i]) for i in range(Sn)])
    assert torch.equal(state, stm)


def test_refusals_leave_the_outputs_untouched(ctx):
    c = ctx
    frames = dev(S.make_stream(3, 6, W, H)[0])
    state = torch.zeros(4, 18, dtype=torch.float64, device="cuda")

    def refused(code, segs, fr=frames, state_in=state, **kw):
        Hb, sb = outputs(11)
        so = torch.full((4, 18), HS, dtype=torch.float64, device="cuda")
        with pytest.raises(EvhError) as e:
            c.streams_homography_batch(fr, segs, Hb, sb, state_in=state_in, state_out=so, **kw)
        c.synchronize()
        assert ("libevhip error %d:" % code) in str(e.value), e.value
        assert bool((Hb == HS).all()) and bool((sb == SS).all()) and bool((so == HS).all())

    refused(-1, [(0, 4, 1), (3, 3, 1)])                 # overlap
    refused(-1, [(0, 3, 1), (4, 2, 1)])                 # gap
    refused(-1, [(0, 3, 1), (3, 2, 1)])                 # ends short of total_frames
    refused(-1, [(0, 3, 1), (3, 4, 1)])                 # ends beyond total_frames
    refused(-1, [(3, 3, 1), (0, 3, 1)])                 # not ascending
    refused(-1, [(0, 5, 1), (5, 1, 1)])                 # nframes < 2
    refused(-1, [(0, 3, 1), (3, 3, 0)], state_in=None)  # a carried stream without d_state_in
    refused(-1, [(0, 6, 1)], features=["ORB", "ORB"])   # a type named twice
    refused(-1, [(0, 6, 1)], features=["SIFT", "ORB"])  # SIFT without evh_sift_enable
    refused(-1, [(0, 6, 1)], features=[7])              # unknown type
    refused(-1, [])                                     # no stream at all
    big = torch.zeros(13, H, W, dtype=torch.uint8, device="cuda")
    refused(-3, [(0, 13, 1)], fr=big)                   # total_frames > max_frames (12)
    # and the same frames are accepted once the table is right
    Hb, sb = outputs(5)
    c.streams_homography_batch(frames, [(0, 3, 1), (3, 3, 1)], Hb, sb, state_in=None, state_out=state[:2])
    c.synchronize()
    assert sb.tolist() == [0, 0, SS, 0, 0]


class _First:
    """The first n frames of a capture (anything the capture offers besides is handed through)."""

    def __init__(self, cap, n):
        self._cap, self._left = cap, n

    def __getattr__(self, name):
        return getattr(self._cap, name)

    def read(self):
        if self._left <= 0:
            return False, None
        self._left -= 1
        return self._cap.read()

    def read_yuv420_into(self, y, cb, cr):
        if self._left <= 0:
            return False
        self._left -= 1
        return self._cap.read_yuv420_into(y, cb, cr)


def _captures(lengths):
    from evenvizion_amd import capture
    return [_First(capture.VideoCapture(VIDEO), n) for n in lengths]


@pytest.fixture(scope="module")
def video_dicts():
    """get_homography_dict on the first n frames of the reference video, once per (n, ingest)."""
    from evenvizion_amd.processing.video_processing import get_homography_dict
    cache = {}

    def get(n, ingest="bgr", features=("ORB",)):
        key = (n, ingest, tuple(features))
        if key not in cache:
            cache[key] = get_homography_dict(_captures([n])[0], features_type_list=list(features), ingest=ingest)
        return cache[key]
    return get


@pytest.mark.parametrize("ingest", ["bgr", "auto"])
def test_driver_equals_one_capture_at_a_time(video_dicts, ingest):
    from evenvizion_amd.processing.video_processing import get_homography_dicts
    lengths = [9, 3, 1, 6, 4]
    got = get_homography_dicts(_captures(lengths), features_type_list=["ORB"], max_streams=2, chunk_frames=4, ingest=ingest)
    want = [video_dicts(n, ingest) for n in lengths]
    assert got == want
    assert got[2] == {"resize_info": want[0]["resize_info"]} and sorted(k for k in got[0] if k != "resize_info") == list(range(2, 10))
    assert got == [video_dicts(n, "bgr") for n in lengths]            # planes or BGR: the same dictionaries


def test_driver_default_detector_list(video_dicts):
    from evenvizion_amd.processing.video_processing import get_homography_dicts
    feats = ["SURF", "SIFT", "ORB"]
    got = get_homography_dicts(_captures([4, 4]), max_streams=2, chunk_frames=3)
    want = video_dicts(4, "bgr", feats)
    assert got == [want, want] and sorted(k for k in want if k != "resize_info") == [2, 3, 4]


def test_driver_capture_without_a_first_frame(video_dicts):
    from evenvizion_amd.processing.video_processing import get_homography_dicts
    lengths = [5, 0, 3]
    with pytest.raises(ValueError):
        get_homography_dicts(_captures(lengths), features_type_list=["ORB"], max_streams=2, chunk_frames=4)
    got = get_homography_dicts(_captures(lengths), features_type_list=["ORB"], max_streams=2, chunk_frames=4,
                               return_exceptions=True)
    assert isinstance(got[1], ValueError) and got[0] == video_dicts(5) and got[2] == video_dicts(3)


def test_component_cli_many_videos(tmp_path, monkeypatch):
    """python -m evenvizion_amd.component --path_to_videos A B: per video the files of the single form, byte for byte."""
    from evenvizion_amd import component
    monkeypatch.chdir(tmp_path)
    specs = ["synthetic:4:400x224:1", "synthetic:3:400x224:2"]
    tail = ["--features", "ORB", "--resize_width", "400"]
    folders = component.main(["--path_to_videos"] + specs + ["--experiment_name", "many", "--max_streams", "2"] + tail)
    assert len(folders) == 2 and len(set(folders)) == 2
    for spec, folder in zip(specs, folders):
        one = component.main(["--path_to_video", spec, "--experiment_name", "one"] + tail)
        assert os.path.basename(one) == os.path.basename(folder)
        for name in ("dict_with_homography_matrix.json", "metrics_file.txt"):
            assert open(os.path.join(folder, name)).read() == open(os.path.join(one, name)).read(), (spec, name)
