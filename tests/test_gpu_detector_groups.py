"""The batch plumbing of the SIFT and SURF units (evh_sift.hip, evh_surf.hip) against the CPU oracle, at the bar of
tests/test_gpu_sift.py: key points, descriptors, the scale space and the integral image BIT FOR BIT.

Both units work through a batch in groups of frames (`for (f0 = 0; f0 < nframes; f0 += group)`): the scale space, or the
integral image and the Hessian layers, of one group is resident at a time and is indexed by the frame's place in the group,
while the lists, counts and flags are indexed by the frame's place in the batch.  At the frame sizes of a test suite one
group holds every batch, so the tests here force small groups with EVH_DETECT_GROUP (read when a detector is enabled: it is
set before the context exists) and hold every frame of every group to the oracle.  Further: which frames the two download
entries for resident data accept, overflow flags per frame across groups and their clearing, the fused multi-type stream
with and without groups, the largest frame geometry SIFT accepts (13-bit row / column packing of the extrema), geometry
changes on one context, and a batch longer than one launch's grid takes."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from evenvizion_amd import synthetic as S  # noqa: E402
from oracle import oracle as O  # noqa: E402
from detector_checks import _same_keypoints, _same_surf, dev, make_ctx, make_surf_ctx  # noqa: E402

DETECT = {"SIFT": lambda img: O.sift_detect(img, cap=65536), "SURF": O.surf_detect}
SAME = {"SIFT": _same_keypoints, "SURF": _same_surf}


def _run(c, det, d):
    (c.sift_detect_batch if det == "SIFT" else c.surf_detect_batch)(d)


def _download(c, det, f):
    return c.sift_download(f) if det == "SIFT" else c.surf_download(f)


def _count(c, det, f):
    return (c.lib.evh_sift_count if det == "SIFT" else c.lib.evh_surf_count)(c.h, f)


def _check_frame(c, det, f, want):
    """frame slot f of the last batch against the oracle's list (an empty list: the count, as a download of nothing)"""
    try:
        if len(want["xy"]) == 0:
            assert _count(c, det, f) == 0
        SAME[det](_download(c, det, f), want)
    except AssertionError as e:
        raise AssertionError("%s frame %d: %s" % (det, f, e)) from e


def _frozen(a):
    """frames shared between tests: nothing may write to them (they go onto the device as writable copies: dev(a.copy()))"""
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def group_frames(w, h, nframes, group):
    """nframes pairwise different frames: a stream, the first frame of the SECOND group flat, the last one frame 0 upside down"""
    fr = S.make_stream(1, nframes, w, h)[0].copy()
    fr[group] = 90
    fr[nframes - 1] = fr[0][::-1]
    return _frozen(fr)


@functools.lru_cache(maxsize=None)
def group_oracle(det, w, h, nframes, group):
    return [DETECT[det](f) for f in group_frames(w, h, nframes, group)]


GROUP_CASES = [(97, 131, 5, 2), (160, 120, 7, 3), (400, 224, 3, 1)]


@pytest.mark.parametrize("w,h,nframes,group", GROUP_CASES)
@pytest.mark.parametrize("det", ["SIFT", "SURF"])
def test_every_frame_of_every_group(monkeypatch, det, w, h, nframes, group):
    """Groups of 2+2+1, 3+3+1 and 1+1+1 frames: every frame's list equals the oracle's.  The flat frame opens the second
    group and the oracle's counts of the frames with content differ pairwise, so no frame can stand in for another.  One
    exception, stated: the oracle's SURF finds as many key points in a frame turned upside down as in the frame (at 160x120
    and 400x224 for every stream seed tried, 1..399: its box filters and sampling grids are symmetric there), so for SURF
    the last frame and frame 0 are told apart by their coordinates instead -- the lists must differ."""
    frames, want = group_frames(w, h, nframes, group), group_oracle(det, w, h, nframes, group)
    counts = [len(o["xy"]) for o in want]
    print("%s %dx%d oracle counts %s" % (det, w, h, counts))
    assert counts[group] == 0
    rest = [f for f in range(nframes) if f != group]
    for i in rest:
        assert counts[i] > 0
        for j in rest:
            if i < j and det == "SURF" and (i, j) == (0, nframes - 1) and counts[i] == counts[j]:
                assert (want[i]["xy"] != want[j]["xy"]).any(axis=1).mean() > 0.9
            elif i < j:
                assert counts[i] != counts[j], counts
    monkeypatch.setenv("EVH_DETECT_GROUP", str(group))
    c = make_ctx(w, h, frames=nframes, sift=4096) if det == "SIFT" else make_surf_ctx(w, h, frames=nframes, surf=4096)
    try:
        _run(c, det, dev(frames.copy()))
        for f in range(nframes):
            _check_frame(c, det, f, want[f])
    finally:
        c.close()


def test_only_the_last_group_is_resident(monkeypatch):
    """5 frames in groups of 2: the scale space and the integral image left behind are frame 4's (g0 = 4); the download
    entries hand out that frame, refuse the frames of earlier groups and the slot past the batch, and a refusal leaves the
    context usable."""
    from evenvizion_amd._lib import EvhError
    w, h, n, group = GROUP_CASES[0]
    frames = group_frames(w, h, n, group)
    monkeypatch.setenv("EVH_DETECT_GROUP", str(group))
    c = make_surf_ctx(w, h, frames=n, surf=4096, sift=4096)
    try:
        d = dev(frames.copy())
        c.sift_detect_batch(d)
        want = O.sift_gauss_pyramid(frames[4])
        assert len(want) == len(c.sift_octaves()) and c.sift_octaves() == O.sift_layout(w, h)
        for o in range(len(want)):
            for l in range(6):
                assert np.array_equal(c.sift_download_gauss(4, o, l), want[o][l]), (o, l)
        for f in (0, 1, 2, 3, 5):
            with pytest.raises(EvhError):
                c.sift_download_gauss(f, 0, 0)
        c.surf_detect_batch(d)
        assert np.array_equal(c.surf_download_integral(4), O.integral(frames[4]))
        for f in (0, 1, 2, 3, 5):
            with pytest.raises(EvhError):
                c.surf_download_integral(f)
        # the lists of every frame are still there, and the context still detects
        for f in range(n):
            _check_frame(c, "SIFT", f, group_oracle("SIFT", w, h, n, group)[f])
            _check_frame(c, "SURF", f, group_oracle("SURF", w, h, n, group)[f])
        back = np.ascontiguousarray(frames[::-1])
        c.sift_detect_batch(dev(back))
        c.surf_detect_batch(dev(back))
        for f in range(n):
            _check_frame(c, "SIFT", f, group_oracle("SIFT", w, h, n, group)[n - 1 - f])
            _check_frame(c, "SURF", f, group_oracle("SURF", w, h, n, group)[n - 1 - f])
        assert np.array_equal(c.sift_download_gauss(4, 1, 3), O.sift_gauss_pyramid(back[4])[1][3])
        assert np.array_equal(c.surf_download_integral(4), O.integral(back[4]))
    finally:
        c.close()


def sparse_frame(w=400, h=224):
    """the bright-squares frame of test_detector_slot_overflow_is_a_pair_status_in_the_fused_path"""
    sparse = np.full((h, w), 100, np.uint8)
    for y in range(50, 170, 24):
        for x in range(50, 350, 24):
            sparse[y:y + 7, x:x + 7] = 220
    return sparse


SIFT_SMALL_CAP, SURF_SMALL_CAP = 512, 448          # between the key-point counts of a sparse and of a textured 400x224 frame


def test_overflow_flags_per_frame_across_groups(monkeypatch):
    """[sparse, textured, sparse, textured, sparse] in groups of 2 with lists too short for a textured frame: frames 1 and 3
    (one per group, at either place in it) are flagged and refuse their download, frames 0, 2 and 4 equal the oracle; a
    following batch of sparse frames clears every flag."""
    from evenvizion_amd._lib import EvhError
    w, h = 400, 224
    tex = S.make_stream(53, 2, w, h)[0]
    sp = [np.roll(sparse_frame(w, h), k, axis=1) for k in (0, 2, 4, 6, 8)]
    frames = np.stack([sp[0], tex[0], sp[1], tex[1], sp[2]])
    caps = {"SIFT": SIFT_SMALL_CAP, "SURF": SURF_SMALL_CAP}
    want = {det: [DETECT[det](f) for f in sp] for det in DETECT}
    for det in DETECT:
        n_sp = [len(o["xy"]) for o in want[det]]
        n_tex = [len(DETECT[det](f)["xy"]) for f in tex]
        print("%s sparse %s textured %s capacity %d" % (det, n_sp, n_tex, caps[det]))
        assert 0 < min(n_sp) and max(n_sp) < caps[det] < min(n_tex)
    monkeypatch.setenv("EVH_DETECT_GROUP", "2")
    c = make_surf_ctx(w, h, frames=5, surf=SURF_SMALL_CAP, sift=SIFT_SMALL_CAP)
    try:
        assert c.lib.evh_sift_capacity(c.h) == SIFT_SMALL_CAP and c.lib.evh_surf_capacity(c.h) == SURF_SMALL_CAP
        for det in DETECT:
            _run(c, det, dev(frames))
            for f in (1, 3):
                with pytest.raises(EvhError):
                    _download(c, det, f)
            for f, k in ((0, 0), (2, 1), (4, 2)):
                _check_frame(c, det, f, want[det][k])
            _run(c, det, dev(np.stack(sp[::-1])))
            for f in range(5):
                _check_frame(c, det, f, want[det][4 - f])
    finally:
        c.close()


def test_fused_stream_with_and_without_groups(monkeypatch):
    """stream_homography_batch_types over SURF + SIFT + ORB on 7 frames, detectors in groups of 3+3+1 and in one group: the
    same H and status bit for bit, and the oracle's stream."""
    w, h = 400, 224
    frames = S.make_stream(73, 7, w, h)[0]
    n = len(frames) - 1
    features = ["SURF", "SIFT", "ORB"]
    Ho, so, rc = O.stream_gray_types(frames, features)
    assert rc == -1 and list(so) == [0] * n
    outs = []
    for group in ("3", None):
        if group is None:
            monkeypatch.delenv("EVH_DETECT_GROUP", raising=False)
        else:
            monkeypatch.setenv("EVH_DETECT_GROUP", group)
        c = make_surf_ctx(w, h, frames=len(frames), surf=4096, sift=4096)
        try:
            H = torch.zeros(n, 9, dtype=torch.float64, device="cuda")
            st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
            c.stream_homography_batch_types(dev(frames), H, st, features)
            c.synchronize()
            outs.append((H.cpu().numpy(), st.cpu().numpy()))
        finally:
            c.close()
    for H, st in outs:
        assert np.array_equal(st, so)
        assert np.allclose(H.reshape(-1, 3, 3), Ho, rtol=1e-9, atol=1e-12)
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][0], outs[1][0])


@pytest.mark.parametrize("w,h", [(4095, 64), (64, 4095)])
def test_largest_frame_coordinates(w, h):
    """The longest frame SIFT accepts: octave 0 is the frame x2, so extrema rows / columns reach 8185 -- past 12 bits of the
    packed candidate (o << 28 | layer << 26 | r << 13 | c) -- and every stride and offset of the scale space is at its
    largest.  The same frame in both slots; SURF at the same geometry."""
    img = S.make_pair(61, w, h)[0]
    want_sift, want_surf = O.sift_detect(img, cap=65536), O.surf_detect(img)
    far = int((want_sift["xy"][:, 0 if w > h else 1] > 4000).sum())
    print("%dx%d oracle: %d SIFT key points, %d beyond 4000, %d SURF key points" % (w, h, len(want_sift["xy"]), far, len(want_surf["xy"])))
    assert far >= 100 and len(want_sift["xy"]) < 16384 and 0 < len(want_surf["xy"]) < 4096
    c = make_surf_ctx(w, h, frames=2, surf=4096, sift=16384)
    try:
        d = dev(np.stack([img, img]))
        c.sift_detect_batch(d)
        for f in range(2):
            _check_frame(c, "SIFT", f, want_sift)
        c.surf_detect_batch(d)
        assert np.array_equal(c.surf_download_integral(1), O.integral(img))
        for f in range(2):
            _check_frame(c, "SURF", f, want_surf)
    finally:
        c.close()


@functools.lru_cache(maxsize=None)
def geometry_batch(w, h):
    fr = _frozen(S.make_stream(79, 3, w, h)[0].copy())
    return fr, [DETECT["SIFT"](f) for f in fr], [DETECT["SURF"](f) for f in fr], [O.integral(f) for f in fr]


@pytest.mark.parametrize("group", [None, 2])
def test_geometry_changes_on_one_context(monkeypatch, group):
    """One 400x224 context, batches of three frames at 400x224, 97x131, 333x217 and the first batch again: the frame's
    strides and tables follow the batch, the per-frame sizes of the buffers stay the context's.  In one group, and in
    groups of 2+1 (then only the last frame's integral image is left to compare)."""
    if group is None:
        monkeypatch.delenv("EVH_DETECT_GROUP", raising=False)
    else:
        monkeypatch.setenv("EVH_DETECT_GROUP", str(group))
    c = make_surf_ctx(400, 224, frames=3, surf=4096, sift=4096)
    got = []
    try:
        for w, h in ((400, 224), (97, 131), (333, 217), (400, 224)):
            fr, want_sift, want_surf, want_sum = geometry_batch(w, h)
            d = dev(fr.copy())
            c.sift_detect_batch(d)
            assert c.sift_octaves() == O.sift_layout(w, h)
            c.surf_detect_batch(d)
            for f in range(3):
                _check_frame(c, "SIFT", f, want_sift[f])
                _check_frame(c, "SURF", f, want_surf[f])
                if group is None or f >= 2:
                    assert np.array_equal(c.surf_download_integral(f), want_sum[f]), (w, h, f)
            got.append([(c.sift_download(f), c.surf_download(f)) for f in range(3)])
        for f in range(3):
            for a, b in zip(got[0][f], got[3][f]):
                assert a.keys() == b.keys()
                for k in a:
                    assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (f, k)
    finally:
        c.close()


def test_more_frames_than_one_launch_takes():
    """3001 frames of 64x64 on a SURF context of 3002 slots: the buffers of all of them fit the memory budget, the grid of one
    launch takes 3000 -- the group size is bounded by both, so the batch runs as 3000 + 1.  (Frame 3000 shows what frame 0
    shows: telling the frames of a later group apart is the business of the tests above.)"""
    n = 3001
    base = np.stack([S.make_pair(s, 64, 64)[0] for s in (3, 7, 11)])
    want = [O.surf_detect(f) for f in base]
    counts = [len(o["xy"]) for o in want]
    print("oracle counts %s" % counts)
    assert min(counts) > 0 and len(set(counts)) == 3 and max(counts) < 256
    frames = np.tile(base, (n // 3 + 1, 1, 1))[:n]
    c = make_surf_ctx(64, 64, frames=n + 1, surf=256)
    try:
        c.surf_detect_batch(dev(frames))
        for f in (0, 1, 2, n - 2, n - 1):
            _check_frame(c, "SURF", f, want[f % 3])
        got = [c.lib.evh_surf_count(c.h, f) for f in range(n)]
        assert got == [counts[f % 3] for f in range(n)]
        assert np.array_equal(c.surf_download_integral(n - 1), O.integral(frames[n - 1]))
    finally:
        c.close()
