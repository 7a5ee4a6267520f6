"""evh_draw_matches, evh_batch_static_rows and get_homography_dict(matching_sink=) on the device.  Every assertion on pictures
is equality of bytes with tests/draw_checks.py (the literal LineIterator loop, checked on the host in test_draw_host.py); the
bytes between picture rows must keep the sentinel the buffers were filled with."""
import json
import os

import numpy as np
import pytest

import draw_checks as DC
from refusal_arena import Arena

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from evenvizion_amd import synthetic as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MP4 = os.path.join(ROOT, "tests", "golden", "ref_test_video.mp4")
GOLD = os.path.join(ROOT, "tests", "golden", "ref_dict_with_homography_matrix.json")
SENTINEL = 0xCD
GEOMS = [(1, 1), (2, 3), (37, 5), (16, 16), (65, 9)]
INVALID, CAPACITY = -1, -3
W, H = 400, 224


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def ctx():
    from evenvizion_amd._lib import Context
    c = Context(device=0, max_w=64, max_h=64, max_features=500, max_frames=2)       # the entry does not depend on these sizes
    yield c
    c.close()


def strided(n, h, w, row_stride, frame_stride, offset, content=None):
    """A [n,h,w,3] view with the given byte strides, `offset` bytes into a buffer of SENTINEL -> (buffer, view, the buffer
    positions of the view's bytes)."""
    at = (offset + np.arange(n, dtype=np.int64)[:, None, None] * frame_stride + np.arange(h, dtype=np.int64)[None, :, None] * row_stride
          + np.arange(3 * w, dtype=np.int64)[None, None, :])
    buf = torch.full((int(at.max()) + 9,), SENTINEL, dtype=torch.uint8, device="cuda")
    view = buf.as_strided((n, h, w, 3), (frame_stride, row_stride, 3, 1), offset)
    if content is not None:
        view.copy_(dev(content))
    return buf, view, at.reshape(-1)


def odd_layouts(w, h):
    """(row stride, frame stride, offset) of pictures and of frames: unaligned pointers, odd strides."""
    ors, frs = 6 * w + 5, 3 * w + 3 + (w % 2 == 0)
    return (ors, h * ors + 3, 1), (frs, h * frs + 2, 3)


def aligned_layouts(w, h):
    ors, frs = (6 * w + 3) // 4 * 4 + 4, (3 * w + 3) // 4 * 4
    return (ors, h * ors + 8, 0), (frs, h * frs, 4)


def run(ctx, frames, rows, counts, status=None, out_layout=None, frame_layout=None, **kw):
    """Context.draw_matches -> u8[npairs,h,2w,3]; default layouts: odd_layouts.  Bytes of the output buffer outside the
    pictures' rows must keep SENTINEL."""
    npairs = rows.shape[0]
    n, h, w = frames.shape[:3]
    lo, lf = odd_layouts(w, h)
    buf, out, at = strided(npairs, h, 2 * w, *(out_layout or lo))
    _, src, _ = strided(n, h, w, *(frame_layout or lf), content=frames)
    ctx.draw_matches(src, dev(rows), dev(np.asarray(counts, np.int32)), out,
                     status=None if status is None else dev(np.asarray(status, np.int32)), **kw)
    ctx.synchronize()
    got = buf.cpu().numpy()
    gaps = np.ones(got.shape, bool)
    gaps[at] = False
    assert (got[gaps] == SENTINEL).all(), "bytes outside the picture rows were written"
    return got[at].reshape(npairs, h, 2 * w, 3)


def check(ctx, frames, rows, counts, status=None, frame_step=1, points="reference", color=(0, 255, 0), **layouts):
    want = DC.draw(frames, rows, counts, status, frame_step, DC.REFERENCE if points == "reference" else DC.OWN_FRAME, color)
    got = run(ctx, frames, rows, counts, status, frame_step=frame_step, points=points, color=color, **layouts)
    print("%dx%d x%d %s: differing bytes %d of %d, line bytes %d" % (frames.shape[2], frames.shape[1], len(want), points,
                                                                      (got != want).sum(), want.size,
                                                                      (want != DC.draw(frames, rows, 0 * np.asarray(counts), None, frame_step)).sum()))
    assert np.array_equal(got, want)
    return got


def row_of(pt1, pt2, w, frac=(0.0, 0.0, 0.0, 0.0)):
    """The row whose REFERENCE line runs from pt1 to pt2 of the picture (fractions are added away from zero)."""
    v = [pt1[0], pt1[1], pt2[0] - w, pt2[1]]
    return [c + (f if c >= 0 else -f) for c, f in zip(v, frac)]


def crafted_rows(w, h, rng):
    W2 = 2 * w
    cx, cy = w, h // 2
    rows = []
    for a, b in ((5, 2), (2, 5), (7, 7), (6, 3), (3, 6), (1, 2), (2, 1), (4, 2), (2, 4)):          # octants, ties D == 2d
        for sx in (1, -1):
            for sy in (1, -1):
                rows.append(row_of((cx, cy), (cx + sx * a, cy + sy * b), w))
                rows.append(row_of((cx + sx * a, cy + sy * b), (cx, cy), w, (0.25, 0.5, 0.75, 0.99)))
    rows += [row_of((0, cy), (W2 - 1, cy), w), row_of((W2 - 1, 0), (0, 0), w), row_of((0, h - 1), (W2 - 1, h - 1), w),      # axis-aligned
             row_of((0, 0), (0, h - 1), w), row_of((w - 1, h - 1), (w - 1, 0), w), row_of((w, 0), (w, h - 1), w),
             row_of((W2 - 1, h - 1), (W2 - 1, 0), w),
             row_of((cx, cy), (cx, cy), w), row_of((0, 0), (0, 0), w), row_of((W2 - 1, h - 1), (W2 - 1, h - 1), w),        # zero length
             row_of((0, 0), (W2 - 1, h - 1), w), row_of((0, h - 1), (W2 - 1, 0), w),                                        # crossing
             row_of((0, 0), (W2 - 1, h - 1), w), row_of((W2 - 1, h - 1), (0, 0), w),                                        # identical, reversed
             row_of((0, 0), (w - 1, h - 1), w), row_of((w - 1, 0), (w, h - 1), w),
             [-0.5, -0.99, w - 0.01 - w, h - 0.5], [w - 0.5, h - 0.01, -0.25, -0.75], [0.99, 0.5, 0.5, 0.99],               # fractional, slightly negative
             row_of((-5, -3), (W2 + 4, h + 2), w), row_of((-1, cy), (W2, cy), w), row_of((cx, -4), (cx + 1, h + 6), w),    # partly off the canvas
             row_of((-10, -10), (-3, -8), w), row_of((0, h + 3), (W2, h + 1), w), row_of((W2 + 2, 0), (W2 + 9, h), w),      # wholly off
             row_of((-1, -1), (-1, -1), w), row_of((W2, h), (W2, h), w),
             row_of((-30000, -20000), (32767 + w, 30000), w), row_of((3, -32768), (4, 32767), w),                           # D >= 2^15
             [32767.5, 0, -32768.5, 0], [-32768.9, 32767.9, 32767.9, -32768.9],
             [np.nan, 1, 2, 3], [1, np.nan, 2, 3], [1, 2, np.nan, 3], [1, 2, 3, np.nan],                                     # skipped
             [np.inf, 0, 0, 0], [0, -np.inf, 0, 0], [0, 0, np.inf, 0], [0, 0, 0, -np.inf],
             [1e9, 0, 0, 0], [0, -1e9, 0, 0], [0, 0, 32768, 0], [0, 0, 0, -32769], [3e38, 0, 0, 0]]
    rows = np.float32(rows)
    extra = np.float32(np.stack([rng.uniform(-3, W2 + 3, 40), rng.uniform(-3, h + 3, 40), rng.uniform(-3, W2 + 3, 40) - w,
                                 rng.uniform(-3, h + 3, 40)], axis=1))
    return np.concatenate([rows, extra])


def random_rows(rng, n, w, h, margin=3):
    return np.float32(np.stack([rng.uniform(-margin, 2 * w + margin, n), rng.uniform(-margin, h + margin, n),
                                rng.uniform(-margin, 2 * w + margin, n) - w, rng.uniform(-margin, h + margin, n)], axis=1))


@pytest.mark.parametrize("points,color", [("reference", (0, 255, 0)), ("own_frame", (201, 7, 94))])
@pytest.mark.parametrize("w,h", GEOMS)
def test_crafted_rows(ctx, w, h, points, color):
    """Three pictures of consecutive frames: every crafted row (count == row_cap); rows that must not be drawn (count 0);
    random rows under a count above row_cap."""
    rng = np.random.default_rng(1000 * w + h)
    crafted = crafted_rows(w, h, rng)
    cap = len(crafted)
    rows = np.stack([crafted, random_rows(rng, cap, w, h), random_rows(rng, cap, w, h)])
    frames = rng.integers(0, 256, (4, h, w, 3), dtype=np.uint8)
    got = check(ctx, frames, rows, [cap, 0, cap + 5], points=points, color=color)
    # the same rows a few to a picture, so that no line hides under the others
    per = 4
    few = np.full((-(-cap // per) * per, 4), np.nan, np.float32)
    few[:cap] = crafted
    few = few.reshape(-1, per, 4)
    check(ctx, rng.integers(0, 256, (len(few) + 1, h, w, 3), dtype=np.uint8), few, [per] * len(few), points=points, color=color)
    assert np.array_equal(got[1], np.concatenate([frames[1], frames[2]], axis=1))
    check(ctx, frames, rows, [-1, cap, 1], points=points, color=color)


@pytest.mark.parametrize("w,h", [(2, 3), (37, 5), (16, 16)])
def test_status_and_frame_step(ctx, w, h):
    rng = np.random.default_rng(77 + w)
    rows = np.stack([random_rows(rng, 12, w, h) for _ in range(3)])
    frames = rng.integers(0, 256, (6, h, w, 3), dtype=np.uint8)
    counts = [12, 12, 7]
    a = check(ctx, frames, rows, counts, status=[0, 0, 0], frame_step=2)
    b = check(ctx, frames, rows, counts, status=None, frame_step=2)
    assert np.array_equal(a, b)
    c = check(ctx, frames, rows, counts, status=[0, 2, 6], frame_step=2)                      # failed pairs: the two frames only
    assert np.array_equal(c[1], np.concatenate([frames[2], frames[3]], axis=1))
    assert np.array_equal(c[2], np.concatenate([frames[4], frames[5]], axis=1))
    d = check(ctx, frames, rows, counts, status=[1, 0, 0], frame_step=1)                      # the same frames as a stream
    assert np.array_equal(d[0], np.concatenate([frames[0], frames[1]], axis=1))


@pytest.mark.parametrize("w,h", [(65, 9), (16, 16)])
def test_more_lines_than_one_workgroup(ctx, w, h):
    """700 rows per pair: the waves of a pair's workgroups take several lines each.  The lines are one or two pixels long, so
    that most of them stay visible beside the others."""
    rng = np.random.default_rng(5 + w)
    rows = np.stack([random_rows(rng, 700, w, h, margin=0), random_rows(rng, 700, w, h, margin=2)])
    rows[:, :, 2] = rows[:, :, 0] - w + rng.integers(-1, 2, (2, 700))
    rows[:, :, 3] = rows[:, :, 1] + rng.integers(-1, 2, (2, 700))
    frames = rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8)
    check(ctx, frames, rows, [700, 650])


@pytest.mark.parametrize("w,h", [(2, 3), (16, 16), (65, 9), (64, 4)])
def test_results_do_not_depend_on_alignment(ctx, w, h):
    """The paste moves words where the pointers, the strides and w allow: every mix of aligned and unaligned sides."""
    rng = np.random.default_rng(9 + w)
    rows = np.stack([random_rows(rng, 9, w, h) for _ in range(2)])
    frames = rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8)
    (lo, lf), (ao, af) = odd_layouts(w, h), aligned_layouts(w, h)
    tight = ((6 * w, 6 * w * h, 0), (3 * w, 3 * w * h, 0))
    outs = [check(ctx, frames, rows, [9, 4], out_layout=o, frame_layout=f)
            for o, f in ((ao, af), (ao, lf), (lo, af), (lo, lf), tight)]
    assert all(np.array_equal(outs[0], x) for x in outs[1:])


def test_refusals_leave_the_outputs_untouched(ctx):
    w, h, cap, npairs = 8, 4, 6, 2
    rng = np.random.default_rng(3)
    A = Arena(4)            # every buffer a fixed distance from the others: which ranges meet is the test's to say
    frames = A.put(rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8))
    rows = A.put(random_rows(rng, npairs * cap, w, h).reshape(npairs, cap, 4))
    counts = A.put(np.int32([cap, cap]))
    out = A.take((npairs * h * 6 * w + 64,), fill=SENTINEL)
    good = dict(frames=frames.data_ptr(), npairs=npairs, step=1, w=w, h=h, rs=3 * w, fs=3 * w * h, rows=rows.data_ptr(), cap=cap,
                counts=counts.data_ptr(), status=None, points=0, color=0x00FF00, out=out.data_ptr(), ors=6 * w, ofs=6 * w * h)

    def call(**kw):
        a = dict(good, **kw)
        rc = ctx.lib.evh_draw_matches(ctx.h, a["frames"], a["npairs"], a["step"], a["w"], a["h"], a["rs"], a["fs"], a["rows"], a["cap"],
                                      a["counts"], a["status"], a["points"], a["color"], a["out"], a["ors"], a["ofs"])
        ctx.synchronize()
        return rc

    NA, EM, STEP = "NULL argument", "empty frame, no row capacity or negative npairs", "frame_step must be 1 or 2"
    PTS, COL = "unknown points value", "color_bgr has bits above 24 set"
    WCAP, SR, SF = "w above 16383 (a picture's columns are held in 16 bits)", "stride smaller than a row", "stride smaller than a frame"
    OVF, OVR = "d_frames overlaps d_out", "d_rows overlaps d_out"
    wide = dict(w=16384, rs=3 * 16384, ors=6 * 16384, fs=3 * 16384 * h, ofs=6 * 16384 * h)
    bad = [(dict(frames=None), INVALID, NA), (dict(rows=None), INVALID, NA), (dict(counts=None), INVALID, NA), (dict(out=None), INVALID, NA),
           (dict(w=0), INVALID, EM), (dict(h=0), INVALID, EM), (dict(cap=0), INVALID, EM), (dict(npairs=-1), INVALID, EM),
           (dict(step=0), INVALID, STEP), (dict(step=3), INVALID, STEP), (dict(points=2), INVALID, PTS), (dict(points=-1), INVALID, PTS),
           (dict(color=0x01000000), INVALID, COL), (dict(rs=3 * w - 1), INVALID, SR), (dict(ors=6 * w - 1), INVALID, SR),
           (dict(fs=3 * w * h - 1), INVALID, SF), (dict(ofs=6 * w * h - 1), INVALID, SF),
           (dict(out=frames.data_ptr()), INVALID, OVF), (dict(out=frames.data_ptr() + 3 * w * h * 3 - 1), INVALID, OVF),
           (dict(out=rows.data_ptr()), INVALID, OVR), (dict(out=rows.data_ptr() + npairs * cap * 16 - 1), INVALID, OVR),
           (wide, CAPACITY, WCAP),
           # two faults: the earlier check of the entry names the refusal
           (dict(frames=None, w=0), INVALID, NA), (dict(step=0, w=0), INVALID, EM), (dict(wide, color=0x01000000), INVALID, COL),
           (dict(wide, rs=3 * 16384 - 1), CAPACITY, WCAP), (dict(rs=3 * w - 1, fs=3 * w * h - 1), INVALID, SR),
           (dict(out=frames.data_ptr(), ofs=6 * w * h - 1), INVALID, SF), (dict(out=frames.data_ptr(), rows=frames.data_ptr()), INVALID, OVF)]
    keep_frames, keep_rows = frames.clone(), rows.clone()
    for kw, code, text in bad:
        assert call(**kw) == code, kw
        assert ctx.lib.evh_last_error_string(ctx.h).decode() == "evh_draw_matches: " + text, kw
    assert bool((out == SENTINEL).all()) and torch.equal(frames, keep_frames) and torch.equal(rows, keep_rows)
    assert call(npairs=0) == 0 and call(npairs=0, fs=0, ofs=0) == 0 and bool((out == SENTINEL).all())       # no pictures: nothing to do
    assert call(npairs=1, ofs=0) == 0                                 # one picture: its stride is not used
    assert call(w=16383, h=1, npairs=0, rs=3 * 16383, ors=6 * 16383) == 0
    assert call() == 0
    got = out[:npairs * h * 6 * w].cpu().numpy().reshape(npairs, h, 2 * w, 3)
    assert np.array_equal(got, DC.draw(frames.cpu().numpy(), rows.cpu().numpy(), [cap, cap]))
    assert bool((out[npairs * h * 6 * w:] == SENTINEL).all())


def test_python_draw_matches_mirrors_the_reference_function():
    from evenvizion_amd import matching_pictures, runtime
    rng = np.random.default_rng(11)
    a, b = rng.integers(0, 256, (2, 9, 21, 3), dtype=np.uint8)
    pa, pb = rng.uniform(0, 21, (15, 2)), rng.uniform(0, 9, (15, 2))
    got = matching_pictures.draw_matches(a, b, pa, pb)
    want = DC.picture(a, b, np.float32(np.concatenate([pa, pb], axis=1)))
    assert got.shape == (9, 42, 3) and np.array_equal(got, want)
    assert np.array_equal(matching_pictures.draw_matches(a, b, [], []), np.concatenate([a, b], axis=1))
    runtime.reset()


# ---- evh_batch_static_rows -----------------------------------------------------------------------------------------------------------
def valid(rows, counts):
    """The rows below every pair's count, as bits."""
    return [rows[p, :int(counts[p])].view(torch.int32).cpu().numpy() for p in range(len(counts))]


@pytest.fixture(scope="module")
def stream_ctx():
    from evenvizion_amd._lib import Context
    c = Context(device=0, max_w=W, max_h=H, max_features=500, max_frames=6)
    yield c
    c.close()


def results(n):
    return torch.zeros(n, 9, dtype=torch.float64, device="cuda"), torch.full((n,), -1, dtype=torch.int32, device="cuda")


def test_static_rows_are_refused_without_a_resident_batch():
    from evenvizion_amd._lib import Context, EvhError
    c = Context(device=0, max_w=W, max_h=H, max_features=500, max_frames=4)
    try:
        cap = c.lib.evh_orb_capacity(c.h)
        assert c.batch_static_info() == (0, 0)
        rows = torch.full((3, cap, 4), -5.0, dtype=torch.float32, device="cuda")
        counts = torch.full((3,), -5, dtype=torch.int32, device="cuda")
        status = torch.full((3,), -5, dtype=torch.int32, device="cuda")

        def raw(first, npairs, row_cap, r=rows, n=counts, s=status):
            rc = c.lib.evh_batch_static_rows(c.h, first, npairs, None if r is None else r.data_ptr(), row_cap,
                                             None if n is None else n.data_ptr(), None if s is None else s.data_ptr())
            c.synchronize()
            return rc
        assert raw(0, 1, cap) == INVALID                                   # before any batch
        frames = dev(S.make_stream(5, 4, W, H)[0])
        Hd, st = results(3)
        c.stream_homography_batch(frames, Hd, st)
        assert c.batch_static_info() == (3, cap)
        for args in ((-1, 1, cap), (0, 0, cap), (0, 4, cap), (3, 1, cap), (2, 2, cap), (0, 3, cap - 1), (0, 3, cap + 1)):
            assert raw(*args) == INVALID, args
        assert raw(0, 3, cap, r=None) == INVALID and raw(0, 3, cap, n=None) == INVALID and raw(0, 3, cap, s=None) == INVALID
        assert bool((rows == -5).all()) and bool((counts == -5).all()) and bool((status == -5).all())
        assert raw(0, 3, cap) == 0 and counts.tolist() != [-5] * 3
        # every entry that rewrites the pair buffers forgets the batch
        pts = rows[0, :int(counts[0])].cpu().numpy()
        c.compute_homography(pts)
        assert c.batch_static_info() == (0, 0) and raw(0, 1, cap) == INVALID
        with pytest.raises(EvhError):
            c.batch_static_rows()
        r1, n1, s1 = c.stream_static_batch(frames)
        assert c.batch_static_info() == (3, cap)
        c.stream_scan(r1, n1, s1)
        assert c.batch_static_info() == (0, 0)
        c.stream_homography_batch(frames, Hd, st)
        assert c.batch_static_info() == (3, cap)
        c.orb_detect_batch(frames[:2])
        assert c.batch_static_info() == (3, cap)                          # detection alone leaves the rows alone
        c.match_static_from_slots(1, 0)
        assert c.batch_static_info() == (0, 0)
        c.stream_homography_batch(frames, Hd, st)
        c.pair_from_slots(1, 0)
        assert c.batch_static_info() == (0, 0)
        with pytest.raises(EvhError):                                     # a batch that fails after its checks forgets too
            c.stream_homography_batch(frames, Hd, st)
            c.stream_homography_batch(torch.zeros((2, 8, 8, 2), dtype=torch.uint8, device="cuda"), Hd, st)
        assert c.batch_static_info() == (0, 0)
    finally:
        c.close()


@pytest.mark.parametrize("async_solve", [False, True])
def test_static_rows_after_a_stream_batch(stream_ctx, async_solve):
    """The rows, counts and front status after evh_stream_homography_batch == evh_stream_static_batch's on the same frames,
    bit for bit; a flat frame fails the front of two pairs, whose final status is the same 1."""
    c = stream_ctx
    fr = S.make_stream(5, 5, W, H)[0].copy()
    fr[2] = 128
    frames = dev(fr)
    want_rows, want_counts, want_st = [t.clone() for t in c.stream_static_batch(frames)]
    c.synchronize()
    assert want_st.tolist() == [0, 1, 1, 0] and int(want_counts[0]) > 20
    cap = want_rows.shape[1]
    assert c.batch_static_info() == (4, cap)
    c.set_async_solve(async_solve)
    try:
        Hd, st = results(4)
        c.stream_homography_batch(frames, Hd, st)
        assert c.batch_static_info() == (4, cap)
        rows, counts, status = c.batch_static_rows()
        part = c.batch_static_rows(1, 3)
        c.synchronize()
    finally:
        c.set_async_solve(False)
    assert st.tolist() == [0, 1, 1, 0]
    assert torch.equal(counts, want_counts) and torch.equal(status, want_st)
    for got, want in zip(valid(rows, counts), valid(want_rows, want_counts)):
        assert np.array_equal(got, want)
    assert torch.equal(part[1], want_counts[1:]) and torch.equal(part[2], want_st[1:])
    assert np.array_equal(valid(part[0], part[1])[2], valid(want_rows, want_counts)[3])


def test_static_rows_after_a_type_list_equal_the_oracle_composition():
    """["SIFT", "ORB"]: per type in list order match_static on the oracle's key points, concatenated, remove_double."""
    from evenvizion_amd._lib import Context
    from oracle import oracle as O
    fr = S.make_stream(5, 3, W, H)[0]
    c = Context(device=0, max_w=W, max_h=H, max_features=500, max_frames=4)
    try:
        c.sift_enable(4096)
        Hd, st = results(2)
        c.stream_homography_batch_types(dev(fr), Hd, st, ["SIFT", "ORB"])
        slots, cap = c.batch_static_info()
        assert slots == 2 and cap > c.lib.evh_orb_capacity(c.h)
        rows, counts, status = c.batch_static_rows()
        c.synchronize()
        sift = [O.sift_detect(f) for f in fr]
        orb = [O.orb_detect(f) for f in fr]
        for p in range(2):
            s1, a1, b1 = O.match_static_f32(sift[p + 1]["xy"], sift[p + 1]["desc"], sift[p]["xy"], sift[p]["desc"])
            s2, a2, b2 = O.match_static(orb[p + 1]["xy"], orb[p + 1]["desc"], orb[p]["xy"], orb[p]["desc"])
            assert s1 == 0 and s2 == 0 and int(status[p]) == 0
            wa, wb = O.remove_double(np.concatenate([a1, a2]), np.concatenate([b1, b2]))
            got = rows[p, :int(counts[p])].cpu().numpy()
            assert int(counts[p]) == len(wa) and np.array_equal(got[:, :2].view(np.int32), wa.view(np.int32))
            assert np.array_equal(got[:, 2:].view(np.int32), wb.view(np.int32))
    finally:
        c.close()


def test_static_rows_of_a_ragged_batch(stream_ctx):
    """Two segments (3 and 2 frames): pair slots 0, 1 are the first stream's, slot 2 lies between the streams, slot 3 is the
    second stream's."""
    c = stream_ctx
    a, b = S.make_stream(81, 3, W, H)[0], S.make_stream(82, 2, W, H)[0]
    wa = [t.clone() for t in c.stream_static_batch(dev(a))]
    wb = [t.clone() for t in c.stream_static_batch(dev(b))]
    Hd, st = results(4)
    state = torch.zeros(2, 18, dtype=torch.float64, device="cuda")
    c.streams_homography_batch(dev(np.concatenate([a, b])), [(0, 3, 1), (3, 2, 1)], Hd, st, state_in=state, state_out=state)
    assert c.batch_static_info() == (4, wa[0].shape[1])
    rows, counts, status = c.batch_static_rows()
    c.synchronize()
    assert counts[:2].tolist() == wa[1].tolist() and int(counts[3]) == int(wb[1][0])
    assert status[:2].tolist() == wa[2].tolist() == [0, 0] and int(status[3]) == int(wb[2][0]) == 0
    got = valid(rows, counts)
    assert all(np.array_equal(got[p], valid(wa[0], wa[1])[p]) for p in range(2)) and np.array_equal(got[3], valid(wb[0], wb[1])[0])


# ---- end to end on the reference's video --------------------------------------------------------------------------------------------
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


def expected_pictures(method, kept, numbers, **kw):
    """For every frame number f: draw_checks on the device-resized frames f - 1 | f and the rows evh_batch_static_rows hands
    out after the batch entry `method` ran on that pair."""
    from evenvizion_amd import runtime
    c = runtime.get_context(W, H, 2)
    want = {}
    for f in numbers:
        small = torch.zeros((2, H, W, 3), dtype=torch.uint8, device="cuda")
        c.resize_area(dev(np.stack([kept[f - 1], kept[f]])), small)
        Hd, st = results(1)
        getattr(c, method)(small, Hd, st, **kw)
        rows, counts, status = c.batch_static_rows()
        c.synchronize()
        assert int(status[0]) == 0 and int(counts[0]) >= 4
        s = small.cpu().numpy()
        want[f] = DC.picture(s[0], s[1], rows[0, :int(counts[0])].cpu().numpy())
    return want


def test_reference_video_orb_with_a_recording_sink():
    """features_type_list=["ORB"]: the dictionary is, bit for bit, the one the same call gives without a sink; 120 pictures
    numbered 2..121; pictures 2, 61 and 121 are draw_checks' on the device-resized frames and the rows of evh_batch_static_rows;
    ingest="auto" (the decoder's planes) gives the same bytes as "bgr"."""
    from evenvizion_amd import capture, runtime
    from evenvizion_amd.processing import get_homography_dict
    runtime.reset()
    plain = get_homography_dict(capture.VideoCapture(MP4), features_type_list=["ORB"])
    rec = Recording(capture.VideoCapture(MP4), (1, 2, 60, 61, 120, 121))
    got = []
    d = get_homography_dict(rec, features_type_list=["ORB"], matching_sink=lambda f, pic: got.append((f, pic)))
    assert d == plain and d["resize_info"] == {"h": H, "w": W}
    assert [f for f, _ in got] == list(range(2, 122))
    assert all(pic.shape == (H, 2 * W, 3) and pic.dtype == np.uint8 for _, pic in got)
    want = expected_pictures("stream_homography_batch", rec.kept, (2, 61, 121))
    for f in (2, 61, 121):
        pic = got[f - 2][1]
        print("picture %d: differing bytes %d, green pixels %d" % (f, (pic != want[f]).sum(), (pic == (0, 255, 0)).all(axis=2).sum()))
        assert np.array_equal(pic, want[f])
    auto = []
    d2 = get_homography_dict(capture.VideoCapture(MP4), features_type_list=["ORB"], ingest="auto", chunk_frames=17,
                             matching_sink=lambda f, pic: auto.append((f, pic)))
    assert d2 == d and [f for f, _ in auto] == list(range(2, 122))
    assert all(np.array_equal(x[1], y[1]) for x, y in zip(auto, got))
    own = []
    get_homography_dict(capture.VideoCapture(MP4), features_type_list=["ORB"], matching_points="own_frame",
                        matching_sink=lambda f, pic: own.append(pic) if f == 61 else None)
    assert len(own) == 1 and not np.array_equal(own[0], got[59][1])
    runtime.reset()


def test_reference_video_default_list_equals_the_recorded_dictionary(tmp_path, monkeypatch):
    """The reference's own detector list, which its recorded dictionary was made with: with a sink the dictionary still equals
    ref_dict_with_homography_matrix.json in all 120 matrices, 120 pictures arrive, and pictures 2, 61 and 121 are draw_checks' on
    the merged rows of the multi-type path.  The command line writes the same pictures as PNG files."""
    import zlib
    from evenvizion_amd import capture, component, runtime
    from evenvizion_amd.processing import get_homography_dict
    runtime.reset()
    rec = Recording(capture.VideoCapture(MP4), (1, 2, 60, 61, 120, 121))
    got = []
    d = get_homography_dict(rec, matching_sink=lambda f, pic: got.append((f, pic)))
    gold = json.load(open(GOLD))
    Hg = np.array([d[k]["H"] for k in range(2, 122)])
    G = np.array([gold[str(k)]["H"] for k in range(2, 122)])
    print("pairs equal to the recorded run to the last digit: %d of 120, max abs difference %.3e"
          % ((np.abs(Hg - G).reshape(120, -1).max(1) == 0).sum(), np.abs(Hg - G).max()))
    assert np.array_equal(Hg, G)
    assert [f for f, _ in got] == list(range(2, 122))
    want = expected_pictures("stream_homography_batch_types", rec.kept, (2, 61, 121), features=["SURF", "SIFT", "ORB"])
    for f in (2, 61, 121):
        assert np.array_equal(got[f - 2][1], want[f]), f
    monkeypatch.chdir(tmp_path)
    folder = component.main(["--path_to_video", MP4, "--experiment_name", "e2e", "--heatmap_visualization", "0",
                             "--matching_pictures", "1"])
    names = sorted(os.listdir(os.path.join(folder, "matching_visualization")))
    assert names == sorted("matching_vis_%d.png" % f for f in range(2, 122))
    data = open(os.path.join(folder, "matching_visualization", "matching_vis_61.png"), "rb").read()
    at = data.index(b"IDAT")
    n = int.from_bytes(data[at - 4:at], "big")
    raw = np.frombuffer(zlib.decompress(data[at + 4:at + 4 + n]), np.uint8).reshape(H, 1 + 6 * W)
    assert np.array_equal(raw[:, 1:].reshape(H, 2 * W, 3)[:, :, ::-1], got[59][1])
    runtime.reset()
