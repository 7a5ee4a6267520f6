"""evh_rows_moving_filter / evh_rows_moving_filter_yuv420 on the device.  Every assertion is equality of bytes or bit patterns with
the numpy restatement of the header's contract (tests/moving_checks.py, itself checked against a literal loop in
test_moving_host.py) or with the library's own entries, on buffers padded with a sentinel that must survive."""
import ctypes
import json
import os

import numpy as np
import pytest

import moving_checks as MC
import plate_checks as P
import warp_checks as W
from refusal_arena import Arena
from test_gpu_warp import NOTHING, rot_zoom_persp

pytestmark = pytest.mark.gpu
SENTINEL = 0xCD
WORD = np.uint32(0xCDCDCDCD)
GUARD = 8                                   # sentinel elements in front of and behind every output
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MP4 = os.path.join(ROOT, "tests", "golden", "ref_test_video.mp4")


@pytest.fixture(scope="module")
def ctx():
    from evenvizion_amd._lib import Context
    c = Context(device=0, max_w=64, max_h=64, max_features=500, max_frames=2)     # the filter does not depend on these sizes
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def padded(shape, dtype):
    """-> (the whole buffer, the contiguous view of `shape` GUARD elements into it), all sentinel bytes; the view of a float32
    buffer starts on a 16-byte boundary."""
    import torch
    size = int(np.prod(shape))
    raw = torch.full(((size + 2 * GUARD) * torch.empty(0, dtype=dtype).element_size(),), SENTINEL, dtype=torch.uint8, device="cuda")
    whole = raw.view(dtype)
    return whole, whole[GUARD:GUARD + size].view(shape)


def sentinel_outputs(npairs, cap):
    return (np.full((npairs, cap, 4), WORD, np.uint32).view(np.float32), np.full(npairs, WORD, np.uint32).view(np.int32),
            np.full(npairs, WORD, np.uint32).view(np.int32), np.full((npairs, cap), SENTINEL, np.uint8))


def run(ctx, frames, mats, plate, count, origin, rows, counts, status1, with_moving=True, with_flags=True, src_pad=0, out_pad=0,
        out_skip=0, size=None, **kw):
    """Through Context.rows_moving_filter -> (out_rows, out_counts, moving or None, flags or None) as numpy.  frames: an array
    u8[n,sh,sw(,3)] (uploaded into rows src_pad pixels wider) or device planes.  plate and count are views of wider, taller
    tensors (out_pad extra pixels per row, starting out_skip pixels in).  The outputs are padded with a sentinel in front and
    behind, which must survive, as must every input."""
    import torch
    if isinstance(frames, np.ndarray):
        n, sh, sw = frames.shape[:3]
        full = torch.full((n, sh + 1, sw + src_pad) + frames.shape[3:], SENTINEL, dtype=torch.uint8, device="cuda")
        full[:, :sh, :sw] = dev(frames)
        src = full[:, :sh, :sw]
    else:
        src = frames
    plate, count = np.asarray(plate), np.asarray(count)
    dh, dw = count.shape
    wide = out_skip + dw + out_pad
    inside = (slice(0, dh), slice(out_skip, out_skip + dw))
    pfull = torch.full((dh + 1, wide) + plate.shape[2:], SENTINEL, dtype=torch.uint8, device="cuda")
    cfull = torch.full((dh + 1, wide), SENTINEL, dtype=torch.uint8, device="cuda")
    pfull[inside] = dev(plate)
    cfull[inside] = dev(count)
    npairs, cap = rows.shape[:2]
    d_rows, d_counts, d_status = dev(np.asarray(rows, np.float32)), dev(np.asarray(counts, np.int32)), dev(np.asarray(status1, np.int32))
    whole, view = zip(padded((npairs, cap, 4), torch.float32), padded((npairs,), torch.int32), padded((npairs,), torch.int32),
                      padded((npairs, cap), torch.uint8))
    ctx.rows_moving_filter(src, dev(np.asarray(mats, np.float64).reshape(-1, 9)), pfull[inside], cfull[inside], origin, d_rows,
                           d_counts, d_status, view[0], view[1], view[2] if with_moving else None, view[3] if with_flags else None,
                           size=size, **kw)
    ctx.synchronize()
    asked = (True, True, with_moving, with_flags)
    out = []
    for w_, v, ask in zip(whole, view, asked):
        raw = w_.view(torch.uint8).cpu().numpy()
        item = w_.element_size()
        assert (raw[:GUARD * item] == SENTINEL).all() and (raw[-GUARD * item:] == SENTINEL).all(), "the guard of an output was written"
        if not ask:
            assert (raw == SENTINEL).all(), "an output that was not handed over was written"
        out.append(v.cpu().numpy() if ask else None)
    assert np.array_equal(d_rows.cpu().numpy().view(np.uint32), np.asarray(rows, np.float32).view(np.uint32))
    assert np.array_equal(pfull[inside].cpu().numpy(), plate) and np.array_equal(cfull[inside].cpu().numpy(), count)
    return tuple(out)


def same(got, want, what=""):
    names = ("out_rows", "out_counts", "moving", "flags")
    for g, w_, name in zip(got, want, names):
        if g is not None:
            a, b = (g.view(np.uint32), w_.view(np.uint32)) if name == "out_rows" else (g, w_)
            print("%s %s: differing elements %d of %d" % (what, name, (a != b).sum(), b.size))
    for g, w_, name in zip(got, want, names):
        if g is not None:
            a, b = (g.view(np.uint32), w_.view(np.uint32)) if name == "out_rows" else (g, w_)
            assert np.array_equal(a, b), "%s %s" % (what, name)


def check(ctx, frames, mats, plate, count, origin, rows, counts, status1, host_frames=None, **kw):
    """The device against the restatement, both starting from sentinel outputs -> the expected outputs."""
    npairs, cap = rows.shape[:2]
    want = MC.rows_filter(frames if host_frames is None else host_frames, mats, plate, count, origin, rows, counts, status1,
                          *sentinel_outputs(npairs, cap),
                          **{k: v for k, v in kw.items() if k not in ("with_moving", "with_flags", "src_pad", "out_pad", "out_skip", "size")})
    got = run(ctx, frames, mats, plate, count, origin, rows, counts, status1, **kw)
    same(got, want, str({k: v for k, v in kw.items()}))
    return want


# ---- against the restatement ------------------------------------------------------------------------------------------------------
SW, SH, DW, DH, ORIGIN = 23, 17, 40, 26, (-4, -3)
ODD = [np.nan, -np.nan, np.inf, -np.inf, 1e30, -1e30, 3e9, 2.0 ** 31, -0.0, -1.0, -0.5, 0.5, 1.5, 2.5, 7.49, 7.51, 22.5, 16.5, 1e-30]


def staggered(gray, projective, seed=70):
    """5 frames of 23 x 17 that show a common background through their matrices, each with its own rectangle of noise, on a canvas
    some of them leave on every side."""
    rng = np.random.default_rng(seed)
    if projective:
        mats = np.stack([rot_zoom_persp(9.0, 1.1, 3.5, -2.25, 1e-3, -2e-3), rot_zoom_persp(-6, 0.95, 8, 3, 5e-4, -3e-4),
                         W.translation(6.25, 2.75), rot_zoom_persp(4, 1.05, 14, 6, 0, 1e-3), np.eye(3)])
    else:
        mats = np.stack([W.translation(-9, -6), W.translation(2, 1), W.translation(7, 3), W.translation(14, 8), W.translation(20, -5)])
    B = rng.integers(0, 256, (80, 100) if gray else (80, 100, 3)).astype(np.uint8)
    frames = []
    for k in range(5):
        # the frame's own picture of the background: the background sampled where the frame's pixels land
        cx, cy, _ = MC.canvas_points(np.stack(np.meshgrid(np.arange(SW), np.arange(SH)), -1).reshape(-1, 2).astype(np.float32), mats[k])
        f = B[np.clip(cy + 30, 0, 79), np.clip(cx + 30, 0, 99)].reshape((SH, SW) + B.shape[2:]).copy()
        x0, y0 = 3 + 3 * k, 2 + 2 * k
        f[y0:y0 + 6, x0:x0 + 7] = rng.integers(0, 256, (6, 7) + B.shape[2:])
        frames.append(f)
    return np.stack(frames), mats


def pixel_rows(npairs, seed, scale=(1.0, 1.0)):
    """Rows from every integer pixel of the frames (a in order, b permuted), then the odd coordinates; in the units row_scale
    takes back to frame pixels."""
    rng = np.random.default_rng(seed)
    grid = np.stack(np.meshgrid(np.arange(SW), np.arange(SH)), -1).reshape(-1, 2).astype(np.float64)
    cap = len(grid) + len(ODD) + 5
    rows = np.full((npairs, cap, 4), 77.0, np.float32)
    for p in range(npairs):
        rows[p, :len(grid), 0:2] = grid / scale
        rows[p, :len(grid), 2:4] = grid[rng.permutation(len(grid))] / scale
        for i, v in enumerate(ODD):
            rows[p, len(grid) + i] = [v, ODD[(i + p + 1) % len(ODD)], ODD[(i + 5) % len(ODD)], 4.0] if i % 2 else [3.0, 5.0, 6.25, v]
    return rows, np.full(npairs, len(grid) + len(ODD), np.int32), cap


CONFIGS = [dict(radius=0, min_hits=1, min_cover=1, threshold=16), dict(radius=1, min_hits=1, min_cover=2, threshold=16),
           dict(radius=1, min_hits=9, min_cover=1, threshold=0), dict(radius=7, min_hits=1, min_cover=2, threshold=16),
           dict(radius=7, min_hits=225, min_cover=1, threshold=0), dict(radius=7, min_hits=40, min_cover=1, threshold=16),
           dict(radius=0, min_hits=1, min_cover=255, threshold=0), dict(radius=1, min_hits=1, min_cover=1, threshold=255),
           dict(radius=1, min_hits=2, min_cover=2, threshold=0, row_scale=(1170 / 400, 658 / 224)),
           dict(radius=0, min_hits=1, min_cover=1, threshold=16, frame_step=2),
           dict(radius=1, min_hits=3, min_cover=1, threshold=16, src_pad=3, out_pad=1, out_skip=0),
           dict(radius=1, min_hits=3, min_cover=1, threshold=16, src_pad=1, out_pad=2, out_skip=1, with_moving=False),
           dict(radius=0, min_hits=1, min_cover=2, threshold=0, src_pad=0, out_pad=1, out_skip=1, with_flags=False)]


@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("projective", [False, True])
def test_against_the_restatement(ctx, gray, projective):
    frames, mats = staggered(gray, projective)
    plates = {mc: P.plate(frames, mats, DW, DH, ORIGIN, None, False, mc, 16)[:2] for mc in (1, 2, 255)}
    assert plates[1][1].max() >= 3 and (plates[1][1] == 0).any()
    seen = set()
    for cfg in CONFIGS:
        step = cfg.get("frame_step", 1)
        rows, counts, cap = pixel_rows(4 // step, 71, cfg.get("row_scale", (1.0, 1.0)))
        plate, count = plates[cfg["min_cover"]]
        want = check(ctx, frames, mats, plate, count, ORIGIN, rows, counts, np.zeros(len(counts), np.int32), min_keep=0, **cfg)
        assert want[2] is not None and (want[1] == counts - want[2]).all()
        if cfg["threshold"] == 255 or cfg["min_cover"] == 255:
            assert not want[2].any()
        seen.update(np.unique(want[3][:, :counts[0]]).tolist())
    assert seen == {0, 1, 2, 3}                          # neither, a only, b only, both


def test_flags_equal_the_masks_of_the_plate_entry(ctx):
    """For the plate's own frames, at radius 0 and min_hits 1, a point is moving iff the mask evh_plate_fixed_plane writes for its
    frame is set at the point's canvas pixel."""
    import torch
    for gray in (False, True):
        for projective in (False, True):
            frames, mats = staggered(gray, projective, seed=72)
            plate = torch.zeros((DH, DW) + frames.shape[3:], dtype=torch.uint8, device="cuda")
            count = torch.zeros((DH, DW), dtype=torch.uint8, device="cuda")
            masks = torch.zeros((5, DH, DW), dtype=torch.uint8, device="cuda")
            ctx.plate_fixed_plane(dev(frames), dev(mats.reshape(5, 9)), plate, ORIGIN, count=count, masks=masks, threshold=12, min_cover=2)
            ctx.synchronize()
            rows, counts, cap = pixel_rows(4, 73)
            got = run(ctx, frames, mats, plate.cpu().numpy(), count.cpu().numpy(), ORIGIN, rows, counts, np.zeros(4, np.int32),
                      threshold=12, min_cover=2, radius=0, min_hits=1, min_keep=0)
            m = masks.cpu().numpy()
            for p in range(4):
                n = counts[p]
                want = np.zeros(n, np.uint8)
                for bit, (cols, f) in enumerate(((slice(0, 2), p + 1), (slice(2, 4), p))):
                    cx, cy, usable = MC.canvas_points(rows[p, :n, cols], mats[f])
                    X, Y = cx - ORIGIN[0], cy - ORIGIN[1]
                    inside = usable & (X >= 0) & (X < DW) & (Y >= 0) & (Y < DH)
                    want |= (inside & (m[f][np.where(inside, Y, 0), np.where(inside, X, 0)] != 0)).astype(np.uint8) << bit
                assert np.array_equal(got[3][p, :n], want) and want.any() and not want.all()


# ---- compaction --------------------------------------------------------------------------------------------------------------------
def hot_and_cold(nframes):
    """Gray frames of 32 x 16 under the identity on a canvas of their size, all 0 but pixel (0, 0) = 255, against a plate of
    zeros that every pixel counts for: with threshold 0 and radius 0 a point is moving iff it rounds to (0, 0)."""
    frames = np.zeros((nframes, 16, 32), np.uint8)
    frames[:, 0, 0] = 255
    return frames, np.stack([np.eye(3)] * nframes), np.zeros((16, 32), np.uint8), np.ones((16, 32), np.uint8)


def pattern_rows(patterns, cap):
    """patterns: one bool array per pair (row i is moving) -> rows whose payload tells them apart: cold points all over the
    frame, and -0.0 and NaN payloads that must come through bit for bit."""
    rows = np.full((len(patterns), cap, 4), 55.0, np.float32)
    for p, moving in enumerate(patterns):
        for i, hot in enumerate(moving):
            rows[p, i] = [0.0 if hot else 1 + i % 31, 0.25 if hot else 1 + (i // 31) % 15, 1 + (i * 7) % 31, 1 + (i * 3) % 15]
            if i % 5 == 1:
                rows[p, i, 3] = -0.0 if hot else np.nan
        bits = rows[p].view(np.uint32)
        bits[np.flatnonzero(~np.asarray(moving, bool))[2::11], 2] = 0x7FC12345        # b.x a NaN with a payload: not moving, kept
    return rows


@pytest.mark.parametrize("with_outputs", [True, False])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129, 500])
def test_compaction_keeps_order_and_bit_patterns(ctx, n, with_outputs):
    frames, mats, plate, count = hot_and_cold(8)
    i = np.arange(n)
    patterns = [np.ones(n, bool), np.zeros(n, bool), i % 2 == 0, i % 2 == 1, i == 0, i == n - 1, (i * 7 % 13) < 5]
    rows = pattern_rows(patterns, 500)
    counts = np.full(len(patterns), n, np.int32)
    want = check(ctx, frames, mats, plate, count, (0, 0), rows, counts, np.zeros(len(patterns), np.int32), threshold=0, min_cover=1,
                 radius=0, min_hits=1, min_keep=0, with_moving=with_outputs, with_flags=with_outputs)
    if n:
        assert want[2].tolist() == [int(np.sum(m)) for m in patterns]
        for p, m in enumerate(patterns):
            assert np.array_equal(want[0][p, :n - m.sum()].view(np.uint32), rows[p, :n][~m].view(np.uint32))
            assert (want[0][p, n - m.sum():].view(np.uint32) == WORD).all()
    else:
        assert want[1].tolist() == [0] * len(patterns) and (want[0].view(np.uint32) == WORD).all()


def test_min_keep(ctx):
    frames, mats, plate, count = hot_and_cold(5)
    moving = np.arange(20) % 5 < 3                                        # 12 of 20 moving: 8 survive
    rows = pattern_rows([moving, moving, np.ones(20, bool), np.ones(20, bool)], 24)
    counts = np.full(4, 20, np.int32)
    kw = dict(threshold=0, min_cover=1, radius=0, min_hits=1)
    at = check(ctx, frames, mats, plate, count, (0, 0), rows, counts, np.zeros(4, np.int32), min_keep=8, **kw)
    assert at[1].tolist() == [8, 8, 20, 20] and at[2].tolist() == [12, 12, 20, 20]
    above = check(ctx, frames, mats, plate, count, (0, 0), rows, counts, np.zeros(4, np.int32), min_keep=9, **kw)
    assert above[1].tolist() == [20] * 4 and above[2].tolist() == [12, 12, 20, 20]
    assert np.array_equal(above[0][:, :20].view(np.uint32), rows[:, :20].view(np.uint32))
    none = check(ctx, frames, mats, plate, count, (0, 0), rows, counts, np.zeros(4, np.int32), min_keep=0, **kw)
    assert none[1].tolist() == [8, 8, 0, 0] and (none[0][2:].view(np.uint32) == WORD).all()


def test_pairs_whose_front_status_is_not_ok(ctx):
    frames, mats = staggered(False, False)
    frames, mats = np.concatenate([frames, frames[:2]]), np.concatenate([mats, mats[:2]])
    plate, count, _ = P.plate(frames, mats, DW, DH, ORIGIN)
    rows, _, cap = pixel_rows(6, 74)
    counts = np.array([cap + 7, 5, -3, 0, 2 ** 31 - 1, cap], np.int32)
    status1 = np.array([0, 3, 0, 0, -2, 0], np.int32)
    want = check(ctx, frames, mats, plate, count, ORIGIN, rows, counts, status1, threshold=16, radius=1, min_keep=3)
    assert want[1][[1, 2, 3, 4]].tolist() == [5, -3, 0, 2 ** 31 - 1] and want[2][[1, 2, 3, 4]].tolist() == [0] * 4
    assert (want[0][1:5].view(np.uint32) == WORD).all() and (want[3][1:5] == SENTINEL).all()
    assert want[2][0] > 0 and want[1][0] == cap - want[2][0] and (want[3][0] != SENTINEL).all()     # a count above the capacity: cap rows


@pytest.mark.parametrize("name", sorted(k for k, v in NOTHING.items() if not v[1]))
def test_matrices_that_cover_nothing(ctx, name):
    bad = NOTHING[name][0]
    frames, mats = staggered(False, False, seed=75)
    good_plate, good_count, _ = P.plate(frames, mats, DW, DH, ORIGIN)
    mats = mats.copy()
    mats[1], mats[3] = bad, bad
    rows, counts, cap = pixel_rows(4, 76)
    with np.errstate(all="ignore"):
        want = check(ctx, frames, mats, good_plate, good_count, ORIGIN, rows, counts, np.zeros(4, np.int32), threshold=0, radius=1,
                     min_hits=1, min_keep=0)
    n = counts[0]
    flags = want[3][:, :n]
    assert not (flags[[0, 2]] & 1).any() and not (flags[[1, 3]] & 2).any()      # no end point on frame 1 or 3 is ever moving
    assert (flags[[0, 2]] & 2).any() and (flags[[1, 3]] & 1).any()              # the frames between them still judge theirs


# ---- planes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(24, 16), (8, 6)])
def test_planes_equal_the_bgr_entry_on_the_converted_frames(ctx, w, h):
    import torch
    rng = np.random.default_rng(77)
    n, cw, ch = 4, (w + 1) // 2, (h + 1) // 2
    planes = [(rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8),
               rng.integers(0, 256, (ch, cw), dtype=np.uint8)) for _ in range(n)]
    bgr = W.planes_to_bgr(planes)
    mats = np.stack([np.eye(3), rot_zoom_persp(12, 1.2, 8, 3, 5e-4, -3e-4), W.translation(6.25, 2.75), W.translation(-2, 3)])
    dw, dh, origin = 44, 30, (-5, -4)
    plate, count, _ = P.plate(bgr, mats, dw, dh, origin, None, False, 1, 10)
    grid = np.stack(np.meshgrid(np.arange(w), np.arange(h)), -1).reshape(-1, 2).astype(np.float32)
    rows = np.zeros((3, len(grid) + 2, 4), np.float32)
    rows[:, :len(grid), 0:2] = grid + 0.25
    rows[:, :len(grid), 2:4] = grid[::-1]
    counts = np.full(3, len(grid), np.int32)
    kw = dict(threshold=10, min_cover=1, radius=1, min_hits=2, min_keep=0)
    want = MC.rows_filter(bgr, mats, plate, count, origin, rows, counts, np.zeros(3, np.int32), *sentinel_outputs(3, len(grid) + 2), **kw)
    assert 0 < want[2].sum() < counts.sum()
    y, cb, cr = (dev(np.stack([p[i] for p in planes])) for i in range(3))
    uv = torch.stack([cb, cr], dim=-1).contiguous()
    packed = dev(np.stack([np.concatenate([a.reshape(-1) for a in p]) for p in planes]))
    conv = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    ctx.yuv420_to_bgr((y, cb, cr), conv)
    ctx.synchronize()
    assert np.array_equal(conv.cpu().numpy(), bgr)
    for name, src, size in (("bgr", conv[:, :h, :w], None), ("i420", (y, cb, cr), None), ("nv12", (y, uv[..., 0], uv[..., 1]), None),
                            ("packed", packed, (w, h))):
        same(run(ctx, src, mats, plate, count, origin, rows, counts, np.zeros(3, np.int32), size=size, **kw), want, name)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(ctx):
    import torch
    from evenvizion_amd._lib import Yuv420
    INVALID, CAPACITY = -1, -3
    n, sw, sh, dw, dh, npairs, cap = 3, 23, 17, 31, 22, 2, 12
    A = Arena(13)           # every buffer a fixed distance from the others: which ranges meet is the test's to say
    src = A.put(np.random.default_rng(78).integers(0, 256, (n, sh, sw, 3), dtype=np.uint8))
    mats = A.put(np.tile(np.eye(3).reshape(1, 9), (n, 1)))
    plate = A.take((dh, dw, 3))
    count = A.take((dh, dw), fill=1)
    rows = A.take((npairs, cap, 4), torch.float32, 1.0)
    counts = A.take((npairs,), torch.int32, cap)
    status = A.take((npairs,), torch.int32)
    out_rows = A.take((npairs, cap, 4), torch.float32, -7.0)
    out_counts = A.take((npairs,), torch.int32, -7)
    moving = A.take((npairs,), torch.int32, -7)
    flags = A.take((npairs, cap), fill=SENTINEL)
    f, m, p, c, r, k, s, o, oc, mv, fl = (t.data_ptr() for t in (src, mats, plate, count, rows, counts, status, out_rows, out_counts,
                                                                   moving, flags))
    rs, fs, prs = sw * 3, sw * sh * 3, dw * 3
    good = dict(ctx=ctx.h, frames=f, n=n, sw=sw, sh=sh, cn=3, rs=rs, fs=fs, M=m, plate=p, prs=prs, count=c, crs=dw, dw=dw, dh=dh,
                ox=0, oy=0, mc=1, thr=16, rad=1, hits=1, sx=1.0, sy=1.0, rows=r, cap=cap, counts=k, st=s, np=npairs, step=1, keep=0,
                orows=o, ocounts=oc, moving=mv, flags=fl)
    tail = ("M", "plate", "prs", "count", "crs", "dw", "dh", "ox", "oy", "mc", "thr", "rad", "hits", "sx", "sy", "rows", "cap",
            "counts", "st", "np", "step", "keep", "orows", "ocounts", "moving", "flags")

    def call(**kw):
        a = dict(good, **kw)
        return ctx.lib.evh_rows_moving_filter(a["ctx"], a["frames"], a["n"], a["sw"], a["sh"], a["cn"], a["rs"], a["fs"],
                                              *[a[t] for t in tail])

    nan, inf = float("nan"), float("inf")
    who, who_yuv = "evh_rows_moving_filter: ", "evh_rows_moving_filter_yuv420: "
    NS, NA, CH, EM = "NULL source", "NULL argument", "channels must be 1 or 3", "empty frame, canvas or row block"
    STEP, MC, TH, RAD = "frame_step must be 1 or 2", "min_cover must lie in 1..255", "threshold must lie in 0..255", "radius must lie in 0..7"
    HITS, KEEP = "min_hits must lie in 1..(2*radius+1)^2", "min_keep must not be negative"
    SXY, NP = "row_sx and row_sy must be finite and positive", "at most 65535 pairs per call"
    BIG, AREA = "source sizes stay below 2^26 (positions are held in 1/32 pixels)", "dw * dh above INT_MAX"
    REACH, SS = "nframes does not reach the last pair's frames", "source stride smaller than a row / frame"
    PS, CTS, AL = "plate stride smaller than a row", "count stride smaller than a row", "d_rows and d_out_rows must be 16-byte aligned"

    def over(a, b):
        return "%s overlaps %s" % (a, b)
    OR, OC, MV, FL, FR = "d_out_rows", "d_out_counts", "d_moving", "d_flags", "the frames"

    def refused(rc, code, text, what):
        assert rc == code, what
        assert ctx.lib.evh_last_error_string(ctx.h).decode() == text, what

    assert call(ctx=None) == INVALID
    invalid = [(dict(frames=None), NS)] + [(dict([(a, None)]), NA) for a in ("M", "plate", "count", "rows", "counts", "st", "orows", "ocounts")]
    invalid += [(dict(cn=2), CH), (dict(cn=0), CH), (dict(cn=4), CH), (dict(sw=0), EM), (dict(sh=0), EM), (dict(dw=0), EM), (dict(dh=-1), EM),
                (dict(cap=0), EM), (dict(n=-1), EM), (dict(np=-1), EM), (dict(step=0), STEP), (dict(step=3), STEP), (dict(n=2), REACH),
                (dict(n=0), REACH), (dict(step=2), REACH), (dict(mc=0), MC), (dict(mc=256), MC), (dict(thr=-1), TH), (dict(thr=256), TH),
                (dict(rad=-1), RAD), (dict(rad=8), RAD), (dict(hits=0), HITS), (dict(hits=10), HITS), (dict(rad=0, hits=2), HITS),
                (dict(rad=7, hits=226), HITS), (dict(keep=-1), KEEP), (dict(sx=0.0), SXY), (dict(sy=-1.0), SXY), (dict(sx=nan), SXY),
                (dict(sy=inf), SXY), (dict(sx=-inf), SXY), (dict(rs=rs - 1), SS), (dict(fs=fs - 1), SS), (dict(prs=prs - 1), PS),
                (dict(crs=dw - 1), CTS), (dict(rows=r + 4), AL), (dict(orows=o + 8), AL),
                # an output over an input or another output
                (dict(orows=r), over(OR, "d_rows")), (dict(orows=r + 16 * (npairs * cap - 1)), over(OR, "d_rows")), (dict(orows=f), over(OR, FR)),
                (dict(ocounts=k), over(OC, "d_counts")), (dict(ocounts=s), over(OC, "d_status1")), (dict(moving=oc), over(OC, MV)),
                (dict(moving=m), over(MV, "d_M")), (dict(flags=p), over(FL, "d_plate")), (dict(flags=c + dw * dh - 1), over(FL, "d_count")),
                (dict(flags=o), over(OR, FL)), (dict(flags=mv), over(MV, FL)), (dict(ocounts=mv + 4), over(OC, MV)),
                (dict(moving=r + 16), over(MV, "d_rows")), (dict(flags=f + n * fs - 1), over(FL, FR)),
                # two faults: the earlier check of the entry names the refusal
                (dict(frames=None, rows=None), NS), (dict(M=None, cn=2), NA), (dict(np=65536, n=65537, mc=0), MC), (dict(prs=prs - 1, rs=rs - 1), PS),
                (dict(orows=r, prs=prs - 1), PS), (dict(rows=r + 4, flags=p), AL), (dict(orows=r, ocounts=k), over(OR, "d_rows")),
                (dict(moving=m, flags=o), over(OR, FL))]
    for kw, text in invalid:
        refused(call(**kw), INVALID, who + text, kw)
    big = 1 << 26
    capacity = [(dict(np=65536, n=65537), NP), (dict(sw=big, rs=big * 3, fs=big * 3 * sh), BIG), (dict(sh=big, fs=sw * 3 * big), BIG),
                (dict(dw=65536, dh=32768, prs=65536 * 3, crs=65536), AREA),
                # two faults: a capacity refusal precedes the reach of the frames, the strides and the overlaps
                (dict(sw=big, rs=big * 3 - 1, fs=big * 3 * sh), BIG), (dict(n=2, sw=big), BIG), (dict(np=65536, n=3), NP), (dict(sh=big, orows=r), BIG)]
    for kw, text in capacity:
        refused(call(**kw), CAPACITY, who + text, kw)
    y = A.take((n, sh, sw))
    cc = A.take((2, n, 9, 12))
    yuv = dict(d_y=y.data_ptr(), d_cb=cc[0].data_ptr(), d_cr=cc[1].data_ptr(), y_stride=sw, c_stride=12, y_frame_stride=sw * sh,
               c_frame_stride=12 * 9, c_pixel_stride=1)

    def call_yuv(desc, **kw):
        a = dict(good, **kw)
        d = None if desc is None else ctypes.byref(Yuv420(**desc))
        return ctx.lib.evh_rows_moving_filter_yuv420(a["ctx"], d, a["n"], a["sw"], a["sh"], *[a[t] for t in tail])

    refused(call_yuv(None), INVALID, who_yuv + NS, "no description")
    CPS, PLANE = "chroma pixel stride must be 1 or 2", "frame stride smaller than a plane"
    for bad, text in ((dict(d_y=None), NS), (dict(d_cb=None), NS), (dict(d_cr=None), NS), (dict(c_pixel_stride=3), CPS),
                      (dict(y_stride=sw - 1), "luma row stride smaller than the width"),
                      (dict(c_stride=11), "chroma row stride smaller than a chroma row"),
                      (dict(y_frame_stride=sw * sh - 1), PLANE), (dict(c_frame_stride=12 * 9 - 1), PLANE)):
        refused(call_yuv(dict(yuv, **bad)), INVALID, who_yuv + text, bad)
    for kw, text in ((dict(M=None), NA), (dict(count=None), NA), (dict(dw=0), EM), (dict(mc=0), MC), (dict(thr=256), TH), (dict(rad=8), RAD),
                     (dict(prs=prs - 1), PS), (dict(n=2), REACH), (dict(orows=r), over(OR, "d_rows")), (dict(flags=y.data_ptr()), over(FL, FR)),
                     (dict(moving=cc[1].data_ptr()), over(MV, FR)), (dict(ocounts=cc[0].data_ptr()), over(OC, FR))):   # the last: over the Cb plane
        refused(call_yuv(yuv, **kw), INVALID, who_yuv + text, kw)
    # two faults, one of them in the description: a NULL plane first, the strides before the planes, the planes before the overlaps
    refused(call_yuv(dict(yuv, d_y=None), M=None), INVALID, who_yuv + NS, "NULL plane before NULL argument")
    refused(call_yuv(dict(yuv, y_stride=sw - 1), prs=prs - 1), INVALID, who_yuv + PS, "strides before the description")
    refused(call_yuv(dict(yuv, c_pixel_stride=3), orows=r), INVALID, who_yuv + CPS, "the description before the overlaps")
    refused(call_yuv(dict(yuv, c_pixel_stride=3), np=65536, n=65537), CAPACITY, who_yuv + NP, "capacity before the description")
    for kw, text in ((dict(np=65536, n=65537), NP), (dict(sw=big), BIG), (dict(dw=65536, dh=32768, prs=65536 * 3, crs=65536), AREA)):
        refused(call_yuv(yuv, **kw), CAPACITY, who_yuv + text, kw)
    assert call(np=0) == 0 and call(np=0, n=0) == 0 and call_yuv(yuv, np=0) == 0           # no pairs: nothing is done
    ctx.synchronize()
    assert (out_rows == -7.0).all() and (out_counts == -7).all() and (moving == -7).all() and (flags == SENTINEL).all()
    # and the same arguments unrefused do write
    assert call() == 0 and call_yuv(yuv, moving=None, flags=None) == 0
    ctx.synchronize()
    assert (out_counts >= 0).all() and (moving >= 0).all() and (flags != SENTINEL).all()


# ---- what it is for ----------------------------------------------------------------------------------------------------------------
def test_panning_scene_rows_lose_the_moving_square(ctx):
    import torch
    from evenvizion_amd._lib import PAIR_OK
    B, frames, mats, squares = P.panning_scene()
    plate = torch.zeros((40, 60, 3), dtype=torch.uint8, device="cuda")
    count = torch.zeros((40, 60), dtype=torch.uint8, device="cuda")
    ctx.plate_fixed_plane(dev(frames), dev(mats.reshape(9, 9)), plate, (0, 0), count=count, min_cover=2)
    ctx.synchronize()
    rows, counts, background, cap = MC.scene_rows()
    status1 = np.zeros(8, np.int32)
    out_rows, out_counts, moving, flags = run(ctx, frames, mats, plate.cpu().numpy(), count.cpu().numpy(), (0, 0), rows, counts, status1,
                                              threshold=0, min_cover=2, radius=0, min_hits=1, min_keep=4)
    clean = np.zeros_like(rows)
    for p in range(8):
        print("pair %d: %d rows, %d moving, %d kept, %d background rows" % (p, counts[p], moving[p], out_counts[p], len(background[p])))
        assert moving[p] == 16 and out_counts[p] == len(background[p]) and np.array_equal(out_rows[p, :out_counts[p]], background[p])
        clean[p, :len(background[p])] = background[p]
    # the solve sees what it would have seen had the square never been matched
    got_H, got_st = ctx.stream_scan(dev(out_rows), dev(out_counts), dev(status1))
    want_H, want_st = ctx.stream_scan(dev(clean), dev(out_counts), dev(status1))
    ctx.synchronize()
    assert np.array_equal(got_H.cpu().numpy().view(np.uint64), want_H.cpu().numpy().view(np.uint64))
    assert np.array_equal(got_st.cpu().numpy(), want_st.cpu().numpy()) and (got_st.cpu().numpy() == PAIR_OK).all()
    assert np.isfinite(got_H.cpu().numpy()).all()


# ---- the second pass on the reference's video --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def passes():
    from evenvizion_amd import capture, moving
    from evenvizion_amd import stabilization as S
    from evenvizion_amd.processing.utils import superposition_dict
    from evenvizion_amd.processing.video_processing import get_homography_dict
    kw = dict(nfeatures=500, chunk_frames=16, features_type_list=["ORB"])
    first = get_homography_dict(capture.VideoCapture(MP4), resize_width=400, ingest="bgr", **kw)
    ri = first["resize_info"]
    sup = superposition_dict({k: v for k, v in first.items() if k != "resize_info"})
    plate = S.background_plate(capture.VideoCapture(MP4), sup, ri, placement="warp", max_frames=16, ingest="bgr")

    def refine(**more):
        return moving.refine_homography_dict(capture.VideoCapture(MP4), first, plate, **dict(kw, **more))
    return first, plate, refine


def test_refine_with_nothing_to_reject_is_the_first_pass(passes):
    first, plate, refine = passes
    refined, stats = refine(threshold=255, ingest="bgr")
    assert list(refined) == list(first) and refined["resize_info"] == first["resize_info"] and len(first) == 121
    for k in first:
        if k != "resize_info":
            assert np.array_equal(np.array(refined[k]["H"]).view(np.uint64), np.array(first[k]["H"]).view(np.uint64)), k
    assert sorted(stats) == list(range(2, 122)) and all(m == 0 and a == b for a, m, b in stats.values())
    assert max(a for a, _, _ in stats.values()) > 8


def test_refine_rejects_rows_and_planes_agree(passes):
    first, plate, refine = passes
    refined, stats = refine(threshold=16, ingest="bgr", min_keep=8)
    print("rows %d, moving %d, handed on %d" % tuple(sum(s[i] for s in stats.values()) for i in range(3)))
    for k, (rows, moving, rows_out) in stats.items():
        assert 0 <= moving <= rows and rows_out == (rows - moving if rows - moving >= 8 else rows), k
        assert np.isfinite(np.array(refined[k]["H"])).all(), k
    assert sum(s[1] for s in stats.values()) > 0
    again, again_stats = refine(threshold=16, ingest="yuv420", min_keep=8)
    assert again == refined and again_stats == stats


def test_refine_translate_placement(passes):
    from evenvizion_amd import capture
    from evenvizion_amd import stabilization as S
    from evenvizion_amd.processing.utils import superposition_dict
    first, _, refine = passes
    sup = superposition_dict({k: v for k, v in first.items() if k != "resize_info"})
    plate = S.background_plate(capture.VideoCapture(MP4), sup, first["resize_info"], placement="translate", max_frames=16, ingest="bgr")
    from evenvizion_amd import moving
    refined, stats = moving.refine_homography_dict(capture.VideoCapture(MP4), first, plate, placement="translate", threshold=16,
                                                   chunk_frames=16, ingest="bgr")
    assert len(refined) == 121 and all(b in (a - m, a) for a, m, b in stats.values())
    with pytest.raises(ValueError, match="placement or scale"):
        moving.refine_homography_dict(capture.VideoCapture(MP4), first, plate, placement="warp", chunk_frames=16, ingest="bgr")


class FirstFrames:
    """The first n frames of the reference's video, as BGR frames or as planes."""

    def __init__(self, n):
        from evenvizion_amd import capture
        self.cap, self.left = capture.VideoCapture(MP4), n
        self.width, self.height, self.bgr_mode = self.cap.width, self.cap.height, self.cap.bgr_mode

    def read(self):
        self.left -= 1
        return self.cap.read() if self.left >= 0 else (False, None)

    def read_yuv420_into(self, y, cb, cr):
        self.left -= 1
        return self.left >= 0 and self.cap.read_yuv420_into(y, cb, cr)


def test_refine_does_not_depend_on_the_chunks():
    """12 frames in chunks of 2 (eleven chunks of one pair, every {H_sup, H_prev} carried) and in one chunk, from BGR frames and
    from planes: the same dictionary and the same counts."""
    from evenvizion_amd import moving
    from evenvizion_amd import stabilization as S
    from evenvizion_amd.processing.utils import superposition_dict
    from evenvizion_amd.processing.video_processing import get_homography_dict
    first = get_homography_dict(FirstFrames(12), resize_width=400, ingest="bgr", chunk_frames=16, features_type_list=["ORB"])
    sup = superposition_dict({k: v for k, v in first.items() if k != "resize_info"})
    plate = S.background_plate(FirstFrames(12), sup, first["resize_info"], placement="warp", max_frames=12, ingest="bgr")
    assert plate.frame_nos == list(range(1, 13))
    got = {(chunk, ingest): moving.refine_homography_dict(FirstFrames(12), first, plate, threshold=16, chunk_frames=chunk, ingest=ingest)
           for chunk in (2, 16) for ingest in ("bgr", "auto")}
    refined, stats = got[(16, "bgr")]
    assert list(refined) == list(range(2, 13)) + ["resize_info"] and sorted(stats) == list(range(2, 13))
    assert sum(s[0] for s in stats.values()) > 0
    for key, (again, again_stats) in got.items():
        assert again == refined and again_stats == stats, key


def test_component_reject_moving_writes_its_files(tmp_path, monkeypatch):
    from evenvizion_amd import component
    monkeypatch.chdir(tmp_path)
    common = ["--path_to_video", MP4, "--features", "ORB"]
    plain = component.main(common + ["--experiment_name", "plain"])
    folder = component.main(common + ["--experiment_name", "second", "--reject_moving", "1", "--plate_frames", "16",
                                      "--registration_report", "1"])
    before = sorted(os.listdir(plain))
    assert sorted(os.listdir(folder)) == sorted(before + ["dict_with_homography_matrix_refined.json", "moving_rows.json",
                                                          "registration_report.json", "registration_report_refined.json"])
    for name in before:                                                   # the existing outputs are what they are without the flag
        assert open(os.path.join(folder, name), "rb").read() == open(os.path.join(plain, name), "rb").read(), name
    refined = json.load(open(os.path.join(folder, "dict_with_homography_matrix_refined.json")))
    first = json.load(open(os.path.join(folder, "dict_with_homography_matrix.json")))
    stats = json.load(open(os.path.join(folder, "moving_rows.json")))
    assert list(refined) == list(first) and sorted(stats, key=int) == [k for k in first if k != "resize_info"]
    assert all(set(v) == {"rows", "moving", "rows_out"} for v in stats.values())
    reports = [json.load(open(os.path.join(folder, name))) for name in ("registration_report.json", "registration_report_refined.json")]
    print("ITF first pass %.4f, refined %.4f" % (reports[0]["itf"], reports[1]["itf"]))
    assert all(np.isfinite(r["itf"]) for r in reports)
