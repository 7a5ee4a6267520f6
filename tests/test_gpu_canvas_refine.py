"""evh_canvas_refine / evh_canvas_refine_yuv420 and the drivers of evenvizion_amd.registration built on them, on the device.  With
the canvas = the previous frame the entry is held to evh_pair_refine byte for byte; on a real canvas with holes the cost is held to
the exact integers and the normal sums to the exact integer sums of the numpy restatement (tests/canvas_checks.py, itself checked in
test_canvas_refine_host.py) within the rounding any order of summation may leave; the loop to its results on crafted canvases with a
known true map; the driver to the restatement's loop on a pan that comes back over its own ground."""
import ctypes
import json
import os

import numpy as np
import pytest

import canvas_checks as CC
import refine_checks as RC
import refine_families as F
import residual_checks as R
import warp_checks as W
from refusal_arena import Arena
from test_gpu_residual import dev, frames_of, strided

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MP4 = os.path.join(ROOT, "tests", "golden", "ref_test_video.mp4")
GOLD = os.path.join(ROOT, "tests", "golden", "ref_dict_with_homography_matrix.json")
U = 2.0 ** -53
STATUS, EVALS, ACCEPTED, COV_IN, SSD_IN, COV_OUT, SSD_OUT, N_IN = range(8)
NAN = np.full((3, 3), np.nan)
# the cases of refine_families at which canvas_checks.refine, on CC.canvas_pair's canvas, ends within 0.25 px (measured 0.037 .. 0.148 px;
# the one left out, seed 122 at 37 x 29, ends at 0.260 px on the host: the minimiser of its noisy residual is that far off)
CONVERGING = [c for c in F.CASES if c[0] != 122]


@pytest.fixture(scope="module")
def ctx():
    from evenvizion_amd._lib import Context
    c = Context(device=0, max_w=64, max_h=64, max_features=500, max_frames=2)     # the entry does not depend on these sizes
    yield c
    c.close()


@pytest.fixture(scope="module")
def family():
    return {case: F.pair(*case) for case in F.CASES}


def image(a, layout=None):
    """One picture u8[h,w(,c)] on the device, tight or at layout = (row stride, -, offset) -> the view"""
    a = np.asarray(a)
    return strided((1,) + a.shape, layout, a[None])[1][0]


def crefine(ctx, frames, canvas, mats, count=None, min_cover=1, iters=8, clip=255, layouts=(None, None, None), in_place=False,
            planes=None, size=None):
    """Context.canvas_refine -> (M_out f64[n,3,3], info int64[n,8], normal f64[n,45]); the outputs go in filled.  layouts: of the
    frames, the canvas and the count.  planes: the source handed to canvas_refine_yuv420 in place of `frames`."""
    import torch
    frames, mats = np.asarray(frames), np.asarray(mats, np.float64).reshape(-1, 9)
    n = len(mats)
    src = strided(frames.shape, layouts[0], frames)[1]
    d_canvas = image(canvas, layouts[1])
    d_count = None if count is None else image(count, layouts[2])
    d_in = dev(mats)
    out = d_in if in_place else torch.full((n, 9), float("nan"), dtype=torch.float64, device="cuda")
    info = torch.full((n, 8), -1, dtype=torch.int64, device="cuda")
    normal = torch.full((n, 45), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    kw = dict(count=d_count, min_cover=min_cover, iters=iters, clip=clip, out=out, info=info, normal=normal)
    got = ctx.canvas_refine(src, d_canvas, d_in, **kw) if planes is None else ctx.canvas_refine_yuv420(planes, d_canvas, d_in, size=size, **kw)
    assert got[0] is out and got[1] is info
    ctx.synchronize()
    M, I, N = out.cpu().numpy().reshape(-1, 3, 3), info.cpu().numpy(), normal.cpu().numpy()
    for p in range(n):                                         # what holds for every frame of every call
        assert int(I[p, SSD_OUT]) * int(I[p, COV_IN]) <= int(I[p, SSD_IN]) * int(I[p, COV_OUT]), "frame %d got worse" % p
        assert 1 <= I[p, EVALS] <= iters + 1 and 0 <= I[p, ACCEPTED] < I[p, EVALS] and I[p, N_IN] == N[p, 44]
        if I[p, ACCEPTED] == 0:
            assert M[p].tobytes() == mats[p].tobytes() and I[p, STATUS] != RC.REFINED, p
        else:
            assert I[p, STATUS] == RC.REFINED and I[p, COV_OUT] > 0 and 10 * I[p, COV_OUT] >= 9 * I[p, COV_IN] and M[p, 2, 2] == 1.0
    return M, I, N


def as_channels(img, gray):
    img = np.asarray(img)
    if gray:
        return R.gray_of(img)
    return img if img.ndim == 3 else np.repeat(img[..., None], 3, 2)


# ---- identity with evh_pair_refine ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [255, 16])
@pytest.mark.parametrize("iters", [0, 8])
@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("size", F.SIZES)
def test_canvas_equal_to_the_previous_frame_is_pair_refine(ctx, family, size, gray, iters, clip):
    """canvas = the previous frame, dw = w, dh = h: d_M_out, d_info and d_normal are evh_pair_refine's for the pair, byte for byte --
    good, NaN and non-covering matrices in one call; without a count, and with a count of 255s at min_cover 255."""
    import torch
    w, h = size
    cases = [c for c in F.CASES if c[1:3] == size]
    prev, cur, _, M_start = family[cases[0]]
    other = family[cases[1]][1]                               # another scene against the same canvas: a poor fit, refined all the same
    prev, cur, other = (as_channels(a, gray) for a in (prev, cur, other))
    curs = np.stack([cur, cur, other, cur, cur])
    mats = np.stack([M_start, NAN, np.dot(M_start, W.translation(0.4, -0.3)), W.translation(5 * w, 0), W.translation(0.75, -0.5)])
    pairs = np.stack([a for c in curs for a in (prev, c)])     # (prev, cur) per pair: frame_step 2
    out, info = ctx.pair_refine(dev(pairs), dev(mats.reshape(-1, 9)), iters=iters, clip=clip, frame_step=2,
                                normal=(normal := torch.full((5, 45), float("nan"), dtype=torch.float64, device="cuda")))
    ctx.synchronize()
    want = (out.cpu().numpy().reshape(-1, 3, 3), info.cpu().numpy(), normal.cpu().numpy())
    assert want[1][:, STATUS].tolist()[1::2] == [RC.NOTHING_COVERED] * 2 and (iters == 0 or clip != 255 or want[1][0, STATUS] == RC.REFINED)
    for count, mc in ((None, 1), (np.full((h, w), 255, np.uint8), 255)):
        got = crefine(ctx, curs, prev, mats, count, mc, iters, clip)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), (count is None)


# ---- sums and cost on a real canvas ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("seed,w,h,dw,dh", [(126, 37, 29, 80, 57), (142, 64, 48, 131, 97)])
def test_sums_and_cost_on_a_canvas_with_holes(ctx, seed, w, h, dw, dh, gray):
    """covered, ssd and n are the restatement's integers; each of the 44 sums is within 2 n 2^-53 sum|t| of the exact sum (the bar of
    test_gpu_refine.test_normal_sums_and_cost), with a count random in 0..3 at min_cover 2 and clip 255, 16 and 0."""
    rng = np.random.default_rng(seed)
    cn = 1 if gray else 3
    f = F.scene(rng, cn)
    canvas = F.render(f, rng, np.eye(3), dw, dh, cn)
    c = F.corners(w, h)
    mats, frames = [], []
    for k in range(3):
        M = F.homography_from_points(c, c + rng.uniform(0, [dw - w, dh - h]) + rng.uniform(-3, 3, (4, 2)))
        frames.append(F.render(f, rng, M, w, h, cn))
        mats.append(np.dot(M, W.translation(0.4 * k, -0.3)))
    frames, mats = np.stack(frames), np.stack(mats)
    count = rng.integers(0, 4, (dh, dw), dtype=np.uint8)
    worst = 0.0
    for clip in (255, 16, 0):
        M, I, N = crefine(ctx, frames, canvas, mats, count, 2, 0, clip)
        for p in range(3):
            J, r = CC.jacobian(canvas, frames[p], mats[p], clip, count, 2)
            exact, mags = RC.normal_exact(J, r)
            n = len(r)
            cost = CC.cost(canvas, frames[p], mats[p], count, 2)
            assert 0 < cost[0] < w * h and (int(I[p, COV_IN]), int(I[p, SSD_IN])) == cost == (int(I[p, COV_OUT]), int(I[p, SSD_OUT]))
            assert I[p, N_IN] == n == exact[44] and N[p, 44] == float(n) and (clip == 0 or n > 0), (clip, p)
            assert I[p, STATUS] == RC.UNCHANGED and I[p, EVALS] == 1
            for k in range(44):
                err = abs(int(N[p, k]) - exact[k] + (N[p, k] - int(N[p, k])))
                assert err <= 2 * n * U * mags[k], (clip, p, k, N[p, k], exact[k])
                if mags[k]:
                    worst = max(worst, err / (n * U * mags[k]))
    print("%dx%d on %dx%d gray %s: worst error %.3g of n u sum|t|" % (w, h, dw, dh, gray, worst))


# ---- the validity rule at its edges --------------------------------------------------------------------------------------------------------
def test_validity_edges(ctx):
    w, h, dw, dh = 24, 18, 40, 30
    canvas, cur = frames_of(9, 1, dw, dh, True)[0], frames_of(10, 1, w, h, True)[0]
    whole, half = W.translation(5, 4), W.translation(5.5, 4)
    count = np.ones((dh, dw), np.uint8)
    count[7, 29] = 0                                           # beside the last column's tap: weight 0, neither read nor asked
    M, I, N = crefine(ctx, cur[None], canvas, whole[None], count, 1, 0)
    assert I[0, COV_IN] == w * h and (int(I[0, COV_IN]), int(I[0, SSD_IN])) == CC.cost(canvas, cur, whole, count, 1) == RC.cost(
        np.ascontiguousarray(canvas[4:4 + h, 5:5 + w]), cur, np.eye(3))
    count[9, 10] = 0                                           # under the one tap of frame pixel (5, 5)
    M, I, N = crefine(ctx, cur[None], canvas, whole[None], count, 1, 0)
    assert I[0, COV_IN] == w * h - 1 and (int(I[0, COV_IN]), int(I[0, SSD_IN])) == CC.cost(canvas, cur, whole, count, 1)
    assert N[0, 44] == len(CC.jacobian(canvas, cur, whole, 255, count, 1)[1]) == (w - 2) * (h - 2) - 1
    # half a pixel to the right: two taps per sample; (4, 5) and (5, 5) meet the hole, and the last column of row 3 now reads (29, 7)
    M, I, N = crefine(ctx, cur[None], canvas, half[None], count, 1, 0)
    assert np.argwhere(~CC.sample(canvas, half, w, h, count, 1)[1]).tolist() == [[3, 23], [5, 4], [5, 5]]
    assert I[0, COV_IN] == w * h - 3 and (int(I[0, COV_IN]), int(I[0, SSD_IN])) == CC.cost(canvas, cur, half, count, 1)
    assert N[0, 44] == len(CC.jacobian(canvas, cur, half, 255, count, 1)[1]) == (w - 2) * (h - 2) - 2
    # a count below min_cover everywhere: nothing is covered, and the input comes back byte for byte, NaN payloads included
    payload = np.frombuffer(np.array([0x7FF8000000001234, 0xFFF0000000000001] + [0x7FF8000000000000 + k for k in range(7)], np.uint64).tobytes(),
                            np.float64).reshape(3, 3)
    count[...] = 1
    mats = np.stack([whole, payload, half])
    M, I, N = crefine(ctx, np.stack([cur] * 3), canvas, mats, count, 2, 4)
    assert M.tobytes() == mats.tobytes() and not N.any()
    for p in range(3):
        assert I[p].tolist() == [RC.NOTHING_COVERED, 1, 0, 0, 0, 0, 0, 0], p
    M, I, N = crefine(ctx, np.stack([cur] * 3), canvas, mats, count, 2, 4, in_place=True)
    assert M.tobytes() == mats.tobytes()
    # 49 valid canvas pixels under interior pixels of the frame: fewer than 64
    count[...] = 0
    count[6:13, 7:14] = 3
    M, I, N = crefine(ctx, cur[None], canvas, whole[None], count, 3, 4)
    assert I[0].tolist()[:4] == [RC.TOO_FEW, 1, 0, 49] and I[0, N_IN] == 49 and M[0].tobytes() == whole.tobytes()
    M, I, N = crefine(ctx, cur[None], canvas, whole[None], count, 4, 4)
    assert I[0, STATUS] == RC.NOTHING_COVERED


# ---- where the canvas ends ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gray", [False, True])
def test_canvas_geometry(ctx, gray):
    w, h = 37, 29
    cur = frames_of(21, 1, w, h, gray)[0]
    big = frames_of(22, 1, 50, 41, gray)[0]
    count = np.random.default_rng(23).integers(0, 2, (41, 50), dtype=np.uint8)
    horizon = np.array([[1, 0, 3], [0, 1, 2], [0.25, 0, -1]], np.float64)          # tw = 0.25 x - 1: negative, zero at x = 4, then positive
    cases = [("partly off", big, count, W.translation(-10.25, -7.5)), ("partly off, far corner", big, count, W.translation(30, 25.5)),
             ("wholly off", big, count, W.translation(500, 0)), ("horizon", big, None, horizon), ("horizon, count", big, count, horizon),
             ("one column", big[:, :1], None, np.array([[0, 0, 0], [0, 1, 2.5], [0, 0, 1.]])),
             ("one column, count", big[:, 7:8], count[:, 7:8], np.array([[0, 0, 0], [0, 1, 2.5], [0, 0, 1.]])),
             ("one row", big[:1], None, np.array([[1, 0, 1.25], [0, 0, 0], [0, 0, 1.]])),
             ("one row, count", big[3:4], count[3:4], np.array([[1, 0, 1.25], [0, 0, 0], [0, 0, 1.]])),
             ("one pixel", big[:1, :1], None, np.array([[0, 0, 0], [0, 0, 0], [0, 0, 1.]]))]
    for name, canvas, cnt, M0 in cases:
        canvas = np.ascontiguousarray(canvas)
        cnt = None if cnt is None else np.ascontiguousarray(cnt)
        M, I, N = crefine(ctx, cur[None], canvas, M0[None], cnt, 1, 0)
        cost = CC.cost(canvas, cur, M0, cnt, 1)
        n = len(CC.jacobian(canvas, cur, M0, 255, cnt, 1)[1])
        print("%s: covered %d of %d, n %d" % (name, cost[0], w * h, n))
        assert (int(I[0, COV_IN]), int(I[0, SSD_IN])) == cost and I[0, N_IN] == n == N[0, 44], name
        assert (cost[0] == 0) == (name == "wholly off") and I[0, STATUS] == (RC.NOTHING_COVERED if cost[0] == 0 else RC.UNCHANGED), name


# ---- convergence ------------------------------------------------------------------------------------------------------------------------
def test_family_converges_on_a_canvas_with_holes(ctx):
    """CC.canvas_pair for the twelve cases of refine_families: a canvas 1.5 times the frame, a count with holes, 8 iterations from a
    start 1.0 .. 1.5 px off.  The bar, test_gpu_refine.test_family_converges' 0.25 px and REFINED, is applied where the restatement,
    run here, meets it: the cases of CONVERGING, which must all do so."""
    held = 0
    for case in F.CASES:
        seed, w, h, cn = case
        canvas, frame, count, M_true, M_start = CC.canvas_pair(*case)
        M, I, _ = crefine(ctx, frame[None], canvas, M_start[None], count, 1, 8)
        host, hinfo = CC.refine(canvas, frame, M_start, 8, 255, count, 1)
        e, eh = RC.corner_error(M[0], M_true, w, h), RC.corner_error(host, M_true, w, h)
        print("seed %d %dx%d cn %d: device %.3f px after %d accepted steps, restatement %.3f px after %d"
              % (seed, w, h, cn, e, I[0, ACCEPTED], eh, hinfo["accepted"]))
        assert (eh <= 0.25 and hinfo["status"] == RC.REFINED) == (case in CONVERGING), case
        assert (int(I[0, COV_IN]), int(I[0, SSD_IN])) == (hinfo["covered_in"], hinfo["ssd_in"])
        if case in CONVERGING:
            assert e <= 0.25 and I[0, STATUS] == RC.REFINED, case
            held += 1
    assert held >= 9


# ---- layouts ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gray", [False, True])
def test_odd_pointers_and_strides(ctx, gray):
    cn = 1 if gray else 3
    w, h = 37, 29
    canvas, frame, count, _, M_start = CC.canvas_pair(137, w, h, cn)
    dh, dw = count.shape
    frames = np.stack([frame, frame[::-1].copy(), frame])
    mats = np.stack([M_start, M_start, NAN])
    want = crefine(ctx, frames, canvas, mats, count, 1, 4)
    assert want[1][0, STATUS] == RC.REFINED
    for fl, cl, kl in (((w * cn + 1, (w * cn + 1) * h + 3, 1), (dw * cn + 3, 0, 5), (dw + 1, 0, 3)),
                       ((w * cn + 5, (w * cn + 5) * (h + 2), 7), (dw * cn + 1, 0, 1), (dw + 7, 0, 1)),
                       (None, (dw * cn + 2, 0, 2), None), ((w * cn + 3, (w * cn + 3) * h, 4), None, (dw + 2, 0, 6))):
        got = crefine(ctx, frames, canvas, mats, count, 1, 4, layouts=(fl, cl, kl))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), (fl, cl, kl)
    got = crefine(ctx, frames, canvas, mats, count, 1, 4, in_place=True)              # d_M_out == d_M_in
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
    again = crefine(ctx, frames, canvas, mats, count, 1, 4)                           # the same call twice: the same bytes
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, want))
    for p in range(3):                                                               # a frame alone: the same bytes as in company
        one = crefine(ctx, frames[p:p + 1], canvas, mats[p:p + 1], count, 1, 4)
        assert all(a.tobytes() == b[p].tobytes() for a, b in zip(one, want)), p


@pytest.mark.parametrize("size", [(37, 29), (24, 18)])
def test_planes_equal_the_bgr_entry_on_the_converted_frames(ctx, size):
    import torch
    rng = np.random.default_rng(31)
    w, h = size
    cw, ch = (w + 1) // 2, (h + 1) // 2
    canvas, frame, count, _, M_start = CC.canvas_pair(141, w, h, 1)
    dh, dw = canvas.shape
    grey = np.full(((dh + 1) // 2, (dw + 1) // 2), 128, np.uint8)
    canvas = W.planes_to_bgr([(canvas, grey, grey)])[0]       # the canvas through the same conversion as the frames
    planes = [(g, rng.integers(96, 160, (ch, cw), dtype=np.uint8), rng.integers(96, 160, (ch, cw), dtype=np.uint8))
              for g in (frame, frame[:, ::-1].copy(), frame)]
    bgr = W.planes_to_bgr(planes)
    mats = np.stack([M_start, NAN, np.dot(M_start, W.translation(0.5, 0.25))])
    want = crefine(ctx, bgr, canvas, mats, count, 1, 4)
    assert want[1][0, STATUS] == RC.REFINED
    y, cb, cr = (dev(np.stack([p[i] for p in planes])) for i in range(3))
    uv = torch.stack([cb, cr], dim=-1).contiguous()
    packed = dev(np.stack([np.concatenate([a.reshape(-1) for a in p]) for p in planes]))
    conv = torch.zeros((3, h, w, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.yuv420_to_bgr((y, cb, cr), conv)
    ctx.synchronize()
    assert np.array_equal(conv.cpu().numpy(), bgr)
    for name, src, sz in (("i420", (y, cb, cr), None), ("nv12", (y, uv[..., 0], uv[..., 1]), None), ("packed", packed, (w, h))):
        got = crefine(ctx, bgr, canvas, mats, count, 1, 4, planes=src, size=sz)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), name


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(ctx):
    import torch
    from evenvizion_amd._lib import Yuv420
    INVALID, CAPACITY = -1, -3
    n, w, h, dw, dh = 3, 23, 17, 31, 25
    A = Arena(10)
    src = A.put(frames_of(80, n, w, h))
    canvas = A.put(frames_of(81, 1, dw, dh)[0])
    count = A.put(np.ones((dh, dw), np.uint8))
    mats = A.put(np.tile(W.translation(3, 4).reshape(1, 9), (n + 1, 1)))
    out = A.take((n + 1, 9), torch.float64, 7.0)
    info = A.take((n + 1, 8), torch.int64, -1)
    normal = A.take((n + 1, 45), torch.float64, 7.0)
    f, cv, k, m, o, i, q = (t.data_ptr() for t in (src, canvas, count, mats, out, info, normal))
    rs, fs, crs = w * 3, w * h * 3, dw * 3
    good = dict(ctx=ctx.h, frames=f, n=n, w=w, h=h, cn=3, rs=rs, fs=fs, canvas=cv, dw=dw, dh=dh, crs=crs, count=k, krs=dw, mc=1, M=m,
                iters=2, clip=255, out=o, info=i, normal=q)

    def call(**kw):
        a = dict(good, **kw)
        return ctx.lib.evh_canvas_refine(a["ctx"], a["frames"], a["n"], a["w"], a["h"], a["cn"], a["rs"], a["fs"], a["canvas"], a["dw"],
                                         a["dh"], a["crs"], a["count"], a["krs"], a["mc"], a["M"], a["iters"], a["clip"], a["out"],
                                         a["info"], a["normal"])

    who, who_yuv = "evh_canvas_refine: ", "evh_canvas_refine_yuv420: "
    NS, NA, CH, EM = "NULL source", "NULL argument", "channels must be 1 or 3", "empty frame or canvas"
    IT, CL, MC = "iters must lie in 0..64", "clip must lie in 0..255", "min_cover must lie in 1..255"
    BIG, B26, AREA = "w and h stay within 4096", "canvas sizes stay below 2^26 (positions are held in 1/32 pixels)", "dw * dh above INT_MAX"
    NF, SS, CS, KS = ("at most 65535 frames per call", "source stride smaller than a row / frame", "canvas stride smaller than a row",
                      "count stride smaller than a row")
    OFR, OC, OK_, OI, ON, IN_, OM, IM, NM = ("d_M_out overlaps the frames", "d_M_out overlaps the canvas", "d_M_out overlaps d_count",
                                             "d_M_out overlaps d_info", "d_M_out overlaps d_normal", "d_info overlaps d_normal",
                                             "d_M_out overlaps d_M_in", "d_info overlaps d_M_in", "d_normal overlaps d_M_in")

    def refused(rc, code, text, what):
        assert rc == code, what
        assert ctx.lib.evh_last_error_string(ctx.h).decode() == text, what

    assert call(ctx=None) == INVALID
    invalid = [(dict(frames=None), NS), (dict(canvas=None), NA), (dict(M=None), NA), (dict(out=None), NA), (dict(info=None), NA),
               (dict(cn=2), CH), (dict(cn=0), CH), (dict(w=0), EM), (dict(h=-1), EM), (dict(dw=0), EM), (dict(dh=-3), EM), (dict(n=-1), EM),
               (dict(iters=-1), IT), (dict(iters=65), IT), (dict(clip=-1), CL), (dict(clip=256), CL), (dict(mc=0), MC), (dict(mc=256), MC),
               (dict(rs=rs - 1), SS), (dict(fs=fs - 1), SS), (dict(crs=crs - 1), CS), (dict(krs=dw - 1), KS),
               (dict(out=f), OFR), (dict(out=f + n * fs - 1), OFR), (dict(out=f - n * 72 + 1), OFR), (dict(info=f + 8), "d_info overlaps the frames"),
               (dict(normal=f + 16), "d_normal overlaps the frames"), (dict(out=cv), OC), (dict(out=cv + dh * crs - 1), OC),
               (dict(info=cv + 8), "d_info overlaps the canvas"), (dict(out=k), OK_), (dict(out=k + dh * dw - 1), OK_),
               (dict(normal=k + 8), "d_normal overlaps d_count"), (dict(out=i), OI), (dict(out=i + n * 64 - 8), OI),
               (dict(info=o + n * 72 - 8), OI), (dict(out=q), ON), (dict(normal=i + 8), IN_), (dict(out=m + 8), OM), (dict(out=m - 8), OM),
               (dict(M=o + 72), OM), (dict(info=m), IM), (dict(normal=m + n * 72 - 8), NM),
               # two faults: the earlier check of the entry names the refusal
               (dict(frames=None, out=None), NS), (dict(M=None, cn=2), NA), (dict(cn=2, n=-1), CH), (dict(dw=0, iters=65), EM),
               (dict(iters=65, clip=256), IT), (dict(clip=256, mc=0), CL), (dict(mc=0, rs=rs - 1), MC), (dict(rs=rs - 1, crs=crs - 1), SS),
               (dict(crs=crs - 1, krs=dw - 1), CS), (dict(krs=dw - 1, out=f), KS), (dict(out=f, info=m), OFR), (dict(out=i, normal=m), OI)]
    for kw, text in invalid:
        refused(call(**kw), INVALID, who + text, kw)
    capacity = [(dict(w=4097, rs=4097 * 3, fs=4097 * 3 * h), BIG), (dict(h=4097, fs=rs * 4097), BIG), (dict(w=4097), BIG),
                (dict(dw=1 << 26, crs=3 << 26), B26), (dict(dh=1 << 26), B26), (dict(dw=1 << 16, dh=1 << 15, crs=3 << 16, krs=1 << 16), AREA),
                (dict(n=65536), NF), (dict(n=65536, fs=fs - 1), NF), (dict(w=4097, dw=1 << 26), BIG), (dict(dw=1 << 26, n=65536), B26)]
    for kw, text in capacity:
        refused(call(**kw), CAPACITY, who + text, kw)
    # what is not looked at: min_cover without a count, the frame stride of a single frame
    assert call(count=None, mc=0, krs=0) == 0 and call(n=1, fs=0) == 0
    ctx.synchronize()
    out.fill_(7.0), info.fill_(-1), normal.fill_(7.0)
    torch.cuda.synchronize()
    cw, ch = 12, 9
    y = A.take((n, h, w))
    c = A.take((2, n, ch, cw))
    torch.cuda.synchronize()
    yuv = dict(d_y=y.data_ptr(), d_cb=c[0].data_ptr(), d_cr=c[1].data_ptr(), y_stride=w, c_stride=cw, y_frame_stride=w * h,
               c_frame_stride=cw * ch, c_pixel_stride=1)

    def call_yuv(desc, **kw):
        a = dict(good, **kw)
        d = None if desc is None else ctypes.byref(Yuv420(**desc))
        return ctx.lib.evh_canvas_refine_yuv420(a["ctx"], d, a["n"], a["w"], a["h"], a["canvas"], a["dw"], a["dh"], a["crs"], a["count"],
                                                a["krs"], a["mc"], a["M"], a["iters"], a["clip"], a["out"], a["info"], a["normal"])

    refused(call_yuv(None), INVALID, who_yuv + NS, "no description")
    for bad, text in ((dict(d_y=None), NS), (dict(d_cr=None), NS), (dict(c_pixel_stride=3), "chroma pixel stride must be 1 or 2"),
                      (dict(y_stride=w - 1), "luma row stride smaller than the width"),
                      (dict(c_frame_stride=cw * ch - 1), "frame stride smaller than a plane")):
        refused(call_yuv(dict(yuv, **bad)), INVALID, who_yuv + text, bad)
    for kw, text in ((dict(M=None), NA), (dict(canvas=None), NA), (dict(w=0), EM), (dict(iters=65), IT), (dict(clip=256), CL), (dict(mc=0), MC),
                     (dict(crs=crs - 1), CS), (dict(out=y.data_ptr() + 7), OFR), (dict(out=c[1].data_ptr()), OFR), (dict(out=cv), OC),
                     (dict(out=i), OI), (dict(info=m), IM)):
        refused(call_yuv(yuv, **kw), INVALID, who_yuv + text, kw)
    for kw, text in ((dict(w=4097), BIG), (dict(dh=1 << 26), B26), (dict(n=65536), NF)):
        refused(call_yuv(yuv, **kw), CAPACITY, who_yuv + text, kw)
    # no frames: success, and nothing is done
    assert call(n=0) == 0 and call_yuv(yuv, n=0) == 0
    ctx.synchronize()
    assert (out == 7.0).all() and (info == -1).all() and (normal == 7.0).all()
    # the same arguments unrefused do write; d_normal may be NULL, d_M_out may be d_M_in
    assert call() == 0 and call(normal=None, out=m + 72 * n, M=m + 72 * n, info=i + 64 * n, n=1) == 0
    ctx.synchronize()
    got = info.cpu().numpy()
    frames_h, canvas_h = src.cpu().numpy(), canvas.cpu().numpy()
    for p in range(n):
        assert (int(got[p, COV_IN]), int(got[p, SSD_IN])) == CC.cost(canvas_h, frames_h[p], W.translation(3, 4))
    assert got[n, COV_IN] == got[0, COV_IN] and got[n, SSD_IN] == got[0, SSD_IN] and (out[n] == 7.0).all() and (normal[n] == 7.0).all()


def test_python_layer_refuses_what_does_not_fit(ctx):
    import torch
    frames = dev(frames_of(81, 3, 16, 12))
    canvas = dev(frames_of(82, 1, 20, 15)[0])
    mats = dev(np.tile(np.eye(3).reshape(1, 9), (3, 1)))
    zeros = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    for bad in (dict(mats=mats.float()), dict(mats=mats[:2]), dict(canvas=canvas[..., 0]), dict(canvas=canvas.cpu()),
                dict(count=zeros((15, 21), torch.uint8)), dict(count=zeros((15, 20), torch.int32)), dict(info=zeros((3, 7), torch.int64)),
                dict(normal=zeros((3, 44), torch.float64)), dict(out=zeros((2, 9), torch.float64))):
        kw = dict(frames=frames, canvas=canvas, mats=mats)
        kw.update(bad)
        with pytest.raises(ValueError):
            ctx.canvas_refine(**kw)
    with pytest.raises(ValueError):
        ctx.canvas_refine(frames[..., 0].contiguous(), canvas, mats)          # gray frames take a gray canvas
    out, info = ctx.canvas_refine(frames[:0], canvas, mats[:0])
    assert out.shape == (0, 9) and info.shape == (0, 8)
    out, info = ctx.canvas_refine(frames, canvas, mats, count=zeros((15, 20), torch.uint8) + 1, iters=0)
    ctx.synchronize()
    assert info.cpu().numpy()[:, COV_IN].tolist() == [16 * 12] * 3


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------
def loop_scene(seed=145, n=16, w=64, h=48, step=6.0, err=0.25):
    """n gray frames of one scene on a pan of `step` pixels per frame, n/2 frames out and n/2 back over the same ground; the
    dictionary's matrices carry `err` pixels more per pair in x -> (frames, truth, given)"""
    rng = np.random.default_rng(seed)
    f = F.scene(rng, 1)
    off = [step * k if k < n // 2 else step * (n - 1 - k) for k in range(n)]
    truth = [W.translation(o, 0.0) for o in off]
    frames = np.stack([F.render(f, rng, S, w, h, 1) for S in truth])
    return frames, truth, [W.translation(o + err * k, 0.0) for k, o in enumerate(off)]


@pytest.fixture(scope="module")
def loop():
    return loop_scene()


@pytest.mark.parametrize("group", [1, 4])
def test_the_seed_of_a_loop(loop, group):
    """16 frames, 8 out and 8 back at 6 px per frame, the dictionary 0.25 px per pair off: S_15 is 3.75 px off while frame 15 looks
    at frame 0's ground.  The mean and the last corner error of S' lie below the dictionary's and within 0.1 px of what the
    restatement's loop reaches (they differ by the rounding of the 44 sums).  Measured on the host: group 1 mean 0.197 px, last
    0.076 px; group 4 mean 0.754 px, last 0.530 px; the dictionary 1.875 px and 3.750 px."""
    from evenvizion_amd import registration
    from evenvizion_amd.stabilization import fixed_plane_bounds
    from evenvizion_amd.synthetic import SyntheticCapture
    frames, truth, given = loop
    w, h = 64, 48
    sup, ri = {k + 1: S for k, S in enumerate(given)}, {"w": w, "h": h}
    got, info = registration.anchor_superposition(SyntheticCapture([np.repeat(a[..., None], 3, 2) for a in frames]), sup, ri, iters=8,
                                                  group=group, margin=8)
    host, hinfo = CC.anchor(frames, given, fixed_plane_bounds(sup, ri), 8, 255, group, "feather", 1024, 0.25, 8)
    err = lambda mats: [RC.corner_error(a, b, w, h) for a, b in zip(mats, truth)]
    e0, e, eh = err(given), err([got[k + 1] for k in range(16)]), err(host)
    print("group %d: dictionary mean %.3f last %.3f px; device mean %.3f last %.3f px; restatement mean %.3f last %.3f px"
          % (group, np.mean(e0), e0[-1], np.mean(e), e[-1], np.mean(eh), eh[-1]))
    assert list(got) == list(sup) == list(info) and np.abs(got[1] - given[0]).max() <= 1e-12
    assert np.mean(e) < np.mean(e0) and e[-1] < e0[-1]
    assert abs(np.mean(e) - np.mean(eh)) <= 0.1 and abs(e[-1] - eh[-1]) <= 0.1
    assert [info[k + 1]["used"] for k in range(16)] == [i["used"] for i in hinfo]
    for k in range(16):                                        # the first evaluation is at the same matrix on the same canvas
        assert not info[k + 1]["used"] or k >= group
        if k < 2 * group:
            assert (info[k + 1]["covered_in"], info[k + 1]["ssd_in"]) == (hinfo[k]["covered_in"], hinfo[k]["ssd_in"]), k


def test_driver_identities(loop):
    from evenvizion_amd import registration
    from evenvizion_amd.synthetic import SyntheticCapture
    frames, truth, given = loop
    bgr = [np.repeat(a[..., None], 3, 2) for a in frames[:8]]
    sup, ri = {k + 1: S for k, S in enumerate(given[:8])}, {"w": 64, "h": 48}
    got, info = registration.anchor_superposition(SyntheticCapture(list(bgr)), sup, ri, iters=0, group=2, margin=4)
    for k in sup:                                              # nothing is stepped: S' is the input
        assert np.abs(got[k] - sup[k]).max() <= 1e-12 * np.abs(sup[k]).max() and not info[k]["used"]
        assert info[k]["status"] == RC.UNCHANGED and (k <= 2 or (info[k]["evals"] == 1 and info[k]["covered_in"] > 0))
    holed = dict(sup)
    holed[4] = None
    got, info = registration.anchor_superposition(SyntheticCapture(list(bgr)), holed, ri, iters=4, margin=4)
    assert np.array_equal(got[4], got[3]) and not info[4]["used"] and info[4]["status"] == RC.NOTHING_COVERED
    assert info[3]["used"] and info[5]["used"] and np.isfinite(got[8]).all()
    got, info = registration.anchor_superposition(SyntheticCapture(list(bgr)), sup, ri, iters=4, min_overlap=1.0, margin=4)
    assert not any(e["used"] for e in info.values()) and any(e["status"] == RC.REFINED for e in info.values())
    assert all(0 < info[k]["overlap"] < 1 for k in range(2, 9))
    for k in sup:
        assert np.abs(got[k] - sup[k]).max() <= 1e-12 * np.abs(sup[k]).max()
    got, info = registration.anchor_superposition(SyntheticCapture(list(bgr)), sup, ri, iters=4, blend="seam", feather_px=4, margin=4)
    assert sum(e["used"] for e in info.values()) >= 5


# ---- the reference's video -----------------------------------------------------------------------------------------------------------------
def test_first_frames_of_the_reference_video():
    """The first 24 frames at 400 x 224 with their recorded matrices: the acceptance rule lets no frame's score against the canvas
    rise, so the sum of ssd_out / covered_out cannot exceed that of ssd_in / covered_in; at least one frame is refined."""
    from evenvizion_amd import capture, registration
    from evenvizion_amd.processing.utils import read_homography_dict, superposition_dict
    hd, ri = read_homography_dict(GOLD)
    sup = superposition_dict(hd)
    first = {k: sup[k] for k in [k for k in sup if k != "resize_info"][:24]}
    got = registration.anchored_homography_dict(lambda: capture.VideoCapture(MP4), first, ri, iters=8)
    info = got["info"]
    assert list(info) == list(first) == list(got["superposition"]) and len(got["homography"]) == 23
    before = sum(e["ssd_in"] / e["covered_in"] for e in info.values() if e["covered_in"])
    after = sum(e["ssd_out"] / e["covered_out"] for e in info.values() if e["covered_out"])
    print("24 frames: canvas score %.2f -> %.2f, %d refined, %d used; ITF %.3f -> %.3f dB"
          % (before, after, sum(e["status"] == RC.REFINED for e in info.values()), sum(e["used"] for e in info.values()),
             got["report_before"]["itf"], got["report_after"]["itf"]))
    assert after <= before and (before, after) == (got["canvas_score_before"], got["canvas_score_after"])
    assert any(e["status"] == RC.REFINED for e in info.values())
    for e in info.values():
        assert e["ssd_out"] * e["covered_in"] <= e["ssd_in"] * e["covered_out"]


def test_component_writes_the_anchored_files_only_on_request(tmp_path, monkeypatch):
    from evenvizion_amd import component
    monkeypatch.chdir(tmp_path)
    base = ["--path_to_video", "synthetic:4:400x224:3", "--features", "ORB"]
    plain = component.main(base + ["--experiment_name", "plain"])
    folder = component.main(base + ["--experiment_name", "anchored", "--anchor_mosaic", "1", "--anchor_group", "2"])
    old = sorted(os.listdir(plain))
    assert sorted(os.listdir(folder)) == sorted(old + ["dict_with_homography_matrix_anchored.json", "anchor_report.json"])
    for name in old:
        with open(os.path.join(plain, name), "rb") as a, open(os.path.join(folder, name), "rb") as b:
            assert a.read() == b.read(), name
    with open(os.path.join(folder, "dict_with_homography_matrix_anchored.json")) as f:
        anchored = json.load(f)
    with open(os.path.join(folder, "anchor_report.json")) as f:
        report = json.load(f)
    assert list(anchored) == ["2", "3", "4", "resize_info"] and anchored["resize_info"] == {"h": 224, "w": 400}
    assert np.asarray(anchored["2"]["H"]).shape == (3, 3)
    assert list(report["info"]) == ["1", "2", "3", "4"] and report["canvas_score_after"] <= report["canvas_score_before"]
    assert set(report) == {"before", "after", "canvas_score_before", "canvas_score_after", "info"}
