"""evh_pair_refine / evh_pair_refine_yuv420 and the drivers of evenvizion_amd.registration built on them, on the device.  The cost
is held to evh_pair_residual's integers, the normal sums to the exact integer sums of the numpy restatement (tests/refine_checks.py,
itself checked in test_refine_host.py) within the rounding any order of summation may leave, one step to the restatement's solve
within the backward-stable bound of an 8x8 LDL', the loop to its results on crafted pairs with a known true map
(tests/refine_families.py).  Every call of the entry goes through refine() below, which also holds EVERY pair to: the costs in
d_info are evh_pair_residual's for d_M_in and d_M_out, and d_M_out is never worse than d_M_in."""
import ctypes
import json
import os

import numpy as np
import pytest

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


@pytest.fixture(scope="module")
def ctx():
    from evenvizion_amd._lib import Context
    c = Context(device=0, max_w=64, max_h=64, max_features=500, max_frames=2)     # the entry does not depend on these sizes
    yield c
    c.close()


@pytest.fixture(scope="module")
def family():
    return {case: F.pair(*case) for case in F.CASES}


def refine(ctx, frames, mats, iters=8, clip=255, frame_step=1, src_layout=None, in_place=False, planes=None, size=None):
    """Context.pair_refine -> (M_out f64[npairs,3,3], info int64[npairs,8], normal f64[npairs,45]).  The outputs go in filled with
    0xFF bytes.  planes: the source handed to pair_refine_yuv420 in place of `frames`, which then are the BGR frames they convert to."""
    import torch
    frames = np.asarray(frames)
    mats = np.asarray(mats, np.float64).reshape(-1, 9)
    npairs = len(mats)
    _, src, _ = strided(frames.shape, src_layout, frames)
    d_in = dev(mats)
    out = d_in if in_place else torch.full((npairs, 9), float("nan"), dtype=torch.float64, device="cuda")
    info = torch.full((npairs, 8), -1, dtype=torch.int64, device="cuda")
    normal = torch.full((npairs, 45), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()                                  # the fills ran on torch's stream, the entry runs on the context's
    if planes is None:
        got = ctx.pair_refine(src, d_in, iters=iters, clip=clip, out=out, info=info, normal=normal, frame_step=frame_step)
    else:
        got = ctx.pair_refine_yuv420(planes, d_in, iters=iters, clip=clip, out=out, info=info, normal=normal, frame_step=frame_step, size=size)
    assert got[0] is out and got[1] is info
    s_in = ctx.pair_residual(src, dev(mats), frame_step=frame_step)
    s_out = ctx.pair_residual(src, out, frame_step=frame_step)
    ctx.synchronize()
    M, I, N = out.cpu().numpy().reshape(-1, 3, 3), info.cpu().numpy(), normal.cpu().numpy()
    s_in, s_out = s_in.cpu().numpy(), s_out.cpu().numpy()
    for p in range(npairs):
        assert (int(I[p, COV_IN]), int(I[p, SSD_IN])) == (int(s_in[p, R.COVERED]), int(s_in[p, R.SSD])), p
        assert (int(I[p, COV_OUT]), int(I[p, SSD_OUT])) == (int(s_out[p, R.COVERED]), int(s_out[p, R.SSD])), p
        assert int(I[p, SSD_OUT]) * int(I[p, COV_IN]) <= int(I[p, SSD_IN]) * int(I[p, COV_OUT]), "pair %d got worse" % p
        assert 1 <= I[p, EVALS] <= iters + 1 and 0 <= I[p, ACCEPTED] < I[p, EVALS] and I[p, N_IN] == N[p, 44]
        if I[p, ACCEPTED] == 0:
            assert M[p].tobytes() == mats[p].tobytes() and I[p, STATUS] != RC.REFINED, p
            assert (I[p, COV_IN], I[p, SSD_IN]) == (I[p, COV_OUT], I[p, SSD_OUT])
        else:
            assert I[p, STATUS] == RC.REFINED and I[p, COV_OUT] > 0 and 10 * I[p, COV_OUT] >= 9 * I[p, COV_IN]
            assert int(I[p, SSD_OUT]) * int(I[p, COV_IN]) < int(I[p, SSD_IN]) * int(I[p, COV_OUT]) and M[p, 2, 2] == 1.0
    return M, I, N


def stack_of(family, size, gray, npairs):
    """Frames and start matrices of `npairs` crafted pairs of one size, laid out for frame_step 2: (prev, cur) per pair"""
    cases = [c for c in F.CASES if c[1:3] == size]
    frames, mats, truth = [], [], []
    for k in range(npairs):
        prev, cur, M_true, M_start = family[cases[k % len(cases)]]
        if gray:
            prev, cur = R.gray_of(prev), R.gray_of(cur)
        elif prev.ndim == 2:
            prev, cur = np.repeat(prev[..., None], 3, 2), np.repeat(cur[..., None], 3, 2)
        if k >= len(cases):                                    # a second use of a case: another start
            M_start = np.dot(M_start, W.translation(0.4, -0.3))
        frames += [prev, cur]
        mats.append(M_start)
        truth.append(M_true)
    return np.stack(frames), np.stack(mats), truth


# ---- the normal equations and the cost ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("size,npairs,frame_step", [((37, 29), 5, 1), ((37, 29), 2, 2), ((64, 48), 3, 2), ((64, 48), 1, 1),
                                                    ((96, 64), 4, 1), ((96, 64), 2, 2)])
def test_normal_sums_and_cost(ctx, family, size, npairs, frame_step, gray):
    """|device - exact| <= 2 n 2^-53 sum|t| for each of the 44 sums (any order of summation of n once-rounded products is within
    it), n itself exactly, at clip 255, 16 and 0; the cost is the restatement's."""
    w, h = size
    frames, mats, _ = stack_of(family, size, gray, (npairs + 1) // 2 + 1 if frame_step == 1 else npairs)
    if frame_step == 1:                                        # consecutive frames: true pairs alternate with in-between ones
        frames = frames[:npairs + 1]
        mats = np.stack([mats[p // 2] if p % 2 == 0 else W.translation(0.75, -0.5) for p in range(npairs)])
    worst = 0.0
    for clip in (255, 16, 0):
        M, I, N = refine(ctx, frames, mats, iters=0, clip=clip, frame_step=frame_step)
        for p in range(npairs):
            prev, cur = frames[p * frame_step], frames[p * frame_step + 1]
            J, r = RC.jacobian(prev, cur, mats[p], clip)
            exact, mags = RC.normal_exact(J, r)
            n = len(r)
            assert I[p, N_IN] == n == exact[44] and N[p, 44] == float(n), (clip, p)
            assert (int(I[p, COV_IN]), int(I[p, SSD_IN])) == RC.cost(prev, cur, mats[p])
            assert I[p, STATUS] == RC.UNCHANGED and I[p, EVALS] == 1
            for k in range(44):
                err = abs(int(N[p, k]) - exact[k] + (N[p, k] - int(N[p, k])))
                assert err <= 2 * n * U * mags[k], (clip, p, k, N[p, k], exact[k])
                if mags[k]:
                    worst = max(worst, err / (n * U * mags[k]))
    print("%s pairs %d step %d gray %s: worst error %.3g of n u sum|t|" % (size, npairs, frame_step, gray, worst))


def test_sums_beyond_2_53(ctx):
    """400 x 224 random bytes: the sums of J_6^2 leave 2^53, so the device's rounding shows and must stay within the same bar"""
    frames = frames_of(8, 2, 400, 224, True)
    M, I, N = refine(ctx, frames, W.translation(0.5, -0.25)[None], iters=0)
    J, r = RC.jacobian(frames[0], frames[1], W.translation(0.5, -0.25))
    exact, mags = RC.normal_exact(J, r)
    n = len(r)
    assert max(mags[:36]) > 2 ** 53 and I[0, N_IN] == n
    errs = [abs(int(N[0, k]) - exact[k] + (N[0, k] - int(N[0, k]))) / (2 * n * U * mags[k]) for k in range(44)]
    print("worst share of the bar: %.3g, sums not exact: %d" % (max(errs), sum(e > 0 for e in errs)))
    assert max(errs) <= 1.0


# ---- one step ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [F.CASES[1], F.CASES[4], F.CASES[9], F.CASES[10]])
def test_one_step_is_the_restatements_solve(ctx, family, case):
    """iters = 1: the device's own sums through the restatement's solve give the Delta the device's trial was made from, within
    64 cond_2(Ah) 2^-53 relative -- the backward-stable bound of an 8x8 LDL' on a damped SPD matrix."""
    seed, w, h, cn = case
    prev, cur, _, M_start = family[case]
    M, I, N = refine(ctx, np.stack([prev, cur]), M_start[None], iters=1)
    assert I[0, ACCEPTED] == 1 and I[0, EVALS] == 2               # the first step from 1.0 .. 1.5 px off is an improvement
    Ah, bh, d = RC.scaled_system(N[0], 1e-3)
    want = -4.0 * RC.ldl_solve(Ah, bh) / d
    got = RC.delta_of(M_start, M[0], w, h)
    rel, bar = np.linalg.norm(got - want) / np.linalg.norm(want), 64 * np.linalg.cond(Ah) * U
    by_numpy = -4.0 * np.linalg.solve(Ah, bh) / d
    print("seed %d: |delta_dev - delta_host| / |delta_host| = %.3g, bar %.3g (cond %.3g); numpy's solve differs by %.3g"
          % (seed, rel, bar, np.linalg.cond(Ah), np.linalg.norm(by_numpy - want) / np.linalg.norm(want)))
    assert rel <= bar
    T = RC.try_matrix(M_start, want, w, h)
    assert np.abs(T - M[0]).max() <= 1e-9


# ---- convergence ------------------------------------------------------------------------------------------------------------------------
def test_family_converges(ctx, family):
    worst = 0.0
    for (seed, w, h, cn), (prev, cur, M_true, M_start) in family.items():
        M, I, _ = refine(ctx, np.stack([prev, cur]), M_start[None], iters=8)
        e = RC.corner_error(M[0], M_true, w, h)
        host, hinfo = RC.refine(prev, cur, M_start, 8)
        print("seed %d %dx%d cn %d: %.3f px after %d accepted steps (restatement: %.3f px, %d)"
              % (seed, w, h, cn, e, I[0, ACCEPTED], RC.corner_error(host, M_true, w, h), hinfo["accepted"]))
        assert e <= 0.25 and I[0, ACCEPTED] >= 1 and I[0, STATUS] == RC.REFINED
        worst = max(worst, e)
    print("worst %.3f px" % worst)


def test_three_levels_from_the_identity_through_the_driver():
    from evenvizion_amd import registration
    from evenvizion_amd.synthetic import SyntheticCapture
    for seed, dx, dy in F.SHIFTS:
        prev, cur, M_true = F.shift_pair(seed, dx, dy)
        bgr = [np.repeat(a[..., None], 3, 2) for a in (prev, cur)]
        sup, ri = {1: np.eye(3), 2: np.eye(3)}, {"w": 96, "h": 64}
        err = {}
        for levels in (1, 3):
            maps, info = registration.refine_pair_maps(SyntheticCapture(list(bgr)), sup, ri, iters=8, levels=levels)
            assert list(maps) == [2] == list(info) and len(info[2]["accepted_by_level"]) == levels
            err[levels] = RC.corner_error(maps[2], M_true, 96, 64)
        print("shift (%g, %g): one level %.3f px, three levels %.3f px" % (dx, dy, err[1], err[3]))
        assert err[3] <= 0.25 < err[1]


def test_fill_missing_starts_a_pair_without_a_map_from_its_neighbour():
    from evenvizion_amd import registration
    from evenvizion_amd.synthetic import SyntheticCapture
    seed, dx, dy = F.SHIFTS[0]
    prev, cur, M_true = F.shift_pair(seed, dx, dy)
    bgr = [np.repeat(a[..., None], 3, 2) for a in (prev, cur, cur)]
    sup, ri = {1: np.eye(3), 2: None, 3: np.eye(3), "resize_info": None}, {"w": 96, "h": 64}
    maps, info = registration.refine_pair_maps(SyntheticCapture(list(bgr)), sup, ri, levels=3)
    assert list(maps) == [2, 3] and all(np.isnan(m).all() for m in maps.values())            # either side of the missing entry
    assert [info[k]["status"] for k in (2, 3)] == [RC.NOTHING_COVERED] * 2 and not info[2]["filled"]
    maps, info = registration.refine_pair_maps(SyntheticCapture(list(bgr)), sup, ri, levels=3, fill_missing=True)
    assert info[2]["filled"] and info[3]["filled"] and info[2]["accepted_by_level"][0] >= 1
    e = RC.corner_error(maps[2], M_true, 96, 64)
    print("the pair without a map, from the identity over three levels: %.3f px" % e)
    assert e <= 0.25                                                                       # the three-level case above, by another door
    # the next pair (the same frame twice) starts from that map, not from the identity, and is walked back to the identity
    assert sum(info[3]["accepted_by_level"]) >= 1 and RC.corner_error(maps[3], np.eye(3), 96, 64) <= 0.25


# ---- edges ---------------------------------------------------------------------------------------------------------------------------------
def test_maps_that_cover_nothing_and_frames_that_say_nothing(ctx, family):
    prev, cur, _, M_start = family[F.CASES[4]]
    pair = np.stack([prev, cur])
    h, w = cur.shape[:2]
    nan_one = np.eye(3)
    nan_one[0, 1] = np.nan
    nothing = [NAN, np.zeros((3, 3)), np.array([[1, 2, 3], [2, 4, 6], [0, 0, 0.]]), nan_one, np.full((3, 3), np.inf),
               W.translation(5 * w, 0), np.full((3, 3), -np.nan)]
    frames = np.concatenate([pair] * len(nothing))
    M, I, N = refine(ctx, frames, np.stack(nothing), iters=4, frame_step=2)
    for p in range(len(nothing)):
        assert I[p].tolist() == [RC.NOTHING_COVERED, 1, 0, 0, 0, 0, 0, 0] and not N[p].any(), p
    # the horizon inside the frame: tw = 0.25 x - 1 is negative left of x = 4, zero there, and covers further right
    horizon = np.array([[1, 0, 0], [0, 1, 0], [0.25, 0, -1]], np.float64)
    M, I, _ = refine(ctx, pair, horizon[None], iters=4)
    assert 0 < I[0, COV_IN] < w * h and I[0, STATUS] in (RC.REFINED, RC.UNCHANGED, RC.TOO_FEW, RC.DEGENERATE)
    # a constant current frame: no gradient, every d_i is 0
    flat = np.stack([prev, np.full_like(cur, 90)])
    M, I, N = refine(ctx, flat, np.eye(3)[None], iters=4)
    assert I[0, STATUS] == RC.DEGENERATE and I[0, EVALS] == 1 and I[0, N_IN] == (w - 2) * (h - 2) and not N[0, :36].any()
    # two pixels wide: no interior; 9 x 9: 49 interior pixels
    M, I, N = refine(ctx, pair[:, :, :2], np.eye(3)[None], iters=4)
    assert I[0, STATUS] == RC.TOO_FEW and I[0, N_IN] == 0 and I[0, COV_IN] == 2 * h and not N[0].any()
    M, I, N = refine(ctx, pair[:, :9, :9], np.eye(3)[None], iters=4)
    assert I[0, STATUS] == RC.TOO_FEW and I[0, N_IN] == 49 and I[0, EVALS] == 1
    M, I, N = refine(ctx, pair[:, :1, :1], np.eye(3)[None], iters=2)
    assert I[0, STATUS] == RC.TOO_FEW and I[0, COV_IN] == 1
    # identical frames: ssd = 0, nothing is better, every trial is rejected
    M, I, _ = refine(ctx, np.stack([cur, cur]), (3.0 * np.eye(3))[None], iters=3)
    assert I[0].tolist() == [RC.UNCHANGED, 4, 0, w * h, 0, w * h, 0, (w - 2) * (h - 2)]


def test_good_nan_good_and_repeats(ctx, family):
    frames, mats, _ = stack_of(family, (64, 48), False, 3)
    mats[1] = NAN
    M, I, N = refine(ctx, frames, mats, iters=5, frame_step=2)
    assert I[0, STATUS] == I[2, STATUS] == RC.REFINED and I[1, STATUS] == RC.NOTHING_COVERED
    for p in range(3):
        M1, I1, N1 = refine(ctx, frames[2 * p:2 * p + 2], mats[p:p + 1], iters=5)
        assert M1.tobytes() == M[p].tobytes() and I1.tobytes() == I[p].tobytes() and N1.tobytes() == N[p].tobytes(), p
    again = refine(ctx, frames, mats, iters=5, frame_step=2)                     # the same call twice: the same bytes
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (M, I, N)))
    in_place = refine(ctx, frames, mats, iters=5, frame_step=2, in_place=True)   # d_M_out == d_M_in
    assert all(a.tobytes() == b.tobytes() for a, b in zip(in_place, (M, I, N)))
    none = refine(ctx, frames, mats, iters=0, frame_step=2)
    assert none[0].tobytes() == mats.tobytes() and none[2].tobytes() == N.tobytes() and (none[1][:, EVALS] == 1).all()
    assert none[1][:, STATUS].tolist() == [RC.UNCHANGED, RC.NOTHING_COVERED, RC.UNCHANGED]
    assert np.array_equal(none[1][:, [COV_IN, SSD_IN, N_IN]], I[:, [COV_IN, SSD_IN, N_IN]])
    onto = refine(ctx, frames, M, iters=5, frame_step=2)                         # onto its own result: deterministic as well
    onto2 = refine(ctx, frames, M, iters=5, frame_step=2)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(onto, onto2))


@pytest.mark.parametrize("gray", [False, True])
def test_odd_pointers_and_strides(ctx, family, gray):
    frames, mats, _ = stack_of(family, (37, 29), gray, 2)
    cn, (h, w) = 1 if gray else 3, frames.shape[1:3]
    want = refine(ctx, frames, mats, iters=4, frame_step=2)
    for layout in ((w * cn + 1, (w * cn + 1) * h + 3, 1), (w * cn + 5, (w * cn + 5) * (h + 2), 7), (w * cn + 3, (w * cn + 3) * h, 4)):
        got = refine(ctx, frames, mats, iters=4, frame_step=2, src_layout=layout)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), layout


@pytest.mark.parametrize("size", [(37, 29), (24, 18)])
def test_planes_equal_the_bgr_entry_on_the_converted_frames(ctx, size):
    import torch
    rng = np.random.default_rng(31)
    w, h = size
    cw, ch = (w + 1) // 2, (h + 1) // 2
    prev, cur, _, M_start = F.pair(141, w, h, 1)
    planes = [(g, rng.integers(96, 160, (ch, cw), dtype=np.uint8), rng.integers(96, 160, (ch, cw), dtype=np.uint8)) for g in (prev, cur, prev, cur)]
    bgr = W.planes_to_bgr(planes)
    mats = np.stack([M_start, NAN, np.eye(3)])
    want = refine(ctx, bgr, mats, iters=4)
    assert want[1][0, STATUS] == RC.REFINED
    y, cb, cr = (dev(np.stack([p[i] for p in planes])) for i in range(3))
    uv = torch.stack([cb, cr], dim=-1).contiguous()
    packed = dev(np.stack([np.concatenate([a.reshape(-1) for a in p]) for p in planes]))
    conv = torch.zeros((4, h, w, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.yuv420_to_bgr((y, cb, cr), conv)
    ctx.synchronize()
    assert np.array_equal(conv.cpu().numpy(), bgr)
    for name, src, sz in (("i420", (y, cb, cr), None), ("nv12", (y, uv[..., 0], uv[..., 1]), None), ("packed", packed, (w, h))):
        got = refine(ctx, bgr, mats, iters=4, planes=src, size=sz)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), name


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(ctx, family):
    import torch
    from evenvizion_amd._lib import Yuv420
    INVALID, CAPACITY = -1, -3
    n, w, h = 3, 23, 17
    A = Arena(9)
    src = A.put(frames_of(80, n + 1, w, h))
    mats = A.put(np.tile(np.eye(3).reshape(1, 9), (n + 1, 1)))
    out = A.take((n + 1, 9), torch.float64, 7.0)
    info = A.take((n + 1, 8), torch.int64, -1)
    normal = A.take((n + 1, 45), torch.float64, 7.0)
    f, m, o, i, q = src.data_ptr(), mats.data_ptr(), out.data_ptr(), info.data_ptr(), normal.data_ptr()
    rs, fs = w * 3, w * h * 3
    good = dict(ctx=ctx.h, frames=f, n=n, step=1, w=w, h=h, cn=3, rs=rs, fs=fs, M=m, iters=2, clip=255, out=o, info=i, normal=q)

    def call(**kw):
        a = dict(good, **kw)
        return ctx.lib.evh_pair_refine(a["ctx"], a["frames"], a["n"], a["step"], a["w"], a["h"], a["cn"], a["rs"], a["fs"], a["M"],
                                       a["iters"], a["clip"], a["out"], a["info"], a["normal"])

    who, who_yuv = "evh_pair_refine: ", "evh_pair_refine_yuv420: "
    NS, NA, CH, STEP = "NULL source", "NULL argument", "channels must be 1 or 3", "frame_step must be 1 or 2"
    EM, IT, CL = "empty frame or negative npairs", "iters must lie in 0..64", "clip must lie in 0..255"
    BIG, NP, NF = "w and h stay within 4096", "at most 65535 pairs per call", "at most 65535 frames per call"
    SS = "source stride smaller than a row / frame"
    OFR, OI, ON, IN_, OM, IM, NM = ("d_M_out overlaps the frames", "d_M_out overlaps d_info", "d_M_out overlaps d_normal",
                                    "d_info overlaps d_normal", "d_M_out overlaps d_M_in", "d_info overlaps d_M_in",
                                    "d_normal overlaps d_M_in")

    def refused(rc, code, text, what):
        assert rc == code, what
        assert ctx.lib.evh_last_error_string(ctx.h).decode() == text, what

    assert call(ctx=None) == INVALID
    invalid = [(dict(frames=None), NS), (dict(M=None), NA), (dict(out=None), NA), (dict(info=None), NA), (dict(cn=2), CH), (dict(cn=0), CH),
               (dict(step=0), STEP), (dict(step=3), STEP), (dict(w=0), EM), (dict(h=-1), EM), (dict(n=-1), EM), (dict(iters=-1), IT),
               (dict(iters=65), IT), (dict(clip=-1), CL), (dict(clip=256), CL), (dict(rs=rs - 1), SS), (dict(fs=fs - 1), SS),
               (dict(n=1, fs=fs - 1), SS), (dict(out=f), OFR), (dict(out=f + (n + 1) * fs - 1), OFR), (dict(out=f - n * 72 + 1), OFR),
               (dict(info=f + 8), "d_info overlaps the frames"), (dict(normal=f + 16), "d_normal overlaps the frames"),
               (dict(out=i), OI), (dict(out=i + n * 64 - 8), OI), (dict(info=o + n * 72 - 8), OI), (dict(out=q), ON), (dict(normal=i + 8), IN_),
               (dict(out=m + 8), OM), (dict(out=m - 8), OM), (dict(M=o + 72), OM), (dict(info=m), IM), (dict(normal=m + n * 72 - 8), NM),
               # two faults: the earlier check of the entry names the refusal
               (dict(frames=None, out=None), NS), (dict(M=None, cn=2), NA), (dict(step=0, n=-1), STEP), (dict(iters=65, clip=256), IT),
               (dict(clip=256, rs=rs - 1), CL), (dict(rs=rs - 1, out=f), SS), (dict(out=f, info=m), OFR), (dict(out=i, normal=m), OI)]
    for kw, text in invalid:
        refused(call(**kw), INVALID, who + text, kw)
    capacity = [(dict(w=4097, rs=4097 * 3, fs=4097 * 3 * h), BIG), (dict(h=4097, fs=rs * 4097), BIG), (dict(n=65536), NP),
                (dict(w=4097), BIG), (dict(n=65536, fs=fs - 1), NP), (dict(h=1 << 26, out=f), BIG), (dict(w=4097, n=65536), BIG)]
    for kw, text in capacity:
        refused(call(**kw), CAPACITY, who + text, kw)
    refused(call(w=4096, rs=4096 * 3 - 1), INVALID, who + SS, "at the limit the ordinary checks apply")
    cw, ch = 12, 9
    y = A.take((n + 1, h, w))
    c = A.take((2, n + 1, ch, cw))
    torch.cuda.synchronize()
    yuv = dict(d_y=y.data_ptr(), d_cb=c[0].data_ptr(), d_cr=c[1].data_ptr(), y_stride=w, c_stride=cw, y_frame_stride=w * h,
               c_frame_stride=cw * ch, c_pixel_stride=1)

    def call_yuv(desc, **kw):
        a = dict(good, **kw)
        d = None if desc is None else ctypes.byref(Yuv420(**desc))
        return ctx.lib.evh_pair_refine_yuv420(a["ctx"], d, a["n"], a["step"], a["w"], a["h"], a["M"], a["iters"], a["clip"], a["out"],
                                              a["info"], a["normal"])

    refused(call_yuv(None), INVALID, who_yuv + NS, "no description")
    for bad, text in ((dict(d_y=None), NS), (dict(d_cr=None), NS), (dict(c_pixel_stride=3), "chroma pixel stride must be 1 or 2"),
                      (dict(y_stride=w - 1), "luma row stride smaller than the width"),
                      (dict(c_frame_stride=cw * ch - 1), "frame stride smaller than a plane")):
        refused(call_yuv(dict(yuv, **bad)), INVALID, who_yuv + text, bad)
    for kw, text in ((dict(M=None), NA), (dict(info=None), NA), (dict(w=0), EM), (dict(step=3), STEP), (dict(iters=65), IT), (dict(clip=256), CL),
                     (dict(out=y.data_ptr() + 7), OFR), (dict(out=c[1].data_ptr()), OFR), (dict(out=i), OI), (dict(info=m), IM)):
        refused(call_yuv(yuv, **kw), INVALID, who_yuv + text, kw)
    refused(call_yuv(dict(yuv, c_pixel_stride=3), n=65535, step=2), CAPACITY, who_yuv + NF, "the frames' capacity before the description")
    for kw, text in ((dict(w=4097), BIG), (dict(n=65536), NP), (dict(n=65535), NF)):
        refused(call_yuv(yuv, **kw), CAPACITY, who_yuv + text, kw)
    # no pairs: success, and nothing is done
    assert call(n=0) == 0 and call_yuv(yuv, n=0) == 0
    ctx.synchronize()
    assert (out == 7.0).all() and (info == -1).all() and (normal == 7.0).all()
    # the same arguments unrefused do write; d_normal may be NULL, d_M_out may be d_M_in
    assert call() == 0 and call(normal=None, out=m + 72 * n, M=m + 72 * n, info=i + 64 * n, n=1) == 0
    ctx.synchronize()
    got = info.cpu().numpy()
    want = R.residual_pairs(src.cpu().numpy(), np.tile(np.eye(3).reshape(1, 9), (n, 1)))[0]
    assert np.array_equal(got[:n, COV_IN], want[:, R.COVERED]) and np.array_equal(got[:n, SSD_IN], want[:, R.SSD])
    assert got[n, COV_IN] == want[0, R.COVERED] and got[n, SSD_IN] == want[0, R.SSD] and (out[n] == 7.0).all() and (normal[n] == 7.0).all()
    assert (normal[:n, 44] == (w - 2) * (h - 2)).all()


def test_python_layer_refuses_what_does_not_fit(ctx):
    import torch
    frames = dev(frames_of(81, 3, 16, 12))
    mats = dev(np.tile(np.eye(3).reshape(1, 9), (2, 1)))
    with pytest.raises(ValueError):
        ctx.pair_refine(frames, mats.float())
    with pytest.raises(ValueError):
        ctx.pair_refine(frames[:2], mats)                       # two pairs take three frames
    with pytest.raises(ValueError):
        ctx.pair_refine(frames, mats, frame_step=3)
    with pytest.raises(ValueError):
        ctx.pair_refine(frames, mats, info=torch.zeros((2, 7), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        ctx.pair_refine(frames, mats, normal=torch.zeros((2, 44), dtype=torch.float64, device="cuda"))
    out, info = ctx.pair_refine(frames, mats[:0])
    assert out.shape == (0, 9) and info.shape == (0, 8)


# ---- the reference's video -----------------------------------------------------------------------------------------------------------------
def test_pairs_16_and_100_of_the_reference_video(ctx):
    """refine_pair_maps over frames 15, 16, 99 and 100 with their recorded matrices: on pairs 16 and 100 the gain in PSNR is at least
    half the gain the restatement reaches on the same device-resized frames."""
    import torch
    from evenvizion_amd import capture, registration
    from evenvizion_amd.processing.utils import read_homography_dict, superposition_dict
    from evenvizion_amd.synthetic import SyntheticCapture
    hd, ri = read_homography_dict(GOLD)
    sup = superposition_dict(hd)
    cap = capture.VideoCapture(MP4)
    kept = {}
    for no in range(1, 101):
        ok, frame = cap.read()
        assert ok
        if no in (15, 16, 99, 100):
            kept[no] = np.ascontiguousarray(frame)
    cap.release()
    nos = sorted(kept)
    maps, info = registration.refine_pair_maps(SyntheticCapture([kept[k] for k in nos]), {k: sup[k] for k in nos}, ri, iters=8)
    assert list(maps) == [16, 99, 100]
    small = torch.zeros((4, ri["h"], ri["w"], 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.resize_area(torch.from_numpy(np.stack([kept[k] for k in nos])).cuda(), small)
    ctx.synchronize()
    small = dict(zip(nos, small.cpu().numpy()))
    start = registration.pair_maps({k: sup[k] for k in nos})
    for no in (16, 100):
        e = info[no]
        assert (e["covered_in"], e["ssd_in"]) == RC.cost(small[no - 1], small[no], start[no])
        assert (e["covered_out"], e["ssd_out"]) == RC.cost(small[no - 1], small[no], maps[no])
        _, host = RC.refine(small[no - 1], small[no], start[no], 8)
        before = registration.psnr(e["covered_in"], e["ssd_in"])
        gain = registration.psnr(e["covered_out"], e["ssd_out"]) - before
        host_gain = registration.psnr(host["covered_out"], host["ssd_out"]) - registration.psnr(host["covered_in"], host["ssd_in"])
        print("pair %d: %.2f dB, device gains %.3f dB in %d steps, the restatement %.3f dB in %d"
              % (no, before, gain, e["accepted"], host_gain, host["accepted"]))
        assert gain >= 0.5 * host_gain and gain >= 0
    assert info[16]["status"] == RC.REFINED


def test_component_writes_the_direct_files_only_on_request(tmp_path, monkeypatch):
    from evenvizion_amd import component
    monkeypatch.chdir(tmp_path)
    base = ["--path_to_video", "synthetic:4:400x224:3", "--features", "ORB", "--registration_report", "1"]
    plain = component.main(base + ["--experiment_name", "plain"])
    folder = component.main(base + ["--experiment_name", "direct", "--refine_direct", "1", "--refine_levels", "2", "--refine_iters", "4"])
    old = sorted(os.listdir(plain))
    assert sorted(os.listdir(folder)) == sorted(old + ["dict_with_homography_matrix_direct.json", "direct_report.json"])
    for name in old:
        with open(os.path.join(plain, name), "rb") as a, open(os.path.join(folder, name), "rb") as b:
            assert a.read() == b.read(), name
    with open(os.path.join(folder, "dict_with_homography_matrix_direct.json")) as f:
        direct = json.load(f)
    with open(os.path.join(folder, "direct_report.json")) as f:
        report = json.load(f)
    assert list(direct) == ["2", "3", "4", "resize_info"] and direct["resize_info"] == {"h": 224, "w": 400}
    assert np.asarray(direct["2"]["H"]).shape == (3, 3)
    assert list(report["info"]) == ["2", "3", "4"] and report["after"]["itf"] >= report["before"]["itf"]
    with open(os.path.join(folder, "registration_report.json")) as f:
        assert json.load(f) == report["before"]
