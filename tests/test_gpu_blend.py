"""evh_blend_fixed_plane / evh_blend_ray_surface / evh_pair_exposure (and their _yuv420 forms) on the device.  Pictures, states
and sums are compared for equality with the numpy restatement of the header's arithmetic (tests/blend_checks.py, itself held
against warp_checks and the contract's identities in test_blend_host.py).  The restatement of a case is computed once per module
and shared."""
import functools

import numpy as np
import pytest

import blend_checks as BC
import surface_checks as SC
import warp_checks as W
from evenvizion_amd import blend as B
from evenvizion_amd import surface as F

pytestmark = pytest.mark.gpu
SENTINEL = 0xCD
SW, SH, DW, DH, ORIGIN = 37, 23, 53, 41, (-7, -5)
MODES = (BC.FEATHER, BC.SEAM)
INVALID, CAPACITY = -1, -3


@pytest.fixture(scope="module")
def ctx():
    from evenvizion_amd._lib import Context
    c = Context(device=0, max_w=64, max_h=64, max_features=500, max_frames=2)     # the entries do not depend on these sizes
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()            # a copy: the shared arrays are read-only


@functools.lru_cache(maxsize=None)
def frames_of(seed, n=5, gray=False, w=SW, h=SH):
    a = np.random.default_rng(seed).integers(0, 256, (n, h, w) if gray else (n, h, w, 3), dtype=np.uint8)
    a.setflags(write=False)
    return a


def matrices(which="a"):
    """frame pixel -> plane point.  a: an integer and a fractional translation, two projective matrices, NaN; b: the integer
    translation, a matrix whose horizon crosses the canvas (tw = 1 - 0.03 X under the adjugate), the fractional translation,
    NaN, a projective matrix."""
    t0, t1 = W.translation(-3, -2), W.translation(4.37, 6.81)
    p0 = np.array([[1.05, 0.08, 2.3], [-0.06, 0.97, 9.1], [6e-4, -3e-4, 1.0]])
    p1 = np.array([[0.9, -0.12, 11.6], [0.1, 1.1, -3.2], [-8e-4, 5e-4, 1.0]])
    nan, horizon = np.full((3, 3), np.nan), np.array([[1.0, 0, 2], [0, 1, 3], [0.03, 0, 1]])
    return np.stack([t0, t1, p0, p1, nan] if which == "a" else [t0, horizon, t1, nan, p1])


GAINS = {"none": None, "ones": np.full((5, 3), 4096, np.uint16),
         "extreme": np.array([[1, 65535, 1], [65535, 1, 65535], [65535, 65535, 65535], [1, 1, 1], [4096, 1, 65535]], np.uint16),
         "mixed": np.array([[3072, 4096, 5120], [5000, 3900, 4100], [4096, 4096, 4096], [2048, 8192, 4097], [1, 2, 3]], np.uint16)}


@functools.lru_cache(maxsize=None)
def want(which, gray, mode, feather, gains):
    """(state) of the restatement for the module's frames and matrices"""
    return BC.blend(frames_of(21, gray=gray), matrices(which), DW, DH, ORIGIN, mode, feather, GAINS[gains])[1]


def run(ctx, frames, mats, mode, feather, gains=None, state=None, background=None, bg_is_out=False, out_pad=0, with_out=True,
        with_acc=True, acc_skew=False, ray=None, inverse_map=False, size=None, shape=(DH, DW), origin=ORIGIN, cn=None):
    """-> (picture or None, state or None) as numpy.  frames: a tensor / planes for Context.blend_*; out_pad: extra pixels per output
    row (must keep SENTINEL); acc_skew: the state starts 8 bytes into its buffer, so it is 8- but not 16-byte aligned."""
    import torch
    n = len(mats)
    dh, dw = shape
    if cn is None:
        cn = 1 if (not isinstance(frames, (tuple, list)) and frames.dim() == 3) else 3
    tail = () if cn == 1 else (3,)
    full = torch.full((dh + 1, dw + out_pad) + tail, SENTINEL, dtype=torch.uint8, device="cuda")
    out = full[:dh, :dw]
    bg = None
    if background is not None:
        if bg_is_out:
            out.copy_(dev(background))
            bg = out
        else:
            bgfull = torch.full((dh + 1, dw + out_pad) + tail, SENTINEL, dtype=torch.uint8, device="cuda")
            bg = bgfull[:dh, :dw]
            bg.copy_(dev(background))
    acc = None
    if with_acc:
        flat = torch.full((dh * dw * (cn + 1) + 2,), -0x3232323232323233, dtype=torch.int64, device="cuda")
        acc = flat[1:-1].view(dh, dw, cn + 1) if acc_skew else flat[:-2].view(dh, dw, cn + 1)
        assert acc.data_ptr() % 16 == (8 if acc_skew else 0)
        if state is not None:
            acc.copy_(dev(BC.state_to_i64(np.asarray(state, object).reshape(dh, dw, cn + 1))))
    kw = dict(out=out if with_out else None, mode=mode, feather=feather, gains=None if gains is None else dev(gains), acc=acc,
              acc_in=state is not None, background=bg, size=size)
    d_m = dev(np.asarray(mats, np.float64).reshape(n, 9)) if n else torch.zeros((0, 9), dtype=torch.float64, device="cuda")
    if ray is not None:
        ctx.blend_ray_surface(frames, d_m, dev(ray[0]), dev(ray[1]), **kw)
    else:
        ctx.blend_fixed_plane(frames, d_m, origin, inverse_map=inverse_map, shape=shape, **kw)
    ctx.synchronize()
    got = full.cpu().numpy()
    if with_out:
        gaps = np.ones(got.shape, bool)
        gaps[:dh, :dw] = False
        assert (got[gaps] == SENTINEL).all(), "bytes outside the canvas rows were written"
    else:
        assert (got == SENTINEL).all()
    st = None
    if with_acc:
        host = flat.cpu().numpy()
        assert host[-1] == -0x3232323232323233 and host[0 if acc_skew else -2] == -0x3232323232323233
        st = acc.cpu().numpy()
    return (got[:dh, :dw] if with_out else None), st


def same_state(got, state):
    return np.array_equal(got, BC.state_to_i64(state))


# ---- the restatement, byte for byte --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("feather", [0, 1, 40, 65535])
@pytest.mark.parametrize("mode", MODES)
def test_pictures_and_states_equal_the_restatement(ctx, mode, feather, gray):
    """Every gain table; the background rotates through NULL, given and d_out itself, the output rows through tight (an odd
    stride) and padded to words, the state through 16- and 8-byte alignment."""
    f = dev(frames_of(21, gray=gray))
    bg = frames_of(22, 1, gray, DW, DH)[0]
    for k, gains in enumerate(GAINS):
        state = want("a", gray, mode, feather, gains)
        background, bg_is_out = (None, False) if k % 3 == 0 else (bg, k % 3 == 2)
        pic, st = run(ctx, f, matrices("a"), mode, feather, GAINS[gains], background=background, bg_is_out=bg_is_out,
                      out_pad=3 * (k % 2), acc_skew=bool(k & 2))
        ref = BC.picture(state, mode, background)
        print("%s F=%d gains=%s: differing bytes %d, differing state words %d" % (mode, feather, gains, (pic != ref).sum(),
                                                                                   (st != BC.state_to_i64(state)).sum()))
        assert np.array_equal(pic, ref) and same_state(st, state)
    if feather == 40:                    # the clamp acts, and so does the feather
        assert (BC.picture(want("a", gray, mode, 40, "extreme"), mode) == 255).any()
        assert not np.array_equal(BC.picture(want("a", gray, mode, 40, "none"), mode), BC.picture(want("a", gray, mode, 0, "none"), mode))


@pytest.mark.parametrize("mode", MODES)
def test_nan_and_horizon_matrices_and_either_output_alone(ctx, mode):
    f, mats = frames_of(21), matrices("b")
    pic_ref, state = BC.blend(f, mats, DW, DH, ORIGIN, mode, 40, GAINS["mixed"])
    covered = np.stack([BC.position(m, SW, SH, DW, DH, ORIGIN)[2] for m in mats])
    assert covered[1].any() and not covered[1].all() and not covered[3].any()               # the horizon lies at X = 33.3
    pic, st = run(ctx, dev(f), mats, mode, 40, GAINS["mixed"])
    assert np.array_equal(pic, pic_ref) and same_state(st, state)
    pic, st = run(ctx, dev(f), mats, mode, 40, GAINS["mixed"], with_acc=False)
    assert np.array_equal(pic, pic_ref) and st is None
    pic, st = run(ctx, dev(f), mats, mode, 40, GAINS["mixed"], with_out=False)
    assert pic is None and same_state(st, state)


# ---- the identities the contract implies ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_identities(ctx, mode):
    import torch
    f, mats = frames_of(21), matrices("a")
    d_f = dev(f)
    # 1. a pixel one frame covers holds the warp entry's byte, for any F
    mosaic = torch.zeros((DH, DW, 3), dtype=torch.uint8, device="cuda")
    ctx.warp_fixed_plane(d_f, dev(mats.reshape(5, 9)), mosaic, "mosaic", ORIGIN)
    ctx.synchronize()
    once = np.stack([BC.position(m, SW, SH, DW, DH, ORIGIN)[2] for m in mats]).sum(axis=0) == 1
    assert once.any()
    for feather in (0, 40, 65535):
        pic, _ = run(ctx, d_f, mats, mode, feather, GAINS["ones"])
        assert np.array_equal(pic[once], mosaic.cpu().numpy()[once]), feather
    # 2. frames that all show the same value blend to it
    flat = np.zeros((5, SH, SW, 3), np.uint8)
    flat[...] = [137, 0, 255]
    pic, _ = run(ctx, dev(flat), mats, mode, 40)
    any_cover = np.stack([BC.position(m, SW, SH, DW, DH, ORIGIN)[2] for m in mats]).any(axis=0)
    assert (pic[any_cover] == [137, 0, 255]).all() and (pic[~any_cover] == 0).all()
    # 3. no gains are gains of 4096
    a, b = run(ctx, d_f, mats, mode, 40, None), run(ctx, d_f, mats, mode, 40, GAINS["ones"])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # 4. three frames, then two on the carried state, are one call of five
    whole = run(ctx, d_f, mats, mode, 40, GAINS["mixed"])
    _, head = run(ctx, d_f[:3], mats[:3], mode, 40, GAINS["mixed"][:3], with_out=False)
    state = np.array([int(v) for v in head.reshape(-1)], object).reshape(head.shape)
    tail = run(ctx, d_f[3:], mats[3:], mode, 40, GAINS["mixed"][3:], state=state)
    assert np.array_equal(whole[0], tail[0]) and np.array_equal(whole[1], tail[1])
    # 5. the ray form with the plane's tables is the plane form with inverse_map, where tw > 0 (everywhere, here)
    inv = np.stack([np.linalg.inv(m) if np.isfinite(m).all() else m for m in mats])
    cols, rows = SC.plane_tables(DW, DH, ORIGIN)
    assert all((SC.ray_frame(f[k], inv[k], cols, rows)[2] > 0).all() for k in range(4))
    a = run(ctx, d_f, inv, mode, 40, GAINS["mixed"], inverse_map=True)
    b = run(ctx, d_f, inv, mode, 40, GAINS["mixed"], ray=(cols, rows))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    ref = BC.blend(f, inv, DW, DH, ORIGIN, mode, 40, GAINS["mixed"], inverse_map=True)
    assert np.array_equal(a[0], ref[0]) and same_state(a[1], ref[1])


@pytest.mark.parametrize("mode", MODES)
def test_planes_equal_the_bgr_entry_on_the_converted_frames(ctx, mode):
    """6. I420, NV12 and packed planes of 38 x 24, on the plane and on a cylinder"""
    import torch
    rng = np.random.default_rng(23)
    n, w, h, cw, ch = 5, 38, 24, 19, 12
    planes = [(rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8),
               rng.integers(0, 256, (ch, cw), dtype=np.uint8)) for _ in range(n)]
    bgr = SC.planes_to_bgr(planes)
    y, cb, cr = (dev(np.stack([p[i] for p in planes])) for i in range(3))
    uv = torch.stack([cb, cr], dim=-1).contiguous()
    packed = dev(np.stack([np.concatenate([a.reshape(-1) for a in p]) for p in planes]))
    conv = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    ctx.yuv420_to_bgr((y, cb, cr), conv)
    ctx.synchronize()
    assert np.array_equal(conv.cpu().numpy(), bgr)
    mats = matrices("a")
    cyl = F.surface_tables("cylinder", 20.0, -26, -20, DW, DH)
    cams = np.stack([F.frame_matrix(np.eye(3), 20.0, None, (w, h), (w, h))] * n)
    cams[1:, 2] += [3.0, -4.5, 7.25, 1.0]                                      # the principal point moved: other parts of the cylinder
    for ray, m in ((None, mats), (cyl, cams)):
        ref = (BC.blend(bgr, m, DW, DH, ORIGIN, mode, 40, GAINS["mixed"]) if ray is None
               else BC.blend_ray(bgr, m, ray[0], ray[1], mode, 40, GAINS["mixed"]))
        assert (ref[0] != 0).any()
        via_bgr = run(ctx, conv, m, mode, 40, GAINS["mixed"], ray=ray)
        assert np.array_equal(via_bgr[0], ref[0]) and same_state(via_bgr[1], ref[1])
        for name, src, size in (("i420", (y, cb, cr), None), ("nv12", (y, uv[..., 0], uv[..., 1]), None), ("packed", packed, (w, h))):
            got = run(ctx, src, m, mode, 40, GAINS["mixed"], ray=ray, size=size, cn=3)
            assert np.array_equal(got[0], via_bgr[0]) and np.array_equal(got[1], via_bgr[1]), name


def test_seam_keeps_the_earliest_of_equal_weights(ctx):
    f = frames_of(24, 2)
    mats = np.stack([W.translation(2, 3)] * 2)
    pic, _ = run(ctx, dev(f), mats, BC.SEAM, 40)
    assert np.array_equal(pic, W.warp_canvases(f[:1], mats[:1], "mosaic", DW, DH, ORIGIN))
    assert not np.array_equal(pic, W.warp_canvases(f, mats, "mosaic", DW, DH, ORIGIN))


# ---- a handed-in state: where a wrong 64-bit division shows ------------------------------------------------------------------------------
def crafted_state(mode, cn):
    """Every pixel another (acc per channel, den): dens up to 2^44 - 1, accs up to 2^62 - 1, and for every den the accs one step to
    either side of the rounding thresholds of the quotients 0, 1, 63, 64, 128, 254, 255, 256 (those that stay below 2^62: above
    den = 2^42 a quotient of 256 would need more), 0, the largest value allowed, and one far above the clamp.  Channel c of a pixel
    takes another threshold of the same den.  Two pixels have den == 0: they take the background, whatever acc holds."""
    top = (1 << 62) - 1
    groups = []
    for den in (1, 2, 3, 255, 65537, (1 << 31) + 7, (1 << 32) - 1, (1 << 42) - 1, (1 << 43) + 12345, (1 << 44) - 1):
        accs = [0, top, min((den << 12) * 300, top)]
        for q in (0, 1, 63, 64, 128, 254, 255, 256):
            edge = q * (den << 12) - (den << 11) if mode == BC.FEATHER else (q << 12) - 2048
            accs += [min(max(edge + e, 0), top) for e in (-1, 0, 1)]
        groups.append((den, accs))
    groups.append((0, [0, 12345, top]))
    st = np.empty((DH, DW, cn + 1), object)
    for k in range(DH * DW):
        den, accs = groups[k % len(groups)]
        for c in range(cn):
            st[k // DW, k % DW, c] = accs[(k // len(groups) + 5 * c) % len(accs)]
        st[k // DW, k % DW, cn] = den
    return st


@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_handed_in_state(ctx, mode, gray):
    import torch
    cn = 1 if gray else 3
    st = crafted_state(mode, cn)
    bg = frames_of(25, 1, gray, DW, DH)[0]
    ref = BC.picture(st, mode, bg)
    values = set(ref.reshape(-1).tolist())
    assert {0, 1, 127, 128, 253, 254, 255} <= values
    none = torch.zeros((0, SH, SW) + (() if gray else (3,)), dtype=torch.uint8, device="cuda")
    # no frames: the picture of the incoming state, the state handed back as it came
    for skew in (False, True):
        pic, back = run(ctx, none, np.zeros((0, 9)), mode, 40, state=st, background=bg, acc_skew=skew)
        print("%s cn=%d: differing bytes %d" % (mode, cn, (pic != ref).sum()))
        assert np.array_equal(pic, ref) and same_state(back, st)
    # and frames on top of it: five frames add up to 5 * 2^41 to acc and 5 * 2^16 to den, so the state handed in is halved to stay
    # inside the bounds for which the header states the formulas
    half = np.array([int(v) >> 1 for v in st.reshape(-1)], object).reshape(st.shape)
    f, mats = frames_of(21, gray=gray), matrices("a")
    more = BC.blend(f, mats, DW, DH, ORIGIN, mode, 40, GAINS["mixed"], state=half, background=bg)
    assert all(int(v) < (1 << 62) for v in more[1][..., :cn].reshape(-1)) and all(int(v) < (1 << 44) for v in more[1][..., cn].reshape(-1))
    pic, back = run(ctx, dev(f), mats, mode, 40, GAINS["mixed"], state=half, background=bg)
    assert np.array_equal(pic, more[0]) and same_state(back, more[1])


# ---- a static scene --------------------------------------------------------------------------------------------------------------------
def test_static_scene_and_exposure_gains(ctx):
    """Frames cut from one texture by integer translations blend to the texture exactly.  With frame k stored as
    rint(gamma_k scene), gamma in [0.75, 1.25], and gains quantise_gains(1 / gamma_k): a stored sample is within 0.5 of gamma s, the
    quantised gain within 1 / 8192 of 1 / gamma, so each corrected sample is within 0.5 / 0.75 + 255 / 8192 < 0.71 of s; a weighted
    mean stays within that, and rounding to a byte gives at most 1."""
    rng = np.random.default_rng(26)
    scene = rng.integers(0, 205, (DH + 8, DW + 8, 3), dtype=np.uint8)             # 204 * 1.25 = 255
    at = [(0, 0), (11, 5), (24, 18), (16, 9), (5, 14)]
    mats = np.stack([W.translation(x, y) for x, y in at])
    cut = np.stack([scene[y:y + SH, x:x + SW] for x, y in at])
    any_cover = np.stack([BC.position(m, SW, SH, DW, DH, (0, 0))[2] for m in mats]).any(axis=0)
    for mode in MODES:
        pic, _ = run(ctx, dev(cut), mats, mode, 40, origin=(0, 0))
        assert np.array_equal(pic[any_cover], scene[:DH, :DW][any_cover]) and (pic[~any_cover] == 0).all()
    gamma = np.array([0.75, 1.25, 0.9, 1.1, 1.0])
    stored = np.rint(gamma[:, None, None, None] * cut).astype(np.uint8)
    gains = B.quantise_gains(np.repeat(1.0 / gamma[:, None], 3, axis=1))
    for mode in MODES:
        pic, st = run(ctx, dev(stored), mats, mode, 40, gains, origin=(0, 0))
        ref = BC.blend(stored, mats, DW, DH, (0, 0), mode, 40, gains)
        assert np.array_equal(pic, ref[0]) and same_state(st, ref[1])
        err = np.abs(pic.astype(int) - scene[:DH, :DW].astype(int))[any_cover]
        plain, _ = run(ctx, dev(stored), mats, mode, 40, origin=(0, 0))
        print("%s: max |blend - scene| %d with gains, %d without" % (mode, err.max(), np.abs(plain.astype(int) - scene[:DH, :DW].astype(int))[any_cover].max()))
        assert err.max() <= 1


# ---- evh_pair_exposure ------------------------------------------------------------------------------------------------------------------
PAIRS = [(0, 0), (0, 1), (4, 0), (5, 0), (1, -1), (2, 3), (3, 2), (1, 4)]


def exposure_maps():
    """pixels of frame i -> pixels of frame j, per pair of PAIRS: (2, 3) has a NaN map, (3, 2) one that covers nothing"""
    m = [np.eye(3), W.translation(2.25, -1.5), np.array([[1.02, 0.03, -1.0], [-0.02, 0.98, 1.7], [2e-4, -1e-4, 1.0]]), np.eye(3), np.eye(3),
         np.full((3, 3), np.nan), W.translation(1000, 0), W.translation(-30.5, 3)]
    return np.stack(m)


@pytest.mark.parametrize("source", ["bgr", "gray", "i420", "nv12"])
def test_pair_exposure_equals_the_restatement(ctx, source):
    import torch
    n = 5
    rng = np.random.default_rng(27)
    if source in ("bgr", "gray"):
        host = np.array(frames_of(28, n, source == "gray"))
        host[1] = host[0] // 2 + 60                                             # frames that share their content: mid-range values
        src, size = dev(host), None
    else:
        w, h, cw, ch = 38, 24, 19, 12
        planes = [(rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(96, 160, (ch, cw), dtype=np.uint8),
                   rng.integers(96, 160, (ch, cw), dtype=np.uint8)) for _ in range(n)]
        host = SC.planes_to_bgr(planes)
        y, cb, cr = (dev(np.stack([p[i] for p in planes])) for i in range(3))
        uv = torch.stack([cb, cr], dim=-1).contiguous()
        src, size = ((y, cb, cr) if source == "i420" else (y, uv[..., 0], uv[..., 1])), None
    maps = exposure_maps()
    d_pairs, d_maps = dev(np.array(PAIRS, np.int32)), dev(maps.reshape(-1, 9))
    stats = torch.full((len(PAIRS), 7), -1, dtype=torch.int64, device="cuda")      # the entry zeroes it itself
    for step in (1, 3, 64):
        for lo, hi in ((0, 255), (8, 247), (100, 100)):
            ref = BC.exposure(host, PAIRS, maps, step, lo, hi)
            got = ctx.pair_exposure(src, d_pairs, d_maps, step=step, lo=lo, hi=hi, stats=stats, size=size)
            ctx.synchronize()
            got = got.cpu().numpy()
            print("%s step %d [%d, %d]: pixels %s" % (source, step, lo, hi, got[:, 0].tolist()))
            assert np.array_equal(got, ref.astype(np.int64)), (step, lo, hi)
            assert not got[3:7].any()                                           # indices out of range, NaN, nothing covered
            if (lo, hi) == (0, 255):
                gw, gh = -(-host.shape[2] // step), -(-host.shape[1] // step)
                assert got[0, 0] == gw * gh and (got[0, 1:4] == got[0, 4:7]).all()
                assert step > 1 or (got[1, 0] > 0 and got[2, 0] > 0 and got[7, 0] > 0)
            if source == "gray":
                assert not got[:, [2, 3, 5, 6]].any()
    assert ctx.pair_exposure(src, d_pairs[:0], d_maps[:0], size=size).shape == (0, 7)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_blend_refusals_leave_the_outputs_alone(ctx):
    import torch
    from evenvizion_amd._lib import Yuv420
    n, dw, dh = 2, 31, 22
    src = dev(frames_of(29, n))
    pc, pr = SC.plane_tables(dw, dh)
    mats, cols, rows = dev(np.tile(np.eye(3).reshape(1, 9), (n, 1))), dev(pc), dev(pr)
    gain = dev(np.full((n, 3), 4096, np.uint16))
    out = torch.full((dh + 2, dw, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    acc = torch.full((dh * dw * 4 + 2,), 0x0123456789ABCDEF, dtype=torch.int64, device="cuda")
    elsewhere = torch.full((dh, dw, 3), 7, dtype=torch.uint8, device="cuda")
    ors = dw * 3
    o = out.data_ptr() + ors                                                     # a row of the buffer on either side of the canvas
    good = dict(ctx=ctx.h, frames=src.data_ptr(), n=n, sw=SW, sh=SH, cn=3, rs=SW * 3, fs=SW * SH * 3, M=mats.data_ptr(), inv=1,
                col=cols.data_ptr(), row=rows.data_ptr(), mode=0, F=40, gain=gain.data_ptr(), acc=acc.data_ptr(), acc_in=0,
                bg=elsewhere.data_ptr(), out=o, dw=dw, dh=dh, ors=ors, ox=0, oy=0)

    def plane(**kw):
        a = dict(good, **kw)
        return ctx.lib.evh_blend_fixed_plane(a["ctx"], a["frames"], a["n"], a["sw"], a["sh"], a["cn"], a["rs"], a["fs"], a["M"], a["inv"],
                                             a["mode"], a["F"], a["gain"], a["acc"], a["acc_in"], a["bg"], a["out"], a["dw"], a["dh"],
                                             a["ors"], a["ox"], a["oy"])

    def ray(**kw):
        a = dict(good, **kw)
        return ctx.lib.evh_blend_ray_surface(a["ctx"], a["frames"], a["n"], a["sw"], a["sh"], a["cn"], a["rs"], a["fs"], a["M"], a["col"],
                                             a["row"], a["mode"], a["F"], a["gain"], a["acc"], a["acc_in"], a["bg"], a["out"], a["dw"],
                                             a["dh"], a["ors"])

    state_bytes = dw * dh * 4 * 8
    invalid = [dict(frames=None), dict(M=None), dict(cn=2), dict(cn=0), dict(sw=0), dict(sh=0), dict(dw=0), dict(dh=-1), dict(n=-1),
               dict(rs=SW * 3 - 1), dict(fs=SW * SH * 3 - 1), dict(ors=ors - 1), dict(mode=2), dict(mode=-1), dict(F=-1), dict(F=65536),
               dict(out=None, acc=None), dict(acc=None, acc_in=1), dict(acc=acc.data_ptr() + 4), dict(acc=acc.data_ptr() + 1),
               dict(bg=o + 3), dict(bg=o + ors), dict(bg=o - ors),                              # only bg == out may overlap
               dict(acc=src.data_ptr()), dict(acc=gain.data_ptr()), dict(acc=mats.data_ptr()), dict(acc=elsewhere.data_ptr()),
               dict(out=acc.data_ptr() + state_bytes - 8), dict(out=src.data_ptr()), dict(out=gain.data_ptr() - dh * ors + 1),
               dict(bg=acc.data_ptr())]
    for call in (plane, ray):
        assert call(ctx=None) == INVALID
        for kw in invalid:
            assert call(**kw) == INVALID, (call.__name__, kw)
            assert ctx.lib.evh_last_error_string(ctx.h).decode().startswith("evh_blend_"), kw
        big = 1 << 26
        for kw in (dict(sw=big, rs=big * 3, fs=big * 3 * SH), dict(sh=big, fs=SW * 3 * big), dict(dw=65536, dh=32768, ors=65536 * 3, out=None),
                   dict(n=65536)):
            assert call(**kw) == CAPACITY, (call.__name__, kw)
    for kw in (dict(col=None), dict(row=None), dict(acc=cols.data_ptr()), dict(acc=rows.data_ptr())):
        assert ray(**kw) == INVALID, kw
    y = Yuv420(src.data_ptr(), src.data_ptr(), src.data_ptr(), SW, (SW + 1) // 2, SW * SH, SW * SH, 1)
    import ctypes
    for bad in (None, ctypes.byref(Yuv420(0, src.data_ptr(), src.data_ptr(), SW, (SW + 1) // 2, SW * SH, SW * SH, 1))):
        assert ctx.lib.evh_blend_fixed_plane_yuv420(ctx.h, bad, n, SW, SH, mats.data_ptr(), 1, 0, 40, None, acc.data_ptr(), 0, None, o, dw,
                                                    dh, ors, 0, 0) == INVALID
        assert ctx.lib.evh_blend_ray_surface_yuv420(ctx.h, bad, n, SW, SH, mats.data_ptr(), cols.data_ptr(), rows.data_ptr(), 0, 40, None,
                                                    acc.data_ptr(), 0, None, o, dw, dh, ors) == INVALID
    assert ctx.lib.evh_blend_fixed_plane_yuv420(ctx.h, ctypes.byref(y), n, SW, SH, mats.data_ptr(), 1, 7, 40, None, acc.data_ptr(), 0, None,
                                                o, dw, dh, ors, 0, 0) == INVALID
    ctx.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all() and (acc.cpu().numpy() == 0x0123456789ABCDEF).all()
    assert (elsewhere.cpu().numpy() == 7).all()
    # what is allowed: bg == out, and each output alone
    assert plane(bg=o) == 0 and plane(out=None, bg=o) == 0 and ray(acc=None, bg=None, gain=None) == 0
    ctx.synchronize()
    got = out.cpu().numpy()
    assert (got[0] == SENTINEL).all() and (got[-1] == SENTINEL).all() and (got[1:-1] != SENTINEL).any()
    assert acc.cpu().numpy()[-2:].tolist() == [0x0123456789ABCDEF] * 2


def test_pair_exposure_refusals_leave_the_sums_alone(ctx):
    import ctypes
    import torch
    from evenvizion_amd._lib import Yuv420
    n, npairs = 3, 2
    src = dev(frames_of(30, n))
    pairs, maps = dev(np.array([(0, 1), (1, 2)], np.int32)), dev(np.tile(np.eye(3).reshape(1, 9), (npairs, 1)))
    stats = torch.full((npairs, 7), -1, dtype=torch.int64, device="cuda")
    good = dict(ctx=ctx.h, frames=src.data_ptr(), n=n, w=SW, h=SH, cn=3, rs=SW * 3, fs=SW * SH * 3, pairs=pairs.data_ptr(), np=npairs,
                M=maps.data_ptr(), step=2, lo=8, hi=247, stats=stats.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return ctx.lib.evh_pair_exposure(a["ctx"], a["frames"], a["n"], a["w"], a["h"], a["cn"], a["rs"], a["fs"], a["pairs"], a["np"],
                                         a["M"], a["step"], a["lo"], a["hi"], a["stats"])

    assert call(ctx=None) == INVALID
    for kw in (dict(frames=None), dict(pairs=None), dict(M=None), dict(stats=None), dict(cn=2), dict(cn=4), dict(w=0), dict(h=0), dict(n=-1),
               dict(np=-1), dict(step=0), dict(step=65), dict(lo=-1), dict(hi=256), dict(lo=9, hi=8), dict(rs=SW * 3 - 1),
               dict(fs=SW * SH * 3 - 1), dict(stats=src.data_ptr()), dict(stats=pairs.data_ptr()), dict(stats=maps.data_ptr())):
        assert call(**kw) == INVALID, kw
        assert ctx.lib.evh_last_error_string(ctx.h).decode().startswith("evh_pair_exposure: "), kw
    big = 1 << 26
    for kw in (dict(w=big, rs=big * 3, fs=big * 3 * SH), dict(h=big, fs=SW * 3 * big), dict(w=65536, h=32768, rs=65536 * 3, fs=1 << 40),
               dict(np=65536), dict(n=65536)):
        assert call(**kw) == CAPACITY, kw
    y = Yuv420(0, src.data_ptr(), src.data_ptr(), SW, (SW + 1) // 2, SW * SH, SW * SH, 1)
    for bad in (None, ctypes.byref(y)):
        assert ctx.lib.evh_pair_exposure_yuv420(ctx.h, bad, n, SW, SH, pairs.data_ptr(), npairs, maps.data_ptr(), 2, 8, 247,
                                                stats.data_ptr()) == INVALID
    ctx.synchronize()
    assert (stats.cpu().numpy() == -1).all()
    assert call(np=0) == 0
    ctx.synchronize()
    assert (stats.cpu().numpy() == -1).all()                                     # no pairs: nothing is done
    assert call() == 0
    ctx.synchronize()
    assert (stats.cpu().numpy()[:, 0] > 0).all()
