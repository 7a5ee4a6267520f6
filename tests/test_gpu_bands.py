"""evh_seam_labels_* and evh_blend_bands_* (and their _yuv420 forms) on the device.  Labels, pictures and states are compared for
equality -- byte for byte, state word for state word -- with the numpy restatement of the header's arithmetic (tests/bands_checks.py,
itself held against the contract's identities in test_bands_host.py).  The restatement of a case is computed once per module and
shared.  Every crafted input stays inside the bounds the header states."""
import functools

import numpy as np
import pytest

import bands_checks as N
import blend_checks as BC
import surface_checks as SC
import warp_checks as W
from evenvizion_amd import surface as F

pytestmark = pytest.mark.gpu
SENTINEL = 0xCD
WORD = -0x3232323232323233
SW, SH, DW, DH, ORIGIN = 32, 24, 45, 37, (-7, -5)           # the canvas is odd at every level: 45, 23, 12, 6, 3, 2
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
    """test_gpu_blend.py's families.  a: an integer and a fractional translation, two projective matrices, NaN; b: the integer
    translation, a matrix whose horizon crosses the canvas, the fractional translation, a singular matrix, a projective one."""
    t0, t1 = W.translation(-3, -2), W.translation(4.37, 6.81)
    p0 = np.array([[1.05, 0.08, 2.3], [-0.06, 0.97, 9.1], [6e-4, -3e-4, 1.0]])
    p1 = np.array([[0.9, -0.12, 11.6], [0.1, 1.1, -3.2], [-8e-4, 5e-4, 1.0]])
    nan, horizon = np.full((3, 3), np.nan), np.array([[1.0, 0, 2], [0, 1, 3], [0.03, 0, 1]])
    singular = np.array([[1.0, 2, 3], [2, 4, 6], [0, 0, 1]])
    return np.stack([t0, t1, p0, p1, nan] if which == "a" else [t0, horizon, t1, singular, p1])


GAINS = {"none": None, "ones": np.full((5, 3), 4096, np.uint16),
         "extreme": np.array([[1, 65535, 1], [65535, 1, 65535], [65535, 65535, 65535], [1, 1, 1], [4096, 1, 65535]], np.uint16),
         "mixed": np.array([[3072, 4096, 5120], [5000, 3900, 4100], [4096, 4096, 4096], [2048, 8192, 4097], [1, 2, 3]], np.uint16)}


@functools.lru_cache(maxsize=None)
def seam_labels(which="a", feather=40, dw=DW, dh=DH):
    best, label = N.labels_plane(matrices(which), SW, SH, dw, dh, ORIGIN, feather)
    best.setflags(write=False)
    label.setflags(write=False)
    return best, label


@functools.lru_cache(maxsize=None)
def crafted_labels(kind):
    """random: any of the five frames per pixel, whether it covers the pixel or not (frame 4 has a NaN matrix); absent: also labels
    of frames that are not in the call and 65535; nobody: all 65535"""
    rng = np.random.default_rng(31)
    if kind == "random":
        a = rng.integers(0, 5, (DH, DW))
    elif kind == "absent":
        a = rng.choice(np.array([0, 1, 2, 3, 4, 5, 9, 65534, 65535]), (DH, DW))
    else:
        a = np.full((DH, DW), N.NOBODY)
    a = a.astype(np.uint16)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def want(which, gray, levels, gains, labels="seam", dw=DW, dh=DH):
    """the state of the restatement for the module's frames and matrices"""
    label = seam_labels(which, 40, dw, dh)[1] if labels == "seam" else crafted_labels(labels)
    st = N.bands_plane(frames_of(21, gray=gray), matrices(which), dw, dh, ORIGIN, label, levels, gains=GAINS[gains])[1]
    st.setflags(write=False)
    return st


def run(ctx, frames, mats, label, levels, gains=None, state=None, background=None, bg_is_out=False, out_pad=0, with_out=True,
        with_state=True, ws_frames=None, ray=None, inverse_map=False, size=None, first_label=0, origin=ORIGIN, cn=None):
    """-> (picture or None, state or None) as numpy.  ws_frames: how many frames' pyramids the workspace holds (None: all); the
    workspace and the state sit between guard words that must survive."""
    import torch
    from evenvizion_amd._lib import bands_frame_ws_bytes, bands_state_elems
    n = len(mats)
    dh, dw = label.shape
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
    elems = bands_state_elems(dw, dh, cn, levels)
    flat = acc = None
    if with_state:
        flat = torch.full((elems + 2,), WORD, dtype=torch.int64, device="cuda")
        acc = flat[1:-1]
        if state is not None:
            acc.copy_(dev(np.asarray(state, np.int64)))
    unit = bands_frame_ws_bytes(dw, dh, cn, levels)
    held = 0 if with_state else 8 * elems
    ws_bytes = held + unit * (max(n, 1) if ws_frames is None else ws_frames)
    wsfull = torch.full((ws_bytes + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    kw = dict(label=dev(label), levels=levels, out=out if with_out else None, first_label=first_label,
              gains=None if gains is None else dev(gains), state=acc, state_in=state is not None, ws=wsfull[8:-8], background=bg, size=size)
    d_m = dev(np.asarray(mats, np.float64).reshape(n, 9)) if n else torch.zeros((0, 9), dtype=torch.float64, device="cuda")
    if ray is not None:
        ctx.blend_bands_ray_surface(frames, d_m, dev(ray[0]), dev(ray[1]), **kw)
    else:
        ctx.blend_bands_fixed_plane(frames, d_m, origin, inverse_map=inverse_map, shape=(dh, dw), **kw)
    ctx.synchronize()
    got = full.cpu().numpy()
    if with_out:
        gaps = np.ones(got.shape, bool)
        gaps[:dh, :dw] = False
        assert (got[gaps] == SENTINEL).all(), "bytes outside the canvas rows were written"
    else:
        assert (got == SENTINEL).all()
    guard = wsfull.cpu().numpy()
    assert (guard[:8] == SENTINEL).all() and (guard[-8:] == SENTINEL).all(), "bytes outside the workspace were written"
    st = None
    if with_state:
        host = flat.cpu().numpy()
        assert host[0] == WORD and host[-1] == WORD, "words outside the state were written"
        st = host[1:-1]
    return (got[:dh, :dw] if with_out else None), st


def picture_of(state, levels, cn, background=None, dw=DW, dh=DH):
    return N.picture(state, dw, dh, cn, levels, background)


# ---- the labels entry -----------------------------------------------------------------------------------------------------------------
def run_labels(ctx, mats, feather, first_label=0, state=None, ray=None, inverse_map=False, shape=(DH, DW)):
    import torch
    dh, dw = shape
    bfull = torch.full((dh * dw + 2,), 0x31313131, dtype=torch.int32, device="cuda")
    lfull = torch.from_numpy(np.full(dh * dw + 2, 0x3131, np.uint16)).cuda()
    best, label = bfull[1:-1].view(dh, dw), lfull[1:-1].view(dh, dw)
    if state is not None:
        best.copy_(dev(state[0].astype(np.int64).astype(np.int32)))
        label.copy_(dev(state[1]))
    n = len(mats)
    d_m = dev(np.asarray(mats, np.float64).reshape(n, 9)) if n else torch.zeros((0, 9), dtype=torch.float64, device="cuda")
    kw = dict(feather=feather, first_label=first_label, best=best, label=label, state_in=state is not None)
    if ray is not None:
        ctx.seam_labels_ray_surface(d_m, (SW, SH), dev(ray[0]), dev(ray[1]), **kw)
    else:
        ctx.seam_labels_fixed_plane(d_m, (SW, SH), ORIGIN, (dh, dw), inverse_map=inverse_map, **kw)
    ctx.synchronize()
    b, l = bfull.cpu().numpy(), lfull.cpu().numpy()
    assert b[0] == 0x31313131 and b[-1] == 0x31313131 and l[0] == 0x3131 and l[-1] == 0x3131
    return b[1:-1].reshape(dh, dw).astype(np.uint32), l[1:-1].reshape(dh, dw)


@pytest.mark.parametrize("which", ["a", "b"])
def test_labels_equal_the_restatement_and_carry_their_state(ctx, which):
    mats = matrices(which)
    for feather in (0, 1, 40, 65535):
        ref = N.labels_plane(mats, SW, SH, DW, DH, ORIGIN, feather)
        got = run_labels(ctx, mats, feather)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), feather
        # SEAM's state holds the same weights, and its picture takes the labelled frame
        assert np.array_equal(ref[0], BC.blend(frames_of(21, gray=True), mats, DW, DH, ORIGIN, BC.SEAM, feather)[1][..., 1].astype(np.uint32))
    ref = N.labels_plane(mats, SW, SH, DW, DH, ORIGIN, 40, first_label=7)
    head = run_labels(ctx, mats[:2], 40, first_label=7)
    mid = run_labels(ctx, mats[2:3], 40, first_label=9, state=head)
    tail = run_labels(ctx, mats[3:], 40, first_label=10, state=mid)
    assert np.array_equal(tail[0], ref[0]) and np.array_equal(tail[1], ref[1])
    none = run_labels(ctx, mats[:0], 40)
    assert (none[0] == 0).all() and (none[1] == N.NOBODY).all()
    back = run_labels(ctx, mats[:0], 40, state=ref)
    assert np.array_equal(back[0], ref[0]) and np.array_equal(back[1], ref[1])


def test_labels_tie_rule_ray_form_and_the_largest_label(ctx):
    twice = run_labels(ctx, np.stack([W.translation(2, 3)] * 2), 40, first_label=65533)
    assert set(twice[1].reshape(-1).tolist()) == {65533, N.NOBODY}
    inv = np.stack([np.linalg.inv(m) if np.isfinite(m).all() else m for m in matrices("a")])
    cols, rows = SC.plane_tables(DW, DH, ORIGIN)
    a, b = run_labels(ctx, inv, 40, inverse_map=True), run_labels(ctx, inv, 40, ray=(cols, rows))
    ref = N.labels_ray(inv, cols, rows, SW, SH, 40)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(b[0], ref[0]) and np.array_equal(b[1], ref[1])
    cyl = F.surface_tables("cylinder", 20.0, -26, -20, DW, DH)
    cams = np.stack([F.frame_matrix(np.eye(3), 20.0, None, (SW, SH), (SW, SH))] * 3)
    cams[1:, 2] += [3.0, -4.5]
    ref = N.labels_ray(cams, cyl[0], cyl[1], SW, SH, 40)
    got = run_labels(ctx, cams, 40, ray=cyl)
    assert (ref[1] != N.NOBODY).any() and (ref[1] == N.NOBODY).any()            # the antipode is not covered
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


# ---- the restatement, byte for byte --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("levels", [0, 1, 2, 5, 8])
def test_pictures_and_states_equal_the_restatement(ctx, levels, gray):
    """Every gain table; the background rotates through NULL, given and d_out itself, the output rows through tight (an odd stride)
    and padded, the workspace through one frame's, two frames' and all frames' size."""
    f = dev(frames_of(21, gray=gray))
    cn = 1 if gray else 3
    bg = frames_of(22, 1, gray, DW, DH)[0]
    label = seam_labels()[1]
    for k, gains in enumerate(GAINS):
        state = want("a", gray, levels, gains)
        background, bg_is_out = (None, False) if k % 3 == 0 else (bg, k % 3 == 2)
        pic, st = run(ctx, f, matrices("a"), label, levels, GAINS[gains], background=background, bg_is_out=bg_is_out,
                      out_pad=3 * (k % 2), ws_frames=(1, None, 2, 5)[k])
        ref = picture_of(state, levels, cn, background)
        print("levels=%d gains=%s: differing bytes %d, differing state words %d" % (levels, gains, (pic != ref).sum(), (st != state).sum()))
        assert np.array_equal(pic, ref) and np.array_equal(st, state)
    assert (picture_of(want("a", gray, levels, "extreme"), levels, cn) == 255).any()         # the clamp acts


@pytest.mark.parametrize("levels", [2, 5])
def test_even_canvas_and_the_other_matrices(ctx, levels):
    """64 x 48, and family b: a horizon across the canvas and a singular matrix"""
    f, mats = frames_of(21), matrices("b")
    label = seam_labels("b", 40, 64, 48)[1]
    state = want("b", False, levels, "mixed", "seam", 64, 48)
    pic, st = run(ctx, dev(f), mats, label, levels, GAINS["mixed"], ws_frames=2)
    assert np.array_equal(pic, picture_of(state, levels, 3, None, 64, 48)) and np.array_equal(st, state)
    valid = [p[2] for p in N.plane_positions(mats, SW, SH, 64, 48, ORIGIN)]
    assert not valid[3].all() and valid[1].sum() > valid[1].size // 2


@pytest.mark.parametrize("labels", ["random", "absent", "nobody"])
def test_crafted_labels(ctx, labels):
    f = frames_of(21)
    bg = frames_of(22, 1, False, DW, DH)[0]
    for levels in (0, 2, 5):
        state = want("a", False, levels, "mixed", labels)
        pic, st = run(ctx, dev(f), matrices("a"), crafted_labels(labels), levels, GAINS["mixed"], background=bg, ws_frames=2)
        assert np.array_equal(pic, picture_of(state, levels, 3, bg)) and np.array_equal(st, state), levels
        if labels == "nobody":
            assert not state.any() and np.array_equal(pic, bg)


def test_the_contexts_own_workspace(ctx):
    """Without ws= the context keeps the workspace: the calls return with their launches only enqueued, and torch allocations made
    right behind them (which would take a freed workspace's memory) leave the results alone.  A larger canvas makes it grow."""
    import torch
    f, mats, label, g = dev(frames_of(21)), dev(matrices("a").reshape(5, 9)), dev(seam_labels()[1]), dev(GAINS["mixed"])
    for with_state in (True, False):
        state = want("a", False, 5, "mixed")
        out = torch.zeros((DH, DW, 3), dtype=torch.uint8, device="cuda")
        acc = torch.zeros(state.size, dtype=torch.int64, device="cuda") if with_state else None
        ctx.blend_bands_fixed_plane(f, mats, ORIGIN, label, levels=5, out=out, gains=g, state=acc)
        fill = [torch.full((1 << 20,), 0x5A, dtype=torch.uint8, device="cuda") for _ in range(4)]
        ctx.synchronize()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), picture_of(state, 5, 3)) and all(bool((t == 0x5A).all()) for t in fill)
        assert acc is None or np.array_equal(acc.cpu().numpy(), state)
    small = ctx._bands_ws.numel()
    big = want("b", False, 2, "mixed", "seam", 64, 48)
    out = torch.zeros((48, 64, 3), dtype=torch.uint8, device="cuda")
    ctx.blend_bands_fixed_plane(f, dev(matrices("b").reshape(5, 9)), ORIGIN, dev(seam_labels("b", 40, 64, 48)[1]), levels=2, out=out, gains=g)
    ctx.synchronize()
    assert ctx._bands_ws.numel() > small and np.array_equal(out.cpu().numpy(), picture_of(big, 2, 3, None, 64, 48))


def test_either_output_alone(ctx):
    f, mats, label = frames_of(21), matrices("a"), seam_labels()[1]
    for levels in (0, 5):
        state = want("a", False, levels, "mixed")
        ref = picture_of(state, levels, 3)
        for ws_frames in (1, 5):
            pic, st = run(ctx, dev(f), mats, label, levels, GAINS["mixed"], with_state=False, ws_frames=ws_frames)
            assert np.array_equal(pic, ref) and st is None
            pic, st = run(ctx, dev(f), mats, label, levels, GAINS["mixed"], with_out=False, ws_frames=ws_frames)
            assert pic is None and np.array_equal(st, state)


# ---- the identities the contract implies ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [0, 1, 3, 5])
def test_one_frame_under_its_own_labels_is_the_warp_entry(ctx, levels):
    """(a)"""
    import torch
    f = frames_of(23)
    for m in matrices("a")[:4]:
        cov = BC.position(m, SW, SH, DW, DH, ORIGIN)[2]
        label = np.where(cov, 0, N.NOBODY).astype(np.uint16)
        mosaic = torch.zeros((DH, DW, 3), dtype=torch.uint8, device="cuda")
        ctx.warp_fixed_plane(dev(f[:1]), dev(m.reshape(1, 9)), mosaic, "mosaic", ORIGIN)
        ctx.synchronize()
        pic, _ = run(ctx, dev(f[:1]), m[None], label, levels, GAINS["ones"][:1])
        assert cov.any() and np.array_equal(pic, mosaic.cpu().numpy())


def test_no_levels_under_seam_labels_are_seam(ctx):
    """(b): both through the device"""
    import torch
    f, mats = frames_of(21), matrices("a")
    for feather in (0, 40, 65535):
        _, label = run_labels(ctx, mats, feather)
        seam = torch.zeros((DH, DW, 3), dtype=torch.uint8, device="cuda")
        ctx.blend_fixed_plane(dev(f), dev(mats.reshape(5, 9)), ORIGIN, out=seam, mode="seam", feather=feather, gains=dev(GAINS["mixed"]))
        ctx.synchronize()
        pic, _ = run(ctx, dev(f), mats, label, 0, GAINS["mixed"])
        assert np.array_equal(pic, seam.cpu().numpy()), feather


def test_constant_frames_and_no_gains(ctx):
    """(c), and d_gain == NULL is a table of 4096"""
    flat = np.zeros((4, SH, SW, 3), np.uint8)
    flat[...] = [137, 0, 255]
    label = np.random.default_rng(3).integers(0, 4, (DH, DW)).astype(np.uint16)
    gain = np.tile(np.array([[5000, 3900, 3000]], np.uint16), (4, 1))
    want_px = np.minimum(255, (np.array([137, 0, 255]) * gain[0].astype(np.int64) + 2048) >> 12)
    for levels in (0, 2, 5, 8):
        pic, _ = run(ctx, dev(flat), matrices("a")[:4], label, levels, gain)
        assert (pic == want_px).all(), levels
    f, mats = dev(frames_of(21)), matrices("a")
    a, b = run(ctx, f, mats, seam_labels()[1], 3, None), run(ctx, f, mats, seam_labels()[1], 3, GAINS["ones"])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_carried_state_and_frame_order(ctx):
    """(d): two calls, three calls, and the frames one by one in another order, each with the workspace of one frame"""
    f, mats, label, g = frames_of(21), matrices("a"), seam_labels()[1], GAINS["mixed"]
    d_f = dev(f)
    state = want("a", False, 5, "mixed")
    ref = picture_of(state, 5, 3)
    for cuts in ((3,), (1, 4)):
        st, pic, first = None, None, 0
        for last in cuts + (5,):
            pic, st = run(ctx, d_f[first:last], mats[first:last], label, 5, g[first:last], state=st, first_label=first, ws_frames=1)
            first = last
        assert np.array_equal(pic, ref) and np.array_equal(st, state), cuts
    st = None
    for k in (3, 0, 4, 2, 1):
        pic, st = run(ctx, d_f[k:k + 1], mats[k:k + 1], label, 5, g[k:k + 1], state=st, first_label=k)
    assert np.array_equal(pic, ref) and np.array_equal(st, state)
    # no frames: the picture of the incoming state, the state handed back as it came
    import torch
    none = torch.zeros((0, SH, SW, 3), dtype=torch.uint8, device="cuda")
    pic, st = run(ctx, none, np.zeros((0, 9)), label, 5, state=state)
    assert np.array_equal(pic, ref) and np.array_equal(st, state)
    pic, st = run(ctx, none, np.zeros((0, 9)), label, 5)
    assert not pic.any() and not st.any()


def test_ray_form_with_the_planes_tables_is_the_plane_form(ctx):
    """(e)"""
    f = frames_of(21)
    inv = np.stack([np.linalg.inv(m) if np.isfinite(m).all() else m for m in matrices("a")])
    cols, rows = SC.plane_tables(DW, DH, ORIGIN)
    assert all((SC.ray_frame(f[k], inv[k], cols, rows)[2] > 0).all() for k in range(4))
    label = N.labels_plane(inv, SW, SH, DW, DH, ORIGIN, 40, inverse_map=True)[1]
    a = run(ctx, dev(f), inv, label, 4, GAINS["mixed"], inverse_map=True)
    b = run(ctx, dev(f), inv, label, 4, GAINS["mixed"], ray=(cols, rows))
    ref = N.bands_plane(f, inv, DW, DH, ORIGIN, label, 4, inverse_map=True, gains=GAINS["mixed"])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[0], ref[0]) and np.array_equal(a[1], ref[1])


def test_planes_equal_the_bgr_entry_on_the_converted_frames(ctx):
    """(e): I420, NV12 and packed planes of 38 x 24, on the plane and on a cylinder (where the antipode is invalid: tw <= 0)"""
    import torch
    rng = np.random.default_rng(24)
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
    cams[1:, 2] += [3.0, -4.5, 7.25, 1.0]
    for ray, m in ((None, mats), (cyl, cams)):
        label = (N.labels_plane(m, w, h, DW, DH, ORIGIN, 40) if ray is None else N.labels_ray(m, ray[0], ray[1], w, h, 40))[1]
        ref = (N.bands_plane(bgr, m, DW, DH, ORIGIN, label, 3, gains=GAINS["mixed"]) if ray is None
               else N.bands_ray(bgr, m, ray[0], ray[1], label, 3, gains=GAINS["mixed"]))
        assert (ref[0] != 0).any()
        via_bgr = run(ctx, conv, m, label, 3, GAINS["mixed"], ray=ray)
        assert np.array_equal(via_bgr[0], ref[0]) and np.array_equal(via_bgr[1], ref[1])
        for name, src, size in (("i420", (y, cb, cr), None), ("nv12", (y, uv[..., 0], uv[..., 1]), None), ("packed", packed, (w, h))):
            got = run(ctx, src, m, label, 3, GAINS["mixed"], ray=ray, size=size, cn=3, ws_frames=2)
            assert np.array_equal(got[0], via_bgr[0]) and np.array_equal(got[1], via_bgr[1]), name


# ---- a handed-in state at the stated bounds ---------------------------------------------------------------------------------------------
def crafted_state(cn, levels):
    """Every state pixel another (A per channel, D) inside the header's bounds for a handed-in state, 0 <= D < 2^25 and
    |A| <= 2^26 D: for a range of D the A one step to either side of the rounding thresholds of the quotients 0, +-1, +-4095,
    +-(2^26 - 1), and the largest values allowed; D = 0 takes the background whatever A holds."""
    groups = []
    for D in (1, 2, 3, 255, 65536, 65537, (1 << 24) + 7, (1 << 25) - 1):
        top = (1 << 26) * D
        As = [0, top, -top]
        for q in (0, 1, -1, 4095, -4095, (1 << 26) - 1, 1 - (1 << 26)):
            edge = (2 * q * D - D + 1) // 2                  # the smallest A with floor((2 A + D) / (2 D)) == q
            As += [min(max(edge + e, -top), top) for e in (-1, 0, 1)]
        groups.append((D, As))
    groups.append((0, [0, 12345, -(1 << 40)]))
    total = N.state_elems(DW, DH, cn, levels) // (cn + 1)
    st = np.zeros((total, cn + 1), np.int64)
    for k in range(total):
        D, As = groups[k % len(groups)]
        for c in range(cn):
            st[k, c] = As[(k // len(groups) + 5 * c) % len(As)]
        st[k, cn] = D
    return st.reshape(-1)


@pytest.mark.parametrize("gray", [False, True])
def test_handed_in_state(ctx, gray):
    import torch
    cn, levels = (1 if gray else 3), 3
    st = crafted_state(cn, levels)
    bg = frames_of(25, 1, gray, DW, DH)[0]
    ref = picture_of(st, levels, cn, bg)
    assert {0, 255} <= set(ref.reshape(-1).tolist()) and len(set(ref.reshape(-1).tolist())) > 16
    none = torch.zeros((0, SH, SW) + (() if gray else (3,)), dtype=torch.uint8, device="cuda")
    label = seam_labels()[1]
    pic, back = run(ctx, none, np.zeros((0, 9)), label, levels, state=st, background=bg)
    print("cn=%d: differing bytes %d" % (cn, (pic != ref).sum()))
    assert np.array_equal(pic, ref) and np.array_equal(back, st)
    # and frames on top of a state of half that size: the sums stay inside the bounds
    half = st >> 1
    f, mats = frames_of(21, gray=gray), matrices("a")
    more = N.bands_plane(f, mats, DW, DH, ORIGIN, label, levels, gains=GAINS["mixed"], state=half, background=bg)
    pic, back = run(ctx, dev(f), mats, label, levels, GAINS["mixed"], state=half, background=bg, ws_frames=2)
    assert np.array_equal(pic, more[0]) and np.array_equal(back, more[1])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_label_refusals_leave_the_outputs_alone(ctx):
    import torch
    n, dw, dh = 2, 31, 22
    pc, pr = SC.plane_tables(dw, dh)
    mats, cols, rows = dev(np.tile(np.eye(3).reshape(1, 9), (n, 1))), dev(pc), dev(pr)
    best = torch.full((dh * dw + 2,), 0x31313131, dtype=torch.int32, device="cuda")
    label = torch.from_numpy(np.full(dh * dw + 2, 0x3131, np.uint16)).cuda()
    good = dict(ctx=ctx.h, n=n, sw=SW, sh=SH, M=mats.data_ptr(), inv=1, col=cols.data_ptr(), row=rows.data_ptr(), F=40, dw=dw, dh=dh,
                ox=0, oy=0, first=0, best=best.data_ptr() + 4, label=label.data_ptr() + 2, state_in=0)

    def plane(**kw):
        a = dict(good, **kw)
        return ctx.lib.evh_seam_labels_fixed_plane(a["ctx"], a["n"], a["sw"], a["sh"], a["M"], a["inv"], a["F"], a["dw"], a["dh"], a["ox"],
                                                   a["oy"], a["first"], a["best"], a["label"], a["state_in"])

    def ray(**kw):
        a = dict(good, **kw)
        return ctx.lib.evh_seam_labels_ray_surface(a["ctx"], a["n"], a["sw"], a["sh"], a["M"], a["col"], a["row"], a["F"], a["dw"], a["dh"],
                                                   a["first"], a["best"], a["label"], a["state_in"])

    invalid = [dict(M=None), dict(best=None), dict(label=None), dict(best=best.data_ptr() + 2), dict(label=label.data_ptr() + 1),
               dict(n=-1), dict(sw=0), dict(sh=0), dict(dw=0), dict(dh=-1), dict(F=-1), dict(F=65536), dict(first=-1), dict(first=65534),
               dict(first=65535, n=0), dict(best=label.data_ptr()), dict(label=best.data_ptr()), dict(best=mats.data_ptr()),
               dict(label=mats.data_ptr())]
    for call in (plane, ray):
        assert call(ctx=None) == INVALID
        for kw in invalid:
            assert call(**kw) == INVALID, (call.__name__, kw)
            assert ctx.lib.evh_last_error_string(ctx.h).decode().startswith("evh_seam_labels_"), kw
        big = 1 << 26
        for kw in (dict(sw=big), dict(sh=big), dict(dw=65536, dh=32768), dict(n=65536)):
            assert call(**kw) == CAPACITY, (call.__name__, kw)
    for kw in (dict(col=None), dict(row=None), dict(best=cols.data_ptr()), dict(label=rows.data_ptr())):
        assert ray(**kw) == INVALID, kw
    ctx.synchronize()
    assert (best.cpu().numpy() == 0x31313131).all() and (label.cpu().numpy() == 0x3131).all()
    assert plane(first=65533) == 0 and ray(n=0, first=65534) == 0
    ctx.synchronize()
    assert best.cpu().numpy()[[0, -1]].tolist() == [0x31313131] * 2 and label.cpu().numpy()[[0, -1]].tolist() == [0x3131] * 2


def test_blend_refusals_leave_the_outputs_alone(ctx):
    import ctypes
    import torch
    from evenvizion_amd._lib import Yuv420, bands_frame_ws_bytes, bands_state_elems
    n, dw, dh, levels = 2, 31, 22, 3
    src = dev(frames_of(29, n))
    pc, pr = SC.plane_tables(dw, dh)
    mats, cols, rows = dev(np.tile(np.eye(3).reshape(1, 9), (n, 1))), dev(pc), dev(pr)
    gain = dev(np.full((n, 3), 4096, np.uint16))
    label = dev(np.zeros((dh, dw), np.uint16))
    elems, unit = bands_state_elems(dw, dh, 3, levels), bands_frame_ws_bytes(dw, dh, 3, levels)
    out = torch.full((dh + 2, dw, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    state = torch.full((elems + 2,), WORD, dtype=torch.int64, device="cuda")
    ws = torch.full((8 * elems + 2 * unit,), SENTINEL, dtype=torch.uint8, device="cuda")
    elsewhere = torch.full((dh, dw, 3), 7, dtype=torch.uint8, device="cuda")
    ors = dw * 3
    o, s = out.data_ptr() + ors, state.data_ptr() + 8
    good = dict(ctx=ctx.h, frames=src.data_ptr(), n=n, sw=SW, sh=SH, cn=3, rs=SW * 3, fs=SW * SH * 3, M=mats.data_ptr(), inv=1,
                col=cols.data_ptr(), row=rows.data_ptr(), levels=levels, label=label.data_ptr(), first=0, gain=gain.data_ptr(), state=s,
                state_in=0, ws=ws.data_ptr(), ws_bytes=2 * unit, bg=elsewhere.data_ptr(), out=o, dw=dw, dh=dh, ors=ors, ox=0, oy=0)

    def plane(**kw):
        a = dict(good, **kw)
        return ctx.lib.evh_blend_bands_fixed_plane(a["ctx"], a["frames"], a["n"], a["sw"], a["sh"], a["cn"], a["rs"], a["fs"], a["M"],
                                                   a["inv"], a["levels"], a["label"], a["first"], a["gain"], a["state"], a["state_in"],
                                                   a["ws"], a["ws_bytes"], a["bg"], a["out"], a["dw"], a["dh"], a["ors"], a["ox"], a["oy"])

    def ray(**kw):
        a = dict(good, **kw)
        return ctx.lib.evh_blend_bands_ray_surface(a["ctx"], a["frames"], a["n"], a["sw"], a["sh"], a["cn"], a["rs"], a["fs"], a["M"],
                                                   a["col"], a["row"], a["levels"], a["label"], a["first"], a["gain"], a["state"],
                                                   a["state_in"], a["ws"], a["ws_bytes"], a["bg"], a["out"], a["dw"], a["dh"], a["ors"])

    invalid = [dict(frames=None), dict(M=None), dict(cn=2), dict(cn=0), dict(sw=0), dict(sh=0), dict(dw=0), dict(dh=-1), dict(n=-1),
               dict(rs=SW * 3 - 1), dict(fs=SW * SH * 3 - 1), dict(ors=ors - 1),
               dict(levels=-1), dict(levels=9), dict(label=None), dict(label=label.data_ptr() + 1), dict(first=-1), dict(first=65534),
               dict(first=65535, n=0), dict(out=None, state=None), dict(state=None, state_in=1), dict(state=s + 4), dict(state=s + 1),
               dict(ws=None), dict(ws=ws.data_ptr() + 4), dict(ws_bytes=unit - 1), dict(ws_bytes=0), dict(ws_bytes=-8),
               dict(state=None, ws_bytes=8 * elems + unit - 1),                           # the state lives in the workspace
               dict(bg=o + 3), dict(bg=o + ors), dict(bg=o - ors),                              # only bg == out may overlap
               dict(state=src.data_ptr()), dict(state=gain.data_ptr()), dict(state=mats.data_ptr()), dict(state=elsewhere.data_ptr()),
               dict(state=label.data_ptr()), dict(out=label.data_ptr()), dict(out=src.data_ptr()), dict(out=gain.data_ptr() - dh * ors + 1),
               dict(ws=s), dict(ws=o - ors), dict(ws=src.data_ptr()), dict(ws=label.data_ptr()), dict(ws=mats.data_ptr()),
               dict(ws=gain.data_ptr()), dict(ws=elsewhere.data_ptr())]
    for call in (plane, ray):
        assert call(ctx=None) == INVALID
        for kw in invalid:
            assert call(**kw) == INVALID, (call.__name__, kw)
            assert ctx.lib.evh_last_error_string(ctx.h).decode().startswith("evh_blend_bands_"), kw
        big = 1 << 26
        for kw in (dict(sw=big, rs=big * 3, fs=big * 3 * SH), dict(sh=big, fs=SW * 3 * big),
                   dict(dw=65536, dh=32768, ors=65536 * 3, out=None), dict(n=65536)):
            assert call(**kw) == CAPACITY, (call.__name__, kw)
    for kw in (dict(col=None), dict(row=None), dict(state=cols.data_ptr()), dict(ws=rows.data_ptr())):
        assert ray(**kw) == INVALID, kw
    for bad in (None, ctypes.byref(Yuv420(0, src.data_ptr(), src.data_ptr(), SW, (SW + 1) // 2, SW * SH, SW * SH, 1))):
        assert ctx.lib.evh_blend_bands_fixed_plane_yuv420(ctx.h, bad, n, SW, SH, mats.data_ptr(), 1, levels, label.data_ptr(), 0, None, s, 0,
                                                          ws.data_ptr(), 2 * unit, None, o, dw, dh, ors, 0, 0) == INVALID
        assert ctx.lib.evh_blend_bands_ray_surface_yuv420(ctx.h, bad, n, SW, SH, mats.data_ptr(), cols.data_ptr(), rows.data_ptr(), levels,
                                                          label.data_ptr(), 0, None, s, 0, ws.data_ptr(), 2 * unit, None, o, dw, dh,
                                                          ors) == INVALID
    ctx.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all() and (state.cpu().numpy() == WORD).all() and (ws.cpu().numpy() == SENTINEL).all()
    assert (elsewhere.cpu().numpy() == 7).all()
    # what is allowed: bg == out, each output alone, the largest label
    assert plane(bg=o) == 0 and plane(out=None, bg=o) == 0 and ray(state=None, ws_bytes=8 * elems + unit, bg=None, gain=None) == 0
    assert plane(first=65533) == 0
    ctx.synchronize()
    got = out.cpu().numpy()
    assert (got[0] == SENTINEL).all() and (got[-1] == SENTINEL).all() and (got[1:-1] != SENTINEL).any()
    assert state.cpu().numpy()[[0, -1]].tolist() == [WORD] * 2


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------
def test_blended_mosaic_in_bands(ctx):
    """blend="bands" through the chunk loop on the reference's video: bands=0 is "seam" byte for byte, the chunk size does not
    matter, the levels act, and seam_labels is the restatement's partition under the driver's own matrices."""
    import os
    from evenvizion_amd import blend as B, capture
    from evenvizion_amd.processing.utils import read_homography_dict, superposition_dict
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    hd, info = read_homography_dict(os.path.join(golden, "ref_dict_with_homography_matrix.json"))
    keep = sorted(k for k in hd if k != "resize_info")[:12]
    sup = superposition_dict({k: hd[k] for k in keep})

    class Head:
        """the first 13 frames of the video"""
        def __init__(self):
            self.cap, self.left = capture.VideoCapture(os.path.join(golden, "ref_test_video.mp4")), 13
            assert self.cap.isOpened()

        def __getattr__(self, name):
            return getattr(self.cap, name)

        def read(self, *a, **kw):
            if self.left <= 0:
                return False, None
            self.left -= 1
            return self.cap.read(*a, **kw)

    kw = dict(feather_px=32, placement="translate", ingest="bgr")
    seam = B.blended_mosaic(Head(), sup, info, blend="seam", **kw)
    none = B.blended_mosaic(Head(), sup, info, blend="bands", bands=0, chunk_frames=5, **kw)
    assert np.array_equal(none, seam) and seam.any()
    a = B.blended_mosaic(Head(), sup, info, blend="bands", bands=4, chunk_frames=5, **kw)
    b = B.blended_mosaic(Head(), sup, info, blend="bands", bands=4, chunk_frames=32, **kw)
    assert np.array_equal(a, b) and not np.array_equal(a, seam)
    label = B.seam_labels(sup, info, (int(info["w"]), int(info["h"])), feather_px=32, placement="translate")
    assert label.shape == seam.shape[:2] and label.dtype == np.uint16 and len(np.unique(label)) > 2
    from evenvizion_amd import stabilization as S
    w, h = int(info["w"]), int(info["h"])
    ox, oy, dw, dh, matrix_of = S._placement(sup, info, "translate", 1.0, w, h, S.MAX_PIXELS)
    ref = N.labels_plane(np.stack([matrix_of(k + 1) for k in range(13)]), w, h, dw, dh, (ox, oy), 32 * 32)[1]
    assert np.array_equal(label, ref)
    # the picture is written exactly where a frame owns the pixel (D0 > 0); the fixture's video has no black pixel there
    assert np.array_equal(a.any(axis=2), label != N.NOBODY) and np.array_equal(seam.any(axis=2), label != N.NOBODY)
