"""GPU: the image front end -- the four resize kernels of evh_image.hip, the gray and pyramid kernels of evh_detect_pyr.h, their
host tables and launch conditions -- on the crafted families of tests/front_families.py.  Every comparison is bit for bit and is
made twice: against the oracle, and against the plain restatement (tests/front_checks.py) without the oracle.  That the
families reach what they are there for is asserted on the CPU in tests/test_oracle_front_edges.py.

  resize entry   T (ties), A (table shapes), E (enlarging and mixed) through evh_resize_area_u8; one case per form with padded
                 strides, a sentinel in the destination's padding and three images
  fused ingest   the same geometries through orb_detect_batch(resize_to=): level 0 is gray of the restated resize, level 1 the
                 restated pyramid of that; one geometry per form from 4:2:0 planes
  pyramid        P (hard content), S (tile seams), X (extremes): all eight levels of every frame, each batch preceded on the same
                 context and geometry by the batch of complement frames, so that a byte no kernel wrote differs
  stride guard   a row stride on either side of 2^24, which turns the fused level-1 kernel off
  alternation    two ingest geometries and a stand-alone resize in turn on one context, nothing synchronised in between"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import front_checks as C  # noqa: E402
import front_families as F  # noqa: E402
from evenvizion_amd import synthetic  # noqa: E402
from oracle import oracle as O  # noqa: E402

SENTINEL = 0xA5


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_at(a, offset):
    """the array on the device with its first byte `offset` bytes past an allocation's start (allocations are 256-byte aligned)"""
    a = np.ascontiguousarray(a)
    flat = torch.zeros(a.size + offset, dtype=torch.uint8, device="cuda")
    flat[offset:] = torch.from_numpy(a.reshape(-1)).cuda()
    t = flat[offset:].view(a.shape)
    assert t.data_ptr() % 4 == offset % 4
    return t


def new_context(**kw):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU; there is no CPU fallback")
    from evenvizion_amd._lib import Context
    return Context(device=0, **kw)


@pytest.fixture(scope="module")
def ctx():
    """every frame of up to 1440 x 768 runs here at its own size, nine frames a call at the most"""
    c = new_context(max_w=1440, max_h=768, max_features=500, max_frames=9)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _reference_order_afterwards():
    yield
    O.set_orb_order(1)


def gray_of(frames):
    return frames if frames.ndim == 3 else np.stack([C.gray(f) for f in frames])


# -------------------------------------------------------------------------------------------------------- resize entry
def _resize_specs():
    """{name: (builder, arguments, dw, dh)} of families T, A and E; the images are built when a test asks for them"""
    out = {}
    for name, isx, isy, cn in F.t_cases():
        out[name] = (F.t_image, (isx, isy, cn)) + F.t_geometry(isx, isy, cn)[2:]
    for name, (sw, sh, dw, dh), cn, kind in F.resize_cases():
        out[name] = (F.content, (kind, sw, sh, dw, dh, cn), dw, dh)
    return out


RESIZE_SPECS = _resize_specs()


def _resize_input(name):
    build, args, dw, dh = RESIZE_SPECS[name]
    return build(*args), dw, dh


@pytest.mark.parametrize("name", sorted(RESIZE_SPECS))
def test_resize_entry(ctx, name):
    """the image and its complement (a tie stays a tie: the block sum s becomes 255 * area - s) as one call of two images"""
    img, dw, dh = _resize_input(name)
    src = np.stack([img, 255 - img])
    out = torch.full((2, dh, dw) + img.shape[2:], SENTINEL, dtype=torch.uint8, device="cuda")
    ctx.resize_area(dev(src), out)
    ctx.synchronize()
    got = out.cpu().numpy()
    for i in range(2):
        assert np.array_equal(got[i], O.resize_area(src[i], dw, dh)), "image %d against the oracle" % i
        assert np.array_equal(got[i], C.resize_area(src[i], dw, dh)), "image %d against the restatement" % i


STRIDED = {"int 4x2": (F.t_image, (4, 2, 3), 86, 5), "int 2x2": (F.t_image, (2, 2, 1), 257, 5),
           "tables": (F.content, ("noise", 258, 9, 257, 6, 3), 257, 6), "enlarge": (F.content, ("noise", 100, 60, 150, 40, 1), 150, 40),
           "copy": (F.content, ("noise", 257, 6, 257, 6, 3), 257, 6)}


@pytest.mark.parametrize("form", sorted(STRIDED))
def test_resize_entry_with_padded_strides(ctx, form):
    """three images with padded row and image strides on both sides; the destination's padding keeps its sentinel"""
    build, args, dw, dh = STRIDED[form]
    img = build(*args)
    assert (form == "copy") == (C.area_form(img.shape[1], img.shape[0], dw, dh) == "copy")
    nimg = 3
    sh, sw = img.shape[:2]
    cn = 1 if img.ndim == 2 else 3
    imgs = [img, 255 - img, np.ascontiguousarray(img[::-1])]
    s_stride, d_stride = sw * cn + 5, dw * cn + 7
    s_img, d_img = sh * s_stride + 11, dh * d_stride + 13
    src = np.random.default_rng(5).integers(0, 256, nimg * s_img, dtype=np.uint8)     # noise in the padding: it must not be read
    want_o, want_c = np.full(nimg * d_img, SENTINEL, np.uint8), np.full(nimg * d_img, SENTINEL, np.uint8)

    def view(flat, h, row, stride, img_stride):
        return np.lib.stride_tricks.as_strided(flat, (nimg, h, row), (img_stride, stride, 1))
    for i in range(nimg):
        view(src, sh, sw * cn, s_stride, s_img)[i] = imgs[i].reshape(sh, sw * cn)
        view(want_o, dh, dw * cn, d_stride, d_img)[i] = O.resize_area(imgs[i], dw, dh).reshape(dh, dw * cn)
        view(want_c, dh, dw * cn, d_stride, d_img)[i] = C.resize_area(imgs[i], dw, dh).reshape(dh, dw * cn)
    d_src, d_dst = dev(src), torch.full((nimg * d_img,), SENTINEL, dtype=torch.uint8, device="cuda")
    ctx.order_after_torch()
    rc = ctx.lib.evh_resize_area_u8(ctx.h, d_src.data_ptr(), nimg, sw, sh, cn, s_stride, s_img, d_dst.data_ptr(), dw, dh,
                                    d_stride, d_img)
    assert rc == 0
    ctx.synchronize()
    got = d_dst.cpu().numpy()
    assert np.array_equal(got, want_o), "against the oracle (padding included)"
    assert np.array_equal(got, want_c), "against the restatement (padding included)"


# -------------------------------------------------------------------------------------------------------- fused ingest
INGEST_NAMES = sorted(n for n, r in RESIZE_SPECS.items() if F.acceptable_orb_frame(r[2], r[3]))


def _check_levels_0_1(c, n, small, what):
    for f in range(n):
        g = small[f] if small[f].ndim == 2 else C.gray(small[f])
        assert np.array_equal(c.download_level(f, 0), g), "%s: level 0 of frame %d against the restatement" % (what, f)
        assert np.array_equal(c.download_level(f, 1), C.orb_pyramid(g)[1]), "%s: level 1 of frame %d" % (what, f)


@pytest.mark.parametrize("name", INGEST_NAMES)
def test_fused_ingest(ctx, name):
    img, dw, dh = _resize_input(name)
    src = np.stack([img, 255 - img])
    ctx.orb_detect_batch(dev(src), resize_to=(dw, dh))
    ctx.synchronize()
    assert ctx.level_info(0)[:2] == (dw, dh)
    for f in range(2):
        o = O.resize_area(src[f], dw, dh)
        assert np.array_equal(ctx.download_level(f, 0), o if o.ndim == 2 else O.bgr2gray(o)), "level 0 against the oracle"
    _check_levels_0_1(ctx, 2, [C.resize_area(s, dw, dh) for s in src], name)


YUV_GEOMETRIES = [("int 2x2", (172, 10, 86, 5)), ("int 2x4", (172, 20, 86, 5)), ("tables", (300, 200, 200, 80)),
                  ("enlarge", (100, 60, 150, 40))]


@pytest.mark.parametrize("form,geo", YUV_GEOMETRIES, ids=[g[0] for g in YUV_GEOMETRIES])
def test_fused_ingest_from_planes(ctx, form, geo):
    """4:2:0 planes through the same kernels: level 0 and 1 are those of the BGR frames the planes convert to"""
    sw, sh, dw, dh = geo
    rng = np.random.default_rng(sw + dw)
    luma = rng.integers(0, 256, (2, sh, sw), dtype=np.uint8)
    planes = [(y,) + tuple(rng.integers(0, 256, ((sh + 1) // 2, (sw + 1) // 2), dtype=np.uint8) for _ in range(2)) for y in luma]
    bgr = [synthetic.yuv420_to_bgr_host(*p) for p in planes]
    packed = np.stack([np.concatenate([a.reshape(-1) for a in p]) for p in planes])
    ctx.orb_detect_batch(dev(255 - np.stack(bgr)), resize_to=(dw, dh))
    ctx.orb_detect_batch_yuv420(dev(packed), size=(sw, sh), resize_to=(dw, dh))
    ctx.synchronize()
    _check_levels_0_1(ctx, 2, [C.resize_area(b, dw, dh) for b in bgr], form)


# -------------------------------------------------------------------------------------------------------------- pyramid
def _pyramids(c, frames, offset=0):
    """the complement batch, then the batch, on the same context and geometry; -> the eight levels of every frame"""
    n, h, w = frames.shape[:3]
    c.orb_detect_batch(dev_at(255 - frames, offset))
    c.synchronize()
    assert c.level_info(0)[:2] == (w, h)
    d = dev_at(frames, offset)
    c.orb_detect_batch(d)
    c.synchronize()
    return [[c.download_level(f, l) for l in range(C.NLEVELS)] for f in range(n)]


def _check_pyramids(got, grays, what):
    for f, g in enumerate(grays):
        want_c, want_o = C.orb_pyramid(g), O.orb_pyramid(g)
        for l in range(C.NLEVELS):
            assert got[f][l].shape == want_c[l].shape, "%s: size of level %d" % (what, l)
            assert np.array_equal(got[f][l], want_o[l]), "%s: frame %d level %d against the oracle" % (what, f, l)
            assert np.array_equal(got[f][l], want_c[l]), "%s: frame %d level %d against the restatement" % (what, f, l)


def _device_kernels(c):
    """which pyramid kernel each level 1 .. 7 takes, from the launcher's own condition on the device's level sizes"""
    dims = [c.level_info(l)[:2] for l in range(C.NLEVELS)]
    return ["walk" if F.walks(dims[l - 1], dims[l]) else "down" for l in range(1, C.NLEVELS)]


P_SETS = {"P": F.p_frames(), "P220": F.p220_frames(), "P120": F.p120_frames()}


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("fam", sorted(P_SETS))
def test_pyramid_content(ctx, fam, cn):
    """hard content, in calls of 2, 3 and 9 frames (a short last call takes the first frames once more)"""
    names = sorted(P_SETS[fam])
    frames = np.stack([P_SETS[fam][n] for n in names])
    start, sizes = 0, [2, 3, 9]
    while start < len(frames):
        n = sizes[0]
        sizes = sizes[1:] + sizes[:1]
        idx = [(start + k) % len(frames) for k in range(n)]
        batch = frames[idx]
        if cn == 3:                                         # three different channels; gray is what the pyramid is built on
            batch = np.stack([batch, np.roll(batch, 3, axis=2), 255 - batch], axis=-1)
        _check_pyramids(_pyramids(ctx, batch), gray_of(batch), "%s %s" % (fam, [names[i] for i in idx]))
        start += n
    assert _device_kernels(ctx) == F.kernel_of_levels(*F.P_SIZES[fam])


S_ALL = list(F.s_frames() + F.s_wide_frames())


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "odd"])
@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("k", range(len(S_ALL)), ids=["%dx%d" % s for s in S_ALL])
def test_seam_sweep(ctx, k, cn, offset):
    """noise at the sizes whose levels 1 and 2 sit around the tile sizes; 2, 3 or 9 frames by the frame's place in the sweep"""
    w, h = S_ALL[k]
    frames = F.noise_frames(w, h, (2, 3, 9)[k % 3], cn, seed=cn)
    _check_pyramids(_pyramids(ctx, frames, offset), gray_of(frames), "%dx%d" % (w, h))
    assert _device_kernels(ctx) == F.kernel_of_levels(w, h)


def _same_orb(g, o, what):
    assert len(g["xy"]) == len(o["xy"]), what
    for k in ("octave", "lx", "ly", "xy", "desc"):
        assert np.array_equal(g[k], o[k]), (what, k)
    for k in ("response", "angle"):
        assert np.array_equal(g[k].view(np.uint32), o[k].view(np.uint32)), (what, k)


def _extreme(c, w, h, cn, offset):
    frames = F.noise_frames(w, h, 2, cn, seed=7)
    grays = gray_of(frames)
    _check_pyramids(_pyramids(c, frames, offset), grays, "%dx%d" % (w, h))
    assert _device_kernels(c) == F.kernel_of_levels(w, h)
    d = dev_at(frames, offset)
    counts = []
    for mode in (0, 1):                                     # canonical and reference key-point order
        c.set_keypoint_order(mode)
        O.set_orb_order(mode)
        try:
            c.orb_detect_batch(d)
            c.synchronize()
            for f in range(2):
                got = c.orb_download(f)
                _same_orb(got, O.orb_detect(grays[f]), "%dx%d frame %d order %d" % (w, h, f, mode))
                counts.append(len(got["xy"]))
        finally:
            c.set_keypoint_order(1)
    return counts


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "odd"])
@pytest.mark.parametrize("w,h,cn", [(4095, 64, 1), (4095, 64, 3), (64, 4095, 1)])
def test_largest_frames(w, h, cn, offset):
    c = new_context(max_w=w, max_h=h, max_features=500, max_frames=2)
    try:
        assert min(_extreme(c, w, h, cn, offset)) > 0
    finally:
        c.close()


@pytest.fixture(scope="module")
def ctx64():
    c = new_context(max_w=64, max_h=64, max_features=500, max_frames=2)
    yield c
    c.close()


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "odd"])
@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("w,h", F.X_SMALL)
def test_smallest_frames(ctx64, w, h, cn, offset):
    """levels down to one pixel, whole levels inside FAST's first tile: every level is right and there is no key point (a key
    point keeps 31 pixels from the border, so a level needs more than 62 on a side)"""
    assert _extreme(ctx64, w, h, cn, offset) == [0, 0, 0, 0]


@pytest.mark.parametrize("w,h", F.X_REFUSED)
def test_a_side_of_one_is_refused(ctx64, w, h):
    """a level without pixels: the entry refuses the frame, says why, launches nothing, and the context goes on working"""
    from evenvizion_amd._lib import _packed
    frames = dev(F.noise_frames(w, h, 2))
    ctx64.order_after_torch()
    rc = ctx64.lib.evh_orb_detect_batch(ctx64.h, *_packed(frames), 500)
    assert rc == -4                                          # EVH_ERR_UNSUPPORTED
    assert "at least 2 pixels" in ctx64.lib.evh_last_error_string(ctx64.h).decode()
    ctx64.synchronize()
    good = F.noise_frames(63, 63, 2)
    _check_pyramids(_pyramids(ctx64, good), good, "63x63 after the refusal")


# --------------------------------------------------------------------------------------------------------- stride guard
@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("row_stride", [(1 << 24) - 4, 1 << 24], ids=["below", "at"])
def test_row_stride_around_the_guard(ctx64, row_stride, cn):
    """64 x 8 frames whose rows lie 2^24 - 4 and 2^24 bytes apart (128 MiB a frame, uninitialised but for the rows): below the
    guard the fused gray + level-1 kernel runs (24-bit multiplies of the stride), at it the unfused pair; the levels are the same"""
    w, h, n = 64, 8, 2
    frames = F.noise_frames(w, h, n, cn, seed=3)
    ctx64.orb_detect_batch(dev(255 - frames))
    ctx64.synchronize()
    buf = torch.empty(n * h * row_stride, dtype=torch.uint8, device="cuda")
    buf.view(n, h, row_stride)[:, :, :w * cn] = dev(frames.reshape(n, h, w * cn))
    ctx64.order_after_torch()
    rc = ctx64.lib.evh_orb_detect_batch(ctx64.h, buf.data_ptr(), n, w, h, cn, row_stride, h * row_stride, 500)
    assert rc == 0, ctx64.lib.evh_last_error_string(ctx64.h).decode()
    ctx64.synchronize()
    got = [[ctx64.download_level(f, l) for l in range(C.NLEVELS)] for f in range(n)]
    del buf
    _check_pyramids(got, gray_of(frames), "row stride %d" % row_stride)


# ---------------------------------------------------------------------------------------------------------- alternation
def test_geometries_alternate_without_a_synchronisation():
    """One context: pairs at 1170 x 658 -> 400 x 224 (tables) and 640 x 360 -> 320 x 180 (integer ratio) in turn, twice, a
    stand-alone resize at a third geometry after each, and no synchronize() until everything is enqueued.  The tap tables
    go through one pinned staging buffer and the area tables cache one geometry: every H, status and resized image must
    be right."""
    from evenvizion_amd._lib import MODE_INDEPENDENT_PAIRS
    geos = [((1170, 658), (400, 224)), ((640, 360), (320, 180))]
    pairs = [synthetic.make_pair_batch(5 + k, 1, *src)[0] for k, (src, _) in enumerate(geos)]
    third = F.content("noise", 300, 200, 200, 80, 3)
    assert [C.area_form(*(s + d)) for s, d in geos] == ["tables", ("int", 2, 2)] and C.area_form(300, 200, 200, 80) == "tables"
    c = new_context(max_w=400, max_h=224, max_features=500, max_frames=2)
    try:
        d_pairs, d_third = [dev(p) for p in pairs], dev(third[None])
        outs = []
        for turn in range(2):
            for k, (_, dst) in enumerate(geos):
                H = torch.zeros(1, 9, dtype=torch.float64, device="cuda")
                st = torch.full((1,), -1, dtype=torch.int32, device="cuda")
                c.pair_homography_batch_types(d_pairs[k], 1, MODE_INDEPENDENT_PAIRS, H, st, ("ORB",), resize_to=dst)
                r = torch.full((1, 80, 200, 3), SENTINEL, dtype=torch.uint8, device="cuda")
                c.resize_area(d_third, r)
                outs.append((k, H, st, r))
        c.synchronize()
        want_r = C.resize_area(third, 200, 80)
        want = []
        for k, (_, (dw, dh)) in enumerate(geos):
            small = np.stack([C.resize_area(f, dw, dh) for f in pairs[k]])
            want.append(O.pairs_gray_batch(small))
        for i, (k, H, st, r) in enumerate(outs):
            assert np.array_equal(st.cpu().numpy(), want[k][1]), "status of call %d" % i
            assert want[k][1][0] == 0
            assert np.array_equal(H.cpu().numpy().reshape(1, 3, 3), want[k][0]), "H of call %d" % i
            assert np.array_equal(r.cpu().numpy()[0], want_r), "resize after call %d" % i
    finally:
        c.close()
