"""K0 after the INTER_AREA fold: the stand-alone resize and the fused ingest share their float-table and enlarging
kernels (k_area, k_resize_linear_area: one thread per output pixel), their dispatch (launch_area) and the context's cached
tables; the integer-ratio form keeps a kernel per caller.  What
that makes possible to get wrong: the packed store with strides that are not the tight ones, for every form of the
dispatch, and the cache when resize and ingest alternate on one context.  Bit-exact against the oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from evenvizion_amd import synthetic as S  # noqa: E402
from oracle import oracle as O  # noqa: E402

# (sw, sh, dw, dh): 257 columns put one pixel into a second workgroup
GEOMETRIES = [(600, 40, 257, 17), (514, 34, 257, 17), (771, 51, 257, 17), (100, 30, 257, 77), (257, 17, 257, 17)]
FORMS = ["tables", "int 2x2", "int 3x3", "enlarge", "copy"]
NIMG, SENTINEL = 3, 0xA5


def form(sw, sh, dw, dh):
    """the launcher's own classification (evh_launch_resize_area / launch_area)"""
    if (dw, dh) == (sw, sh):
        return "copy"
    sx, sy = 1. / (dw / sw), 1. / (dh / sh)
    if sx < 1 or sy < 1:
        return "enlarge"
    ix, iy = int(round(sx)), int(round(sy))
    if abs(sx - ix) < 2.220446049250313e-16 and abs(sy - iy) < 2.220446049250313e-16:
        return "int %dx%d" % (ix, iy)
    return "tables"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def new_context(**kw):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU; there is no CPU fallback")
    from evenvizion_amd._lib import Context
    return Context(device=0, **kw)


@pytest.fixture(scope="module")
def ctx():
    c = new_context(max_w=640, max_h=360, max_features=500, max_frames=2)
    yield c
    c.close()


def test_the_five_geometries_are_the_five_forms():
    assert [form(*g) for g in GEOMETRIES] == FORMS


def images_in(flat, n, h, row_bytes, stride, img_stride):
    """the n images of h rows x row_bytes inside a flat byte buffer, as a view"""
    return np.lib.stride_tricks.as_strided(flat, (n, h, row_bytes), (img_stride, stride, 1))


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=FORMS)
def test_strided_resize(ctx, geometry, cn):
    """nimg = 3 through the C entry with padded row and image strides on both sides: every image equals the oracle's, and
    the destination's padding keeps its sentinel."""
    sw, sh, dw, dh = geometry
    rng = np.random.default_rng(sw * 7 + cn)
    s_stride, d_stride = sw * cn + 5, dw * cn + 7
    s_img, d_img = sh * s_stride + 11, dh * d_stride + 13
    src = rng.integers(0, 256, NIMG * s_img, dtype=np.uint8)          # the padding is noise as well: it must not be read into the result
    want = np.full(NIMG * d_img, SENTINEL, np.uint8)
    S_, W_ = images_in(src, NIMG, sh, sw * cn, s_stride, s_img), images_in(want, NIMG, dh, dw * cn, d_stride, d_img)
    for i in range(NIMG):
        img = S_[i].reshape(sh, sw, cn) if cn == 3 else S_[i]
        W_[i] = O.resize_area(np.ascontiguousarray(img), dw, dh).reshape(dh, dw * cn)
    d_src, d_dst = dev(src), torch.full((NIMG * d_img,), SENTINEL, dtype=torch.uint8, device="cuda")
    ctx.order_after_torch()
    rc = ctx.lib.evh_resize_area_u8(ctx.h, d_src.data_ptr(), NIMG, sw, sh, cn, s_stride, s_img, d_dst.data_ptr(), dw, dh,
                                    d_stride, d_img)
    assert rc == 0
    ctx.synchronize()
    got = d_dst.cpu().numpy()
    G_ = images_in(got, NIMG, dh, dw * cn, d_stride, d_img)
    for i in range(NIMG):
        assert np.array_equal(G_[i], W_[i]), "image %d" % i
    assert np.array_equal(got, want), "padding overwritten"


def test_resize_and_ingest_share_the_table_cache():
    """One context, two table geometries in turn: resize 600x40 -> 257x17, fused ingest 1170x658 -> 400x224, and both
    again.  Each call rebuilds the tables the other one replaced; nothing may be served from the wrong geometry.  Then
    the resize once more with other pixels: a call that finds its tables cached."""
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (1, 40, 600, 3), dtype=np.uint8)
    want_small = O.resize_area(img[0], 257, 17)
    g, _ = S.make_stream(41, 2, 1170, 658)
    full = np.stack([g, np.roll(g, 7, axis=2), 255 - g], axis=-1)     # three different channels, so that the gray weights matter
    want_level0 = [O.bgr2gray(O.resize_area(f, 400, 224)) for f in full]
    c = new_context(max_w=400, max_h=224, max_features=500, max_frames=2)
    try:
        d_img, d_full = dev(img), dev(full)
        for turn in range(2):
            out = torch.zeros((1, 17, 257, 3), dtype=torch.uint8, device="cuda")
            c.resize_area(d_img, out)
            c.synchronize()
            assert np.array_equal(out.cpu().numpy()[0], want_small), "resize, turn %d" % turn
            c.orb_detect_batch(d_full, resize_to=(400, 224))
            c.synchronize()
            for f in range(2):
                assert np.array_equal(c.download_level(f, 0), want_level0[f]), "level 0 of frame %d, turn %d" % (f, turn)
        for im in (img, 255 - img):
            out = torch.zeros((1, 17, 257, 3), dtype=torch.uint8, device="cuda")
            c.resize_area(dev(im), out)
            c.synchronize()
            assert np.array_equal(out.cpu().numpy()[0], O.resize_area(im[0], 257, 17))
    finally:
        c.close()
