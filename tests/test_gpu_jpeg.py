"""evh_jpeg_encode against its numpy restatement (jpeg_checks.encode), for EQUALITY of every file's bytes and length.  Every call
goes through check(): the outputs start as 0xFF, and no byte past a file's end, past out_cap or between the slots changes."""
import ctypes as C

import numpy as np
import pytest

import jpeg_checks as J
from refusal_arena import Arena

pytestmark = pytest.mark.gpu
ONES = np.ones((2, 64), np.uint16)
LAYOUTS = [(1, "444"), (3, "444"), (3, "420")]


@pytest.fixture(scope="module")
def ctx():
    from evenvizion_amd import runtime
    return runtime.get_context(64, 64)


def noise(seed, n, h, w, cn):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w) if cn == 1 else (n, h, w, 3), dtype=np.uint8)


def raw_call(ctx, view, qt, sub, out, stride, cap, sizes):
    """evh_jpeg_encode on a tensor view [n,h,w(,3)] -> its return code"""
    import torch
    cn = 1 if view.dim() == 3 else 3
    n, h, w = view.shape[:3]
    q = np.ascontiguousarray(qt, np.uint16)
    spare = torch.zeros(16, dtype=torch.uint8, device="cuda")           # an empty view has no address; n == 0 reads nothing
    ctx._enter()
    rc = ctx.lib.evh_jpeg_encode(ctx.h, view.data_ptr() or spare.data_ptr(), n, w, h, view.stride(1) if h > 1 else w * cn, view.stride(0) if n > 1 else 0, cn,
                                 J.SUBSAMPLINGS[sub], q.ctypes.data_as(C.c_void_p), out.data_ptr(), stride, cap, sizes.data_ptr())
    ctx.synchronize()
    return rc


def check(ctx, view, qt, sub, cap=None, want=None):
    """One call on a device view; cap None: the largest file's length.  -> the files the restatement gives."""
    import torch
    pics = view.cpu().numpy()
    n = pics.shape[0]
    want = [J.encode(p, qt, sub) for p in pics] if want is None else want
    cap = max([len(f) for f in want] + [0]) if cap is None else cap
    stride = cap + 5
    out = torch.full((max(n, 1) * stride + 7,), 0xFF, dtype=torch.uint8, device="cuda")
    sizes = torch.full((max(n, 1) + 1,), -1, dtype=torch.int64, device="cuda")
    assert raw_call(ctx, view, qt, sub, out, stride, cap, sizes) == 0
    got, lengths = out.cpu().numpy(), sizes.cpu().numpy()
    assert lengths[n:].tolist() == [-1] * (len(lengths) - n)
    assert lengths[:n].tolist() == [len(f) for f in want]
    for p in range(n):
        kept = min(len(want[p]), cap)
        slot = got[p * stride:(p + 1) * stride]
        assert slot[:kept].tobytes() == want[p][:kept], (p, first_difference(slot[:kept].tobytes(), want[p][:kept]))
        assert np.all(slot[kept:] == 0xFF), "bytes past the file or past out_cap changed"
    assert np.all(got[n * stride:] == 0xFF)
    return want


def first_difference(a, b):
    k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return k, a[k:k + 8].hex(), b[k:k + 8].hex()


@pytest.mark.parametrize("cn,sub", LAYOUTS)
@pytest.mark.parametrize("w,h", [(1, 1), (8, 8), (9, 7), (16, 16), (17, 9), (33, 17)])
def test_small_shapes(ctx, w, h, cn, sub):
    import torch
    pics = noise(w * 100 + h, 2, h, w, cn)
    check(ctx, torch.from_numpy(pics).cuda(), ONES, sub)                      # the longest codes, many 0xFF bytes
    check(ctx, torch.from_numpy(pics).cuda(), J.quant_tables(50), sub)
    check(ctx, torch.from_numpy(pics).cuda(), J.quant_tables(90), sub)


@pytest.mark.parametrize("w,h,cn,sub", [(8, 80, 1, "444"), (16, 160, 3, "420")])
def test_ten_rows_wrap_the_restart_counter(ctx, w, h, cn, sub):
    import torch
    files = check(ctx, torch.from_numpy(noise(5, 1, h, w, cn)).cuda(), J.quant_tables(50), sub)
    assert J.parse(files[0])["rst"] == [0, 1, 2, 3, 4, 5, 6, 7, 0]


@pytest.mark.parametrize("w,h,cn,sub", [(2064, 8, 1, "444"), (4112, 16, 3, "420")])
def test_a_row_longer_than_a_workgroup(ctx, w, h, cn, sub):
    import torch
    pics = noise(6, 1, h, w, cn)
    check(ctx, torch.from_numpy(pics).cuda(), ONES, sub)                      # 258 and 257 MCUs: the scan and the packing cross waves
    check(ctx, torch.from_numpy(pics).cuda(), J.quant_tables(90), sub)


def test_the_widest_row(ctx):
    import torch
    check(ctx, torch.from_numpy(noise(7, 1, 1, 65535, 1)).cuda(), J.quant_tables(50), "444")


@pytest.mark.parametrize("cn,sub", LAYOUTS)
def test_flat_and_striped_pictures(ctx, cn, sub):
    import torch
    h, w = 24, 40
    shape = (h, w) if cn == 1 else (h, w, 3)
    pics = [np.full(shape, v, np.uint8) for v in (0, 128, 255)]               # EOB only: one pattern repeated across the word seams
    vertical, horizontal = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    vertical[:, ::2] = 255
    horizontal[::2] = 255
    if cn == 3:
        vertical[:, 1::4, 0] = 90
        horizontal[1::4, :, 2] = 200
    check(ctx, torch.from_numpy(np.stack(pics + [vertical, horizontal])).cuda(), J.quant_tables(90), sub)
    check(ctx, torch.from_numpy(np.stack(pics + [vertical, horizontal])).cuda(), ONES, sub)


@pytest.mark.parametrize("cn,sub", LAYOUTS)
def test_counts_and_strides(ctx, cn, sub):
    import torch
    h, w, qt = 19, 21, J.quant_tables(75)
    for n in (0, 1, 3):
        check(ctx, torch.from_numpy(noise(n, max(n, 1), h, w, cn)).cuda()[:n], qt, sub)
    # rows wider than the pictures', picture bases at odd addresses
    pics = noise(11, 3, h, w, cn)
    row, pic = w * cn + 5, (w * cn + 5) * h + 3
    flat = torch.zeros(1 + 3 * pic, dtype=torch.uint8, device="cuda")
    view = flat[1:].as_strided((3, h, w) if cn == 1 else (3, h, w, 3), (pic, row, 1) if cn == 1 else (pic, row, 3, 1))
    view.copy_(torch.from_numpy(pics))
    assert view.data_ptr() % 2 == 1 and (view.data_ptr() + pic) % 2 == 0
    want = check(ctx, view, qt, sub)
    # a picture alone is the picture among neighbours, and the same call twice gives the same bytes
    assert check(ctx, view[1:2], qt, sub) == want[1:2]
    assert check(ctx, view, qt, sub) == want


def test_a_view_cut_out_of_a_larger_canvas(ctx):
    import torch
    canvas = torch.from_numpy(noise(12, 2, 60, 70, 3)).cuda()
    view = canvas[:, 7:40, 9:60]
    assert not view.is_contiguous()
    want = check(ctx, view, J.quant_tables(90), "420")
    assert ctx.jpeg_encode(view, J.quant_tables(90), "420") == want
    # a channel of a BGR view has a pixel stride of 3: not packed pixels
    with pytest.raises(ValueError):
        ctx.jpeg_encode(view[:, :, :, 1], J.quant_tables(90))


def test_the_wrapper_repeats_a_call_that_was_too_small(ctx):
    import torch
    pics = noise(13, 2, 64, 64, 3)                     # noise under all-ones tables: far more than a quarter of the raw size
    want = [J.encode(p, ONES, "444") for p in pics]
    assert min(len(f) for f in want) > 64 * 64 * 3 // 4
    assert ctx.jpeg_encode(torch.from_numpy(pics).cuda(), ONES, "444") == want


@pytest.mark.parametrize("cn,sub", LAYOUTS)
def test_caps(ctx, cn, sub):
    import torch
    qt = J.quant_tables(75)
    pics = noise(14, 3, 17, 23, cn)
    view = torch.from_numpy(pics).cuda()
    want = [J.encode(p, qt, sub) for p in pics]
    head = len(J.header(23, 17, cn, J.SUBSAMPLINGS[sub], qt))
    for cap in (len(want[1]), len(want[1]) - 1, head, head - 1, 1, 0):
        check(ctx, view, qt, sub, cap=cap, want=want)


def test_refusals_leave_the_outputs_untouched(ctx):
    import torch
    A = Arena(4)
    w, h, n = 16, 12, 2
    pics = A.put(noise(15, n, h, w, 3))
    out = A.take((n, 4000), fill=0xFF)
    sizes = A.take((n,), torch.int64, fill=-1)
    qt = np.ascontiguousarray(J.quant_tables(75))

    def call(pics=pics.data_ptr(), n=n, w=w, h=h, row=w * 3, pic=w * h * 3, cn=3, sub=1, q=qt, out=out.data_ptr(), stride=4000, cap=4000,
             sizes=sizes.data_ptr(), handle=None):
        ctx._enter()
        rc = ctx.lib.evh_jpeg_encode(ctx.h if handle is None else handle, pics, n, w, h, row, pic, cn, sub,
                                     None if q is None else q.ctypes.data_as(C.c_void_p), out, stride, cap, sizes)
        ctx.synchronize()
        return rc
    bad_low, bad_high = qt.copy(), qt.copy()
    bad_low[0, 5], bad_high[1, 63] = 0, 256
    refused = [dict(w=0), dict(w=65536), dict(h=0), dict(h=65536), dict(cn=2), dict(cn=4), dict(sub=2), dict(sub=-1), dict(cn=1, sub=1),
               dict(q=bad_low), dict(q=bad_high), dict(pics=None), dict(q=None), dict(out=None), dict(sizes=None), dict(n=-1),
               dict(row=w * 3 - 1), dict(stride=3999), dict(cap=-1)]
    for kw in refused:
        assert call(**kw) == -1, kw
        assert ctx.lib.evh_last_error_string(ctx.h).decode().startswith("evh_jpeg_encode: "), kw
        assert bool((out == 0xFF).all()) and bool((sizes == -1).all()), kw
    assert ctx.lib.evh_jpeg_encode(None, pics.data_ptr(), n, w, h, w * 3, w * h * 3, 3, 1, qt.ctypes.data_as(C.c_void_p), out.data_ptr(), 4000,
                                   4000, sizes.data_ptr()) == -1
    assert call(n=0) == 0 and bool((out == 0xFF).all()) and bool((sizes == -1).all())
    assert call() == 0
    host = out.cpu().numpy()
    for p in range(n):
        want = J.encode(pics[p].cpu().numpy(), qt, "420")
        assert int(sizes[p]) == len(want) and host[p, :len(want)].tobytes() == want
