"""evh_mask_components on the device.  Labels, nobjects and tables must EQUAL the plain restatement of the header's contract
(tests/components_checks.py, itself held to hand-written expectations in test_components_host.py).  All outputs sit inside
buffers padded with a sentinel that must survive."""
import json
import os

import numpy as np
import pytest

import components_checks as K
import plate_checks as P
from refusal_arena import Arena

pytestmark = pytest.mark.gpu
SENTINEL = -0x32323233          # 0xCDCDCDCD as an int32: what fills the label buffers
FILL64 = -0x3232323232323233    # the same bytes as an int64: what fills the tables
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MP4 = os.path.join(ROOT, "tests", "golden", "ref_test_video.mp4")
GOLD = os.path.join(ROOT, "tests", "golden", "ref_dict_with_homography_matrix.json")


def tile():
    from evenvizion_amd._lib import COMPONENTS_TILE
    return COMPONENTS_TILE


@pytest.fixture(scope="module")
def ctx():
    from evenvizion_amd._lib import Context
    c = Context(device=0, max_w=64, max_h=64, max_features=500, max_frames=2)     # the entry does not depend on these sizes
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(ctx, masks, connectivity=8, open_radius=0, min_area=1, max_objects=None, mask_pad=0, label_pad=0, skip=0, work=None):
    """masks u8[n,h,w] through Context.mask_components -> (labels i32[n,h,w], nobjects i32[n], table [n,max_objects] or None).
    Masks and labels are views of wider, taller tensors filled with a sentinel, starting `skip` elements into their rows; the
    table has one spare row per mask's worth behind it.  Everything outside must still hold the sentinel afterwards, and so
    must every table row past min(K, max_objects)."""
    import torch
    from evenvizion_amd._lib import Context
    masks = np.asarray(masks, np.uint8)
    n, h, w = masks.shape
    src = torch.full((n, h + 1, skip + w + mask_pad), 0xCD, dtype=torch.uint8, device="cuda")
    src[:, :h, skip:skip + w] = dev(masks)
    full = torch.full((n, h + 1, skip + w + label_pad), SENTINEL, dtype=torch.int32, device="cuda")
    inside = (slice(None), slice(0, h), slice(skip, skip + w))
    nobj = torch.full((n + 1,), SENTINEL, dtype=torch.int32, device="cuda")
    objects = None
    if max_objects:
        objects = torch.full((n + 1, max_objects, 5), FILL64, dtype=torch.int64, device="cuda")
    ctx.mask_components(src[inside], full[inside], connectivity, open_radius, min_area, objects=None if objects is None else objects[:n],
                        nobjects=nobj[:n], work=work)
    ctx.synchronize()
    got = full.cpu().numpy()
    gaps = np.ones(got.shape, bool)
    gaps[inside] = False
    assert (got[gaps] == SENTINEL).all(), "elements outside the label rows were written"
    assert int(nobj[n]) == SENTINEL
    counts = nobj[:n].cpu().numpy()
    table = None
    if objects is not None:
        assert (objects[n] == FILL64).all()
        table = Context.components_table(objects[:n])
        raw = objects[:n].cpu().numpy()
        for m in range(n):
            assert (raw[m, min(int(counts[m]), max_objects):] == FILL64).all(), "table rows past K were written"
    return got[inside], counts, table


def check(ctx, masks, connectivity=8, open_radius=0, min_area=1, max_objects=None, want=None, **kw):
    """-> the expected [(labels, objects)] per mask, for further assertions and for reuse as `want`.  max_objects=None: K + 2."""
    masks = np.asarray(masks, np.uint8)
    if want is None:
        want = [K.components(m, connectivity, open_radius, min_area) for m in masks]
    most = max(len(o) for _, o in want)
    cap = most + 2 if max_objects is None else max_objects
    labels, counts, table = run(ctx, masks, connectivity, open_radius, min_area, cap, **kw)
    for m, (wl, wo) in enumerate(want):
        print("mask %d %dx%d c%d r%d a%d: K %d (want %d), differing labels %d" % (m, masks.shape[2], masks.shape[1], connectivity, open_radius,
                                                                             min_area, counts[m], len(wo), (labels[m] != wl).sum()))
    for m, (wl, wo) in enumerate(want):
        assert counts[m] == len(wo), "nobjects of mask %d" % m
        assert np.array_equal(labels[m], wl), "labels of mask %d" % m
        if table is not None:
            rows = [tuple(int(v) for v in table[m, k]) for k in range(min(len(wo), cap))]
            assert rows == K.table(wo)[:cap], "table of mask %d" % m
    return want


def random_mask(seed, w, h, density, n=1):
    return (np.random.default_rng(seed).random((n, h, w)) < density).astype(np.uint8) * 255


# ---- sizes around the tile ----------------------------------------------------------------------------------------------------------
def sizes(t):
    return [1, 2, t - 1, t, t + 1, 2 * t + 1]


@pytest.mark.parametrize("iw", range(6))
@pytest.mark.parametrize("ih", range(6))
def test_sizes_around_the_tile(ctx, iw, ih):
    w, h = sizes(tile()[0])[iw], sizes(tile()[1])[ih]
    masks = np.concatenate([random_mask(100 + 7 * iw + ih, w, h, 0.55), np.full((1, h, w), 1, np.uint8)])
    for c in (4, 8):
        check(ctx, masks, c)
    check(ctx, masks, 8, open_radius=1)


@pytest.mark.parametrize("w,h", [(1, 1), (1, 137), (199, 1), (1, 2), (2, 1)])
def test_lines_of_pixels(ctx, w, h):
    masks = np.concatenate([random_mask(3, w, h, 0.7), random_mask(4, w, h, 0.3), np.full((1, h, w), 255, np.uint8)])
    for c in (4, 8):
        check(ctx, masks, c)


# ---- mask batches ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 300])
def test_mask_batches(ctx, n):
    w, h = (9, 7) if n == 300 else (45, 23)
    masks = random_mask(11 + n, w, h, 0.5, n)
    assert len({m.tobytes() for m in masks}) == n            # every mask different
    check(ctx, masks, 4, mask_pad=1, label_pad=3)
    check(ctx, masks, 8)


def test_groups_of_masks(ctx):
    """Five masks of 4096 x 2048: the work size stops at four of them (256 MiB), so the entry labels a group of four and a group
    of one.  The masks are empty but for a small random patch each, so the expectation is the patch's, moved."""
    import torch
    from evenvizion_amd._lib import Context, mask_components_work_bytes
    dw, dh, n, pw, ph, ox, oy = 4096, 2048, 5, 45, 23, 4096 - 45, 2048 - 23
    need = mask_components_work_bytes(dw, dh, n)
    assert need == 4 * 8 * dw * dh
    patches = random_mask(31, pw, ph, 0.5, n)
    masks = torch.zeros((n, dh, dw), dtype=torch.uint8, device="cuda")
    masks[:, oy:, ox:] = dev(patches)
    labels = torch.full((n, dh, dw), SENTINEL, dtype=torch.int32, device="cuda")
    objects = torch.full((n, 64, 5), FILL64, dtype=torch.int64, device="cuda")
    work = torch.empty(need // 4, dtype=torch.int32, device="cuda")
    nobj = ctx.mask_components(masks, labels, 8, 0, 1, objects=objects, work=work)
    ctx.synchronize()
    table = Context.components_table(objects)
    expected = torch.zeros((n, dh, dw), dtype=torch.int32, device="cuda")
    for m in range(n):
        wl, wo = K.components(patches[m], 8)
        expected[m, oy:, ox:] = dev(wl)
        assert int(nobj[m]) == len(wo) <= 64
        moved = [(o["x0"] + ox, o["y0"] + oy, o["x1"] + ox, o["y1"] + oy, o["area"], (o["first"] // pw + oy) * dw + o["first"] % pw + ox,
                  o["sx"] + o["area"] * ox, o["sy"] + o["area"] * oy) for o in wo]
        assert [tuple(int(v) for v in table[m, k]) for k in range(len(wo))] == moved, "table of mask %d" % m
    assert bool((labels == expected).all())


# ---- contents -------------------------------------------------------------------------------------------------------------------------
def canvas():
    tw, th = tile()
    return 2 * tw + 7, 2 * th + 5


def spiral(w, h):
    """a rectangular spiral of one-pixel arms two pixels apart, wound inwards from (0, 0)"""
    m = np.zeros((h, w), np.uint8)
    x0, y0, x1, y1 = 0, 0, w - 1, h - 1
    m[0, :] = 1
    while True:
        if x1 - x0 < 2 or y1 - y0 < 2:
            break
        m[y0:y1 + 1, x1] = 1          # down the right side
        m[y1, x0:x1 + 1] = 1          # back along the bottom
        y0 += 2
        if y1 - y0 < 2:
            break
        m[y0:y1 + 1, x0] = 1          # up the left side to two below the previous top
        x1 -= 2
        m[y0, x0:x1 + 1] = 1          # along the new top
        x0 += 2
        y1 -= 2
    return m


def contents():
    w, h = canvas()
    tw, th = tile()
    yy, xx = np.mgrid[0:h, 0:w]
    out = {"empty": np.zeros((h, w), np.uint8), "full": np.ones((h, w), np.uint8), "checkerboard": ((xx + yy) & 1 == 0).astype(np.uint8)}
    corners = [(cx, cy) for cx in range(tw, w, tw) for cy in range(th, h, th)]
    for name, offsets in (("corner_diagonal", ((-1, -1), (0, 0))), ("corner_antidiagonal", ((0, -1), (-1, 0))),
                          ("corner_left_pair", ((-1, -1), (-1, 0))), ("corner_top_pair", ((-1, -1), (0, -1))),
                          ("corner_three", ((-1, -1), (0, -1), (0, 0))), ("corner_upper_left", ((-1, -1),)), ("corner_upper_right", ((0, -1),)),
                          ("corner_lower_left", ((-1, 0),)), ("corner_lower_right", ((0, 0),))):
        m = np.zeros((h, w), np.uint8)
        for cx, cy in corners:
            for i, j in offsets:
                m[cy + j, cx + i] = 1
        out[name] = m
    out["horizontal"] = (yy == th + 3).astype(np.uint8) | (yy == th - 1).astype(np.uint8) | (yy == 2 * th).astype(np.uint8)
    out["vertical"] = (xx == tw + 3).astype(np.uint8) | (xx == tw - 1).astype(np.uint8) | (xx == 2 * tw).astype(np.uint8)
    out["diagonal"] = ((xx - yy) % 9 == 0).astype(np.uint8)
    out["antidiagonal"] = ((xx + yy) % 9 == 0).astype(np.uint8)
    comb = np.zeros((h, w), np.uint8)
    comb[h - 1, :] = 1
    comb[:, ::2] = 1                                     # the teeth meet only in the last row
    out["comb"] = comb
    serp = np.zeros((h, w), np.uint8)
    serp[::2, :] = 1
    serp[1::4, w - 1] = 1
    serp[3::4, 0] = 1
    out["serpentine"] = serp
    sideways = np.zeros((h, w), np.uint8)
    sideways[:, ::2] = 1
    sideways[h - 1, 1::4] = 1
    sideways[0, 3::4] = 1
    out["serpentine_columns"] = sideways
    out["spiral"] = spiral(w, h)
    u = np.zeros((h, w), np.uint8)
    u[2:h - 2, 3] = 1
    u[1:h - 2, w - 4] = 1                                # the first pixel is the right arm's top, in the last tile across
    u[h - 3, 3:w - 3] = 1
    out["u"] = u
    ring = np.zeros((h, w), np.uint8)
    ring[1, tw + 2:w - 1] = 1                            # the top starts in the second tile; the left side hangs below the first
    ring[h - 2, 2:w - 1] = 1
    ring[2:h - 2, 2] = 1
    ring[1:h - 1, w - 2] = 1
    out["ring"] = ring
    return out


def test_contents_cover_what_they_claim():
    """the crafted masks, checked on the host: the spiral is one component that visits every tile, the U's first pixel is not in
    the first tile, ..."""
    C = contents()
    w, h = canvas()
    tw, th = tile()
    assert len(K.components(C["spiral"], 4)[1]) == 1 and C["spiral"][::th, ::tw].size >= 9
    for name in ("u", "ring", "comb", "serpentine", "serpentine_columns"):
        assert len(K.components(C[name], 4)[1]) == 1, name
    assert K.components(C["u"], 4)[1][0]["first"] % w >= 2 * tw and K.components(C["ring"], 4)[1][0]["first"] % w >= tw
    assert len(K.components(C["checkerboard"], 4)[1]) == (w * h + 1) // 2 and len(K.components(C["checkerboard"], 8)[1]) == 1
    assert len(K.components(C["corner_diagonal"], 4)[1]) == 2 * len(K.components(C["corner_diagonal"], 8)[1]) == 8


@pytest.mark.parametrize("name", sorted(contents()))
def test_contents(ctx, name):
    m = contents()[name][None]
    for c in (4, 8):
        check(ctx, m, c, mask_pad=1, label_pad=1)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("density", [0.1, 0.4, 0.59, 0.9])
def test_random_masks(ctx, density, connectivity):
    check(ctx, random_mask(int(density * 100), 200, 140, density, 2), connectivity)


# ---- parameters -----------------------------------------------------------------------------------------------------------------------
def blobs(seed, w, h):
    """filled boxes and discs, thin bridges between them, one-pixel noise, foreground on every canvas edge"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), bool)
    for _ in range(14):
        cx, cy, r = rng.integers(0, w), rng.integers(0, h), rng.integers(2, 11)
        m |= ((xx - cx) ** 2 + (yy - cy) ** 2 <= r * r) if rng.random() < 0.5 else ((abs(xx - cx) <= r) & (abs(yy - cy) <= r // 2 + 1))
    for _ in range(6):
        y, x = rng.integers(0, h), rng.integers(0, w)
        m[y, min(x, w - 30):min(x, w - 30) + 30] = True          # bridges one pixel thick
        m[min(y, h - 20):min(y, h - 20) + 20, x] = True
    m ^= rng.random((h, w)) < 0.02                                # noise: single pixels set and holes punched
    m[0:8, 0:9] = m[h - 9:h, w - 8:w] = m[0:7, w - 10:w] = m[h - 8:h, 0:8] = True     # blocks in the corners survive every radius
    return m.astype(np.uint8)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("r", [0, 1, 2, 3])
def test_opening(ctx, r, connectivity):
    m = blobs(40 + r, 117, 83)
    want = check(ctx, m[None], connectivity, open_radius=r, skip=1, label_pad=2)
    assert len(want[0][1]) >= 2
    if r:
        assert (want[0][0] != 0).sum() < m.sum()                  # the opening removed something


def test_min_area(ctx):
    m = random_mask(50, 90, 61, 0.45)
    areas = sorted(o["area"] for o in K.components(m[0], 4)[1])
    largest = areas[-1]
    assert areas[0] == 1 and largest > 2
    for a in (1, 2, largest, largest + 1):
        want = check(ctx, m, 4, min_area=a)
        assert len(want[0][1]) == sum(v >= a for v in areas)
    assert not K.components(m[0], 4, 0, largest + 1)[1]


def test_max_objects(ctx):
    m = random_mask(51, 70, 50, 0.3, 2)
    want = [K.components(x, 8) for x in m]
    k = len(want[0][1])
    assert k > 6 and len(want[1][1]) != k
    base, counts, none = run(ctx, m, 8, max_objects=0)            # a NULL table
    assert none is None and counts.tolist() == [len(o) for _, o in want]
    for cap in (1, k, k + 5):
        check(ctx, m, 8, max_objects=cap, want=want)               # run() holds rows past K to the sentinel
        assert np.array_equal(run(ctx, m, 8, max_objects=cap)[0], base), "max_objects changed a label"


def test_strides_and_a_skipped_base(ctx):
    m = random_mask(52, 67, 35, 0.5, 3)
    want = check(ctx, m, 8)
    for mask_pad, label_pad, skip in ((3, 0, 0), (0, 5, 0), (1, 3, 1), (2, 1, 3)):
        check(ctx, m, 8, want=want, mask_pad=mask_pad, label_pad=label_pad, skip=skip)


def test_two_calls_give_the_same_bytes(ctx):
    m = np.concatenate([random_mask(53, 150, 100, 0.59), np.ones((1, 100, 150), np.uint8)])
    a = run(ctx, m, 8, max_objects=64)
    b = run(ctx, m, 8, max_objects=64)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2].tobytes() == b[2].tobytes()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(ctx):
    import torch
    from evenvizion_amd._lib import mask_components_work_bytes
    INVALID, CAPACITY = -1, -3
    n, dw, dh, cap = 2, 31, 22, 6
    A = Arena(8)
    mask = A.put(random_mask(60, dw, dh, 0.5, n))
    labels = A.take((n, dh, dw), torch.int32, fill=SENTINEL)
    objects = A.take((n, cap, 5), torch.int64, fill=FILL64)
    nobj = A.take((n,), torch.int32, fill=SENTINEL)
    wb = mask_components_work_bytes(dw, dh, n)
    assert wb == 8 * dw * dh * n
    work = A.take((wb // 4,), torch.int32, fill=SENTINEL)
    k, l, o, c, w = (t.data_ptr() for t in (mask, labels, objects, nobj, work))
    good = dict(ctx=ctx.h, mask=k, n=n, dw=dw, dh=dh, mrs=dw, mfs=dw * dh, conn=8, r=1, area=1, labels=l, lrs=dw, lfs=dw * dh, objects=o,
                cap=cap, nobj=c, work=w, wb=wb)
    order = ("ctx", "mask", "n", "dw", "dh", "mrs", "mfs", "conn", "r", "area", "labels", "lrs", "lfs", "objects", "cap", "nobj", "work", "wb")

    def call(**kw):
        a = dict(good, **kw)
        return ctx.lib.evh_mask_components(*[a[t] for t in order])

    who = "evh_mask_components: "
    NA, MO = "NULL argument", "max_objects must not be negative, and d_objects may be NULL only when it is 0"
    CO, RA, MA, EM = "connectivity must be 4 or 8", "open_radius must lie in 0..3", "min_area must be at least 1", "empty canvas or negative nmasks"
    MS, LS = "mask stride smaller than a row / picture", "label stride smaller than a row / picture"
    AL4, AL8, WB = "d_labels, d_nobjects and d_work must be 4-byte aligned", "d_objects must be 8-byte aligned", "work_bytes below evh_mask_components_work_bytes"
    AREA, MANY = "dw * dh above INT_MAX", "at most 65535 masks per call"

    def over(a, b):
        return "%s overlaps %s" % (a, b)
    LB, OB, NB, WK, MK = "d_labels", "d_objects", "d_nobjects", "d_work", "d_mask"

    def refused(rc, code, text, what):
        assert rc == code, what
        assert ctx.lib.evh_last_error_string(ctx.h).decode() == text, what

    assert call(ctx=None) == INVALID
    invalid = [(dict(mask=None), NA), (dict(labels=None), NA), (dict(nobj=None), NA), (dict(work=None), NA), (dict(objects=None), MO),
               (dict(cap=-1), MO), (dict(conn=6), CO), (dict(conn=0), CO), (dict(r=-1), RA), (dict(r=4), RA), (dict(area=0), MA),
               (dict(area=-3), MA), (dict(dw=0), EM), (dict(dh=0), EM), (dict(dh=-1), EM), (dict(n=-1), EM), (dict(mrs=dw - 1), MS),
               (dict(mfs=dw * dh - 1), MS), (dict(lrs=dw - 1), LS), (dict(lfs=dw * dh - 1), LS), (dict(labels=l + 2), AL4),
               (dict(nobj=c + 1), AL4), (dict(work=w + 2), AL4), (dict(objects=o + 4), AL8), (dict(wb=wb - 1), WB), (dict(wb=0), WB),
               # an output or the work buffer over the mask or another output
               (dict(labels=k), over(LB, MK)), (dict(labels=k + 4 * ((n * dw * dh + 3) // 4) - 4), over(LB, MK)), (dict(objects=k), over(OB, MK)),
               (dict(nobj=k + 8), over(NB, MK)), (dict(work=k), over(WK, MK)), (dict(objects=l + 8), over(LB, OB)), (dict(nobj=l), over(LB, NB)),
               (dict(work=l + 4 * n * dw * dh - 4), over(LB, WK)), (dict(nobj=o + 40 * n * cap - 4), over(OB, NB)), (dict(work=o), over(OB, WK)),
               (dict(nobj=w + wb - 4), over(NB, WK)),
               # two faults: the earlier check of the entry names the refusal
               (dict(mask=None, conn=5), NA), (dict(conn=5, r=7), CO), (dict(mrs=dw - 1, lrs=dw - 1), MS), (dict(lrs=dw - 1, labels=l + 1), LS),
               (dict(wb=wb - 1, work=k), WB)]
    for kw, text in invalid:
        refused(call(**kw), INVALID, who + text, kw)
    wide = dict(dw=65536, dh=32768, mrs=65536, mfs=1 << 31, lrs=65536, lfs=1 << 31)
    for kw, text in ((wide, AREA), (dict(n=65536), MANY), (dict(wide, mrs=1), AREA), (dict(n=65536, wb=0), MANY)):
        refused(call(**kw), CAPACITY, who + text, kw)
    ctx.synchronize()
    assert (labels == SENTINEL).all() and (objects == FILL64).all() and (nobj == SENTINEL).all() and (work == SENTINEL).all()
    # no masks: nothing is done; frame strides do not count for one mask; a NULL table with max_objects == 0 is fine
    assert call(n=0) == 0 and call(n=0, wb=0) == 0
    ctx.synchronize()
    assert (labels == SENTINEL).all() and (nobj == SENTINEL).all()
    assert call(n=1, mfs=0, lfs=0, objects=None, cap=0, wb=mask_components_work_bytes(dw, dh, 1)) == 0
    ctx.synchronize()
    want = K.components(mask[0].cpu().numpy(), 8, 1, 1)
    assert np.array_equal(labels[0].cpu().numpy(), want[0]) and int(nobj[0]) == len(want[1]) and int(nobj[1]) == SENTINEL
    assert (labels[1] == SENTINEL).all() and (objects == FILL64).all()
    assert call() == 0
    ctx.synchronize()
    assert np.array_equal(labels[1].cpu().numpy(), K.components(mask[1].cpu().numpy(), 8, 1, 1)[0])


# ---- what the labels are for ---------------------------------------------------------------------------------------------------------
def test_panning_scene_yields_one_object_per_mask(ctx):
    import torch
    B, frames, mats, squares = P.panning_scene()
    dw, dh, n = 60, 40, len(frames)
    plate = torch.zeros((dh, dw, 3), dtype=torch.uint8, device="cuda")
    count = torch.zeros((dh, dw), dtype=torch.uint8, device="cuda")
    masks = torch.zeros((n, dh, dw), dtype=torch.uint8, device="cuda")
    ctx.plate_fixed_plane(dev(frames), dev(np.asarray(mats, np.float64).reshape(n, 9)), plate, (0, 0), count=count, masks=masks, threshold=0,
                          min_cover=2)
    labels = torch.full((n, dh, dw), SENTINEL, dtype=torch.int32, device="cuda")
    objects = torch.full((n, 4, 5), FILL64, dtype=torch.int64, device="cuda")
    nobj = ctx.mask_components(masks, labels, 8, 0, 1, objects=objects)
    ctx.synchronize()
    table = ctx.components_table(objects)
    twice = count.cpu().numpy() >= 2
    assert nobj.cpu().numpy().tolist() == [1] * n
    for k in range(n):
        ys, xs = np.nonzero(squares[k] & twice)
        o = table[k, 0]
        assert (o["x0"], o["y0"], o["x1"], o["y1"], o["area"]) == (xs.min(), ys.min(), xs.max(), ys.max(), len(xs))
        assert np.array_equal(labels[k].cpu().numpy() == 1, squares[k] & twice)


# ---- the driver on the reference video ---------------------------------------------------------------------------------------------
from test_gpu_plate import recorded_plate          # noqa: E402,F401  (the fixture: plate_checks on device-resized frames)

OBJECTS = dict(connectivity=8, open_radius=0, min_area=9, max_objects=64)


@pytest.fixture(scope="module")
def recorded_objects(recorded_plate):
    """moving_objects over the recorded dictionary from BGR frames, and what components_checks makes of plate_checks' masks."""
    from evenvizion_amd import capture
    from evenvizion_amd.moving import moving_objects
    sup, ri, nos, _, want, origin = recorded_plate
    got = moving_objects(capture.VideoCapture(MP4), sup, ri, placement="translate", max_frames=16, min_cover=1, threshold=16, ingest="bgr",
                         labels=True, **OBJECTS)
    expected = [K.components(m, OBJECTS["connectivity"], OBJECTS["open_radius"], OBJECTS["min_area"]) for m in want[2]]
    return got, expected


def test_moving_objects_on_the_reference_video(recorded_plate, recorded_objects):
    sup, ri, nos, _, want, origin = recorded_plate
    got, expected = recorded_objects
    ox, oy = origin
    assert got["frame_nos"] == nos and got["origin"] == origin and got["size"] == (want[2].shape[2], want[2].shape[1])
    assert sum(len(o) for _, o in expected) > 0
    seen = set()
    for k, no in enumerate(nos):
        wl, wo = expected[k]
        frame = got["frames"][no]
        print("frame %d: K %d (want %d), differing labels %d" % (no, frame["count"], len(wo), (got["labels"][k] != wl).sum()))
        assert frame["count"] == len(wo) and frame["truncated"] == (len(wo) > OBJECTS["max_objects"])
        assert np.array_equal(got["labels"][k], wl)
        assert len(frame["objects"]) == min(len(wo), OBJECTS["max_objects"])
        for o, w_ in zip(frame["objects"], wo):
            assert o["box_canvas"] == (w_["x0"], w_["y0"], w_["x1"], w_["y1"]) and o["area"] == w_["area"]
            assert o["box_plane"] == (w_["x0"] + ox, w_["y0"] + oy, w_["x1"] + ox, w_["y1"] + oy)
            assert o["centre_plane"] == (w_["sx"] / w_["area"] + ox, w_["sy"] / w_["area"] + oy)
            assert len(o["box_frame"]) == 4 and len(o["centre_frame"]) == 2 and np.isfinite(o["box_frame"] + o["centre_frame"]).all()
    for t in got["tracks"]:                                    # every object in exactly one track, frames ascending
        assert [f for f, _ in t] == sorted({f for f, _ in t})
        for step in t:
            assert step not in seen
            seen.add(step)
    assert len(seen) == sum(len(got["frames"][no]["objects"]) for no in nos)


def test_moving_objects_from_planes_equal_the_bgr_ones(recorded_objects):
    from evenvizion_amd import capture
    from evenvizion_amd.moving import moving_objects
    from evenvizion_amd.processing.utils import read_homography_dict, superposition_dict
    hd, ri = read_homography_dict(GOLD)
    planes = moving_objects(capture.VideoCapture(MP4), superposition_dict(hd), ri, placement="translate", max_frames=16, min_cover=1,
                            threshold=16, ingest="yuv420", labels=True, **OBJECTS)
    got = recorded_objects[0]
    assert np.array_equal(planes["labels"], got["labels"]) and planes["frames"] == got["frames"] and planes["tracks"] == got["tracks"]


def test_stabilize_writes_the_objects(recorded_objects, tmp_path, monkeypatch):
    from evenvizion_amd import stabilize
    got = recorded_objects[0]
    monkeypatch.chdir(tmp_path)
    folder = stabilize.main(["--path_to_homography_dict", GOLD, "--path_to_video", MP4, "--experiment_name", "run", "--plate", "1",
                             "--plate_frames", "16", "--plate_masks", "1", "--plate_objects", "1", "--object_open", "0",
                             "--object_min_area", "9", "--object_max", "64"])
    nos = got["frame_nos"]
    names = sorted(os.listdir(folder))
    assert names == sorted(["plate.ppm", "plate_count.png", "moving_objects.json"] + ["mask_%06d.png" % k for k in nos] +
                           ["labels_%06d.png" % k for k in nos])
    report = json.load(open(os.path.join(folder, "moving_objects.json")))
    assert sorted(report) == ["frame_nos", "frames", "origin", "parameters", "size", "tracks"]
    assert report["frame_nos"] == nos and report["parameters"]["min_area"] == 9 and report["parameters"]["connectivity"] == 8
    assert [report["frames"][str(k)]["count"] for k in nos] == [got["frames"][k]["count"] for k in nos]
    assert [len(report["frames"][str(k)]["objects"]) for k in nos] == [len(got["frames"][k]["objects"]) for k in nos]
    assert len(report["tracks"]) == len(got["tracks"])
