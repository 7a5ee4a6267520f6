"""The device's matchers and match filters (evh_match.hip, static_filter_block in evh_ransac.hip) on the adversarial
families of tests/match_families.py, through the C ABI: Context.knn2 (L2 and Hamming), knn2_f32, ratio_unique_filter,
ratio_unique_filter_f32, static_filter and remove_double_matching, against the oracle and, where one exists, the plain
reference (tests/test_oracle_match_edges.py holds the oracle to that reference on the same cases).  Everything is bit
for bit -- indices, integer distances, float distance bits, row bits, counts, statuses; output buffers are pre-filled with
a sentinel and must be untouched past the returned count."""
import ctypes as C

import numpy as np
import pytest

import match_families as F
from oracle import oracle as O
from match_checks import oracle_filter, oracle_static, same_rows

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CTX_ARGS = dict(device=0, max_w=640, max_h=480, max_features=1200, max_frames=4)     # 1728 rows x 4 slots: n = 4000 fits
SENTINEL = -7
ERR_INVALID, ERR_CAPACITY = -1, -3


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU; there is no CPU fallback")
    from evenvizion_amd._lib import Context
    c = Context(**CTX_ARGS)
    yield c
    c.close()


def cu(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def sentinel(shape, dtype):
    return torch.full(shape, SENTINEL, dtype=dtype, device="cuda")


def refused(code):
    from evenvizion_amd._lib import EvhError
    return pytest.raises(EvhError, match=r"libevhip error %d:" % code)


# ---- K1 / K2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hamming", [False, True], ids=["l2", "hamming"])
def test_k1_knn2_ties_tiles_and_the_second_query_trip(ctx, hamming):
    for name, kind, q, t in F.k1_cases():
        idx = sentinel((len(q), 2), torch.int32); d2 = sentinel((len(q), 2), torch.int32)
        ctx.knn2(cu(q), cu(t), idx, d2, hamming=hamming)
        ctx.synchronize()
        gi = idx.cpu().numpy(); gd = d2.cpu().numpy().view(np.uint32)
        for who, (wi, wd) in (("oracle", O.knn2(q, t, hamming)), ("reference", F.ref_knn2_u8(q, t, hamming))):
            bad = np.flatnonzero((gi != wi).any(1) | (gd != wd).any(1))
            assert len(bad) == 0, (name, who, bad[:8], gi[bad[:4]], wi[bad[:4]], gd[bad[:4]], wd[bad[:4]])


def test_k2_knn2_f32_ties_across_the_waves_ranges(ctx):
    for name, kind, q, t in F.k2_cases():
        idx = sentinel((len(q), 2), torch.int32); dist = sentinel((len(q), 2), torch.float32)
        ctx.knn2_f32(cu(q), cu(t), idx, dist)
        ctx.synchronize()
        gi = idx.cpu().numpy(); gd = dist.cpu().numpy()
        want = [("oracle", O.knn2_f32(q, t))]
        if kind != "frac":
            want.append(("reference", F.ref_knn2_f32_int(q, t)[:2]))
        for who, (wi, wd) in want:
            bad = np.flatnonzero((gi != wi).any(1) | (F.bits(gd) != F.bits(wd)).any(1))
            assert len(bad) == 0, (name, who, bad[:8], gi[bad[:4]], wi[bad[:4]], gd[bad[:4]], wd[bad[:4]])


def test_knn2_f32_refuses_other_widths(ctx):
    from evenvizion_amd._lib import EvhError
    q = torch.zeros(4, 32, device="cuda"); idx = sentinel((4, 2), torch.int32); dist = sentinel((4, 2), torch.float32)
    with pytest.raises(EvhError):
        ctx.knn2_f32(q, q, idx, dist)
    ctx.synchronize()
    assert (idx.cpu().numpy() == SENTINEL).all()
    q = torch.zeros(4, 64, device="cuda")
    ctx.knn2_f32(q, q, idx, dist)
    ctx.synchronize()
    assert np.array_equal(idx.cpu().numpy(), np.tile(np.array([0, 1], np.int32), (4, 1)))


# ---- the filter ------------------------------------------------------------------------------------------------------------
def gpu_filter(ctx, c, min_matches, dev=None):
    """-> (status, rows f32[count,4]); asserts that rows past the count keep the sentinel.  dev: device tensors to use
    instead of uploading c's idx and distances (the chained test)."""
    f32 = "dist" in c
    nq = len(c["idx"])
    idx, d = dev if dev is not None else (cu(c["idx"]), cu(c["dist"] if f32 else c["d2"]))
    xy_q, xy_t = cu(c["xy_q"]), cu(c["xy_t"])
    pts = sentinel((nq, 4), torch.float32)
    f = ctx.ratio_unique_filter_f32 if f32 else ctx.ratio_unique_filter
    n, st = f(idx, d, xy_q, xy_t, pts, ratio=c["ratio"], min_matches=min_matches)
    ctx.synchronize()
    out = pts.cpu().numpy()
    assert 0 <= n <= nq and (out[n:] == SENTINEL).all(), (n, nq)
    return st, out[:n].copy()


def check_filter(ctx, c, min_matches, tag):
    f32 = "dist" in c
    d = c["dist"] if f32 else c["d2"]
    dist = c["dist"].astype(np.float64) if f32 else F.u8_distances(c["d2"])
    st_g, rows_g = gpu_filter(ctx, c, min_matches)
    st_o, rows_o = oracle_filter(c["idx"], d, c["xy_q"], c["xy_t"], c["ratio"], min_matches, f32)
    st_r, rows_r = F.ref_filter(c["idx"], dist, c["xy_q"], c["xy_t"], c["ratio"], min_matches)
    assert st_g == st_o == st_r, (tag, st_g, st_o, st_r)
    for who, want in (("oracle", rows_o), ("reference", rows_r)):
        assert same_rows(rows_g, want), (tag, who, len(rows_g), len(want),
                                         np.flatnonzero((F.bits(rows_g[:len(want)]) != F.bits(want[:len(rows_g)])).any(1))[:8])
    return st_g, rows_g


def test_f1_ratio_boundary_integer_and_float_form(ctx):
    for name, c in F.f1_cases() + F.f1_cases_f32():
        st, rows = check_filter(ctx, c, 4, name)
        assert st == F.OK and len(rows) > 0


def test_f2_claims_and_survivor_counts_at_the_compaction_chunks(ctx):
    for name, c, mm in F.f2_cases():
        st, rows = check_filter(ctx, c, mm, name)
        assert st == (F.FEW_MATCHES if c["m"] < mm else F.OK) and len(rows) == (0 if c["m"] < mm else c["m"]), name


def test_f2_no_descriptors(ctx):
    """nq = 0 and nt = 0 give EVH_PAIR_NO_DESCRIPTORS and no rows, in both forms"""
    one_i = torch.zeros(4, 2, dtype=torch.int32, device="cuda"); one_f = torch.ones(4, 2, dtype=torch.float32, device="cuda")
    xy = torch.zeros(4, 2, dtype=torch.float32, device="cuda")
    for f, d in ((ctx.lib.evh_ratio_unique_filter, one_i), (ctx.lib.evh_ratio_unique_filter_f32, one_f)):
        for nq, nt in ((0, 4), (4, 0), (0, 0)):
            pts = sentinel((4, 4), torch.float32)
            n = C.c_int(-1); st = C.c_int(-1)
            ctx._enter()
            rc = f(ctx.h, one_i.data_ptr(), d.data_ptr(), nq, nt, xy.data_ptr(), xy.data_ptr(), 0.5, 0, pts.data_ptr(),
                   C.byref(n), C.byref(st))
            ctx.synchronize()
            assert (rc, n.value, st.value) == (0, 0, F.NO_DESCRIPTORS), (nq, nt, rc, n.value, st.value)
            assert (pts.cpu().numpy() == SENTINEL).all()


def test_f3_duplicate_coordinates_among_survivors(ctx):
    for name, c in F.f3_cases():
        st, rows = check_filter(ctx, c, 4, name)
        assert st == F.OK and len(rows) < c["m"]


def test_f4_every_form_returns_the_same_rows(ctx):
    """kcap 2457 (default dynamic LDS), 2458 (opt-in above 48 KB), 7680 (last LDS size), 7681 and 65535 (k_filter<true> +
    k_filter_dup + k_filter_out in a global scratch); 65536 is refused and the context stays usable.  A second input with
    4203 survivors (three tiles of k_filter_dup) at kcap 7680 and 7681"""
    c3, pad3 = F.f4_case_three_tiles()
    first3 = None
    for kcap in F.F4_THREE_TILES_KCAPS:
        st, rows = check_filter(ctx, dict(c3, xy_t=pad3(kcap)), 4, "f4_three_tiles_kcap%d" % kcap)
        assert st == F.OK
        if first3 is None:
            first3 = rows
        assert same_rows(rows, first3), kcap
    c, pad = F.f4_case()
    first = None
    for kcap in F.F4_KCAPS:
        st, rows = check_filter(ctx, dict(c, xy_t=pad(kcap)), 4, "f4_kcap%d" % kcap)
        assert st == F.OK
        if first is None:
            first = rows
        assert same_rows(rows, first), kcap
    big = dict(c, xy_t=pad(F.F4_REFUSED))
    idx, d2, xy_q, xy_t = cu(big["idx"]), cu(big["d2"]), cu(big["xy_q"]), cu(big["xy_t"])
    pts = sentinel((len(big["idx"]), 4), torch.float32)
    with refused(ERR_CAPACITY):
        ctx.ratio_unique_filter(idx, d2, xy_q, xy_t, pts)
    ctx.synchronize()
    assert (pts.cpu().numpy() == SENTINEL).all()
    st, rows = check_filter(ctx, dict(c, xy_t=pad(2457)), 4, "f4_after_refusal")
    assert st == F.OK and same_rows(rows, first)


# ---- D1: evh_remove_double_matching -----------------------------------------------------------------------------------------
def test_d1_remove_double_matching_entry(ctx):
    for name, rows in F.d1_cases():
        out = sentinel((len(rows), 4), torch.float32)
        n = ctx.remove_double_matching(cu(rows).reshape(-1, 4), out)
        ctx.synchronize()
        got = out.cpu().numpy()
        assert (got[n:] == SENTINEL).all(), name
        want = F.ref_remove_double(rows)
        assert same_rows(got[:n], want), (name, n, len(want))
        if len(rows):
            a, b = O.remove_double(rows[:, :2], rows[:, 2:])
            assert same_rows(got[:n], np.ascontiguousarray(np.c_[a, b], dtype=np.float32)), name


def test_d1_refusals_leave_the_context_usable(ctx):
    name, rows = F.d1_cases()[4]
    want = F.ref_remove_double(rows)
    big = torch.zeros(3 * 65535 + 1, 4, dtype=torch.float32, device="cuda")
    out = sentinel((3 * 65535 + 1, 4), torch.float32)
    with refused(ERR_CAPACITY):
        ctx.remove_double_matching(big, out)
    flat = torch.zeros(4 * len(rows) + 4, dtype=torch.float32, device="cuda")
    with refused(ERR_INVALID):                         # 16-byte alignment, as the sibling entries ask
        ctx.remove_double_matching(flat[1:1 + 4 * len(rows)].reshape(-1, 4), out)
    with refused(ERR_INVALID):
        ctx.remove_double_matching(cu(rows), out.reshape(-1)[1:1 + 4 * len(rows)].reshape(-1, 4))
    both = cu(np.r_[rows, rows])
    with refused(ERR_INVALID):                         # input and output overlap
        ctx.remove_double_matching(both[:len(rows)], both[len(rows) - 1:2 * len(rows) - 1])
    ctx.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()
    n = ctx.remove_double_matching(cu(rows), out)
    ctx.synchronize()
    assert same_rows(out.cpu().numpy()[:n], want)


# ---- S1 - S4 -----------------------------------------------------------------------------------------------------------------
STATIC = F.static_cases()


def gpu_static(ctx, H, rows):
    out = sentinel((len(rows), 4), torch.float32)
    n = ctx.static_filter(H, cu(rows), out)
    ctx.synchronize()
    got = out.cpu().numpy()
    assert 0 <= n <= len(rows) and (got[n:] == SENTINEL).all(), (n, len(rows))
    return got[:n].copy()


@pytest.mark.parametrize("name,H,rows", STATIC, ids=[s[0] for s in STATIC])
def test_static_filter_rounding_ties_and_large_displacements(ctx, name, H, rows):
    """S4 (s4_horizon): displacements above 2^31 are finite and distinct; a device that converts them to one saturated int
    puts them all in one bin and returns that bin instead of the reference's largest group."""
    got = gpu_static(ctx, H, rows)
    want_o = oracle_static(H, rows)
    want_r, _ = F.ref_static(H, rows)
    assert same_rows(got, want_o), (name, "oracle", len(got), len(want_o))
    assert same_rows(got, want_r), (name, "reference", len(got), len(want_r))


def test_static_filter_refuses_more_rows_than_the_context_holds(ctx):
    cap = int(ctx.lib.evh_orb_capacity(ctx.h)) * CTX_ARGS["max_frames"]
    assert cap >= 4000
    rows = torch.zeros(cap + 1, 4, dtype=torch.float32, device="cuda")
    out = sentinel((cap + 1, 4), torch.float32)
    with refused(ERR_CAPACITY):
        ctx.static_filter(F.EYE, rows, out)
    ctx.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()
    name, H, r = STATIC[0]
    assert same_rows(gpu_static(ctx, H, r), oracle_static(H, r))


# ---- the chained stage -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["u8", "f32"])
def test_chain_knn2_into_the_filters_on_device(ctx, form):
    """2-NN output fed straight into the ratio / one-to-one / duplicate filter and on into the static filter without
    leaving the device: equals the oracle's match_static composition without the solver (H given)."""
    q, t, xy_q, xy_t = F.chain_case()
    H = F.CHAIN_H
    idx = sentinel((len(q), 2), torch.int32)
    if form == "u8":
        d = sentinel((len(q), 2), torch.int32)
        ctx.knn2(cu(q), cu(t), idx, d)
        oi, od = O.knn2(q, t)
        c = dict(idx=oi, d2=od, xy_q=xy_q, xy_t=xy_t, ratio=0.5)
    else:
        qf = np.ascontiguousarray(np.tile(q, (1, 2)), dtype=np.float32); tf = np.ascontiguousarray(np.tile(t, (1, 2)), dtype=np.float32)
        d = sentinel((len(q), 2), torch.float32)
        ctx.knn2_f32(cu(qf), cu(tf), idx, d)
        oi, od = O.knn2_f32(qf, tf)
        c = dict(idx=oi, dist=od, xy_q=xy_q, xy_t=xy_t, ratio=0.5)
    st_g, rows_g = gpu_filter(ctx, c, 4, dev=(idx, d))
    st_o, rows_o = oracle_filter(oi, od, xy_q, xy_t, 0.5, 4, form == "f32")
    assert st_g == st_o == F.OK and same_rows(rows_g, rows_o) and len(rows_g) > 600
    got = gpu_static(ctx, H, rows_g)
    want = oracle_static(H, rows_o)
    assert same_rows(got, want) and 0 < len(want) < len(rows_o)
