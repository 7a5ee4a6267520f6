"""GPU parity: every stage of libevhip.so (called through the C ABI) against the CPU oracle on the same seeded
inputs.  Bar: bit-exact for integer / byte / index work (pyramid, FAST candidates, keypoint sets, descriptors,
matches, masks); H within 1e-3 relative error (north_star), and in practice bit-identical f64.
Run with: python -m pytest tests -m gpu   (on the MI355X box)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from evenvizion_amd import synthetic as S  # noqa: E402
from oracle import oracle as O  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU; there is no CPU fallback")
    from evenvizion_amd._lib import Context
    c = Context(device=0, max_w=1280, max_h=720, max_features=500, max_frames=8)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(autouse=True)
def _reference_order_by_default():
    """Oracle and product default to the reference's key-point order (OpenCV 3.4.2 on libstdc++, pinned by the reference's own
    golden run: tests/test_capture_golden.py).  Tests that exercise the canonical mode (all ties kept, (level, y, x) order --
    the mode FAST threshold lifting applies to) switch both sides through `order()` and this puts the oracle back."""
    yield
    O.set_orb_order(1)


def order(c, mode):
    """both sides to key-point order `mode` (0 canonical, 1 reference)"""
    c.set_keypoint_order(mode)
    O.set_orb_order(mode)


def h_err(H, Href):
    """BASELINE.md section 4 metric: entry-wise relative error with floors + corner reprojection."""
    H = H / H[2, 2]; Href = Href / Href[2, 2]
    floor = np.array([[1e-3, 1e-3, 1.0], [1e-3, 1e-3, 1.0], [1e-6, 1e-6, 1.0]])
    return float(np.max(np.abs(H - Href) / np.maximum(np.abs(Href), floor)))


def corner_err(H, Href, w, h):
    c = np.array([[0, 0, 1], [w, 0, 1], [0, h, 1], [w, h, 1]], np.float64).T
    a = H @ c; b = Href @ c
    return float(np.abs(a[:2] / a[2] - b[:2] / b[2]).max())


SIZES = [(400, 224), (1280, 720), (333, 217)]


@pytest.mark.parametrize("w,h", SIZES)
def test_pyramid_and_gray(ctx, w, h):
    prev, cur, _ = S.make_pair(7, w, h)
    rng = np.random.default_rng(3)
    bgr = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    ctx.orb_detect_batch(dev(bgr))
    for f in range(2):
        assert np.array_equal(ctx.download_level(f, 0), O.bgr2gray(bgr[f]))
    ctx.orb_detect_batch(dev(np.stack([prev, cur])))
    for f, img in enumerate((prev, cur)):
        want = O.orb_pyramid(img)
        for l in range(8):
            got = ctx.download_level(f, l)
            assert got.shape == want[l].shape
            assert np.array_equal(got, want[l]), "level %d differs" % l


# levels whose rounded size shrinks by more than 1.21 on an axis: evh_launch_pyramid builds them with k_pyr_down
PYR_DOWN_LEVELS = {(1170, 165): [3, 5], (238, 165): [3, 5, 7], (400, 220): [7]}


@pytest.mark.parametrize("w,h", sorted(PYR_DOWN_LEVELS))
def test_pyramid_down_levels(ctx, w, h):
    """k_pyr_walk stages at most 1.21 x its tile per axis; the levels ORB's rounding shrinks by more go to k_pyr_down
    (128 x 64 tiles).  The device's geometry must select exactly the listed levels (k_pyr_walk's condition in
    evh_launch_pyramid), and all 8 levels must be the oracle's bytes (frame_processing.py:60-61).
    1170 x 165 level 3 (677 x 95) is 6 x 2 tiles at an odd width; 238 x 165 takes k_pyr_down on the last level."""
    prev, cur, _ = S.make_pair(7, w, h)
    ctx.orb_detect_batch(dev(np.stack([prev, cur])))
    dims = [ctx.level_info(l)[:2] for l in range(8)]
    down = [l for l in range(1, 8)
            if not (dims[l - 1][0] * 100 <= dims[l][0] * 121 and dims[l - 1][1] * 100 <= dims[l][1] * 121)]
    assert down == PYR_DOWN_LEVELS[(w, h)], dims
    for f, img in enumerate((prev, cur)):
        want = O.orb_pyramid(img)
        for l in range(8):
            assert np.array_equal(ctx.download_level(f, l), want[l]), "%dx%d level %d differs" % (w, h, l)


@pytest.mark.parametrize("w,h", SIZES)
def test_fast_candidates(ctx, w, h):
    prev, cur, _ = S.make_pair(11, w, h)
    ctx.set_fast_lift(False)          # dense FAST: the candidate lists then hold every corner at threshold 20
    try:
        ctx.orb_detect_batch(dev(np.stack([prev, cur])))
    finally:
        ctx.set_fast_lift(True)
    pyr = O.orb_pyramid(cur)
    for l in range(8):
        gx, gy, gs = ctx.download_candidates(1, l)
        ox, oy, os_ = O.fast_nms(pyr[l], 20)
        lh, lw = pyr[l].shape
        keep = (ox >= 31) & (ox < lw - 31) & (oy >= 31) & (oy < lh - 31)
        want = sorted(zip(oy[keep].tolist(), ox[keep].tolist(), os_[keep].tolist()))
        got = sorted(zip(gy.tolist(), gx.tolist(), gs.tolist()))
        assert got == want, "level %d: %d vs %d candidates" % (l, len(got), len(want))


@pytest.mark.parametrize("w,h", SIZES)
def test_orb_keypoints_and_descriptors(ctx, w, h):
    prev, cur, _ = S.make_pair(13, w, h)
    ctx.orb_detect_batch(dev(np.stack([prev, cur])))
    for f, img in enumerate((prev, cur)):
        g = ctx.orb_download(f)
        o = O.orb_detect(img)
        assert len(g["xy"]) == len(o["xy"]) > 0
        for k in ("octave", "lx", "ly"):
            assert np.array_equal(g[k], o[k]), k          # bit-exact keypoint indices, canonical order
        assert np.array_equal(g["xy"], o["xy"])
        assert np.array_equal(g["response"].view(np.uint32), o["response"].view(np.uint32))
        assert np.array_equal(g["angle"].view(np.uint32), o["angle"].view(np.uint32))
        assert np.array_equal(g["desc"], o["desc"])


@pytest.mark.parametrize("mode", [0, 1])
def test_fast_threshold_lifting_is_exact(ctx, mode):
    """(mode 0: the canonical order, where lifting applies; mode 1: the reference order, which scores densely whatever the switch
    says -- same inputs, same bar.)  Lifted FAST (default) == dense FAST == oracle, including the redo path: texture placed ONLY in the tiles the
    sampling lattice looks at makes the sampled histogram over-estimate the level, the lifted pass comes up short
    of 2*quota corners and the level must be redone at threshold 20."""
    _, tex, _ = S.make_pair(17, 1280, 720)
    frames = []
    for f in range(2):
        img = np.full((720, 1280), 120, np.uint8)
        for t in range(240):                          # level 0 = 10 x 24 tiles of 128 x 28, grid origin (24, 31)
            if t % 27 == (f * 5) % 27:                # k_fast_sample's lattice for level 0 (every 27th tile)
                ty, tx = divmod(t, 10)
                ys, xs = slice(31 + ty * 28, 31 + (ty + 1) * 28), slice(24 + tx * 128, 24 + (tx + 1) * 128)
                img[ys, xs] = tex[ys, xs]
        frames.append(img)
    frames.append(tex)
    rng = np.random.default_rng(8)
    frames.append(rng.integers(0, 256, (720, 1280), dtype=np.uint8))   # white noise: the pre-test passes almost everywhere
    # binary noise: the integer FAST score ties massively at the retainBest cut (all ties are kept, so stage 1 of the
    # selection holds far more survivors than its LDS list: the spill path of k_select)
    frames.append((rng.integers(0, 2, (720, 1280)) * 255).astype(np.uint8))
    frames = np.stack(frames)
    order(ctx, mode)
    res = {}
    for lift in (True, False):
        ctx.set_fast_lift(lift)
        ctx.orb_detect_batch(dev(frames))
        res[lift] = [ctx.orb_download(f) for f in range(len(frames))]
    ctx.set_fast_lift(True)
    for f in range(len(frames)):
        o = O.orb_detect(frames[f])
        assert len(o["xy"]) > 50
        for lift in (True, False):
            g = res[lift][f]
            for k in ("octave", "lx", "ly"):
                assert np.array_equal(g[k], o[k]), (lift, f, k)
            assert np.array_equal(g["desc"], o["desc"]) and np.array_equal(g["xy"], o["xy"])
    order(ctx, 1)


def _dots(h, w, step, shift=(0, 0)):
    """isolated bright pixels on a lattice: every one is a FAST corner with the same score AND the same Harris
    response, i.e. one big tie at both retainBest cuts"""
    img = np.full((h, w), 40, np.uint8)
    for y in range(40 + shift[1], h - 40, step):
        for x in range(40 + shift[0], w - 40, step):
            img[y, x] = 230
    return img


@pytest.mark.parametrize("mode", [0, 1])
def test_tied_key_points_are_all_kept(ctx, mode):
    """(mode 0, canonical: every tie at the cut is kept.  Mode 1, the reference: OpenCV 3.4.2 compares the tail with whatever
    nth_element left at position n - 1, so ties survive only when that is the smallest of the best n -- the SET follows
    libstdc++'s permutation, and the product reproduces it.)  retainBest keeps EVERY tie at the cut (frame_processing.py:59-61 -> KeyPointsFilter::retainBest): a lattice of
    identical corners gives far more key points than nfeatures on level 0 (324 where the quota is 104), saturated /
    binary content ties on the FAST score.  Key-point sets, descriptors and the pair result equal the oracle's."""
    prev, cur, _ = S.make_pair(31, 400, 224)
    binary = [((a > 128) * 255).astype(np.uint8) for a in (prev, cur)]          # saturated 0 / 255 blocks
    frames = np.stack([_dots(224, 400, 12), _dots(224, 400, 12, (3, 2)), _dots(224, 400, 16), _dots(224, 400, 16, (2, 1)),
                       binary[0], binary[1]])
    order(ctx, mode)
    ctx.orb_detect_batch(dev(frames))
    counts = []
    for f in range(len(frames)):
        g, o = ctx.orb_download(f), O.orb_detect(frames[f])
        counts.append(len(o["xy"]))
        for k in ("octave", "lx", "ly"):
            assert np.array_equal(g[k], o[k]), (f, k)
        assert np.array_equal(g["desc"], o["desc"]) and np.array_equal(g["xy"], o["xy"])
        assert np.array_equal(g["response"].view(np.uint32), o["response"].view(np.uint32))
    if mode == 0:
        assert counts[0] > 600 and counts[0] <= ctx.lib.evh_orb_capacity(ctx.h)      # 609 key points for nfeatures = 500
    print("key points per frame in order mode %d: %s" % (mode, counts))
    n = 3
    H = torch.zeros(n, 9, dtype=torch.float64, device="cuda")
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ctx.pair_homography_batch(dev(frames), n, 0, H, st)
    ctx.synchronize()
    Ho, so = O.pairs_gray_batch(frames)
    assert np.array_equal(st.cpu().numpy(), so)
    Hg = H.cpu().numpy().reshape(-1, 3, 3)
    for p in range(n):
        if so[p] == 0:
            assert np.allclose(Hg[p], Ho[p], rtol=1e-9, atol=1e-12)
    order(ctx, 1)


def test_frame_capacity_is_a_pair_status(ctx):
    """The one hard bound: a frame slot holds evh_orb_capacity() key points.  A frame whose tie set is larger (here
    1000 identical corners for nfeatures = 500; the oracle counts them) gives EVH_PAIR_CAPACITY for ITS pairs only --
    the other pairs of the batch are computed, the call succeeds -- and the Python stream driver re-runs the chunk on a
    context with larger frame slots instead of repeating the previous H."""
    from evenvizion_amd._lib import EvhError, PAIR_CAPACITY
    from evenvizion_amd.processing import get_homography_dict
    cap = ctx.lib.evh_orb_capacity(ctx.h)
    prev, cur, _ = S.make_pair(33, 400, 224)
    crowded = _dots(224, 400, 8)
    assert len(O.orb_detect(crowded)["xy"]) > cap
    frames = np.stack([prev, cur, crowded, _dots(224, 400, 8, (2, 1)), prev, cur])
    H = torch.zeros(3, 9, dtype=torch.float64, device="cuda")
    st = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    ctx.pair_homography_batch(dev(frames), 3, 0, H, st)
    ctx.synchronize()
    Ho, so = O.pairs_gray_batch(frames[:2])
    assert st.cpu().tolist() == [int(so[0]), PAIR_CAPACITY, int(so[0])]
    Hg = H.cpu().numpy().reshape(-1, 3, 3)
    assert np.allclose(Hg[0], Ho[0], rtol=1e-9, atol=1e-12) and np.array_equal(Hg[0], Hg[2])
    with pytest.raises(EvhError):
        ctx.orb_download(2)
    assert len(ctx.orb_download(1)["xy"]) == len(O.orb_detect(cur)["xy"])
    # the Python stream driver re-runs such a chunk on larger frame slots (test_tie_heavy_frame_mid_stream_...)
    d = get_homography_dict(S.SyntheticCapture([S.gray_to_bgr(f) for f in (prev, cur, crowded, cur)]), resize_width=400,
                            features_type_list=["ORB"])
    Hs, ss, _ = O.stream_gray(np.stack([prev, cur, crowded, cur]))
    assert np.allclose(np.array([d[k]["H"] for k in (2, 3, 4)]), Hs, rtol=1e-9, atol=1e-12)


def test_flat_frame_has_no_keypoints(ctx):
    flat = np.full((2, 224, 400), 77, np.uint8)
    ctx.orb_detect_batch(dev(flat))
    assert len(ctx.orb_download(0)["xy"]) == 0
    H = torch.zeros(1, 9, dtype=torch.float64, device="cuda"); st = torch.zeros(1, dtype=torch.int32, device="cuda")
    ctx.pair_homography_batch(dev(flat), 1, 0, H, st)
    ctx.synchronize()
    assert st.cpu().tolist() == [1]      # descriptors None -> NoMatchesException path
    assert O.pair_gray(flat[1], flat[0])[0] == 1


def test_knn2_l2_and_hamming(ctx):
    rng = np.random.default_rng(5)
    for nq, nt in [(500, 500), (37, 611), (1, 1), (130, 2), (600, 1)]:
        q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
        t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
        if nt > 10:
            t[7] = t[3]                      # exact duplicates: ties must resolve to the lowest train index
            q[0] = t[3]
        for ham in (False, True):
            idx = torch.zeros(nq, 2, dtype=torch.int32, device="cuda")
            d2 = torch.zeros(nq, 2, dtype=torch.int32, device="cuda")
            ctx.knn2(dev(q), dev(t), idx, d2, hamming=ham)
            ctx.synchronize()
            oi, od = O.knn2(q, t, hamming=ham)
            assert np.array_equal(idx.cpu().numpy(), oi)
            assert np.array_equal(d2.cpu().numpy().view(np.uint32), od)


def test_ratio_unique_filter(ctx, goldens):
    rng = np.random.default_rng(9)
    for c in goldens["lowes_ratio_test"]:
        idx = np.array(c["idx"], np.int32); d2 = np.array(c["d2"], np.uint32)
        nq = len(idx); nt = int(max(idx.max(), 0)) + 1
        xy_q = (rng.integers(0, 8, (nq, 2)) * 1.2).astype(np.float32)   # duplicates on purpose
        xy_t = rng.uniform(0, 100, (nt, 2)).astype(np.float32)
        pts = torch.zeros(max(nq, 1), 4, dtype=torch.float32, device="cuda")
        n, st = ctx.ratio_unique_filter(dev(idx), dev(d2.view(np.int32)), dev(xy_q), dev(xy_t), pts, ratio=c["ratio"])
        oq, ot = O.ratio_unique(idx, d2, c["ratio"])
        assert [[int(a), int(b)] for a, b in zip(ot, oq)] == c["matches"]
        if len(oq) < 4:
            assert st == 2 and n == 0
            continue
        oa, ob = O.remove_double(xy_q[oq], xy_t[ot])
        got = pts.cpu().numpy()[:n]
        assert st == 0 and n == len(oa)
        assert np.array_equal(got[:, :2], oa) and np.array_equal(got[:, 2:], ob)


def _point_sets():
    rng = np.random.default_rng(21)
    sets = []
    for case in range(10):
        n = [4, 5, 8, 30, 120, 300, 499, 64, 65, 200][case]
        Ht = S.random_h(rng, 400) if case % 2 else S.random_h(rng, 1280)
        a = rng.uniform(0, 1280, (n, 2))
        p = (Ht @ np.c_[a, np.ones(n)].T).T
        b = p[:, :2] / p[:, 2:] + rng.normal(0, 0.4, (n, 2))
        nout = int(n * [0, 0.2, 0.1, 0.3, 0.45, 0.05, 0.6, 0.2, 0.2, 0.8][case])
        if nout:
            b[rng.choice(n, nout, replace=False)] = rng.uniform(0, 1280, (nout, 2))
        sets.append(np.c_[a, b].astype(np.float32))
    sets.append(np.c_[np.arange(12), np.arange(12), np.arange(12), np.arange(12)].astype(np.float32))  # collinear: no H
    sets.append(np.zeros((3, 4), np.float32))                                                              # n < 4
    return sets


def test_find_homography_ransac(ctx):
    for pts in _point_sets():
        Hg, mg, ig = ctx.find_homography(dev(pts))
        Ho, mo, io = O.find_homography(pts[:, :2], pts[:, 2:])
        assert (Hg is None) == (Ho is None)
        assert np.array_equal(mg, mo)
        assert np.array_equal(ig, io), (ig, io)      # ransac iterations, inlier count, LM iterations
        if Ho is not None:
            assert h_err(Hg, Ho) <= 1e-3            # north_star tolerance
            assert np.allclose(Hg, Ho, rtol=1e-9, atol=1e-12)


def test_find_homography_many_inliers():
    """From 512 inlier rows on, the refinement's passes with the Jacobian run on all four waves of the workgroup
    (lm_eval_mw: products formed ahead by helper waves, additions in the operator's order).  Row counts on both sides of
    that switch and with every kind of remainder (mod 2, 16, 64) against the oracle, bit for bit (utils.py:351-359)."""
    from evenvizion_amd._lib import Context
    rng = np.random.default_rng(77)
    c = Context(device=0, max_w=1280, max_h=720, max_features=4000, max_frames=2)
    try:
        seen_mw = 0
        for n in (520, 545, 560, 577, 600, 641, 705, 777, 1030, 1541, 2049, 3000, 3999):
            Ht = S.random_h(rng, 1280)
            a = rng.uniform(0, 1280, (n, 2))
            p = (Ht @ np.c_[a, np.ones(n)].T).T
            b = p[:, :2] / p[:, 2:] + rng.normal(0, 0.5, (n, 2))
            nout = int(n * rng.uniform(0.0, 0.12))
            if nout:
                b[rng.choice(n, nout, replace=False)] = rng.uniform(0, 1280, (nout, 2))
            pts = np.c_[a, b].astype(np.float32)
            Hg, mg, ig = c.find_homography(dev(pts))
            Ho, mo, io = O.find_homography(pts[:, :2], pts[:, 2:])
            assert Ho is not None and Hg is not None
            assert np.array_equal(mg, mo) and np.array_equal(ig, io), (n, ig, io)
            assert np.array_equal(Hg, Ho), (n, np.abs(Hg - Ho).max())
            seen_mw += int(mo.sum() >= 512)
        assert seen_mw >= 8
    finally:
        c.close()


def test_find_homography_fixed_iterations(ctx):
    """force_max_iters (BASELINE configs[2] "RANSAC 2000 iters"): every accepted sample up to max_iters is evaluated;
    the oracle's forced mode is the same loop without RANSACUpdateNumIters.  Also a short bound (37) that ends inside
    a hypothesis chunk, and the degenerate inputs."""
    for k, pts in enumerate(_point_sets()):
        for max_iters in ((2000, 37) if k in (3, 4, 6, 9) else (2000,)):
            Hg, mg, ig = ctx.find_homography(dev(pts), max_iters=max_iters, force_max_iters=True)
            Ho, mo, io = O.find_homography(pts[:, :2], pts[:, 2:], max_iters=max_iters, force_max_iters=True)
            assert (Hg is None) == (Ho is None)
            assert np.array_equal(ig, io), (k, max_iters, ig, io)
            if len(pts) > 4 and Ho is not None:
                assert io[0] == max_iters
            assert np.array_equal(mg, mo)
            if Ho is not None:
                assert np.allclose(Hg, Ho, rtol=1e-9, atol=1e-12)


def test_static_filter(ctx, goldens):
    for c in goldens["static_filter"]:
        a = np.float32(c["a"]); b = np.float32(c["b"])
        pts = np.c_[a, b].astype(np.float32)
        out = torch.zeros(len(pts), 4, dtype=torch.float32, device="cuda")
        n = ctx.static_filter(np.array(c["H"]), dev(pts), out)
        got = out.cpu().numpy()[:n]
        assert np.array_equal(got[:, :2], np.float32(c["out_a"]).reshape(-1, 2))
        assert np.array_equal(got[:, 2:], np.float32(c["out_b"]).reshape(-1, 2))


@pytest.mark.parametrize("w,h,npairs", [(400, 224, 3), (1280, 720, 2)])
def test_pair_batch_vs_oracle(ctx, w, h, npairs):
    frames, Ht = S.make_pair_batch(2, npairs, w, h)
    H = torch.zeros(npairs, 9, dtype=torch.float64, device="cuda")
    st = torch.full((npairs,), -1, dtype=torch.int32, device="cuda")
    for cn in (1, 3):
        fr = frames if cn == 1 else S.gray_to_bgr(frames)
        ctx.pair_homography_batch(dev(fr), npairs, 0, H, st)
        ctx.synchronize()
        Ho, so = O.pairs_gray_batch(frames)
        assert np.array_equal(st.cpu().numpy(), so)
        Hg = H.cpu().numpy().reshape(-1, 3, 3)
        for p in range(npairs):
            if so[p] == 0:
                assert h_err(Hg[p], Ho[p]) <= 1e-3
                assert np.allclose(Hg[p], Ho[p], rtol=1e-9, atol=1e-12)
                assert corner_err(Hg[p], Ht[p], w, h) < 0.03 * w   # sanity against the analytic ground truth
                assert corner_err(Hg[p], Ho[p], w, h) <= 0.05


def test_failure_statuses_in_a_batch_and_in_a_stream(ctx):
    """The reference's failure branches (matching.py:104-107, :113; video_processing.py:83-105 none_H_processing):
    a flat frame has no descriptors (status 1), unrelated / low-contrast frames leave < 4 matches (status 2); good
    pairs in the same batch are unaffected; in a stream a failing pair repeats the previous H and the superposition
    carries on; a failing FIRST pair has no previous H (the reference raises: NaN + stop here)."""
    w, h = 400, 224
    a0, b0, _ = S.make_pair(1, w, h)
    a1, b1, _ = S.make_pair(2, w, h)
    flat = np.full((h, w), 128, np.uint8)
    lc0 = ((a0.astype(np.int32) - 128) // 6 + 128).astype(np.uint8)
    lc1 = ((b0.astype(np.int32) - 128) // 6 + 128).astype(np.uint8)
    pairs = [(a0, b0), (flat, b0), (a0, flat), (a0, b1), (a1, b1), (lc0, lc1)]
    frames = np.stack([f for p in pairs for f in p])
    n = len(pairs)
    H = torch.zeros(n, 9, dtype=torch.float64, device="cuda")
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    from evenvizion_amd._lib import Context
    c = Context(device=0, max_w=w, max_h=h, max_features=500, max_frames=2 * n)
    try:
        c.pair_homography_batch(dev(frames), n, 0, H, st)
        c.synchronize()
        Ho, so = O.pairs_gray_batch(frames)
        assert list(so) == [0, 1, 1, 2, 0, 2]
        assert np.array_equal(st.cpu().numpy(), so)
        Hg = H.cpu().numpy().reshape(-1, 3, 3)
        for p in range(n):
            if so[p] == 0:
                assert np.allclose(Hg[p], Ho[p], rtol=1e-9, atol=1e-12)
        # stream with a failure in the middle: H repeats, the scan continues
        fr, _ = S.make_stream(9, 6, w, h)
        s1 = np.stack([fr[0], fr[1], flat, fr[2], fr[3], fr[4]])
        H1 = torch.zeros(5, 9, dtype=torch.float64, device="cuda")
        st1 = torch.full((5,), -1, dtype=torch.int32, device="cuda")
        c.pair_homography_batch(dev(s1), 5, 1, H1, st1)
        c.synchronize()
        Ho1, so1, rc1 = O.stream_gray(s1)
        assert rc1 == -1 and list(so1) == [0, 1, 1, 0, 0]
        assert np.array_equal(st1.cpu().numpy(), so1)
        H1g = H1.cpu().numpy().reshape(-1, 3, 3)
        assert np.allclose(H1g, Ho1, rtol=1e-9, atol=1e-12)
        assert np.array_equal(H1g[1], H1g[0]) and np.array_equal(H1g[2], H1g[0])
        # stream whose first pair fails
        s2 = np.stack([flat, fr[1], fr[2], fr[3]])
        H2 = torch.zeros(3, 9, dtype=torch.float64, device="cuda")
        st2 = torch.full((3,), -1, dtype=torch.int32, device="cuda")
        c.pair_homography_batch(dev(s2), 3, 1, H2, st2)
        c.synchronize()
        _, so2, rc2 = O.stream_gray(s2)
        assert rc2 == 0 and so2[0] == 1
        assert st2.cpu().numpy()[0] == 1 and bool(torch.isnan(H2[0]).all())
    finally:
        c.close()


def test_async_solve_back_to_back_batches(ctx):
    """RANSAC on the solve stream overlapping the next batch's detect kernels must not change any result."""
    batches = [S.make_pair_batch(30 + i, 3, 400, 224)[0] for i in range(3)]
    outs = []
    ctx.set_async_solve(True)
    try:
        inputs = [dev(fr) for fr in batches]     # inputs must stay alive until the context has consumed them
        torch.cuda.synchronize()
        for d_fr in inputs:            # enqueue all three without synchronising in between
            H = torch.zeros(3, 9, dtype=torch.float64, device="cuda")
            st = torch.full((3,), -1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()   # the fills above run on torch's stream, the context on its own
            ctx.pair_homography_batch(d_fr, 3, 0, H, st)
            outs.append((H, st))
        ctx.synchronize()
    finally:
        ctx.set_async_solve(False)
    for fr, (H, st) in zip(batches, outs):
        Ho, so = O.pairs_gray_batch(fr)
        assert np.array_equal(st.cpu().numpy(), so)
        Hg = H.cpu().numpy().reshape(-1, 3, 3)
        ok = so == 0
        assert np.allclose(Hg[ok], Ho[ok], rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("w,h,nfeat", [(1280, 720, 2000), (1920, 1080, 2000), (3840, 2160, 4000)])
def test_other_baseline_configs_one_pair(w, h, nfeat):
    """BASELINE.json configs 2-4 geometry (ORB 2000 @720p/1080p, ORB 4000 @4K): one pair each, full path vs oracle."""
    from evenvizion_amd._lib import Context
    prev, cur, Ht = S.make_pair(4000 + w, w, h)
    c = Context(device=0, max_w=w, max_h=h, max_features=nfeat, max_frames=2)
    try:
        fr = dev(np.stack([prev, cur]))
        c.orb_detect_batch(fr, nfeatures=nfeat)
        for f, img in enumerate((prev, cur)):
            g = c.orb_download(f)
            o = O.orb_detect(img, nfeatures=nfeat)
            assert len(g["xy"]) == len(o["xy"]) > nfeat // 2
            assert np.array_equal(g["octave"], o["octave"]) and np.array_equal(g["lx"], o["lx"]) and np.array_equal(g["ly"], o["ly"])
            assert np.array_equal(g["desc"], o["desc"])
        H = torch.zeros(1, 9, dtype=torch.float64, device="cuda"); st = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        c.pair_homography_batch(fr, 1, 0, H, st, nfeatures=nfeat)
        c.synchronize()
        so, Ho = O.pair_gray(cur, prev, nfeatures=nfeat)
        assert st.cpu().tolist() == [so]
        if so == 0:
            assert np.allclose(H.cpu().numpy().reshape(3, 3), Ho, rtol=1e-9, atol=1e-12)
            assert corner_err(Ho, Ht, w, h) < 0.03 * w
    finally:
        c.close()


def test_stream_vs_oracle(ctx):
    frames, _ = S.make_stream(5, 7, 400, 224)
    n = len(frames) - 1
    H = torch.zeros(n, 9, dtype=torch.float64, device="cuda")
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ctx.pair_homography_batch(dev(frames), n, 1, H, st)
    ctx.synchronize()
    Ho, so, rc = O.stream_gray(frames)
    assert rc == -1
    assert np.array_equal(st.cpu().numpy(), so)
    Hg = H.cpu().numpy().reshape(-1, 3, 3)
    for p in range(n):
        assert h_err(Hg[p], Ho[p]) <= 1e-3
        assert np.allclose(Hg[p], Ho[p], rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("force", [False, True])
def test_config2_stream_720p_2000kp(force):
    """BASELINE.json configs[2] on its own workload shape: a 1280x720 STREAM (running superposition), ORB 2000 key
    points, RANSAC bound 2000 -- adaptive as the reference runs it, and with the bound forced (all 2000 samples of
    both RANSACs of every pair evaluated).  Status, H bit-level equal to the oracle stream."""
    frames, _ = S.make_stream(23, 6, 1280, 720)
    n = len(frames) - 1
    from evenvizion_amd._lib import Context
    c = Context(device=0, max_w=1280, max_h=720, max_features=2000, max_frames=len(frames))
    try:
        H = torch.zeros(n, 9, dtype=torch.float64, device="cuda")
        st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        c.stream_homography_batch(dev(frames), H, st, nfeatures=2000, force_max_iters=force)
        c.synchronize()
        Ho, so, rc = O.stream_gray(frames, nfeatures=2000, force_max_iters=force)
        assert rc == -1
        assert np.array_equal(st.cpu().numpy(), so)
        Hg = H.cpu().numpy().reshape(-1, 3, 3)
        for p in range(n):
            assert h_err(Hg[p], Ho[p]) <= 1e-3
            assert np.allclose(Hg[p], Ho[p], rtol=1e-9, atol=1e-12)
    finally:
        c.close()


def test_two_phase_stream_equals_whole_stream(ctx):
    """phase 1 on blocks that overlap by one frame (what 3 GPUs would each do) + ONE phase-2 scan over the
    concatenated static rows == the stream path on the whole stream, bit for bit; and == the oracle."""
    from evenvizion_amd.sharding import stream_block
    frames, _ = S.make_stream(21, 8, 400, 224)       # the module context holds 8 frame slots
    n = len(frames) - 1
    d = dev(frames)
    H = torch.zeros(n, 9, dtype=torch.float64, device="cuda")
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ctx.pair_homography_batch(d, n, 1, H, st)
    ctx.synchronize()
    for world in (1, 3):
        parts = []
        for r in range(world):
            f_lo, f_hi, p_lo, p_hi = stream_block(len(frames), r, world)
            parts.append(ctx.stream_static_batch(d[f_lo:f_hi].contiguous()))
            assert parts[-1][0].shape[0] == p_hi - p_lo
        rows = torch.cat([p[0] for p in parts]); counts = torch.cat([p[1] for p in parts]); st1 = torch.cat([p[2] for p in parts])
        state = torch.zeros(18, dtype=torch.float64, device="cuda")
        H2, st2 = ctx.stream_scan(rows, counts, st1, state_out=state)
        ctx.synchronize()
        assert torch.equal(st2, st) and torch.equal(H2, H)
    # chunked scan with carried state == one scan
    k = 3
    sa = torch.zeros(18, dtype=torch.float64, device="cuda")
    Ha, sta = ctx.stream_scan(rows[:k], counts[:k], st1[:k], state_out=sa)
    Hb, stb = ctx.stream_scan(rows[k:], counts[k:], st1[k:], state_in=sa)
    ctx.synchronize()
    assert torch.equal(torch.cat([Ha, Hb]), H) and torch.equal(torch.cat([sta, stb]), st)
    Ho, so, _ = O.stream_gray(frames)
    assert np.array_equal(st.cpu().numpy(), so)
    assert np.allclose(H.cpu().numpy().reshape(-1, 3, 3), Ho, rtol=1e-9, atol=1e-12)


def test_config3_1080p_two_phase_stream_2000kp():
    """BASELINE.json configs[3] on its own workload shape: one 1920x1080 STREAM, ORB 2000, split the way two GPUs
    would take it (phase 1 on two blocks that overlap by one frame, ONE scan over the gathered static rows).  Equal,
    bit for bit, to the single-call stream path, and equal to the oracle stream."""
    from evenvizion_amd._lib import Context
    from evenvizion_amd.sharding import stream_block
    frames, _ = S.make_stream(31, 5, 1920, 1080)
    n = len(frames) - 1
    c = Context(device=0, max_w=1920, max_h=1080, max_features=2000, max_frames=len(frames))
    try:
        d = dev(frames)
        H = torch.zeros(n, 9, dtype=torch.float64, device="cuda")
        st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        c.stream_homography_batch(d, H, st, nfeatures=2000)
        c.synchronize()
        parts = []
        for r in range(2):
            f_lo, f_hi, p_lo, p_hi = stream_block(len(frames), r, 2)
            parts.append(c.stream_static_batch(d[f_lo:f_hi].contiguous(), nfeatures=2000))
            assert parts[-1][0].shape[0] == p_hi - p_lo
        rows = torch.cat([p_[0] for p_ in parts]); counts = torch.cat([p_[1] for p_ in parts]); st1 = torch.cat([p_[2] for p_ in parts])
        H2, st2 = c.stream_scan(rows, counts, st1)
        c.synchronize()
        assert torch.equal(st2, st) and torch.equal(H2, H)
        Ho, so, rc = O.stream_gray(frames, nfeatures=2000)
        assert rc == -1 and np.array_equal(st.cpu().numpy(), so) and (so == 0).all()
        assert np.allclose(H.cpu().numpy().reshape(-1, 3, 3), Ho, rtol=1e-9, atol=1e-12)
    finally:
        c.close()


def test_config4_4k_streams_4000kp():
    """BASELINE.json configs[4] on its own workload shape: 3840x2160 STREAMS, ORB 4000 -- two streams of three frames
    through the multi-stream entry (concurrent scans) and one of them through the single-stream entry; statuses and H
    equal to the oracle stream."""
    from evenvizion_amd._lib import Context
    w, h, F = 3840, 2160, 3
    s0, _ = S.make_stream(41, F, w, h)
    s1, _ = S.make_stream(42, F, w, h)
    c = Context(device=0, max_w=w, max_h=h, max_features=4000, max_frames=2 * F)
    try:
        both = dev(np.stack([s0, s1]))
        H = torch.zeros(2, F - 1, 9, dtype=torch.float64, device="cuda")
        st = torch.full((2, F - 1), -1, dtype=torch.int32, device="cuda")
        c.multi_stream_homography_batch(both, H, st, nfeatures=4000)
        c.synchronize()
        H1 = torch.zeros(F - 1, 9, dtype=torch.float64, device="cuda")
        st1 = torch.full((F - 1,), -1, dtype=torch.int32, device="cuda")
        c.stream_homography_batch(both[1], H1, st1, nfeatures=4000)
        c.synchronize()
        assert torch.equal(H1, H[1]) and torch.equal(st1, st[1])
        for i, fr in enumerate((s0, s1)):
            Ho, so, rc = O.stream_gray(fr, nfeatures=4000)
            assert rc == -1 and np.array_equal(st[i].cpu().numpy(), so) and (so == 0).all()
            assert np.allclose(H[i].cpu().numpy().reshape(-1, 3, 3), Ho, rtol=1e-9, atol=1e-12)
    finally:
        c.close()


def test_multi_stream_batch_equals_each_stream_alone():
    """evh_multi_stream_homography_batch: S streams scanned concurrently (one wavefront each) == each stream through
    evh_stream_homography_batch on its own, bit for bit, including carried state and a stream with a failing pair."""
    from evenvizion_amd._lib import Context
    w, h, S_, F = 400, 224, 3, 5
    streams = [S.make_stream(40 + i, 2 * F - 1, w, h)[0] for i in range(S_)]
    streams[1][2] = 128                                   # a flat frame inside stream 1: two failing pairs
    c = Context(device=0, max_w=w, max_h=h, max_features=500, max_frames=S_ * F)
    try:
        # reference: every stream alone, in two chunks (F frames, then F frames overlapping by one) with carried state
        ref_H, ref_st = [], []
        for fr in streams:
            Hs, sts = [], []
            state = torch.zeros(18, dtype=torch.float64, device="cuda")
            for k, chunk in enumerate((fr[:F], fr[F - 1:])):
                H = torch.zeros(F - 1, 9, dtype=torch.float64, device="cuda")
                st = torch.full((F - 1,), -1, dtype=torch.int32, device="cuda")
                c.stream_homography_batch(dev(chunk), H, st, state_in=state if k else None, state_out=state)
                c.synchronize()
                Hs.append(H.clone()); sts.append(st.clone())
            ref_H.append(torch.cat(Hs)); ref_st.append(torch.cat(sts))
        # all streams at once, same two chunks
        state = torch.zeros(S_, 18, dtype=torch.float64, device="cuda")
        got_H, got_st = [], []
        for k in range(2):
            batch = np.stack([fr[:F] if k == 0 else fr[F - 1:] for fr in streams])
            H = torch.zeros(S_, F - 1, 9, dtype=torch.float64, device="cuda")
            st = torch.full((S_, F - 1), -1, dtype=torch.int32, device="cuda")
            d = dev(batch)
            c.multi_stream_homography_batch(d, H, st, state_in=state if k else None, state_out=state)
            c.synchronize()
            got_H.append(H.clone()); got_st.append(st.clone())
        for i in range(S_):
            Hi = torch.cat([got_H[0][i], got_H[1][i]]); sti = torch.cat([got_st[0][i], got_st[1][i]])
            assert torch.equal(sti, ref_st[i]), (i, sti, ref_st[i])
            assert torch.equal(Hi, ref_H[i])
        assert int((ref_st[1] != 0).sum()) == 2 and int((ref_st[0] != 0).sum()) == 0
    finally:
        c.close()


def test_fixed_iterations_in_every_batch_form():
    """force_max_iters through the other entry points (the per-lane solver in k_ransac_static / _final_pairs /
    _final_stream with several workgroups): independent pairs == the first pair of a two-frame stream, several streams
    at once == each stream alone; the single stream itself is checked against the oracle in
    test_config2_stream_720p_2000kp."""
    from evenvizion_amd._lib import Context
    w, h = 400, 224
    streams = [S.make_stream(60 + i, 4, w, h)[0] for i in range(2)]
    c = Context(device=0, max_w=w, max_h=h, max_features=500, max_frames=8)
    try:
        ref = []
        for fr in streams:
            H = torch.zeros(3, 9, dtype=torch.float64, device="cuda"); st = torch.full((3,), -1, dtype=torch.int32, device="cuda")
            c.stream_homography_batch(dev(fr), H, st, force_max_iters=True); c.synchronize()
            ref.append((H.clone(), st.clone()))
        Hm = torch.zeros(2, 3, 9, dtype=torch.float64, device="cuda"); sm = torch.full((2, 3), -1, dtype=torch.int32, device="cuda")
        c.multi_stream_homography_batch(dev(np.stack(streams)), Hm, sm, force_max_iters=True); c.synchronize()
        for i in range(2):
            assert torch.equal(sm[i], ref[i][1]) and torch.equal(Hm[i], ref[i][0])
        pairs = np.stack([streams[0][0], streams[0][1], streams[1][0], streams[1][1]])     # (prev0, cur0, prev1, cur1)
        Hp = torch.zeros(2, 9, dtype=torch.float64, device="cuda"); sp = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        c.pair_homography_batch(dev(pairs), 2, 0, Hp, sp, force_max_iters=True); c.synchronize()
        for i in range(2):
            assert int(sp[i]) == int(ref[i][1][0]) == 0 and torch.equal(Hp[i], ref[i][0][0])
    finally:
        c.close()


def test_fixed_iteration_scan_forms(monkeypatch):
    """The fixed-iteration stream scan spreads the samples of a pair over many workgroups (k_scan_hyp + k_scan_finish,
    VERDICT r2 item 6a).  Every form must give the oracle's stream: the default table (all samples ahead), a short
    table (EVH_SCAN_CHUNKS=3: 48 samples ahead, the rest in the chunk loop of k_scan_finish) and the single-workgroup
    kernel (EVH_SCAN_ONE_WG=1); with a failing pair mid-stream (H repeats, state carried between the launches), state
    carried across two calls, and a failing first pair (NaN + stop)."""
    from evenvizion_amd._lib import Context
    w, h = 400, 224
    fr, _ = S.make_stream(9, 7, w, h)
    flat = np.full((h, w), 128, np.uint8)
    s1 = np.stack([fr[0], fr[1], flat, fr[2], fr[3], fr[4], fr[5]])
    s2 = np.stack([flat, fr[1], fr[2], fr[3]])
    Ho1, so1, rc1 = O.stream_gray(s1, force_max_iters=True)
    _, so2, rc2 = O.stream_gray(s2, force_max_iters=True)
    assert rc1 == -1 and list(so1) == [0, 1, 1, 0, 0, 0] and rc2 == 0
    c = Context(device=0, max_w=w, max_h=h, max_features=500, max_frames=8)
    try:
        for env in ({}, {"EVH_SCAN_CHUNKS": "3"}, {"EVH_SCAN_ONE_WG": "1"}):
            monkeypatch.delenv("EVH_SCAN_CHUNKS", raising=False); monkeypatch.delenv("EVH_SCAN_ONE_WG", raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            H1 = torch.zeros(6, 9, dtype=torch.float64, device="cuda"); st1 = torch.full((6,), -1, dtype=torch.int32, device="cuda")
            c.stream_homography_batch(dev(s1), H1, st1, force_max_iters=True); c.synchronize()
            assert np.array_equal(st1.cpu().numpy(), so1), env
            assert np.allclose(H1.cpu().numpy().reshape(-1, 3, 3), Ho1, rtol=1e-9, atol=1e-12), env
            # the same stream in two calls with the state handed over
            state = torch.zeros(18, dtype=torch.float64, device="cuda")
            Ha = torch.zeros(3, 9, dtype=torch.float64, device="cuda"); sa = torch.full((3,), -1, dtype=torch.int32, device="cuda")
            Hb = torch.zeros(3, 9, dtype=torch.float64, device="cuda"); sb = torch.full((3,), -1, dtype=torch.int32, device="cuda")
            c.stream_homography_batch(dev(s1[:4]), Ha, sa, state_out=state, force_max_iters=True)
            c.stream_homography_batch(dev(s1[3:]), Hb, sb, state_in=state, state_out=state, force_max_iters=True); c.synchronize()
            assert torch.equal(torch.cat([Ha, Hb]), H1) and torch.equal(torch.cat([sa, sb]), st1), env
            H2 = torch.zeros(3, 9, dtype=torch.float64, device="cuda"); st2 = torch.full((3,), -1, dtype=torch.int32, device="cuda")
            c.stream_homography_batch(dev(s2), H2, st2, force_max_iters=True); c.synchronize()
            assert st2.cpu().tolist() == [1, 1, 1] and bool(torch.isnan(H2).all()), env
    finally:
        c.close()


def test_fixed_iteration_stream_of_20_frames(monkeypatch):
    """A longer fixed-iteration stream (19 pairs per call: RANSAC #1 of all of them spread over 141 x 19 workgroups, then
    the scan pair by pair) against the oracle, and the single-workgroup kernels on the same frames."""
    from evenvizion_amd._lib import Context
    w, h = 400, 224
    fr, _ = S.make_stream(41, 20, w, h)
    n = len(fr) - 1
    Ho, so, rc = O.stream_gray(fr, force_max_iters=True)
    assert rc == -1 and n >= 16
    c = Context(device=0, max_w=w, max_h=h, max_features=500, max_frames=len(fr))
    try:
        for env in ({}, {"EVH_SCAN_ONE_WG": "1"}):
            monkeypatch.delenv("EVH_SCAN_ONE_WG", raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            H = torch.zeros(n, 9, dtype=torch.float64, device="cuda"); st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
            c.stream_homography_batch(dev(fr), H, st, force_max_iters=True); c.synchronize()
            assert np.array_equal(st.cpu().numpy(), so), env
            assert np.allclose(H.cpu().numpy().reshape(-1, 3, 3), Ho, rtol=1e-9, atol=1e-12), env
    finally:
        c.close()


def test_resize_area(ctx):
    rng = np.random.default_rng(4)
    for (sw, sh, width, cn) in [(1170, 658, 400, 3), (1280, 720, 320, 3), (800, 600, 400, 1), (900, 300, 300, 3),
                                (640, 360, 640, 3),
                                # resize_width LARGER than the frame: INTER_AREA's bilinear emulation
                                (320, 180, 400, 3), (399, 224, 400, 3), (250, 141, 400, 1), (64, 48, 1000, 3)]:
        img = rng.integers(0, 256, (sh, sw, cn) if cn == 3 else (sh, sw), dtype=np.uint8)
        dw, dh = O.resize_dims(sw, sh, width)
        want = O.resize_area(img, dw, dh)
        out = torch.zeros((1, dh, dw, cn) if cn == 3 else (1, dh, dw), dtype=torch.uint8, device="cuda")
        ctx.resize_area(dev(img[None]), out)
        ctx.synchronize()
        assert np.array_equal(out.cpu().numpy()[0], want)


@pytest.mark.parametrize("cn", [3, 1])
@pytest.mark.parametrize("sw,sh,width", [(1170, 658, 400), (1280, 720, 320), (320, 180, 400)])
def test_fused_ingest_equals_resize_then_detect(sw, sh, width, cn):
    """N2: imutils.resize(frame, width) (INTER_AREA, video_processing.py:62,73) fused into the ingest kernel.  Level 0
    (and level 1, key points, the whole stream) from the FULL-SIZE frames equal the oracle's resize -> gray -> ORB;
    1170x658 -> 400x224 is the reference example's geometry (fractional scale: the float tables), 1280x720 -> 320x180
    the integer-scale path, 320x180 -> 400x225 the reference's default resize_width on a smaller source (enlargement:
    the operator's bilinear emulation of INTER_AREA)."""
    from evenvizion_amd._lib import Context
    from evenvizion_amd.processing.video_processing import resized_shape
    g, _ = S.make_stream(41, 4, sw, sh)
    if cn == 3:      # three different channels, so that the gray weights matter
        full = np.stack([g, np.roll(g, 7, axis=2), 255 - g], axis=-1)
    else:
        full = g
    dw, dh = resized_shape(full.shape[1:], width)
    small = [O.resize_area(f, dw, dh) for f in full]
    gray = np.stack([O.bgr2gray(f) if cn == 3 else f for f in small])
    c = Context(device=0, max_w=dw, max_h=dh, max_features=500, max_frames=len(full))
    try:
        c.orb_detect_batch(dev(full), resize_to=(dw, dh))
        for f in range(len(full)):
            assert np.array_equal(c.download_level(f, 0), gray[f])
            assert np.array_equal(c.download_level(f, 1), O.orb_pyramid(gray[f])[1])
        got, want = c.orb_download(1), O.orb_detect(gray[1])
        for k in ("octave", "lx", "ly"):
            assert np.array_equal(got[k], want[k])
        assert np.array_equal(got["desc"], want["desc"])
        n = len(full) - 1
        H = torch.zeros(n, 9, dtype=torch.float64, device="cuda")
        st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        c.stream_homography_batch(dev(full), H, st, resize_to=(dw, dh))
        c.synchronize()
        Ho, so, rc = O.stream_gray(gray)
        assert rc == -1 and np.array_equal(st.cpu().numpy(), so)
        Hg = H.cpu().numpy().reshape(-1, 3, 3)
        for p in range(n):
            assert np.allclose(Hg[p], Ho[p], rtol=1e-9, atol=1e-12)
    finally:
        c.close()


def test_single_frame_convenience_entries(ctx):
    """evh_orb_detect_compute / evh_resize_area_u8c3 (the single-image forms SURVEY 8b lists) == the batch entries."""
    a, _, _ = S.make_pair(77, 640, 360)
    bgr = S.gray_to_bgr(a)
    xy, desc, oc = ctx.orb_detect_compute(dev(bgr), 500)
    o = O.orb_detect(a)
    assert np.array_equal(xy, o["xy"]) and np.array_equal(desc, o["desc"]) and np.array_equal(oc, o["octave"])
    xy1, desc1, _ = ctx.orb_detect_compute(dev(a), 500)          # gray input
    assert np.array_equal(xy1, xy) and np.array_equal(desc1, desc)
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (658, 1170, 3), dtype=np.uint8)
    dw, dh = O.resize_dims(1170, 658, 400)
    out = torch.zeros((dh, dw, 3), dtype=torch.uint8, device="cuda")
    ctx.resize_area_bgr(dev(img), out)
    ctx.synchronize()
    assert np.array_equal(out.cpu().numpy(), O.resize_area(img, dw, dh))


# ---- the Python mirror of evenvizion.processing, end to end on the GPU -----------------------------------------------
def test_python_api_mirror_vs_oracle():
    from evenvizion_amd.processing import FrameProcessing, KeyPoints, NoMatchesException, compute_homography, \
        get_homography_dict, HomographyException
    from evenvizion_amd import runtime
    runtime.reset()
    frames, _ = S.make_stream(9, 6, 400, 224)
    bgr = S.gray_to_bgr(frames)
    # per-call API (frame_processing.py / matching.py / utils.py signatures)
    fa, fb = FrameProcessing(bgr[1], ["ORB"]), FrameProcessing(bgr[0], ["ORB"])
    xy, desc = fa.detect_and_describe_features("ORB")
    o = O.orb_detect(frames[1])
    assert xy.dtype == np.float32 and desc.dtype == np.uint8 and np.array_equal(xy, o["xy"]) and np.array_equal(desc, o["desc"])
    with pytest.raises(ValueError):
        fa.detect_and_describe_features("BRISK")
    pa, pb = fa.concatenate_all_features_types(fb)
    ob = O.orb_detect(frames[0])
    st, sa, sb = O.match_static(o["xy"], o["desc"], ob["xy"], ob["desc"])
    assert st == 0 and np.array_equal(np.array(pa), sa) and np.array_equal(np.array(pb), sb)
    H = compute_homography(pa, pb, None)
    st2, Ho = O.compute_homography(sa, sb, None)
    assert st2 == 0 and np.allclose(H, Ho, rtol=1e-9, atol=1e-12)
    ka, kb = KeyPoints(xy, desc), KeyPoints(ob["xy"], ob["desc"])
    ma, mb = ka.match_kps(kb)
    assert len(ma) == len(mb) >= len(sa)
    with pytest.raises(NoMatchesException):
        KeyPoints(xy, None).match_kps(kb)
    with pytest.raises(NoMatchesException):
        KeyPoints(xy[:3], desc[:3]).match_kps(kb)
    with pytest.raises(HomographyException):
        compute_homography(sa[:3], sb[:3])
    # the driver (video_processing.get_homography_dict), chunked so that state is carried across GPU calls
    Hs, sts, rc = O.stream_gray(frames)
    assert rc == -1
    for chunk in (64, 3):
        d = get_homography_dict(S.SyntheticCapture(list(bgr)), resize_width=400, chunk_frames=chunk, features_type_list=["ORB"])
        assert list(d.keys()) == [2, 3, 4, 5, 6, "resize_info"] and d["resize_info"] == {"h": 224, "w": 400}
        for k in range(2, 7):
            assert np.allclose(np.array(d[k]["H"]), Hs[k - 2], rtol=1e-9, atol=1e-12)
    # resize_width smaller than the frame: INTER_AREA on the GPU, then the same path
    d = get_homography_dict(S.SyntheticCapture(list(bgr)), resize_width=320, features_type_list=["ORB"])
    small = np.stack([O.bgr2gray(O.resize_area(f, 320, 179)) for f in bgr])
    Hs2, st2, rc2 = O.stream_gray(small)
    assert d["resize_info"] == {"h": 179, "w": 320} and rc2 == -1
    for k in range(2, 7):
        assert np.allclose(np.array(d[k]["H"]), Hs2[k - 2], rtol=1e-9, atol=1e-12)
    runtime.reset()


def test_heatmap_field_in_reference_order_reproduces_metrics_file():
    """N3: the GPU coordinate field reproduces the reference's committed metrics_file.txt bit for bit
    (Maximum movement during the entire video: 863.0428982580879) from the committed H JSON, and its field is the
    reference's own np.apply_along_axis(homography_transformation) (fma(h0, x, h1*y) + h2), not an unfused
    ((h0*x + h1*y) + h2) restatement, which differs at ~10^4 coordinates of a frame."""
    import os
    from evenvizion_amd import heatmap, runtime
    from evenvizion_amd.processing import utils
    gold = os.path.join(os.path.dirname(__file__), "golden")
    hd, ri = utils.read_homography_dict(os.path.join(gold, "ref_dict_with_homography_matrix.json"))
    sup = utils.superposition_dict(hd)
    want = float(open(os.path.join(gold, "ref_metrics_file.txt")).read().split(":")[1])
    runtime.reset()
    assert heatmap.max_movement(sup, ri) == want == 863.0428982580879
    keys, m = heatmap.frame_maxima(sup, ri)
    assert keys[0] == 1 and m[0] == 399.0          # frame 1 = identity: max(x) over the 400 x 224 grid
    # frame 61 against the reference's own np.apply_along_axis(homography_transformation) (tests/golden/plane_goldens.json)
    # and the oracle's restatement of its arithmetic order, fma(h0, x, h1*y) + h2
    import hashlib
    import json
    rec = json.load(open(os.path.join(gold, "plane_goldens.json")))["video"]["frames"][60]
    Hk = np.asarray(sup[keys[60]], np.float64)
    assert rec["frame"] == keys[60] and Hk.ravel().tolist() == rec["H"]
    assert m[60] == rec["max"]
    import torch
    field = torch.zeros(1, ri["h"], ri["w"], 2, dtype=torch.float64, device="cuda")
    ctx = runtime.get_context(400, 224)
    ctx.fixed_plane_max(Hk[None], ri["w"], ri["h"], field=field)
    got = field.cpu().numpy()[0]
    want, want_max = O.fixed_plane_field(Hk, ri["w"], ri["h"])
    assert np.array_equal(got, want[0]) and want_max[0] == rec["max"]
    assert hashlib.sha256(got.tobytes()).hexdigest() == rec["field_sha256"]
    runtime.reset()


def test_component_cli_outputs(tmp_path, monkeypatch):
    """evenvizion_amd.component: the argument surface and the non-visual outputs of evenvizion_component.py:101-140
    (dict_with_homography_matrix.json, metrics_file.txt) + fixed_coordinates.json, on a synthetic stream."""
    import json
    from evenvizion_amd import component, heatmap
    from evenvizion_amd.processing.utils import read_homography_dict, superposition_dict
    monkeypatch.chdir(tmp_path)
    n = 7
    coords = {str(k): [{"x1": 100.5 + k, "y1": 80.25}, {"x1": 300.0, "y1": 150.0 - k}] for k in range(1, n + 1)}
    (tmp_path / "coords.json").write_text(json.dumps(coords))
    folder = component.main(["--path_to_video", "synthetic:%d:640x360:3" % n, "--experiment_name", "exp",
                             "--resize_width", "400", "--path_to_original_coordinate", str(tmp_path / "coords.json")])
    assert folder == str(tmp_path / "exp" / ("synthetic_%d_640x360_3" % n))
    d = json.load(open(folder + "/dict_with_homography_matrix.json"))
    assert list(d.keys()) == [str(k) for k in range(2, n + 1)] + ["resize_info"]        # keys start at 2, resize_info last
    assert d["resize_info"] == {"h": 225, "w": 400}                                        # int(360 * 400 / 640)
    assert all(np.asarray(d[str(k)]["H"]).shape == (3, 3) for k in range(2, n + 1))
    Hs, ri = read_homography_dict(folder + "/dict_with_homography_matrix.json")
    txt = open(folder + "/metrics_file.txt").read()
    assert txt == "Maximum movement during the entire video: {}".format(heatmap.max_movement(superposition_dict(Hs), ri))
    fixed = json.load(open(folder + "/fixed_coordinates.json"))
    assert set(fixed.keys()) == set(coords.keys()) and len(fixed["3"]) == 2 and set(fixed["3"][0]) == {"x1", "y1"}
    with pytest.raises(NotImplementedError):
        component.main(["--show_matching_visualization", "True"])


@pytest.mark.parametrize("w,h", [(64, 64), (70, 90), (97, 131), (129, 257), (255, 255), (1000, 70), (1023, 577)])
def test_odd_and_small_sizes_full_path(w, h):
    """Ragged geometry: widths that are not multiples of 4, levels smaller than the 31-px border (no key points at
    all -> status 1), single-tile levels, very wide/flat frames; synthetic texture and white noise.  Key points,
    descriptors, statuses and H must equal the oracle's."""
    from evenvizion_amd._lib import Context
    rng = np.random.default_rng(w * 7919 + h)
    c = Context(device=0, max_w=w, max_h=h, max_features=500, max_frames=2)
    try:
        for kind in ("synth", "noise"):
            if kind == "synth":
                a, b, _ = S.make_pair(int(rng.integers(1, 1000)), w, h)
            else:
                a = rng.integers(0, 256, (h, w), dtype=np.uint8)
                b = np.roll(a, 3, axis=1)
            fr = np.stack([a, b])
            H = torch.zeros(1, 9, dtype=torch.float64, device="cuda")
            st = torch.full((1,), -1, dtype=torch.int32, device="cuda")
            c.pair_homography_batch(dev(fr), 1, 0, H, st)
            c.synchronize()
            for f in range(2):
                o = O.orb_detect(fr[f])
                g = c.orb_download(f) if len(o["xy"]) else None
                if g is None:
                    assert c.lib.evh_orb_count(c.h, f) == 0
                else:
                    assert np.array_equal(g["xy"], o["xy"]) and np.array_equal(g["desc"], o["desc"])
                    assert np.array_equal(g["octave"], o["octave"])
            Ho, so = O.pairs_gray_batch(fr)
            assert st.cpu().numpy()[0] == so[0]
            if so[0] == 0:
                assert np.allclose(H.cpu().numpy().reshape(3, 3), Ho[0], rtol=1e-9, atol=1e-12)
    finally:
        c.close()


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 7, 9, 16])   # covers every width residue mod 4 x {gray, BGR}
def test_random_geometry_sweep(seed):
    """Seeded random geometry: frame sizes from 80x80 to 640x400 (widths with every residue mod 4), 2..9 frames per
    call (the XCD-ordered grids are padded to multiples of 8 in both dimensions), gray and BGR input, 300..700 key
    points.  Every frame's pyramid, key points and descriptors and the whole stream of homographies must equal the
    oracle's."""
    from evenvizion_amd._lib import Context
    rng = np.random.default_rng(seed)
    w = int(rng.integers(80, 641)); h = int(rng.integers(80, 401))
    nfr = int(rng.choice([2, 3, 5, 9])); cn = int(rng.choice([1, 3])); nfeat = int(rng.integers(300, 701))
    gray, _ = S.make_stream(seed, nfr, w, h)
    if rng.random() < 0.3:                               # sometimes hard content: uniform noise frames, shifted
        base = rng.integers(0, 256, (h, w), dtype=np.uint8)
        gray = np.stack([np.roll(base, 2 * i, axis=1) for i in range(nfr)])
    frames = gray if cn == 1 else S.gray_to_bgr(gray)
    want_gray = gray if cn == 1 else np.stack([O.bgr2gray(f) for f in frames])
    c = Context(device=0, max_w=w, max_h=h, max_features=nfeat, max_frames=nfr)
    try:
        n = nfr - 1
        H = torch.zeros(n, 9, dtype=torch.float64, device="cuda")
        st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        c.stream_homography_batch(dev(frames), H, st, nfeatures=nfeat)
        c.synchronize()
        for f in range(nfr):
            pyr = O.orb_pyramid(want_gray[f])
            for l in range(8):
                assert np.array_equal(c.download_level(f, l), pyr[l]), (w, h, cn, f, l)
            o = O.orb_detect(want_gray[f], nfeatures=nfeat)
            if len(o["xy"]) == 0:
                assert c.lib.evh_orb_count(c.h, f) == 0
            else:
                g = c.orb_download(f)
                assert np.array_equal(g["xy"], o["xy"]) and np.array_equal(g["desc"], o["desc"]), (w, h, cn, f)
        Ho, so, rc = O.stream_gray(want_gray, nfeatures=nfeat)
        assert np.array_equal(st.cpu().numpy(), so), (w, h, cn, nfr)
        Hg = H.cpu().numpy().reshape(-1, 3, 3)
        for p_ in range(n):
            if so[p_] == 0:
                assert np.allclose(Hg[p_], Ho[p_], rtol=1e-9, atol=1e-12), (w, h, cn, p_)
    finally:
        c.close()


@pytest.mark.parametrize("cn", [1, 3])
def test_unaligned_and_padded_input_layout(ctx, cn):
    """Frames handed over with an odd base address, padded rows and padded frames take the byte-wise gray path and
    the unfused level-1 kernel; every pyramid level and the key points must still equal the oracle's."""
    w, h = 333, 217
    a, b, _ = S.make_pair(5, w, h)
    gray = np.stack([a, b])
    src = gray if cn == 1 else S.gray_to_bgr(gray)
    row_stride = w * cn + 5
    frame_stride = row_stride * h + 3
    buf = np.zeros(1 + 2 * frame_stride + 64, np.uint8)
    for f in range(2):
        for y in range(h):
            o = 1 + f * frame_stride + y * row_stride
            buf[o:o + w * cn] = src[f, y].reshape(-1)
    d = dev(buf)
    ctx._check(ctx.lib.evh_orb_detect_batch(ctx.h, d.data_ptr() + 1, 2, w, h, cn, row_stride, frame_stride, 500))
    ctx.synchronize()
    for f in range(2):
        want = O.orb_pyramid(gray[f])
        for l in range(8):
            assert np.array_equal(ctx.download_level(f, l), want[l]), "level %d" % l
        o = O.orb_detect(gray[f]); g = ctx.orb_download(f)
        assert np.array_equal(g["xy"], o["xy"]) and np.array_equal(g["desc"], o["desc"])
    # aligned base but padded rows (stride multiple of 4): the fused path with a non-tight layout
    row_stride = (w * cn + 7) // 4 * 4
    frame_stride = row_stride * h + 8
    buf = np.zeros(2 * frame_stride + 64, np.uint8)
    for f in range(2):
        for y in range(h):
            o = f * frame_stride + y * row_stride
            buf[o:o + w * cn] = src[f, y].reshape(-1)
    d = dev(buf)
    ctx._check(ctx.lib.evh_orb_detect_batch(ctx.h, d.data_ptr(), 2, w, h, cn, row_stride, frame_stride, 500))
    ctx.synchronize()
    for f in range(2):
        want = O.orb_pyramid(gray[f])
        for l in range(8):
            assert np.array_equal(ctx.download_level(f, l), want[l]), "level %d" % l


@pytest.mark.parametrize("mode", [0, 1])
def test_shared_threshold_between_consecutive_frames_is_exact(mode):
    """Pair / stream entries let the second frame of a pair (odd frames of a stream) reuse the sampled FAST score
    histogram of the frame before it.  When the frames do NOT look alike -- a corner-rich frame followed by a
    corner-poor one and the reverse -- the borrowed threshold is wrong and the dense redo must restore the exact
    result; key points, descriptors and H still equal the oracle's."""
    from evenvizion_amd._lib import Context
    w, h = 1280, 720
    rich, rich2, _ = S.make_pair(11, w, h)
    poor = rich2.copy()
    for _ in range(8):                                    # 8 passes of a 3x3 box blur: few, weak corners
        g = np.pad(poor.astype(np.uint16), 1, mode="edge")
        poor = ((sum(g[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)) + 4) // 9).astype(np.uint8)
    frames = np.stack([rich, poor, poor, rich, rich, rich2])     # pairs: (rich, poor), (poor, rich), (rich, rich2)
    c = Context(device=0, max_w=w, max_h=h, max_features=500, max_frames=6)
    try:
        order(c, mode)     # the shortcuts act in mode 0 only; mode 1 runs the same sequence of calls
        H = torch.zeros(3, 9, dtype=torch.float64, device="cuda")
        st = torch.full((3,), -1, dtype=torch.int32, device="cuda")
        c.pair_homography_batch(dev(frames), 3, 0, H, st)
        c.synchronize()
        for f in range(6):
            o = O.orb_detect(frames[f]); g = c.orb_download(f)
            assert np.array_equal(g["xy"], o["xy"]) and np.array_equal(g["desc"], o["desc"]), "frame %d" % f
        Ho, so = O.pairs_gray_batch(frames)
        assert np.array_equal(st.cpu().numpy(), so)
        Hg = H.cpu().numpy().reshape(-1, 3, 3)
        for p in range(3):
            if so[p] == 0:
                assert np.allclose(Hg[p], Ho[p], rtol=1e-9, atol=1e-12)
        # sharing off: same result
        c.set_fast_share(False)
        Hn = torch.zeros(3, 9, dtype=torch.float64, device="cuda")
        stn = torch.full((3,), -1, dtype=torch.int32, device="cuda")
        c.pair_homography_batch(dev(frames), 3, 0, Hn, stn)
        c.synchronize()
        assert torch.equal(stn, st) and torch.equal(Hn, H)
        c.set_fast_share(True)
        # the same frames as one stream (odd frames borrow from the frame before)
        H5 = torch.zeros(5, 9, dtype=torch.float64, device="cuda")
        st5 = torch.full((5,), -1, dtype=torch.int32, device="cuda")
        c.pair_homography_batch(dev(frames), 5, 1, H5, st5)
        c.synchronize()
        for f in range(6):
            o = O.orb_detect(frames[f]); g = c.orb_download(f)
            assert np.array_equal(g["xy"], o["xy"]) and np.array_equal(g["desc"], o["desc"]), "stream frame %d" % f
    finally:
        c.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_threshold_hint_across_calls_is_exact(mode):
    """The sample pass of a detect call uses the lifted thresholds of the PREVIOUS call of the same context as a hint
    (lifted scoring at 5/8 of it instead of dense scoring).  A stale hint -- rich content, then poor content, then rich
    again, and a flat frame in between -- must never change a key point."""
    from evenvizion_amd._lib import Context
    w, h = 1280, 720
    rich, rich2, _ = S.make_pair(21, w, h)
    poor = rich2.copy()
    for _ in range(8):
        g = np.pad(poor.astype(np.uint16), 1, mode="edge")
        poor = ((sum(g[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)) + 4) // 9).astype(np.uint8)
    flat = np.full((h, w), 77, np.uint8)
    O.set_orb_order(mode)
    want = {id(x): O.orb_detect(x) for x in (rich, rich2, poor, flat)}
    c = Context(device=0, max_w=w, max_h=h, max_features=500, max_frames=2)
    try:
        order(c, mode)
        for seq in ([rich, rich2], [rich2, rich], [poor, poor], [rich, poor], [flat, rich], [rich, rich2], [poor, rich]):
            c.orb_detect_batch(dev(np.stack(seq)))
            c.synchronize()
            for f, img in enumerate(seq):
                o = want[id(img)]
                if len(o["xy"]) == 0:
                    assert c.lib.evh_orb_count(c.h, f) == 0
                    continue
                g = c.orb_download(f)
                assert np.array_equal(g["xy"], o["xy"]) and np.array_equal(g["desc"], o["desc"])
    finally:
        c.close()


@pytest.mark.parametrize("nfeat", [37, 137, 1000, 3000])
def test_other_key_point_budgets(nfeat):
    """ORB's per-level quotas, the select capacities and the match/RANSAC row capacities all derive from nfeatures:
    unusual budgets (tiny, odd, larger than the frame can deliver) must still reproduce the oracle."""
    from evenvizion_amd._lib import Context
    w, h = 640, 360
    a, b, _ = S.make_pair(300 + nfeat, w, h)
    fr = np.stack([a, b])
    c = Context(device=0, max_w=w, max_h=h, max_features=nfeat, max_frames=2)
    try:
        H = torch.zeros(1, 9, dtype=torch.float64, device="cuda")
        st = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        c.pair_homography_batch(dev(fr), 1, 0, H, st, nfeatures=nfeat)
        c.synchronize()
        for f in range(2):
            o = O.orb_detect(fr[f], nfeatures=nfeat); g = c.orb_download(f)
            assert np.array_equal(g["xy"], o["xy"]) and np.array_equal(g["desc"], o["desc"])
        Ho, so = O.pairs_gray_batch(fr, nfeatures=nfeat)
        assert st.cpu().numpy()[0] == so[0]
        if so[0] == 0:
            assert np.allclose(H.cpu().numpy().reshape(3, 3), Ho[0], rtol=1e-9, atol=1e-12)
    finally:
        c.close()


# ---- long streams --------------------------------------------------------------------------------
def test_long_pan_stream_600_frames_chunked():
    """BASELINE configs[2] is a 10 001-frame stream; the regime it adds to the short-stream tests is the running
    superposition drifting far from the origin (utils.py:351-355: both point sets are mapped through H_sup in f64,
    then cast to fp32 inside findHomography) and {H_sup, H_prev} carried across dozens of chunks with
    state_in == state_out.  600 frames at 400x224 panning 6 px per frame (H_sup translates by > 2000 px), two flat
    frames mid-stream (status 1, H repeated), through get_homography_dict(chunk_frames=17) AND through
    evh_stream_homography_batch in 23-frame chunks: statuses equal and H equal to the oracle's sequential stream."""
    from evenvizion_amd._lib import Context
    from evenvizion_amd.processing import get_homography_dict, superposition_dict
    w, h, n = 400, 224, 600
    frames = S.make_pan_stream(71, n, w, h, step=6.0)
    frames[301] = 90; frames[302] = 90                    # two flat frames: pairs 300..302 fail, the scan carries on
    Ho, so, rc = O.stream_gray(frames)
    assert rc == -1 and list(so[300:303]) == [1, 1, 1] and (so == 0).sum() >= n - 1 - 3 - 5
    # (1) the Python stream driver, chunked + double-buffered
    d = get_homography_dict(S.SyntheticCapture([S.gray_to_bgr(f) for f in frames]), resize_width=w, chunk_frames=17,
                            features_type_list=["ORB"])
    assert d["resize_info"] == {"h": h, "w": w} and sorted(k for k in d if k != "resize_info") == list(range(2, n + 1))
    Hd = np.array([d[k]["H"] for k in range(2, n + 1)])
    assert np.allclose(Hd, Ho, rtol=1e-9, atol=1e-12)
    sup = superposition_dict({k: d[k] for k in range(2, n + 1)})
    assert abs(sup[n][0][2]) > 2000                        # the fixed plane really is > 2000 px away by the end
    # failed pairs repeat the previous H (video_processing.py:94-98)
    assert np.array_equal(Hd[300], Hd[299]) and np.array_equal(Hd[302], Hd[299])
    # (2) the C-ABI stream entry in chunks, the state tensor aliased in and out
    c = Context(device=0, max_w=w, max_h=h, max_features=500, max_frames=23)
    try:
        state = torch.zeros(18, dtype=torch.float64, device="cuda")
        Hs, sts, k0 = [], [], 0
        dfr = dev(frames)
        while k0 < n - 1:
            k1 = min(k0 + 23, n)
            m = k1 - k0 - 1
            H = torch.zeros(m, 9, dtype=torch.float64, device="cuda")
            st = torch.full((m,), -1, dtype=torch.int32, device="cuda")
            c.stream_homography_batch(dfr[k0:k1], H, st, state_in=state if k0 else None, state_out=state)
            c.synchronize()
            Hs.append(H.cpu().numpy()); sts.append(st.cpu().numpy())
            k0 = k1 - 1
        Hc = np.concatenate(Hs).reshape(-1, 3, 3); sc = np.concatenate(sts)
        assert np.array_equal(sc, so)
        assert np.array_equal(Hc, Hd)                      # both device routes agree bit for bit
        for p in range(n - 1):
            assert h_err(Hc[p], Ho[p]) <= 1e-3
    finally:
        c.close()


def test_tie_heavy_frame_mid_stream_reruns_on_larger_slots():
    """A frame with more tied key points than a frame slot holds (EVH_PAIR_CAPACITY) no longer aborts the video
    (VERDICT r2): get_homography_dict re-runs that chunk from its saved entry state on a context with doubled frame
    slots and carries on, like the reference does (frame_processing.py:59-61 keeps every tie).  Result == oracle."""
    from evenvizion_amd.processing import get_homography_dict
    w, h = 400, 224
    fr, _ = S.make_stream(13, 12, w, h)
    crowded = [_dots(h, w, 8), _dots(h, w, 8, (2, 1))]
    frames = np.stack(list(fr[:5]) + crowded + list(fr[5:]))
    assert len(O.orb_detect(crowded[0])["xy"]) > 832       # evh_orb_capacity() for nfeatures = 500
    Ho, so, rc = O.stream_gray(frames)
    assert rc == -1
    for chunk in (4, 64):
        d = get_homography_dict(S.SyntheticCapture([S.gray_to_bgr(f) for f in frames]), resize_width=w, chunk_frames=chunk,
                                features_type_list=["ORB"])
        Hd = np.array([d[k]["H"] for k in range(2, len(frames) + 1)])
        assert np.allclose(Hd, Ho, rtol=1e-9, atol=1e-12), chunk


def test_fast_solver_mode():
    """EVH_SOLVER_FAST (include/evhip.h): LM's 8x8 systems by LDL^T instead of the operator's Jacobi eigen-solve, and the sums of
    the refit and of the LM evaluations by partial sums + a tree instead of the operator's point order.  The draw and the masks
    are untouched, so statuses must be identical.  What can be asked of H, measured before the bars below
    were written: findHomography refines on raw pixel coordinates, so J^T J is graded over 14 orders of magnitude (the
    oracle's eigen-solves on this stream: smallest eigenvalue = 5 x the truncation threshold 2 eps trace); along its weakest
    direction ANY two solvers differ in the leading digits of the step, LM is cut off after 10 iterations, and the end points
    differ where the data do not determine H: corners up to 6e-4 px, the perspective row 4e-9 absolute, SURVEY 8d's
    floored-relative h_err 3.6e-3 (exact mode: 1e-9).  So the fast mode is NOT inside the north-star's 1e-3 on every pair --
    it is an opt-in for callers who care about the geometry (sub-milli-pixel) rather than about OpenCV's digits; the default
    stays exact.  Bars: corners 5e-3 px, perspective row 1e-7, affine part 1e-2 floored-relative, h_err 2e-2."""
    from evenvizion_amd._lib import Context, SOLVER_EXACT, SOLVER_FAST
    seen = {"h_err": 0.0, "corner": 0.0, "abs": 0.0, "aff_rel": 0.0, "pairs": 0}

    def check(Hg, Hw, status, w, h):
        for p in range(len(status)):
            if status[p] != 0:
                continue
            seen["pairs"] += 1
            seen["h_err"] = max(seen["h_err"], h_err(Hg[p], Hw[p]))
            seen["corner"] = max(seen["corner"], corner_err(Hg[p], Hw[p], w, h))
            seen["abs"] = max(seen["abs"], float(np.abs(Hg[p][2, :2] - Hw[p][2, :2]).max()))
            seen["aff_rel"] = max(seen["aff_rel"], float((np.abs(Hg[p][:2] - Hw[p][:2]) / np.maximum(np.abs(Hw[p][:2]), [[1e-3, 1e-3, 1.0]] * 2)).max()))

    frames, _ = S.make_pair_batch(4, 6, 400, 224)
    Ho, so = O.pairs_gray_batch(frames)
    c = Context(device=0, max_w=400, max_h=224, max_features=500, max_frames=64)
    try:
        assert c.get_solver_mode() == SOLVER_EXACT
        c.set_solver_mode(SOLVER_FAST)
        H = torch.zeros(6, 9, dtype=torch.float64, device="cuda"); st = torch.full((6,), -1, dtype=torch.int32, device="cuda")
        c.pair_homography_batch(dev(frames), 6, 0, H, st)
        c.synchronize()
        assert np.array_equal(st.cpu().numpy(), so)
        check(H.cpu().numpy().reshape(-1, 3, 3), Ho, so, 400, 224)
        pan = S.make_pan_stream(71, 61, 400, 224, step=6.0)
        for force in (False, True):
            Hs, ss, rc = O.stream_gray(pan, force_max_iters=force)
            H = torch.zeros(60, 9, dtype=torch.float64, device="cuda"); st = torch.full((60,), -1, dtype=torch.int32, device="cuda")
            c.stream_homography_batch(dev(pan), H, st, force_max_iters=force)
            c.synchronize()
            assert rc == -1 and np.array_equal(st.cpu().numpy(), ss), force
            check(H.cpu().numpy().reshape(-1, 3, 3), Hs, ss, 400, 224)
    finally:
        c.close()
    fr, _ = S.make_stream(12, 7, 1280, 720)
    Hs, ss, rc = O.stream_gray(fr, nfeatures=2000)
    c = Context(device=0, max_w=1280, max_h=720, max_features=2000, max_frames=8)
    try:
        c.set_solver_mode(SOLVER_FAST)
        H = torch.zeros(6, 9, dtype=torch.float64, device="cuda"); st = torch.full((6,), -1, dtype=torch.int32, device="cuda")
        c.stream_homography_batch(dev(fr), H, st, nfeatures=2000)
        c.synchronize()
        assert np.array_equal(st.cpu().numpy(), ss)
        check(H.cpu().numpy().reshape(-1, 3, 3), Hs, ss, 1280, 720)
    finally:
        c.close()
    # the reference's default detector list (SURF, SIFT, ORB): ~1 900 merged rows per pair -- where the tree-reduced sums of the
    # tolerance mode (lm_eval_fast, dlt_rows_fast) replace the longest point-order chains
    fr3, _ = S.make_stream(31, 9, 400, 224)
    Hs, ss, rc = O.stream_gray_types(fr3, ["SURF", "SIFT", "ORB"])
    c = Context(device=0, max_w=400, max_h=224, max_features=500, max_frames=len(fr3))
    try:
        c.sift_enable(6144); c.surf_enable(4096)
        c.set_solver_mode(SOLVER_FAST)
        H = torch.zeros(len(fr3) - 1, 9, dtype=torch.float64, device="cuda"); st = torch.full((len(fr3) - 1,), -1, dtype=torch.int32, device="cuda")
        c.stream_homography_batch_types(dev(S.gray_to_bgr(fr3)), H, st, ["SURF", "SIFT", "ORB"])
        c.synchronize()
        assert rc == -1 and np.array_equal(st.cpu().numpy(), ss)
        check(H.cpu().numpy().reshape(-1, 3, 3), Hs, ss, 400, 224)
    finally:
        c.close()
    print("fast solver against the oracle over %(pairs)d pairs: h_err %(h_err).2e, corners %(corner).2e px, perspective row %(abs).2e "
          "absolute, affine part %(aff_rel).2e relative" % seen)
    assert seen["corner"] <= BAR_CORNER and seen["abs"] <= BAR_ABS and seen["aff_rel"] <= BAR_AFF and seen["h_err"] <= BAR_HERR, seen


BAR_CORNER, BAR_ABS, BAR_AFF, BAR_HERR = 5e-3, 1e-7, 1e-2, 2e-2
