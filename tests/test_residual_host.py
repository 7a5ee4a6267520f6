"""The host side of the registration score: the numpy restatement of evh_pair_residual (tests/residual_checks.py) against plain
differences, registration.pair_maps against the recorded dictionary, the report's formulas, the refusals, and the measure itself
on the reference's video with the matrices its authors recorded.  No GPU: the device is held to residual_checks in
test_gpu_residual.py."""
import math
import os

import numpy as np
import pytest

import residual_checks as R
import warp_checks as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MP4 = os.path.join(ROOT, "tests", "golden", "ref_test_video.mp4")
GOLD = os.path.join(ROOT, "tests", "golden", "ref_dict_with_homography_matrix.json")


def frames_of(seed, n, w, h, gray=False):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w) if gray else (n, h, w, 3), dtype=np.uint8)


def host_superposition(hd):
    """utils.superposition_dict in numpy (the product's own runs its scan on the device): S_1 = I, S_k = H_k . S_{k-1} / [2][2];
    a None H keeps the running matrix."""
    sup = {1: np.eye(3)}
    S = np.eye(3)
    for k, v in hd.items():
        if v["H"] is not None:
            S = np.dot(np.asarray(v["H"], np.float64), S)
            S = S / S[2, 2]
        sup[k] = S
    return sup


@pytest.fixture(scope="module")
def recorded():
    from evenvizion_amd.processing.utils import read_homography_dict
    hd, ri = read_homography_dict(GOLD)
    assert len(hd) == 120 and ri == {"h": 224, "w": 400}
    return hd, host_superposition(hd)


# ---- the restatement against plain differences ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("gray", [False, True])
def test_identity_is_the_plain_difference(gray):
    f = frames_of(61, 2, 13, 11, gray)
    stats, pic, mask = R.residual(f[0], f[1], np.eye(3), threshold=40)
    d = np.abs(R.gray_of(f[1]).astype(int) - R.gray_of(f[0]).astype(int))
    assert stats[R.COVERED] == 13 * 11
    assert stats[R.SAD] == stats[R.SAD0] == d.sum() and stats[R.SSD] == stats[R.SSD0] == (d * d).sum()
    assert stats[R.MOVING] == (d > 40).sum() and 0 < stats[R.MOVING] < 13 * 11
    assert np.array_equal(pic, d) and np.array_equal(mask, np.where(d > 40, 255, 0))
    assert all(type(v) is int for v in stats)
    if not gray:                                                         # the weights by hand on one pixel
        b, g, r = (int(v) for v in f[0, 3, 5])
        assert R.gray_of(f[0])[3, 5] == (b * 1868 + g * 9617 + r * 4899 + 8192) >> 14


@pytest.mark.parametrize("shift", [(3, 2), (-4, 1), (0, -5), (12, 0)])
def test_integer_translation_is_the_shifted_difference_over_the_overlap(shift):
    dx, dy = shift
    w, h = 13, 11
    f = frames_of(62, 2, w, h)
    stats, pic, _ = R.residual(f[0], f[1], W.translation(dx, dy))           # current (x, y) -> previous (x + dx, y + dy)
    gp, gc = R.gray_of(f[0]).astype(int), R.gray_of(f[1]).astype(int)
    x0, x1, y0, y1 = max(0, -dx), min(w, w - dx), max(0, -dy), min(h, h - dy)
    d = np.abs(gc[y0:y1, x0:x1] - gp[y0 + dy:y1 + dy, x0 + dx:x1 + dx])
    d0 = np.abs(gc[y0:y1, x0:x1] - gp[y0:y1, x0:x1])
    assert stats[:5] == ((x1 - x0) * (y1 - y0), d.sum(), (d * d).sum(), d0.sum(), (d0 * d0).sum())
    want = np.zeros((h, w), np.uint8)
    want[y0:y1, x0:x1] = d
    assert np.array_equal(pic, want)


def test_nothing_covered_gives_six_zeros():
    f = frames_of(63, 2, 9, 7)
    # the singular one has tw = 0 everywhere; a singular matrix with tw != 0 sends every pixel to one point and may cover
    for M in (np.full((3, 3), np.nan), np.zeros((3, 3)), np.array([[1, 2, 3], [2, 4, 6], [0, 0, 0]], np.float64)):
        stats, pic, mask = R.residual(f[0], f[1], M)
        assert stats == (0, 0, 0, 0, 0, 0) and not pic.any() and not mask.any()
    one_point = np.outer([1.0, 2.0, 0.5], [3.0, -1.0, 2.0])              # every pixel -> (2, 4) of the previous frame
    stats, pic, _ = R.residual(f[0], f[1], one_point)
    g = R.gray_of(f).astype(int)
    assert stats[R.COVERED] > 0 and np.array_equal(pic[pic > 0], np.abs(g[1] - g[0, 4, 2])[pic > 0])


# ---- pair_maps -----------------------------------------------------------------------------------------------------------------------
def test_pair_maps_recompose_the_recorded_superposition(recorded):
    """S_{k-1} . M_k = S_k relative to S_k's largest entry.  What float64 solve leaves, measured over the 120 recorded pairs:
    worst 1.396e-16 (under one unit of 2^-52); the margin is 8 times that, 1.117e-15."""
    from evenvizion_amd.registration import pair_maps
    _, sup = recorded
    maps = pair_maps(sup)
    keys = list(sup)
    assert list(maps) == keys[1:] == list(range(2, 122))
    worst = 0.0
    for k0, k1 in zip(keys, keys[1:]):
        assert maps[k1].shape == (3, 3) and maps[k1].dtype == np.float64
        worst = max(worst, np.abs(np.dot(sup[k0], maps[k1]) - sup[k1]).max() / np.abs(sup[k1]).max())
    print("pair_maps: worst relative residual of S_{k-1} . M_k - S_k over 120 pairs: %.3e" % worst)
    assert worst <= 1.117e-15


def test_pair_maps_gives_nan_for_what_cannot_be_inverted():
    from evenvizion_amd.registration import pair_maps
    good = np.array([[1.0, 0.1, 3], [0, 1.1, -2], [1e-4, 0, 1]])
    one_nan = good.copy()
    one_nan[1, 1] = np.nan
    bad = {"none": None, "nan": one_nan, "inf": np.full((3, 3), np.inf), "zero": np.zeros((3, 3)),
           "rank2": np.array([[1, 2, 3], [2, 4, 6], [1, 1, 1]], np.float64), "short": [1.0, 2.0]}
    for name, B in bad.items():
        maps = pair_maps({1: good, 2: B, 3: good.tolist(), 4: good})
        assert list(maps) == [2, 3, 4]
        assert np.isnan(maps[2]).all() and np.isnan(maps[3]).all(), name       # either side of the pair
        assert np.allclose(maps[4], np.eye(3), atol=1e-15), name
    assert pair_maps({}) == {} and pair_maps({7: good}) == {}
    keyed = pair_maps({"resize_info": {"w": 4, "h": 4}, 5: good, 9: good})       # the dictionary's order, whatever the keys
    assert list(keyed) == [9]


# ---- the report ----------------------------------------------------------------------------------------------------------------------
def test_report_formulas_from_hand_made_stats():
    from evenvizion_amd.registration import report_from_stats
    stats = {2: (100, 500, 6502, 900, 65025, 7),          # psnr 10 log10(65025 * 100 / 6502), unregistered 20 dB
             3: (50, 0, 0, 10, 100, 0),                   # ssd == 0: inf
             4: (0, 0, 0, 0, 0, 0),                       # nothing covered: None
             5: (200, 400, 130050, 300, 13005, 90)}       # registered 20 dB, unregistered 30 dB: the matrix made it worse
    rep = report_from_stats(stats)
    f = rep["frames"]
    assert list(f) == [2, 3, 4, 5]
    assert f[2] == dict(covered=100, sad=500, ssd=6502, sad_unregistered=900, ssd_unregistered=65025, moving=7,
                        psnr=10 * math.log10(65025 * 100 / 6502), psnr_unregistered=20.0)
    assert abs(f[2]["psnr"] - 30.000334) < 1e-6
    assert f[3]["psnr"] == math.inf and f[3]["psnr_unregistered"] == 10 * math.log10(65025 * 50 / 100)
    assert f[4]["psnr"] is None and f[4]["psnr_unregistered"] is None and f[4]["covered"] == 0
    assert abs(f[5]["psnr"] - 20.0) < 1e-12 and abs(f[5]["psnr_unregistered"] - 30.0) < 1e-12
    assert abs(rep["itf"] - (f[2]["psnr"] + f[5]["psnr"]) / 2) < 1e-12                          # the finite ones only
    assert abs(rep["itf_unregistered"] - (20.0 + f[3]["psnr_unregistered"] + 30.0) / 3) < 1e-12
    assert rep["worst"] == [4, 5, 2, 3]                  # no score, -10 dB, +10 dB, +inf
    empty = report_from_stats({})
    assert empty == {"frames": {}, "itf": None, "itf_unregistered": None, "worst": []}
    assert report_from_stats({9: (5, 0, 0, 0, 0, 0)})["worst"] == [9]                          # inf against inf: a gain of 0


class NeverRead:
    def __getattr__(self, name):
        raise AssertionError("the capture was touched: %s" % name)


@pytest.mark.parametrize("bad", [dict(ingest="rgb"), dict(threshold=-1), dict(threshold=256), dict(threshold=1.5), dict(chunk_frames=0),
                                 dict(chunk_frames=2.5), dict(resize_info={"w": 0, "h": 4}), dict(resize_info={"w": 4, "h": -1}),
                                 dict(kind="sum")])
def test_drivers_refuse_bad_arguments_before_anything_is_opened(bad, monkeypatch):
    from evenvizion_amd import registration, runtime

    def no_context(*a, **k):
        raise AssertionError("a context was opened")

    monkeypatch.setattr(runtime, "get_context", no_context)
    kw = dict(resize_info={"w": 8, "h": 4})
    kw.update(bad)
    ri = kw.pop("resize_info")
    sup = {1: np.eye(3), 2: np.eye(3)}
    with pytest.raises(ValueError):
        registration.residual_frames(NeverRead(), sup, ri, **kw)
    if "kind" not in bad:
        with pytest.raises(ValueError):
            registration.registration_report(NeverRead(), sup, ri, **kw)


# ---- the measure on the reference's video --------------------------------------------------------------------------------------------
def test_recorded_matrices_register_the_reference_video(recorded):
    """The reference's test_video.mp4 decoded by libevcap, frames cut to 400x224 by nearest-neighbour subsampling, its recorded
    dictionary: with M_k the registered SSD lies below the unregistered one on at least 114 of 120 pairs (measured: 120 of 120,
    worst ratio 0.716); with H_k in place of M_k on fewer than 90 (measured: 56), so a wrong composition is noticed."""
    from evenvizion_amd import capture
    from evenvizion_amd.registration import pair_maps
    hd, sup = recorded
    maps = pair_maps(sup)
    cap = capture.VideoCapture(MP4)
    assert cap.isOpened()
    ys, xs = (np.arange(224) * 658) // 224, (np.arange(400) * 1170) // 400
    prev, better, better_h, ratios, nos = None, 0, 0, [], []
    for no in sup:
        ok, frame = cap.read()
        assert ok, no
        cur = np.ascontiguousarray(frame[ys][:, xs])
        if prev is not None:
            s = R.residual(prev, cur, maps[no])[0]
            sh = R.residual(prev, cur, np.asarray(hd[no]["H"], np.float64))[0]
            assert 2 * s[R.COVERED] > 400 * 224          # a score over less than half the frame would not be the frame's (measured: 96.5 % at least)
            better += s[R.SSD] < s[R.SSD0]
            better_h += sh[R.SSD] < sh[R.SSD0]
            ratios.append(s[R.SSD] / s[R.SSD0])
            nos.append(no)
        prev = cur
    cap.release()
    print("M_k: registered below unregistered on %d of %d pairs, ratio median %.3f worst %.3f at frame %d; H_k: %d of %d"
          % (better, len(ratios), np.median(ratios), max(ratios), nos[int(np.argmax(ratios))], better_h, len(ratios)))
    assert len(ratios) == 120
    assert better >= 114
    assert better_h < 90
