"""CPU: the oracle's SURF (oracle/evz_surf.cpp: integral, Hessian layers, maxima and fit, deletion, orientation, descriptor, order)
held to the plain float64 restatement of tests/surf_checks.py on the crafted frames of tests/surf_families.py.  The device is held
to the oracle, bit for bit, and to the same restatement in tests/test_gpu_surf_edges.py; a mistake the oracle and the kernels
share shows here.  The oracle's threshold is fixed at 400; other thresholds are judged on the device alone."""
from fractions import Fraction

import numpy as np
import pytest

import sift_checks
import surf_checks as S
import surf_families as F
from oracle import oracle as O

NAMES = sorted(F.FRAMES)


@pytest.fixture(scope="module")
def detected():
    return {n: O.surf_detect(F.FRAMES[n]) for n in NAMES}


def test_restatement_on_hand_made_cases():
    """the restatement's own pieces on inputs whose answer is known by hand"""
    assert S.ANGLE_BOUND == sift_checks.ANGLE_BOUND == 2 * 0.009552
    assert [(o, l, s, st) for o, l, s, st in S.layers()][::5] == [(0, 0, 9, 1), (1, 0, 18, 2), (2, 0, 36, 4), (3, 0, 72, 8)]
    assert S.layers()[19] == (3, 4, 264, 8)
    # the 9 x 9 pattern at size 15: stripes of 5 x 9
    assert S.scaled_boxes(S.DXX, 9, 15) == [(0, 3, 5, 12, Fraction(1, 45)), (5, 3, 10, 12, Fraction(-2, 45)), (10, 3, 15, 12, Fraction(1, 45))]
    assert S.scaled_boxes(S.GRAD_X, 4, 6) == [(0, 0, 3, 6, Fraction(-1, 18)), (3, 0, 6, 6, Fraction(1, 18))]
    img = np.arange(12, dtype=np.uint8).reshape(3, 4)
    assert S.integral(img)[3, 4] == 66 and S.integral(img)[2, 2] == 0 + 1 + 4 + 5 and not S.integral(img)[0].any()
    # a frame of one value: every Haar value is zero (the weights of a pattern sum to zero)
    flat = S.hessian(np.full((40, 40), 77, np.uint8))
    assert all(np.abs(L["det"]).max() < 1e-9 for L in flat) and [L["built"] for L in flat[:6]] == [True] * 5 + [True]
    assert not flat[7]["built"] and flat[6]["built"]                   # octave 1: 18, 30 fit into 40, 42 does not
    # windows: sizes 15 and 30 are the integer ratios 2 and 4, 46 and 47 lie either side of 128
    assert [S.scalars(v)[2] for v in (9, 15, 30, 46, 47, 264)] == [25, 42, 84, 128, 131, 739]
    assert [S.scalars(v)[1] for v in (9, 15, 264)] == [4, 8, 140]
    for win in (25, 43, 131, 669):
        Wm = S._area_weights(win)
        assert np.allclose(Wm.sum(1), 1.0) and np.allclose(Wm.sum(0), 21.0 / win)
    # the order: response, size, octave descending, y descending, x ascending
    recs = [(5.0, 1.0, 20.0, 900.0, 1), (4.0, 1.0, 20.0, 900.0, 1), (4.0, 2.0, 20.0, 900.0, 1), (0.0, 0.0, 20.0, 900.0, 2),
            (0.0, 0.0, 21.0, 900.0, 0), (0.0, 0.0, 9.0, 901.0, 0)]
    keys = [S.order_key(*r) for r in recs]
    assert sorted(keys) == keys[::-1]
    # a ramp: gradient along +x, the orientation is 0 (atan2(-0, +)); along +y (down the image) it is 90
    ramp = np.tile(np.arange(80, dtype=np.uint8) * 3, (80, 1))
    o = S.orientation(S.integral(ramp), np.float32(40), np.float32(40), 20.0)
    assert o["nangle"] == 113 and (o["angle"] < 1e-6 or o["angle"] > 360 - 1e-6)
    o = S.orientation(S.integral(ramp.T.copy()), np.float32(40), np.float32(40), 20.0)
    assert abs(o["angle"] - 90.0) < 1e-6
    assert S.deleted(np.float32(2), np.float32(2), 100.0, (30, 30)) and not S.deleted(np.float32(40), np.float32(40), 20.0, (80, 80))


@pytest.mark.parametrize("fam", sorted(F.FAMILIES))
def test_frames_are_what_the_family_says(fam):
    print("%s: %s" % (fam, F.check_premise(fam)))


@pytest.mark.parametrize("name", NAMES)
def test_integral_is_the_cumulative_sum(name):
    img = F.FRAMES[name]
    want = np.zeros((img.shape[0] + 1, img.shape[1] + 1))
    want[1:, 1:] = img.astype(np.float64).cumsum(0).cumsum(1)
    got = O.integral(img)
    assert got.dtype == np.int32 and np.array_equal(got.astype(np.float64), want)
    assert np.array_equal(S.integral(img), got)


@pytest.mark.parametrize("name", NAMES)
def test_keypoints_against_the_plain_restatement(detected, name):
    fig = S.check_keypoints(F.FRAMES[name], detected[name], 400.0, name)
    print("%s: %s" % (name, fig))
    if name in F.NONE:
        assert len(detected[name]["xy"]) == 0


@pytest.mark.parametrize("name", NAMES)
def test_descriptors_against_the_plain_restatement(detected, name):
    kp = detected[name]
    fig = S.check_descriptors(F.FRAMES[name], kp, name)
    print("%s: %s" % (name, fig))
    assert fig["checked"] + fig["undecided"] == len(kp["xy"]) and fig["undecided"] <= 0.1 * max(fig["checked"], 1)


def test_every_window_class_is_described(detected):
    """the oracle's own records reach the identity-free classes of the area average: ratio 2, a larger integer ratio, general
    ratios below and above 128, and a window larger than its frame"""
    wins = set()
    for n in NAMES:
        h, w = F.FRAMES[n].shape
        for v in detected[n]["size"]:
            win = S.scalars(float(v))[2]
            wins.add(win)
            wins.add("larger" if win > max(h, w) else "fits")
    assert {42, 84, 128, 131, "larger"} <= wins and 21 not in wins and min(v for v in wins if isinstance(v, int)) >= 25


def test_paths_no_emitted_size_reaches():
    """the branches of the describe stage that no emitted key point can take, from the restatement's arithmetic: a fit accepts
    |x_2| <= 1, so a key point of middle layer (octave, layer) has a size within one layer step of its layer's.  Over all of them:
      * the window side int(21 s) runs from 25 to 739: never the identity 21, never below 1 or above 768;
      * the wavelet side g is at most the smallest frame side that admits a sample of that layer, plus one: `srows < g` is false;
      * the centre sample (offset 0, 0) of the 113 is inside for every admissible sample and every accepted fit: nangle >= 1.
    So the deletion test deletes nothing the detector emits, and a raw list cannot overflow alone."""
    wins = set()
    for o in range(S.OCTAVES):
        for l in range(1, S.LAYERS + 1):
            step = 1 << o
            size, ds, above = (9 + 6 * l) << o, 6 << o, (9 + 6 * (l + 1)) << o
            mg, m = (above // 2) // step + 1, (size // 2) // step
            side = (2 * mg + 1) * step                    # rows - 2 mg >= 1 with rows = side / step
            for v in range(size - ds, size + ds + 1):
                _, g, win, _ = S.scalars(v)
                wins.add(win)
                assert side + 1 >= g
                # the point lies within one step of the pattern's centre; the corner of its centre wavelet is
                # round(c - (g - 1) / 2), at the least for the first admissible sample, at the most for the last (there counted
                # from step * rows <= the frame's side)
                lo = step * (mg - m) + (size - 1) / 2 - step - (g - 1) / 2 - 0.5
                hi = step * (-mg - 1 - m) + (size - 1) / 2 + step - (g - 1) / 2 + 0.5
                assert lo >= 0 and hi < 1 - g, (o, l, v, g, lo, hi)
    assert min(wins) == 25 and max(wins) == 739 and 21 not in wins


def test_nothing_is_deleted_on_these_frames():
    """the figure behind leaving out the test of a raw list that overflows alone: the restatement deletes no key point of any frame"""
    assert sum(1 for n in NAMES for q in S.keypoints(F.FRAMES[n]) if q["deleted"]) == 0
