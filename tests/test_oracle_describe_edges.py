"""CPU: the oracle's describe stage (oracle/evz_orb.cpp: harris_response, ic_angle, evo_gaussian_blur7, the steered tests of
evo_orb_detect) held to the plain restatement of tests/describe_checks.py on the crafted frames of tests/describe_families.py.
The device is held to the oracle, bit for bit, and to the same restatement in tests/test_gpu_describe_edges.py; a mistake the
oracle and the kernel share shows here."""
import numpy as np
import pytest

import describe_checks as D
import describe_families as F
from oracle import oracle as O

NAMES = sorted(F.FRAMES)
# the float32 tail of the Harris response against float64, relative to max(|r|, smallest |response| kept in the family):
# the largest error measured on family H is 1.4144e-5 (3.3e-7 on the others); twice that
RESPONSE_BOUND = 2 * 1.4144e-5


def keypoints(name):
    k = F.info(name)["kp"]
    return list(zip(k["octave"].tolist(), k["lx"].tolist(), k["ly"].tolist()))


def test_restatement_is_the_documented_filter_and_disc():
    assert D.gauss_taps().tolist() == [18, 34, 49, 55, 49, 34, 18]
    assert D.DISC == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]      # the published half-widths of the 31-pixel patch
    b, c = D.blur7_u8(np.full((20, 20), 255, np.uint8))
    assert (b == 255).all() and c.all()
    b, c = D.blur7_u8(np.full((20, 20), 253, np.uint8))
    assert (b == 255).all() and not c.any()


@pytest.mark.parametrize("fam", sorted(F.FAMILIES))
def test_frames_are_what_the_family_says(fam):
    print("%s: %s" % (fam, F.check_premise(fam)))


@pytest.mark.parametrize("fam", sorted(F.FAMILIES))
def test_half_integer_taps_stay_rare(fam):
    """by the plain restatement alone: at most 0.5 % of a family's taps lie within 1e-4 of a half-integer"""
    near = [F.half_integer_share(n) for n in F.FAMILIES[fam]]
    n, total = sum(a for a, _ in near), sum(b for _, b in near)
    print("%s: %d of %d tests near a half-integer" % (fam, n, total))
    assert total > 0 and n <= 0.005 * total, (fam, n, total)


@pytest.mark.parametrize("name", NAMES)
def test_blur_of_every_level(name):
    """byte for byte; with a plain byte cast in place of the saturating store the S frames with 254 / 255 fail here (the
    wrapped bytes are 0 and 1 where 255 belongs)"""
    i = F.info(name)
    for l, lv in enumerate(i["pyr"]):
        got = O.gaussian_blur7(lv)
        diff = int((got != i["blur"][l]).sum())
        assert diff == 0, "%s level %d: %d bytes differ, %d pixels clipped" % (name, l, diff, int(i["clipped"][l].sum()))


def test_fast_atan2_error_is_the_polynomials():
    """Measured: 0.009552 degrees at the worst over 200 001 ratios in [0, 1] on both branches and in all four quadrants, and
    0.009552 over the families' own moments (test_angles); D.ANGLE_BOUND is twice that.  The error belongs to the degree-7
    polynomial in the ratio, so a coarser sweep of the ratio sees the same maximum: 20 001 ratios here."""
    worst = 0.0
    for t in np.linspace(0.0, 1.0, 20001):
        for y, x in ((t * 1e5, 1e5), (1e5, t * 1e5)):
            y, x = float(np.float32(y)), float(np.float32(x))
            for sy, sx in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
                if (y == 0 and sy < 0) or (x == 0 and sx < 0):
                    continue
                e = abs(O.fast_atan2(sy * y, sx * x) - D.angle_exact(sx * x, sy * y))
                worst = max(worst, min(e, 360.0 - e))
    print("largest error of fast_atan2 over the sweep: %.6f degrees" % worst)
    assert 0.009 <= worst <= D.ANGLE_BOUND        # the sweep does reach the polynomial's maximum
    for y, x, want in ((0, 0, 0.0), (0, 5, 0.0), (7, 0, 90.0), (0, -3, 180.0), (-2, 0, 270.0)):
        assert O.fast_atan2(y, x) == want


@pytest.mark.parametrize("name", NAMES)
def test_angles(name):
    i = F.info(name)
    worst = D.check_angles(i["kp"]["angle"], i["mom"], name)
    print("%s: largest angle error %.6f degrees on %d key points" % (name, worst, len(i["mom"])))


@pytest.mark.parametrize("name", NAMES)
def test_descriptors_float32_rotation(name):
    """all 256 bits of every key point, taps rotated in float32 one operation at a time and read from the plain blur"""
    i = F.info(name)
    k = i["kp"]
    for j, (l, x, y) in enumerate(keypoints(name)):
        want = D.brief_bits(i["blur"][l], x, y, k["angle"][j])[0]
        assert np.array_equal(k["desc"][j], want), "%s key point %d (level %d, %d, %d): %d bits differ" % (
            name, j, l, x, y, int(D.unpack_bits(k["desc"][j] ^ want).sum()))


@pytest.mark.parametrize("name", NAMES)
def test_descriptors_float64_rotation(name):
    """every bit whose taps are not within 1e-4 of a half-integer in float64"""
    i = F.info(name)
    k = i["kp"]
    for j, (l, x, y) in enumerate(keypoints(name)):
        _, want, near = D.brief_bits(i["blur"][l], x, y, k["angle"][j])
        bad = (D.unpack_bits(k["desc"][j] ^ want) != 0) & ~near
        assert not bad.any(), "%s key point %d: tests %s differ" % (name, j, np.nonzero(bad)[0].tolist())


@pytest.mark.parametrize("fam", sorted(F.FAMILIES))
def test_harris_response(fam):
    """Measured on H (gradient sums up to 5e7, products near 2e15, where (float)a is inexact): 1.4144e-5 of
    max(|r|, r_floor) at the worst; 3.3e-7 on the other families.  RESPONSE_BOUND is twice the former."""
    got, want = [], []
    for n in F.FAMILIES[fam]:
        i = F.info(n)
        got.append(i["kp"]["response"].astype(np.float64))
        want.append(np.array([D.harris_f64(i["pyr"][l], x, y) for l, x, y in keypoints(n)]))
    got, want = np.concatenate(got), np.concatenate(want)
    floor = np.abs(got).min()
    assert floor > 0
    scale = np.maximum(np.abs(want), floor)
    rel = np.abs(got - want) / scale
    print("%s: r_floor %.4g, largest error %.4g of max(|r|, r_floor), %d negative" % (fam, floor, rel.max(), int((want < 0).sum())))
    assert rel.max() <= RESPONSE_BOUND, (fam, rel.max())
    sure = np.abs(want) > RESPONSE_BOUND * scale
    assert np.array_equal(np.sign(got[sure]), np.sign(want[sure]))
