"""CPU: the oracle's SIFT stages after the scale space (oracle/evz_sift.cpp: find_extrema, adjust_local_extrema,
calc_orientation_hist, calc_descriptor, remove_duplicated_sorted) held to the plain float64 restatement of tests/sift_checks.py
on the crafted frames of tests/sift_families.py.  The device is held to the oracle, bit for bit, and to the same restatement in
tests/test_gpu_sift_edges.py; a mistake the oracle and the kernels share shows here."""
import ctypes
import math

import numpy as np
import pytest

import describe_checks as D
import sift_checks as S
import sift_families as F
from oracle import oracle as O

NAMES = sorted(F.FRAMES)


def test_fast_atan2_error_is_the_polynomials():
    """SIFT's gradients go through the same fastAtan2 as ORB's moments (evo_fast_atan2), so the bound is the one measured in
    tests/test_oracle_describe_edges.py: 0.009552 degrees at the worst, S.ANGLE_BOUND twice that.  Measured again here at the
    magnitudes of float gradients (ratios in [0, 1] on both branches, all quadrants, lengths 1e-3, 3.7 and 1e5)."""
    assert S.ANGLE_BOUND == D.ANGLE_BOUND
    worst = 0.0
    for scale in (1e-3, 3.7, 1e5):
        for t in np.linspace(0.0, 1.0, 5001):
            for y, x in ((t * scale, scale), (scale, t * scale)):
                y, x = float(np.float32(y)), float(np.float32(x))
                for sy, sx in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
                    if (y == 0 and sy < 0) or (x == 0 and sx < 0):
                        continue
                    want = math.degrees(math.atan2(sy * y, sx * x)) % 360.0
                    e = abs(O.fast_atan2(sy * y, sx * x) - want)
                    worst = max(worst, min(e, 360.0 - e))
    print("largest error of fast_atan2 over the sweep: %.6f degrees" % worst)
    assert 0.009 <= worst <= 0.009552 * 1.001 and 2 * worst <= S.ANGLE_BOUND * 1.001
    assert O.fast_atan2(0, 0) == 0.0                    # exactly flat ground: bin 0, weight 0


def test_exp32f_error_is_within_the_bound():
    """hal::exp32f over the exponents the weights use (0 down to -9 in the orientation window, -3.2 in the descriptor's, and
    beyond): relative error against math.exp of the float32 argument at most S.EXP_REL = 4e-7"""
    lib = O.lib()
    lib.evo_sift_exp32f.restype = ctypes.c_float
    lib.evo_sift_exp32f.argtypes = [ctypes.c_float]
    worst = 0.0
    for x in np.linspace(-12.0, 0.0, 24001):
        x = float(np.float32(x))
        worst = max(worst, abs(lib.evo_sift_exp32f(x) / math.exp(x) - 1.0))
    print("largest relative error of exp32f on [-12, 0]: %.3g" % worst)
    assert worst <= S.EXP_REL


def test_restatement_on_hand_made_cases():
    """the restatement's own pieces on inputs whose answer is known by hand"""
    # the final order: x, y, size descending, angle, response descending, octave descending; duplicates in (x, y, size, angle) go
    a = (1.0, 2.0, 3.0, 10.0, 0.5, 7)
    recs = [(1.0, 2.0, 3.0, 10.0, 0.25, 9), a, (1.0, 2.0, 4.0, 0.0, 0.1, 1), (0.5, 9.0, 1.0, 0.0, 0.1, 1), (1.0, 2.0, 3.0, 5.0, 0.1, 1)]
    assert S.final_order(recs) == [recs[3], recs[2], recs[4], a]
    assert S.unpack_octave(255 | 2 << 8 | 128 << 16) == (-1, 2, 128) and S.unpack_octave(3 | 1 << 8) == (3, 1, 0)
    # a quadratic D has its extremum where the fit says, in one step
    oct_ = np.zeros((6, 16, 16), np.float32)
    yy, xx = np.mgrid[0:16, 0:16]
    for l in range(6):
        oct_[l] = 0 if l == 0 else oct_[l - 1] + (60.0 - 2.0 * (xx - 8.25) ** 2 - 3.0 * (yy - 7.75) ** 2 - 5.0 * (l - 1 - 2.125) ** 2)
    fit = S.refine([oct_], [(0, 2, 8, 8)])[0]
    assert fit["status"] == "kp" and fit["steps"] == 0 and fit["decided"]
    r = fit["rec"]
    assert abs(r["xc"] - 0.25) < 1e-9 and abs(r["xr"] + 0.25) < 1e-9 and abs(r["xi"] - 0.125) < 1e-9
    assert abs(r["size"] - 1.6 * 2 ** (2.125 / 3)) < 1e-9 and abs(r["x"] - 8.25 / 2) < 1e-9
    assert S.extrema([oct_]) == [(0, 2, 8, 8)]
    # a ramp along +x under a Gaussian window: one peak, gradient angle 0 -> bin 0 -> angle 0 (360 -> 0)
    ramp = np.tile(np.arange(40, dtype=np.float32) * 3, (6, 40, 1))
    o = S.orientations([ramp], dict(o=0, layer=1, r=20, c=20, scl=2.0, rel_size=1e-6))
    assert o["radius"] == 9 and [p["bin"] for p in o["peaks"]] == [0] and o["peaks"][0]["angle"] == 0.0 and o["peaks"][0]["sure"]


@pytest.mark.parametrize("fam", sorted(F.FAMILIES))
def test_frames_are_what_the_family_says(fam):
    print("%s: %s" % (fam, F.check_premise(fam)))


@pytest.mark.parametrize("name", NAMES)
def test_pyramid_layout(name):
    i = F.info(name)
    h, w = F.FRAMES[name].shape
    assert [p.shape for p in i["pyr"]] == [(6, b, a) for a, b in O.sift_layout(w, h)]


@pytest.mark.parametrize("name", NAMES)
def test_keypoints_against_the_plain_restatement(name):
    """every decided key point of the restatement is in the oracle's list within its bars, the list holds nothing the restatement
    does not hold possible, and it is in the final order"""
    i = F.info(name)
    fig = S.check_keypoints(i["pyr"], i["kp"], name)
    print("%s: %d records, %s" % (name, len(i["kp"]["xy"]), fig))
    assert fig["unjudged"] == 0 or name[0] == "N", fig


@pytest.mark.parametrize("name", NAMES)
def test_descriptors_against_the_plain_restatement(name):
    """every byte of every descriptor: rint of the float64 value, or one off where the value lies within its bound of a half"""
    i = F.info(name)
    n, und, off, big = S.check_descriptors(i["pyr"], i["kp"], name)
    print("%s: %d descriptors, %d undecided, %d bytes one off, largest bound %.3f" % (name, n, und, off, big))
    assert n + und == len(i["kp"]["xy"]) and und <= 0.1 * max(n, 1)
