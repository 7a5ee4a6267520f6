"""The oracle's findHomography / compute_homography on the adversarial families of tests/solver_families.py, against a
float64 reference that does not go through the oracle (SVD refit, reprojection cost, float32 inlier evaluation, the
iteration bound at 50 digits).  Runs without a GPU: the families are developed and their branches confirmed here, and
tests/test_gpu_solver_edges.py holds the device to the oracle on the same sets."""
import math

import numpy as np
import pytest

import solver_families as F
from oracle import oracle as O

SETS = F.all_sets()
IDS = ["%s-%s" % (fam, name) for fam, name, _ in SETS]
RUNS = ((False, 2000), (True, 2000), (True, 37))        # plain, force_max_iters at 2000 and at a short bound


def _find(rows, force=False, max_iters=2000):
    return O.find_homography_stats(rows[:, :2], rows[:, 2:], max_iters=max_iters, force_max_iters=force)


def _gate(s, n):
    """compute_homography's `s < 0.7 n` in exact rational arithmetic (0.7 * n is exact in double for these n)"""
    return 10 * s < 7 * n


@pytest.mark.parametrize("fam,name,rows", SETS, ids=IDS)
def test_oracle_against_float64_reference(fam, name, rows):
    """Every H the oracle finds is finite, LM ends at or below the cost of its seed (the float64 SVD refit on the mask rows),
    every mask row lies within MASK_RADIUS * thr of it; compute_homography's status follows the mask by the 0.7 gate and
    its H is find_homography's."""
    for force, max_iters in RUNS:
        H, mask, info, stats = _find(rows, force, max_iters)
        assert (H is None) == (info[1] == 0 or len(rows) < 4), (name, info)
        assert int(mask.sum()) == (info[1] if H is not None else 0), (name, info, mask.sum())
        if H is not None:
            F.check_solution(H, mask, rows, "%s force=%s max_iters=%d" % (name, force, max_iters))
            assert 0 <= info[2] <= 10
    H, mask, info, _ = _find(rows)
    st, Hc = O.compute_homography(rows[:, :2], rows[:, 2:])
    n, s = len(rows), int(mask.sum())
    assert st == (O.LOW_INLIER_RATIO if _gate(s, n) else O.NO_FINAL_H if H is None else O.OK), (name, st, s, n)
    if st == O.OK:
        assert np.array_equal(Hc, H)


def test_draw_reaches_the_attempt_loop():
    """F1-F3 drive get_subset's attempt loop (stats[0]: subsets rejected by checkSubset); 'f1_rare' exhausts the 10000
    attempts of a draw while valid subsets exist; the mirrored H is found through negative == 4; the half-mirrored set
    rejects most of its mixed subsets."""
    got = {name: _find(rows) for fam, name, rows in SETS if fam in ("F1", "F2", "F3")}
    for name, (H, mask, info, stats) in got.items():
        assert stats[0] > 0 or name in ("f1_grid_exact", "f3_mirror0"), (name, stats)
        assert stats[2] == 0 or name == "f1_rare", (name, stats)
    H, mask, info, stats = got["f1_rare"]
    assert stats[1] == 1 and stats[0] >= 10000 and info[0] < 2000, (info, stats)
    rows = dict((n, r) for _, n, r in SETS)["f1_rare"]
    # a valid subset exists: three line rows in the same order on both sides and the off-line row last
    a, b = rows[:, :2], rows[:, 2:]
    order = np.argsort(b[:, 0])
    i, j, k = order[0], order[1], order[2]
    assert a[i, 0] != a[j, 0] and O.dlt(np.r_[a[[i, j, k]], a[[750]]], np.r_[b[[i, j, k]], b[[750]]]) is not None
    for name in ("f3_mirror0", "f3_mirror1"):
        H, mask, info, stats = got[name]
        assert H is not None and np.linalg.det(H) < 0, name          # only negative == 4 subsets exist
    assert got["f3_mirror0"][2][1] == 80
    assert got["f3_half_mirrored"][3][0] >= 100
    assert got["f2_dup90"][3][0] > 0


@pytest.mark.parametrize("name,rows", F.f4_boundary())
def test_inlier_boundary(name, rows):
    """F4: the mask is is_inlier's float32 evaluation under the exact translation (the consensus the plain draw settles on),
    rows at err == 9 exactly included (err <= t, not err < t)."""
    err, expect = F.boundary_expected(rows, F.F4_H)
    assert (err == np.float32(9)).sum() >= 4 and ((err > 9) & (err < 9.0001)).sum() >= 4
    H, mask, info, _ = _find(rows)
    assert np.array_equal(mask.astype(bool), expect), (name, np.flatnonzero(mask.astype(bool) != expect), err[mask.astype(bool) != expect])


def test_f5_pairs_are_the_closest():
    half, edge = F.f5_search(1200)
    assert [p for p, _ in half] == F.F5_HALF and [p for p, _ in edge] == F.F5_EDGE[:len(edge)]
    assert all(d < 3e-6 for _, d in half)


@pytest.mark.parametrize("n,good", F.F5_HALF + F.F5_EDGE)
def test_iteration_bound(n, good):
    """F5: with the exact consensus found, the plain draw stops at RANSACUpdateNumIters' bound; at the half-integer pairs
    rint(num / denom) decides it, and the float64 chain rounds the way the 50-digit value does."""
    import mpmath
    mpmath.mp.dps = 50
    rows = dict((nm, r) for fam, nm, r in SETS if fam == "F5")["f5_%s_%d_%d" % ("half" if (n, good) in F.F5_HALF else "edge", n, good)]
    H, mask, info, _ = _find(rows)
    assert info[1] == good
    bound, x = F.num_iters64(n, good)
    xe = mpmath.log(1 - mpmath.mpf(F.CONF)) / mpmath.log(1 - (mpmath.mpf(good) / n) ** 4)
    assert bound == (2000 if xe >= 2000 else int(mpmath.nint(xe))) or abs(xe - 2000) < 0.5
    assert info[0] == bound, (n, good, info, bound, x)


def test_gate_at_seven_tenths():
    """F8: s == 0.7 n exactly passes compute_homography's gate, one inlier less does not."""
    for name, rows in F.f8_gate():
        s, n = (int(v) for v in name.split("_")[1::2])
        H, mask, info, _ = _find(rows)
        assert int(mask.sum()) == s, name
        st, _ = O.compute_homography(rows[:, :2], rows[:, 2:])
        assert st == (O.LOW_INLIER_RATIO if _gate(s, n) else O.OK), (name, st)
        assert (st == O.OK) == (10 * s == 7 * n)


def test_stream_mirror_on_crafted_pairs():
    """The Python mirror of the stream scan (solver_families.scan_mirror) against the oracle's own loop shape: a failing
    pair repeats the previous H, a failing first pair ends the scan with NaN, and a split with carried state is the
    single call."""
    pairs = F.scan_pairs(kcap=1728)
    st1 = np.array([p[1] for p in pairs], np.int32)
    Hs, sts = F.scan_mirror([p[0] for p in pairs], st1)
    assert list(sts[st1 != 0]) == list(st1[st1 != 0])
    for p in range(len(pairs)):
        if sts[p] != O.OK and p:
            assert np.array_equal(Hs[p], Hs[p - 1])
    k = len(pairs) // 2
    Ha, sa, state = F.scan_mirror([p[0] for p in pairs[:k]], st1[:k], return_state=True)
    Hb, sb = F.scan_mirror([p[0] for p in pairs[k:]], st1[k:], state=state)
    assert np.array_equal(np.r_[Ha, Hb], Hs) and np.array_equal(np.r_[sa, sb], sts)
    Hf, sf = F.scan_mirror([p[0] for p in pairs[:3]], np.array([2, 0, 0], np.int32))
    assert list(sf) == [2, 2, 2] and np.isnan(Hf).all()
    assert math.isfinite(float(np.abs(Hs[1:]).max()))
