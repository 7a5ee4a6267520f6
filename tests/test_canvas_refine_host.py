"""The host side of frame-to-mosaic registration: the numpy restatement of evh_canvas_refine (tests/canvas_checks.py) against the
restatement of evh_pair_refine it generalises, its validity rule by hand, the algebra of the driver's loop
(registration.anchor_groups) on scripted results, the drivers' refusals and the header.  No GPU: the device is held to
canvas_checks in test_gpu_canvas_refine.py."""
import os
import re

import numpy as np
import pytest

import canvas_checks as CC
import refine_checks as RC
import refine_families as F
import warp_checks as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def frames_of(seed, n, w, h, gray=False):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w) if gray else (n, h, w, 3), dtype=np.uint8)


# ---- the restatement against the one it generalises ----------------------------------------------------------------------------------
@pytest.mark.parametrize("gray", [False, True])
def test_canvas_is_the_previous_frame(gray):
    """canvas = the previous frame, no count (and a count that is valid everywhere): cost, jacobian and refine are refine_checks'"""
    rng = np.random.default_rng(3)
    f = frames_of(4, 2, 23, 17, gray)
    full = np.full((17, 23), 255, np.uint8)
    for k in range(5):
        M = np.eye(3) + rng.normal(0, [[.02, .02, 2], [.02, .02, 2], [1e-4, 1e-4, 0]])
        for count, mc in ((None, 1), (full, 255)):
            assert CC.cost(f[0], f[1], M, count, mc) == RC.cost(f[0], f[1], M)
            for clip in (255, 16, 0):
                a, b = CC.jacobian(f[0], f[1], M, clip, count, mc), RC.jacobian(f[0], f[1], M, clip)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for case in (F.CASES[0], F.CASES[5]):
        prev, cur, _, M_start = F.pair(*case)
        want, winfo = RC.refine(prev, cur, M_start, 6, 255)
        got, ginfo = CC.refine(prev, cur, M_start, 6, 255)
        assert got.tobytes() == want.tobytes() and ginfo == winfo and winfo["accepted"] >= 1
    nan = np.full((3, 3), np.nan)
    got, info = CC.refine(f[0], f[1], nan, 4)
    assert got is not None and got.tobytes() == nan.tobytes() and info["status"] == RC.NOTHING_COVERED


def test_validity_rule_by_hand():
    canvas = frames_of(9, 1, 40, 30, True)[0]
    cur = frames_of(10, 1, 24, 18, True)[0]
    count = np.ones((30, 40), np.uint8)
    whole = CC.sample(canvas, W.translation(5, 4), 24, 18, count, 1)[1]
    assert whole.all()
    count[7, 29] = 0                                           # right of the last column's tap: weight 0, never asked
    assert CC.sample(canvas, W.translation(5, 4), 24, 18, count, 1)[1].all()
    count[9, 10] = 0                                           # under the tap of frame pixel (5, 5)
    cov = CC.sample(canvas, W.translation(5, 4), 24, 18, count, 1)[1]
    assert np.argwhere(~cov).tolist() == [[5, 5]]
    cov = CC.sample(canvas, W.translation(5.5, 4), 24, 18, count, 1)[1]      # two taps per sample: x = 4 and x = 5 meet the hole
    assert np.argwhere(~cov).tolist() == [[3, 23], [5, 4], [5, 5]]           # and the last column now reads (29, 7) too
    count[...] = 1
    assert CC.cost(canvas, cur, W.translation(5, 4), count, 2) == (0, 0)
    out, info = CC.refine(canvas, cur, W.translation(5, 4), 4, 255, count, 2)
    assert info["status"] == RC.NOTHING_COVERED and info["evals"] == 1
    count[...] = 0
    count[6:13, 7:14] = 1                                       # 49 canvas pixels under interior pixels of the frame: fewer than 64
    out, info = CC.refine(canvas, cur, W.translation(5, 4), 4, 255, count, 1)
    assert info["status"] == RC.TOO_FEW and info["n_in"] == 49 == info["covered_in"]


def test_canvas_pair_converges_on_the_host():
    canvas, frame, count, M_true, M_start = CC.canvas_pair(141, 64, 48, 1)
    assert RC.corner_error(M_start, M_true, 64, 48) >= 0.9 and (count == 0).sum() > 0
    M, info = CC.refine(canvas, frame, M_start, 8, 255, count, 1)
    e = RC.corner_error(M, M_true, 64, 48)
    print("64 x 48 against 96 x 72 with holes: %.3f px after %d accepted steps, %d of %d covered" % (e, info["accepted"], info["covered_in"], 64 * 48))
    assert e <= 0.25 and info["status"] == RC.REFINED and info["covered_in"] < 64 * 48


# ---- the driver's algebra ------------------------------------------------------------------------------------------------------------------
def chain(n, seed=11):
    rng = np.random.default_rng(seed)
    S = [np.eye(3)]
    for _ in range(n - 1):
        H = np.eye(3) + rng.normal(0, [[.01, .01, 3], [.01, .01, 3], [1e-5, 1e-5, 0]])
        T = np.dot(H, S[-1])
        S.append(T / T[2, 2])
    return S


def rows_of(n, status=RC.REFINED, covered=5000):
    rows = np.zeros((n, 8), np.int64)
    rows[:, 0], rows[:, 3], rows[:, 5] = status, covered, covered
    return rows


@pytest.mark.parametrize("group", [1, 3])
def test_algebra_of_the_loop_on_scripted_results(group):
    from evenvizion_amd.registration import anchor_groups
    S, T = chain(8), W.translation(40, 25)
    w, h = 100, 80
    painted, seen = [], []
    nudge = W.translation(0.5, -0.25)

    def refine(first, start):
        seen.append((first, start.copy()))
        return np.stack([np.dot(nudge, m) for m in start]), rows_of(len(start))

    def paint(first, mats):
        painted.append((first, mats.copy()))

    out, info = anchor_groups(S, T, w, h, group, 0.25, refine, paint)
    assert len(out) == len(info) == 8 and [p[0] for p in painted] == list(range(0, 8, group)) == [0] + [s[0] for s in seen]
    assert np.abs(out[0] - S[0]).max() <= 1e-12 and not info[0]["used"] and all(e["used"] for e in info[group:])
    # every refined group moved every later start by the same nudge: after j refined groups the correction is nudge^j in canvas
    # coordinates, D = T^-1 nudge^j T
    Tinv = np.linalg.inv(T)
    for k in range(8):
        j = k // group
        want = np.dot(np.dot(Tinv, np.linalg.matrix_power(nudge, j)), np.dot(T, S[k]))
        assert np.abs(out[k] - want / want[2, 2]).max() <= 1e-9 * np.abs(want).max(), k
    for first, start in seen:                                    # a group starts where the last one ended: T D S_k
        j = first // group - 1
        want = np.dot(np.linalg.matrix_power(nudge, j), np.dot(T, S[first]))
        assert np.abs(start[0] - want / want[2, 2]).max() <= 1e-9 * np.abs(want).max()
    for (first, mats), k in zip(painted, range(0, 8, group)):     # what is painted is T S'_k
        want = np.dot(T, out[k])
        assert np.abs(mats[0] - want / want[2, 2]).max() <= 1e-9 * np.abs(want).max()


def test_min_overlap_status_and_missing_matrices():
    from evenvizion_amd.registration import anchor_groups
    S, T = chain(6), W.translation(10, 10)
    S[3] = np.full((3, 3), np.nan)
    w, h = 100, 80
    nudge = W.translation(1, 0)
    statuses = {1: RC.REFINED, 2: RC.UNCHANGED, 3: RC.NOTHING_COVERED, 4: RC.REFINED, 5: RC.REFINED}
    covered = {1: 2000, 2: 8000, 3: 0, 4: 1999, 5: 7999}       # 0.25 * 8000 = 2000: frame 1 is just in, frame 4 just out

    def refine(first, start):
        rows = rows_of(1, statuses[first], covered[first])
        return np.stack([np.dot(nudge, m) for m in start]), rows

    out, info = anchor_groups(S, T, w, h, 1, 0.25, refine, lambda first, mats: None)
    assert [e["used"] for e in info] == [False, True, False, False, False, True]
    assert [e["overlap"] for e in info] == [0.0, 0.25, 1.0, 0.0, 1999 / 8000.0, 7999 / 8000.0]
    assert np.array_equal(out[3], out[2])                        # the missing entry repeats the running S'
    moved = lambda k, j: np.dot(np.dot(np.linalg.inv(T), np.linalg.matrix_power(nudge, j)), np.dot(T, S[k]))
    for k, j in ((0, 0), (1, 1), (2, 1), (4, 1), (5, 2)):       # an unused frame keeps its start, which carries the earlier nudges
        want = moved(k, j)
        assert np.abs(out[k] - want / want[2, 2]).max() <= 1e-9 * np.abs(want).max(), k
    none, info = anchor_groups(S, T, w, h, 1, 1.0, refine, lambda first, mats: None)
    assert not any(e["used"] for e in info)
    for k in (0, 1, 2, 4, 5):
        assert np.abs(none[k] - S[k]).max() <= 1e-12 * np.abs(S[k]).max()


def test_anchored_dictionary_recomposes(monkeypatch):
    """H'_k = S'_k S'_{k-1}^-1: the reference's superposition of the H' gives the S' back"""
    from evenvizion_amd import registration
    S = chain(6)
    sup = {k + 1: m for k, m in enumerate(S)}
    shifted = {k: np.dot(W.translation(0.1 * k, 0), m) for k, m in sup.items()}
    infos = {k: dict(zip(("status", "evals", "accepted", "covered_in", "ssd_in", "covered_out", "ssd_out", "n_in"),
                         (0, 2, 1, 100, 900 + k, 100, 400, 90)), used=True, overlap=0.5) for k in sup}
    infos[1].update(covered_in=0, covered_out=0)
    monkeypatch.setattr(registration, "anchor_superposition", lambda *a, **k: (shifted, infos))
    monkeypatch.setattr(registration, "registration_report", lambda cap, d, *a, **k: {"itf": float(len(d))})
    got = registration.anchored_homography_dict(lambda: None, sup, {"w": 8, "h": 4})
    assert list(got["homography"]) == [2, 3, 4, 5, 6] and got["superposition"] is shifted and got["info"] is infos
    T = shifted[1]
    for k in range(2, 7):
        T = np.dot(np.asarray(got["homography"][k]["H"]), T)
        T = T / T[2, 2]
        assert np.abs(T - shifted[k] / shifted[k][2, 2]).max() <= 1e-9 * np.abs(shifted[k]).max()
    assert got["canvas_score_before"] == pytest.approx(sum((900 + k) / 100.0 for k in range(2, 7)))
    assert got["canvas_score_after"] == pytest.approx(5 * 4.0)


class NeverRead:
    def __getattr__(self, name):
        raise AssertionError("the capture was touched: %s" % name)


@pytest.mark.parametrize("bad", [dict(ingest="rgb"), dict(iters=-1), dict(iters=65), dict(iters=2.5), dict(clip=-1), dict(clip=256),
                                 dict(group=0), dict(group=True), dict(group=1.5), dict(blend="mean"), dict(feather_px=-1), dict(feather_px="8"),
                                 dict(min_overlap=-0.1), dict(min_overlap=1.5), dict(min_overlap=True), dict(margin=-1), dict(chunk_frames=0),
                                 dict(chunk_frames=2.5), dict(resize_info={"w": 0, "h": 4}), dict(resize_info={"w": 4097, "h": 4})])
def test_drivers_refuse_bad_arguments_before_anything_is_opened(bad, monkeypatch):
    from evenvizion_amd import registration, runtime

    def no_context(*a, **k):
        raise AssertionError("a context was opened")

    def no_capture():
        raise AssertionError("the capture was opened")

    monkeypatch.setattr(runtime, "get_context", no_context)
    kw = dict(resize_info={"w": 8, "h": 4})
    kw.update(bad)
    ri = kw.pop("resize_info")
    sup = {1: np.eye(3), 2: np.eye(3)}
    with pytest.raises(ValueError):
        registration.anchor_superposition(NeverRead(), sup, ri, **kw)
    with pytest.raises(ValueError):
        registration.anchored_homography_dict(no_capture, sup, ri, **kw)
    with pytest.raises(ValueError):
        registration.anchored_homography_dict(no_capture, sup, ri, threshold=300)


def test_header_and_signature_table_declare_both_entries():
    from evenvizion_amd import _lib
    text = open(os.path.join(ROOT, "include", "evhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("evh_canvas_refine", "evh_canvas_refine_yuv420"):
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["evh_canvas_refine"][1]) == 21 and len(_lib.SIGNATURES["evh_canvas_refine_yuv420"][1]) == 18
    assert hasattr(_lib.Context, "canvas_refine") and hasattr(_lib.Context, "canvas_refine_yuv420")
