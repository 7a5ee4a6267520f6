"""GPU: SURF's seven kernels on the crafted frames of tests/surf_families.py (key points of both signs in every middle layer, the
window classes of the area average and both launches of the describe kernel, the margins' first and last samples, frames at
which a layer is just built or just not, responses around the threshold, fits near 1, orientations round the circle, ties of the
order, saturated and flat content).

One context per frame size, two frames per surf_detect_batch call.  Per frame
  * the integral image is the exact one;
  * bit for bit: the key-point list (x, y, size, angle, response, every descriptor float as bit patterns, octave, laplacian)
    is the oracle's;
  * without the oracle: the device's own records and descriptors are held to the plain float64 restatement (tests/surf_checks.py)
    of the frame -- every decided key point present within its bars, nothing extra, the orientation, the final order, every
    descriptor float within its bound.
Frames of every family also run at thresholds 100 and 5000, which only the restatement can judge, and through a group boundary
(frames 0 and 3 of a four-frame call in groups of two).  One context runs every geometry frame after a dense batch at full size:
the Hessian planes are never cleared, so a layer read where this geometry did not build it would show.  That the frames are what
the families say is asserted on the CPU in tests/test_oracle_surf_edges.py.

A raw list that overflows alone (capacity below the candidates, at least the kept) needs a frame that deletes key points; the
restatement deletes none on any frame here (profiles/surf_edges.txt shows why none can), so that case is left out."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import surf_checks as S  # noqa: E402
import surf_families as F  # noqa: E402
from detector_checks import _same_surf, dev, make_surf_ctx  # noqa: E402
from oracle import oracle as O  # noqa: E402

NAMES = sorted(F.FRAMES)
GEOMETRY = F.FAMILIES["G"]
# one or two frames per family for the other thresholds
THRESHOLD_FRAMES = ("L_bright", "L_top_dark", "W_30", "W_46", "B_a", "G_h054+0", "G_tiny", "T_contrast", "O_a", "R_tiled", "S_binary")


def _ctx(w, h, frames=4, surf=4096):
    """a context takes 64 x 64 at the least; a smaller frame runs in it at its own size"""
    return make_surf_ctx(max(w, 64), max(h, 64), frames=frames, surf=surf)


@pytest.fixture(scope="module")
def detected():
    """{name: key points}, {name: integral}: every frame through surf_detect_batch, two frames a call (an odd one out goes with the
    frame before it once more, a single one with itself); one context per frame size"""
    kps, sums = {}, {}
    for (w, h), names in F.by_size().items():
        ctx = _ctx(w, h)
        try:
            for k in range(0, len(names), 2):
                pair = names[k:k + 2] if k + 1 < len(names) else [names[k - 1], names[k]]
                ctx.surf_detect_batch(dev(np.stack([F.FRAMES[n] for n in pair])))
                for f, n in enumerate(pair):
                    kps[n] = ctx.surf_download(f)
                    sums[n] = ctx.surf_download_integral(f)
        finally:
            ctx.close()
    return kps, sums


@pytest.mark.parametrize("name", NAMES)
def test_integral_is_exact(detected, name):
    assert np.array_equal(detected[1][name], S.integral(F.FRAMES[name]))


@pytest.mark.parametrize("name", NAMES)
def test_keypoints_and_descriptors_are_the_oracles(detected, name):
    _same_surf(detected[0][name], O.surf_detect(F.FRAMES[name]))


@pytest.mark.parametrize("name", NAMES)
def test_keypoints_against_the_plain_restatement(detected, name):
    """nothing of the oracle's in here: the frame, the device's records, numpy for the rest"""
    kp = detected[0][name]
    fig = S.check_keypoints(F.FRAMES[name], kp, 400.0, name)
    print("%s: %s" % (name, fig))                                  # the family's share of undecided ones is asserted on the CPU
    if name in F.NONE:                                             # ties and flat ground: the restatement decides no key point,
        assert len(kp["xy"]) == 0                                  # and a strict maximum leaves none (asserted in the premise)


@pytest.mark.parametrize("name", NAMES)
def test_descriptors_against_the_plain_restatement(detected, name):
    kp = detected[0][name]
    fig = S.check_descriptors(F.FRAMES[name], kp, name)
    print("%s: %s" % (name, fig))
    assert fig["checked"] + fig["undecided"] == len(kp["xy"]) and fig["undecided"] <= 0.1 * max(fig["checked"], 1)


@pytest.mark.parametrize("thr", [100.0, 5000.0])
@pytest.mark.parametrize("name", THRESHOLD_FRAMES)
def test_other_thresholds_against_the_plain_restatement(name, thr):
    """hessian_threshold 100 and 5000: the oracle is fixed at 400, so the restatement alone judges these"""
    img = F.FRAMES[name]
    h, w = img.shape
    ctx = _ctx(w, h, frames=2, surf=8192)
    try:
        ctx.surf_detect_batch(dev(np.stack([img, img])), hessian_threshold=thr)
        kp = ctx.surf_download(1)
    finally:
        ctx.close()
    fig = S.check_keypoints(img, kp, thr, "%s at %g" % (name, thr))
    dfig = S.check_descriptors(img, kp, "%s at %g" % (name, thr))
    print("%s at %g: %s %s" % (name, thr, fig, dfig))
    assert (kp["response"] > thr).all()
    assert dfig["checked"] + dfig["undecided"] == len(kp["xy"]) and dfig["undecided"] <= 0.1 * max(dfig["checked"], 1)


def _pair_of(fam):
    """two frames of the family of one size (the same one twice where no two share a size)"""
    names = F.FAMILIES[fam]
    for a in names:
        for b in reversed(names):
            if a != b and F.FRAMES[a].shape == F.FRAMES[b].shape:
                return a, b
    return names[0], names[0]


@pytest.mark.parametrize("fam", sorted(F.FAMILIES))
def test_frames_across_a_group_boundary(monkeypatch, detected, fam):
    """two frames of the family as frames 0 and 3 of a four-frame call in groups of two: the lists of the two-frame calls"""
    monkeypatch.setenv("EVH_DETECT_GROUP", "2")
    a, b = _pair_of(fam)
    h, w = F.FRAMES[a].shape
    ctx = _ctx(w, h)
    try:
        ctx.surf_detect_batch(dev(np.stack([F.FRAMES[n] for n in (a, b, b, b)])))
        got = [ctx.surf_download(0), ctx.surf_download(3)]
    finally:
        ctx.close()
    _same_surf(got[0], detected[0][a])
    _same_surf(got[1], detected[0][b])


def test_stale_planes_of_unbuilt_layers_are_not_read(detected):
    """one 256 x 240 context: a dense noise batch at full size fills every Hessian plane, then every geometry frame runs at its own
    smaller size.  The planes are not cleared and the det kernel writes no margins, so only the margins of the maxima kernel keep
    the layers this geometry does not build unread: the lists are those of a fresh context, and pass the restatement"""
    rng = np.random.default_rng(7)
    noise = rng.integers(0, 256, (2, F.H, F.W), dtype=np.uint8)
    ctx = make_surf_ctx(F.W, F.H, frames=2, surf=16384)
    try:
        for n in GEOMETRY:
            ctx.surf_detect_batch(dev(noise))
            assert ctx.lib.evh_surf_count(ctx.h, 0) > 500
            img = F.FRAMES[n]
            ctx.surf_detect_batch(dev(np.stack([img, img])))
            kp = ctx.surf_download(1)
            _same_surf(kp, detected[0][n])
            _same_surf(ctx.surf_download(0), detected[0][n])
            S.check_keypoints(img, kp, 400.0, n)
    finally:
        ctx.close()
