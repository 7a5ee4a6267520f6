"""GPU: SIFT's stages after the scale space on the crafted frames of tests/sift_families.py (extrema of both signs in every layer
and on the border and tile edges, fits that move and leave, rejects, many-peaked and wrapping orientations, descriptor windows
cut by the image and capped by its diagonal, ties of mirrored frames, near-flat noise).

One context per frame size, two frames per sift_detect_batch call.  Per frame
  * bit for bit: the six Gaussian layers of every octave and the key-point list (x, y, size, angle, response as bit patterns,
    packed octave, every descriptor byte) are the oracle's (the bar of test_gpu_sift.py);
  * without the oracle: the pyramid downloaded from the device goes into the plain float64 restatement (tests/sift_checks.py),
    and the device's own records and descriptors are held to it -- every decided key point present within its bars, nothing
    extra, the final order, every descriptor byte within the byte rule.
Frames of every family also go through a group boundary (frames 0 and 3 of a four-frame call, in groups of four, two and one), and
one frame overflows the candidate list alone.  That the frames are what the families say is asserted on the CPU in
tests/test_oracle_sift_edges.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import sift_checks as S  # noqa: E402
import sift_families as F  # noqa: E402
from detector_checks import _same_keypoints, dev, make_ctx  # noqa: E402
from oracle import oracle as O  # noqa: E402

NAMES = sorted(F.FRAMES)
OVERFLOW = ("R_ridges", 64)        # a frame with many candidates and few key points, and the capacity it overflows alone


def _pyramid(ctx, f):
    return [np.stack([ctx.sift_download_gauss(f, o, l) for l in range(6)]) for o in range(len(ctx.sift_octaves()))]


@pytest.fixture(scope="module")
def detected():
    """{name: key points} and {name: pyramid}: every frame through sift_detect_batch, two frames a call (an odd one out goes with
    the frame before it once more); one context per frame size, downloads kept"""
    kps, pyrs = {}, {}
    for (w, h), names in F.by_size().items():
        ctx = make_ctx(w, h, frames=4, sift=4096)
        try:
            for k in range(0, len(names), 2):
                pair = names[k:k + 2] if k + 1 < len(names) else [names[k - 1], names[k]]
                ctx.sift_detect_batch(dev(np.stack([F.FRAMES[n] for n in pair])))
                assert ctx.sift_octaves() == O.sift_layout(w, h)
                for f, n in enumerate(pair):
                    kps[n] = ctx.sift_download(f)
                    pyrs[n] = _pyramid(ctx, f)
        finally:
            ctx.close()
    return kps, pyrs


@pytest.mark.parametrize("name", NAMES)
def test_scale_space_is_the_oracles(detected, name):
    want = F.info(name)["pyr"]
    got = detected[1][name]
    assert len(got) == len(want)
    for o in range(len(want)):
        for l in range(6):
            assert np.array_equal(got[o][l].view(np.uint32), want[o][l].view(np.uint32)), "%s octave %d layer %d: max |diff| %g" % (
                name, o, l, np.abs(got[o][l] - want[o][l]).max())


@pytest.mark.parametrize("name", NAMES)
def test_keypoints_and_descriptors_are_the_oracles(detected, name):
    _same_keypoints(detected[0][name], F.info(name)["kp"])


@pytest.mark.parametrize("name", NAMES)
def test_keypoints_against_the_plain_restatement(detected, name):
    """nothing of the oracle's in here: the device's pyramid, the device's records, numpy for the rest"""
    kp, pyr = detected[0][name], detected[1][name]
    fig = S.check_keypoints(pyr, kp, name)
    print("%s: %d records, %s" % (name, len(kp["xy"]), fig))
    assert fig["unjudged"] == 0 or name[0] == "N", fig


@pytest.mark.parametrize("name", NAMES)
def test_descriptors_against_the_plain_restatement(detected, name):
    kp, pyr = detected[0][name], detected[1][name]
    n, und, off, big = S.check_descriptors(pyr, kp, name)
    print("%s: %d descriptors, %d undecided, %d bytes one off, largest bound %.3f" % (name, n, und, off, big))
    assert n + und == len(kp["xy"]) and und <= 0.1 * max(n, 1)


@pytest.mark.parametrize("group", [None, 2, 1])
@pytest.mark.parametrize("fam", sorted(F.FAMILIES))
def test_frames_across_a_group_boundary(monkeypatch, detected, fam, group):
    """two frames of the family as frames 0 and 3 of a four-frame call -- max_frames cannot make a group of one frame hold two, so
    the four frames form one group (None) or, with EVH_DETECT_GROUP as in tests/test_gpu_detector_groups.py, two groups of two
    (frame 0 in the first, frame 3 in the second) or four groups of one -- and each alone: the lists equal those of the
    two-frame calls"""
    if group is None:
        monkeypatch.delenv("EVH_DETECT_GROUP", raising=False)
    else:
        monkeypatch.setenv("EVH_DETECT_GROUP", str(group))
    a, b = F.FAMILIES[fam][0], F.FAMILIES[fam][-1]
    h, w = F.FRAMES[a].shape
    assert F.FRAMES[b].shape == (h, w)
    ctx = make_ctx(w, h, frames=4, sift=4096)
    try:
        ctx.sift_detect_batch(dev(np.stack([F.FRAMES[n] for n in (a, b, a, b)])))
        four = [ctx.sift_download(0), ctx.sift_download(3)]
        alone = []
        for n in (a, b):
            ctx.sift_detect_batch(dev(np.stack([F.FRAMES[n]])))
            alone.append(ctx.sift_download(0))
    finally:
        ctx.close()
    for n, x, y in zip((a, b), four, alone):
        _same_keypoints(x, detected[0][n])
        _same_keypoints(y, detected[0][n])


def test_candidate_list_overflow_alone():
    """the candidate list holds 4 * capacity entries: a frame whose candidates do not fit while its key points do is flagged
    (EvhError on download, as in test_sift_capacity_is_flagged), and passes the bit-for-bit leg with an ample capacity"""
    from evenvizion_amd._lib import EvhError
    name, cap = OVERFLOW
    i = F.info(name)
    ref = i["ref"]
    # on the CPU: more candidates than 4 * cap; at most cap records before the duplicates go (every peak the restatement holds
    # possible counted) and at most cap in the oracle's list
    raw = sum(len(o["peaks"]) for o in ref["ori"].values()) + sum(len(f["maybe"]) for f in ref["fits"]) * 36
    assert len(ref["cand"]) > 4 * cap and raw <= cap and len(i["kp"]["xy"]) <= cap, (len(ref["cand"]), raw, len(i["kp"]["xy"]))
    img = F.FRAMES[name]
    h, w = img.shape
    c = make_ctx(w, h, frames=2, sift=cap)
    try:
        c.sift_detect_batch(dev(np.stack([img, img])))
        with pytest.raises(EvhError):
            c.sift_download(0)
    finally:
        c.close()
    c = make_ctx(w, h, frames=2, sift=4096)
    try:
        c.sift_detect_batch(dev(np.stack([img, img])))
        _same_keypoints(c.sift_download(1), i["kp"])
    finally:
        c.close()
