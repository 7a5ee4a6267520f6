"""GPU: ORB's describe stage on the crafted frames of tests/describe_families.py (saturating blur, exact and general angles,
every alignment of the staged patch and the 31-pixel border, Harris sums beyond 2^24, many tap roundings).

Every frame runs alone and as one batch of all frames of its size, in the reference and in the canonical key-point order:
  * the 8 pyramid levels are the oracle's bytes;
  * the key points are the oracle's in octave, lx, ly, xy, in response and angle as bit patterns and in every descriptor byte
    (the bar of test_gpu_parity.py::test_orb_keypoints_and_descriptors);
  * without the oracle: the descriptors equal the plain float32 restatement (tests/describe_checks.py: brief_bits (a)) read
    from the device's own level, lx, ly and angle, and the device's angles meet the exact-angle cases and the bound of
    tests/test_oracle_describe_edges.py against atan2 of the plain moments.
One pair of S frames goes through the ordinary pair entry to the oracle's H.  That the frames are what the families say is
asserted on the CPU in tests/test_oracle_describe_edges.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import describe_checks as D  # noqa: E402
import describe_families as F  # noqa: E402
from evenvizion_amd._lib import Context  # noqa: E402
from oracle import oracle as O  # noqa: E402

NAMES = sorted(F.FRAMES)
FORMS = ("alone", "batch")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def detected():
    """{(name, form, mode): key points} and {(name, form): the 8 levels}: every frame through orb_detect_batch alone and in the
    batch of its size, in the reference (1) and the canonical (0) order; one context per frame size, downloads kept"""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU; there is no CPU fallback")
    kps, levels = {}, {}
    for (w, h), names in F.by_size().items():
        ctx = Context(device=0, max_w=w, max_h=h, max_features=500, max_frames=len(names))
        try:
            batch = dev(np.stack([F.FRAMES[n] for n in names]))
            for mode in (1, 0):
                ctx.set_keypoint_order(mode)
                ctx.orb_detect_batch(batch)
                ctx.synchronize()
                for f, n in enumerate(names):
                    kps[(n, "batch", mode)] = ctx.orb_download(f)
                    if mode == 1:
                        levels[(n, "batch")] = [ctx.download_level(f, l) for l in range(F.NLEVELS)]
                for f, n in enumerate(names):
                    ctx.orb_detect_batch(batch[f:f + 1])
                    ctx.synchronize()
                    kps[(n, "alone", mode)] = ctx.orb_download(0)
                    if mode == 1:
                        levels[(n, "alone")] = [ctx.download_level(0, l) for l in range(F.NLEVELS)]
        finally:
            ctx.close()
    return kps, levels


@pytest.mark.parametrize("name", NAMES)
def test_levels_are_the_oracles(detected, name):
    want = F.info(name)["pyr"]
    for form in FORMS:
        got = detected[1][(name, form)]
        for l in range(F.NLEVELS):
            assert got[l].shape == want[l].shape and np.array_equal(got[l], want[l]), "%s %s level %d" % (name, form, l)


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("name", NAMES)
def test_keypoints_and_descriptors_are_the_oracles(detected, name, mode):
    o = F.info(name)["kp" if mode == 1 else "kp0"]
    assert len(o["xy"]) > 0
    for form in FORMS:
        g = detected[0][(name, form, mode)]
        what = "%s %s order %d" % (name, form, mode)
        assert len(g["xy"]) == len(o["xy"]), what
        for k in ("octave", "lx", "ly"):
            assert np.array_equal(g[k], o[k]), (what, k)
        assert np.array_equal(g["xy"], o["xy"]), what
        assert np.array_equal(g["response"].view(np.uint32), o["response"].view(np.uint32)), what
        assert np.array_equal(g["angle"].view(np.uint32), o["angle"].view(np.uint32)), what
        bad = np.nonzero((g["desc"] != o["desc"]).any(axis=1))[0]
        assert len(bad) == 0, "%s: descriptors of %d key points differ, first %d" % (what, len(bad), bad[0])


@pytest.mark.parametrize("name", NAMES)
def test_descriptors_and_angles_against_the_plain_restatement(detected, name):
    """nothing of the oracle's in here: the device's level, position and angle, numpy for the rest"""
    for form in FORMS:
        g = detected[0][(name, form, 1)]
        lv = detected[1][(name, form)]
        blur = [D.blur7_u8(a)[0] for a in lv]
        at = list(zip(g["octave"].tolist(), g["lx"].tolist(), g["ly"].tolist()))
        assert len(at) > 0
        D.check_angles(g["angle"], [D.moments(lv[l], x, y) for l, x, y in at], "%s %s" % (name, form))
        for j, (l, x, y) in enumerate(at):
            want = D.brief_bits(blur[l], x, y, g["angle"][j])[0]
            assert np.array_equal(g["desc"][j], want), "%s %s key point %d (level %d, %d, %d): %d bits differ" % (
                name, form, j, l, x, y, int(D.unpack_bits(g["desc"][j] ^ want).sum()))


def test_saturated_pair_through_the_pair_entry():
    """two S frames (dark marks on 255, the second moved by (5, 3)) as one pair: status and H are the oracle's, at the bar of
    test_gpu_parity.py::test_pair_batch_vs_oracle -- the saturated descriptors reach the matcher and the solver once"""
    frames = np.stack([F.FRAMES[n] for n in F.STREAM_PAIR])
    Ho, so = O.pairs_gray_batch(frames)
    assert so.tolist() == [0] and np.abs(Ho[0] / Ho[0][2, 2] - [[1, 0, 5], [0, 1, 3], [0, 0, 1]]).max() < 0.1
    h, w = frames.shape[1:]
    ctx = Context(device=0, max_w=w, max_h=h, max_features=500, max_frames=2)
    try:
        H = torch.zeros(1, 9, dtype=torch.float64, device="cuda")
        st = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        ctx.pair_homography_batch(dev(frames), 1, 0, H, st)
        ctx.synchronize()
        assert st.cpu().numpy().tolist() == [0]
        Hg = H.cpu().numpy().reshape(3, 3)
    finally:
        ctx.close()
    a, b = Hg / Hg[2, 2], Ho[0] / Ho[0][2, 2]
    floor = np.array([[1e-3, 1e-3, 1.0], [1e-3, 1e-3, 1.0], [1e-6, 1e-6, 1.0]])
    assert float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor))) <= 1e-3
    assert np.allclose(Hg, Ho[0], rtol=1e-9, atol=1e-12)
    c = np.array([[0, 0, 1], [w, 0, 1], [0, h, 1], [w, h, 1]], np.float64).T
    pa, pb = Hg @ c, Ho[0] @ c
    assert float(np.abs(pa[:2] / pa[2] - pb[:2] / pb[2]).max()) <= 0.05
