"""GPU: FAST in the reference key-point order on frames that pin the polarity of every corner.

k_fast_main's segment test hands the side of a corner's arc (ring darker / ring brighter than the centre) to the scorer,
which then evaluates one side only, on the raw bytes (evh_detect_fast.h: corner16_pass4, fast_score_one_sided).  A wrong
polarity bit, a wrong complement or a wrong arc gives another score byte, so the candidate lists (position and score of
every corner that survives the 3 x 3 maximum test) are compared with the oracle's on frames with corners of both kinds, of
one kind only, with the largest score a byte holds, and with scores right at the threshold at both ends of the grey range.

320 x 160: level 0 spans 3 x 5 FAST tiles with edge tiles on both sides, the eight levels have odd widths and levels 6-7 fall
under the 62-pixel border rule; 97 x 131 is the odd size of tests/test_gpu_order.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from evenvizion_amd._lib import Context  # noqa: E402
from oracle import oracle as O  # noqa: E402

W, H = 320, 160


def _blobs(rng, w, h, back, fore):
    img = np.full((h, w), back, np.uint8)
    ys, xs, size = rng.integers(0, h - 2, 400), rng.integers(0, w - 2, 400), rng.integers(1, 4, 400)
    for s, y, x in zip(size.tolist(), ys.tolist(), xs.tolist()):
        img[y:y + s, x:x + s] = fore
    return img


def _near(rng, w, h, base):
    step = rng.choice(np.array([-21, -20, 0, 20, 21]), size=(h, w), p=[.3, .1, .2, .1, .3])
    return np.clip(base + step, 0, 255).astype(np.uint8)


def _make_cases():
    rng = np.random.default_rng(7)
    c = {}
    c["noise"] = (W, H, rng.integers(0, 256, (H, W), dtype=np.uint8))
    c["bright_blobs"] = (W, H, _blobs(rng, W, H, 30, 200))
    c["dark_blobs"] = (W, H, _blobs(rng, W, H, 225, 55))
    c["binary_15"] = (W, H, np.where(rng.random((H, W)) < 0.15, 255, 0).astype(np.uint8))
    c["binary_85"] = (W, H, np.where(rng.random((H, W)) < 0.85, 255, 0).astype(np.uint8))
    for base in (128, 10, 245):
        c["near_%d" % base] = (W, H, _near(rng, W, H, base))
    c["noise_97x131"] = (97, 131, rng.integers(0, 256, (131, 97), dtype=np.uint8))
    return c


CASES = _make_cases()
# what each case is there for: polarity of its corners (d = ring darker, b = ring brighter) and the range of its scores
EXPECT = {"noise": ("db", 20, 254), "bright_blobs": ("d", 169, 169), "dark_blobs": ("b", 169, 169),
          "binary_15": ("d", 254, 254), "binary_85": ("b", 254, 254),
          "near_128": ("db", 20, 41), "near_10": ("db", 20, 41), "near_245": ("db", 20, 41), "noise_97x131": ("db", 20, 254)}

RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0),
        (-3, 1), (-2, 2), (-1, 3)]


def polarity_counts(img, T=20):
    """corners of the interior of `img` by the definition: nine contiguous ring pixels all < centre - T / all > centre + T"""
    a = img.astype(np.int32)
    h, w = a.shape
    c = a[3:h - 3, 3:w - 3]
    ring = np.stack([a[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in RING])

    def nine(m):
        m2 = np.concatenate([m, m[:8]])
        return np.any(np.stack([np.all(m2[k:k + 9], axis=0) for k in range(16)]), axis=0)
    darker, brighter = nine(ring < c - T), nine(ring > c + T)
    assert not np.any(darker & brighter)          # two 9-arcs of a 16-ring overlap
    return int(darker.sum()), int(brighter.sum())


def oracle_candidates(level_img):
    ox, oy, os_ = O.fast_nms(level_img, 20)
    lh, lw = level_img.shape
    keep = (ox >= 31) & (ox < lw - 31) & (oy >= 31) & (oy < lh - 31)
    return sorted(zip(oy[keep].tolist(), ox[keep].tolist(), os_[keep].tolist()))


def same_keypoints(g, o):
    return (len(g["xy"]) == len(o["xy"]) and all(np.array_equal(g[k], o[k]) for k in ("octave", "lx", "ly"))
            and np.array_equal(g["xy"], o["xy"]) and np.array_equal(g["desc"], o["desc"])
            and np.array_equal(g["response"].view(np.uint32), o["response"].view(np.uint32)))


@pytest.fixture(scope="module")
def contexts():
    made = {}

    def get(w, h):
        if (w, h) not in made:
            made[(w, h)] = Context(device=0, max_w=w, max_h=h, max_frames=2)
        return made[(w, h)]
    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def detected(contexts):
    """every case once through orb_detect_batch (the frame and its 180-degree turn as the batch of two), downloads kept"""
    out = {}
    for name, (w, h, img) in CASES.items():
        frames = [img, np.ascontiguousarray(img[::-1, ::-1])]
        ctx = contexts(w, h)
        ctx.orb_detect_batch(torch.from_numpy(np.stack(frames)).cuda())
        ctx.synchronize()
        cand = [[ctx.download_candidates(f, l) for l in range(8)] for f in range(2)]
        kp = [ctx.orb_download(f) if ctx.lib.evh_orb_count(ctx.h, f) else None for f in range(2)]
        out[name] = (frames, cand, kp)
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_candidates_per_level(detected, name):
    frames, cand, _ = detected[name]
    pol, smin, smax = EXPECT[name]
    for f, img in enumerate(frames):
        pyr = O.orb_pyramid(img)
        want = [oracle_candidates(pyr[l]) for l in range(8)]
        n0, ntot = len(want[0]), sum(len(x) for x in want)
        print("%s frame %d: oracle candidates level 0 %d, all levels %d" % (name, f, n0, ntot))
        assert n0 >= 50 and ntot >= 300, (n0, ntot)
        s0 = [s for _, _, s in want[0]]
        assert min(s0) >= smin and max(s0) <= smax and (smin != smax or set(s0) == {smin}), (min(s0), max(s0))
        if name.startswith("near") or name == "noise":
            assert min(s0) == 20                  # best = 21, the lowest corner there is (beside pixels of best = 20, which are none)
        for l in range(8):
            gx, gy, gs = cand[f][l]
            got = sorted(zip(gy.tolist(), gx.tolist(), gs.tolist()))
            assert got == want[l], "frame %d level %d: %d vs %d candidates" % (f, l, len(got), len(want[l]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_level0_polarity_is_what_the_case_says(name):
    """the frames hold the corners they are meant to hold (numpy, from the definition; no device involved in the count)"""
    nd, nb = polarity_counts(CASES[name][2])
    pol = EXPECT[name][0]
    print("%s: level-0 corners ring darker %d, ring brighter %d" % (name, nd, nb))
    if pol == "db":
        assert nd >= 40 and nb >= 40, (nd, nb)
    else:                                         # a gap between blobs can be a corner of the other kind: one in a hundred at most
        major, minor = (nd, nb) if pol == "d" else (nb, nd)
        assert major >= 1000 and 100 * minor <= major, (nd, nb)
    if name == "noise":
        assert nd >= 1000 and nb >= 1000 and 0.8 < nd / nb < 1.25, (nd, nb)


@pytest.mark.parametrize("name", sorted(CASES))
def test_keypoints_and_descriptors(detected, name):
    frames, _, kp = detected[name]
    for f, img in enumerate(frames):
        o = O.orb_detect(img)
        assert len(o["xy"]) > 0
        assert kp[f] is not None and same_keypoints(kp[f], o), f
