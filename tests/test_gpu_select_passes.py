"""GPU: k_select_cv's passes over memory (row-major placement, per-wave partition sweeps, the lists cut to the pairs that can
swap) on level-0 corner lists of chosen length and chosen score sequence.

The frames are dot lattices: flat background 0, one pixel of value score + 1 every 5 pixels from (31, 31), filled row by row
from a list of FAST scores.  Level 0 then has exactly the dots as corners, in row-major order with exactly those scores, so
the sequence nth_element / partition permute is the list itself.  Two faint pixels per dot (values 0..20, off every ring)
vary the Harris response without touching the FAST score: the second retainBest does not tie even where the first does.
Every frame is compared with the oracle as tests/test_gpu_order.py does: order, octave, level coordinates, response bits,
descriptors."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from evenvizion_amd._lib import Context  # noqa: E402
from oracle import oracle as O  # noqa: E402

PITCH = 5
QUOTA0 = 109   # level-0 quota at 500 features: retainBest(2 * QUOTA0) by FAST score, then retainBest(QUOTA0) by Harris

# Lengths of the level-0 list.
#   217 218 219 222: around 2 * quota = 218 (retainBest returns early up to it) and introselect's "<= 3 left" insertion sort
#   255 .. 2049:     powers of two +-1, among them
#     CV_SMALL = 2048 (the LDS range of retainBest; up to it the row-major pass writes straight into LDS; 2049 is the first
#     length whose passes run on global memory with 32-bit lists)
#   2045 2049 2050:  the first Hoare pass runs over [1, n) and gives each of the four waves seg = ceil((n - 1) / 4) elements,
#     swept CV_WSTEP = 512 at a time: seg = 511 at 2045 (one short step, in LDS), 512 at 2049 (exactly one full step, global),
#     513 at 2050 (a full step and a step of one element, global)
#   2245 6960:       beyond the 400 x 224 lattice (2244 dots): several steps per wave, global lists
LENGTHS_SMALL = [217, 218, 219, 222, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2045, 2047, 2048, 2049, 2050]
LENGTHS_MID = [2245, 6960]
# Frame sizes around the two switches of the row-major tables, whose size depends on the tile grid alone
# (TY * (88 * TX + 112) bytes; 1280 wide: TX = 10, 992 bytes per tile row):
#   CV_TAB_BYTES - 4 * CV_SMALL = 16384: 1280 x 510 (16 tile rows, 15872) stages the sequence in LDS, 1280 x 511 (17) does not
#   CV_TAB_BYTES = 24576:                1280 x 734 (24 tile rows, 23808) keeps the tables in LDS, 1280 x 735 (25) in global memory
TABLE_SWITCH = [(1280, 510, 2000), (1280, 511, 2000), (1280, 734, 20000), (1280, 735, 20000)]

KINDS = ["random", "three", "equal", "falling", "rising", "cut"]


def scores_of(kind, n, rng):
    if kind == "random":
        return rng.integers(21, 255, n)
    if kind == "three":        # nearly every element stops both scans; the tail partition has hundreds of ties
        return rng.choice([60, 61, 200], n)
    if kind == "equal":
        return np.full(n, 137)
    if kind in ("falling", "rising"):   # monotone in row-major order, ties where n > 234
        up = 21 + (np.arange(n) * 234) // n
        return up if kind == "rising" else up[::-1]
    if kind == "cut":          # exactly 217 above the cut: position n - 1 of the best 218 holds one of the 50s, no tie survives
        s = np.full(n, 50)
        s[:217] = 200
        return rng.permutation(s)
    raise ValueError(kind)


def lattice_sites(w, h):
    gx, gy = np.meshgrid(np.arange(31, w - 31, PITCH), np.arange(31, h - 31, PITCH))
    return gx.ravel(), gy.ravel()


def lattice(w, h, scores, rng):
    px, py = lattice_sites(w, h)
    n = len(scores)
    assert n <= len(px)
    px, py = px[:n], py[:n]
    img = np.zeros((h, w), np.uint8)
    img[py, px] = np.asarray(scores) + 1
    img[py + 1, px + 1] = rng.integers(0, 21, n)
    img[py - 1, px + 1] = rng.integers(0, 21, n)
    return img


def same_keypoints(g, o):
    return (len(g["xy"]) == len(o["xy"]) and all(np.array_equal(g[k], o[k]) for k in ("octave", "lx", "ly"))
            and np.array_equal(g["xy"], o["xy"]) and np.array_equal(g["desc"], o["desc"])
            and np.array_equal(g["response"].view(np.uint32), o["response"].view(np.uint32)))


def check_batch(w, h, score_lists, seed):
    """one orb_detect_batch over one lattice frame per score list, each frame against the oracle"""
    rng = np.random.default_rng(seed)
    frames = np.stack([lattice(w, h, s, rng) for s in score_lists])
    c = Context(device=0, max_w=w, max_h=h, max_features=500, max_frames=max(2, len(frames)))
    try:
        cap = c.lib.evh_orb_capacity(c.h)
        c.orb_detect_batch(torch.from_numpy(frames).cuda())
        for f, (img, s) in enumerate(zip(frames, score_lists)):
            xs, ys, sc = O.fast_nms(img)
            order = np.lexsort((xs, ys))
            assert len(sc) == len(s), (f, len(sc), len(s))                 # level 0 has exactly the dots as corners ...
            assert np.array_equal(sc[order], np.asarray(s)), f            # ... with the chosen scores in row-major order
            want = O.orb_detect(img)
            assert len(want["xy"]) <= cap, (f, len(want["xy"]), cap)
            assert same_keypoints(c.orb_download(f), want), (f, len(s))
    finally:
        c.close()


@pytest.mark.parametrize("n", LENGTHS_SMALL)
def test_lengths_on_the_small_lattice(n):
    kinds = KINDS if n > 2 * QUOTA0 else ["random"]
    rng = np.random.default_rng(1000 + n)
    check_batch(400, 224, [scores_of(k, n, rng) for k in kinds], 2000 + n)


@pytest.mark.parametrize("n", LENGTHS_MID)
def test_lengths_beyond_the_small_lattice(n):
    rng = np.random.default_rng(1000 + n)
    check_batch(640, 360, [scores_of(k, n, rng) for k in KINDS], 2000 + n)


@pytest.mark.parametrize("w,h,n", TABLE_SWITCH)
def test_table_placement_switches(w, h, n):
    rng = np.random.default_rng(1000 + h)
    check_batch(w, h, [scores_of(k, n, rng) for k in ("random", "three")], 2000 + h)


def test_frames_of_different_length_in_one_batch():
    """per-workgroup state: neighbours in the batch take different paths (early return, LDS, global lists)"""
    rng = np.random.default_rng(7)
    lens = [2049, 219, 1025, 217, 2244, 256]
    check_batch(400, 224, [scores_of(k, n, rng) for n, k in zip(lens, ["three", "random", "cut", "random", "equal", "rising"])], 8)


@pytest.mark.parametrize("kind", ["random", "three"])
def test_level_longer_than_16_bit_positions(kind):
    """66 000 corners on level 0: more than 65 535 elements in one range, dozens of steps per wave"""
    rng = np.random.default_rng(66)
    check_batch(1600, 1200, [scores_of(kind, 66000, rng)], 67)
