"""The heat-map colouring on the host: tests/heatmap_checks.py (the expected value of every comparison in test_gpu_heatmap.py)
against the reference's own expression on reference-captured fields, the blend against integer arithmetic, jet_lut against
values worked out by hand, and the argument checks of heatmap_frames."""
import json
import os

import numpy as np
import pytest

import heatmap_checks as HC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def grids():
    with open(os.path.join(ROOT, "tests", "golden", "plane_goldens.json")) as f:
        return json.load(f)["grids"]


def test_index_equals_the_reference_expression_on_the_captured_fields(grids):
    """processing_visualization.py:337-339 on all 45 fields, at every pixel whose cast is defined (t finite, below 2^31).  The
    reference's np.power(s, 0.5) is pow, one ulp off sqrt at some pixels: a pixel may be left out only if t lies within 1e-9 of
    an integer, and on these fields none is."""
    assert len(grids) == 45 and {"horizon", "nan", "huge", "pm_inf", "all_neg_inf"} <= {c["name"] for c in grids}
    compared = left_out = total = 0
    t_max = 0.0
    for c in grids:
        F = np.array(c["field"], np.float64).reshape(c["h"], c["w"], 2)
        with np.errstate(all="ignore"):
            want = np.uint8(255 * (np.power(np.sum(np.power(F, 2), axis=-1), 0.5) / 1000))
            t = 255.0 * (np.sqrt(F[..., 0] * F[..., 0] + F[..., 1] * F[..., 1]) / 1000.0)
            defined = np.isfinite(t) & (t < 2.0 ** 31)
            near = defined & (np.abs(t - np.rint(t)) < 1e-9)
        got = HC.color_index(F, 1000.0)
        assert got.min() >= 0 and got.max() <= 255
        differ = defined & (got != want)
        assert not (differ & ~near).any(), (c["name"], c["w"], c["h"])
        left_out += int((differ & near).sum())
        compared += int(defined.sum())
        total += defined.size
        if defined.any():
            t_max = max(t_max, float(t[defined & (t < 1e6)].max(initial=0.0)))
        # outside the defined range the index is 0 by this project's rule
        assert (got[~defined] == 0).all()
    print("pixels compared %d, left out %d, largest moderate t %.1f" % (compared, left_out, t_max))
    assert left_out == 0 and total == 4977 and 2 * compared > total     # most pixels have a defined cast
    assert t_max > 256                                     # the wrap is exercised


def test_saturating_and_non_finite_rules_on_hand_written_values():
    r = np.array([0.0, 3.9, 4.0, 999.9, 1000.0, 1003.9, 1004.0, 2000.0, 2 ** 31 / 255.0 * 1000 * 0.999, 8.5e9, 1e300, np.inf,
                  np.nan])
    F = np.stack([r, np.zeros_like(r)], axis=-1).reshape(1, -1, 2)
    with np.errstate(all="ignore"):
        t = 255.0 * (r / 1000.0)
    assert t[1] < 1 <= t[2] and t[3] < 255 == t[4] and t[5] < 256 <= t[6] and t[8] < 2 ** 31 < t[9]
    wrap = HC.color_index(F, 1000.0)[0]
    assert wrap.tolist() == [0, 0, 1, 254, 255, 255, 0, 510 & 255, int(t[8]) & 255, 0, 0, 0, 0]
    sat = HC.color_index(F, 1000.0, saturate=True)[0]
    assert sat.tolist() == [0, 0, 1, 254, 255, 255, 255, 255, 255, 255, 255, 255, 0]
    # both coordinates count, negative ones too, and the constant divides
    assert HC.color_index(np.array([[[-300.0, 400.0]]]), 1000.0)[0, 0] == 127        # r = 500, t = 127.5
    assert HC.color_index(np.array([[[-300.0, 400.0]]]), 37.5)[0, 0] == 3400 & 255 == 72
    assert HC.color_index(np.array([[[-np.inf, 1.0]], [[np.inf, -np.inf]], [[np.nan, 0.0]]]), 1000.0).ravel().tolist() == [0, 0, 0]
    assert HC.color_index(np.array([[[-np.inf, 1.0]], [[np.nan, 0.0]]]), 1000.0, saturate=True).ravel().tolist() == [255, 0]


@pytest.mark.parametrize("alpha", [0.8, 0.0, 1.0, 2.5])
def test_blend_exhaustively(alpha):
    c, p = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    got = HC.blend(c, p, alpha).astype(np.int64)
    if alpha == 0.8:
        want = np.minimum(255, p + (8 * c + 5) // 10)
        # the form the kernel takes behind its exact test for 0.8: the table byte scaled once, then an integer sum
        assert np.array_equal(np.minimum(255, p + np.rint(c * 0.8).astype(np.int64)), want)
    elif alpha == 0.0:
        want = p
    elif alpha == 1.0:
        want = np.minimum(255, c + p)
    else:
        twice = 5 * c + 2 * p                               # 2 * (2.5 c + p), exact: an odd value is a half
        want = np.minimum(255, twice // 2 + ((twice & 1) & ((twice // 2) & 1)))
        assert (twice & 1).any()
    assert np.array_equal(got, want)
    # and element by element against Python's round(), which rounds halves to even
    for ci, pi in ((0, 0), (1, 0), (1, 1), (3, 0), (5, 7), (255, 0), (255, 255), (101, 4)):
        assert got[ci, pi] == min(255, round(float(ci) * alpha + float(pi)))
    # without frames (p = 0) the scaled table is the picture, whatever alpha
    assert np.array_equal(got[:, 0], np.minimum(255, np.rint(np.arange(256) * np.float64(alpha))))


def test_jet_lut():
    from evenvizion_amd.heatmap import jet_lut
    lut = jet_lut()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    # v2 = clamp(765 - 2 * |4 j - 255 k|, 0, 510), halves to even; B, G, R = k 1, 2, 3
    by_hand = {0: (128, 0, 0),            # 255/2 = 127.5 -> 128
               32: (255, 0, 0),           # 511 -> 510; 1/2 -> 0
               96: (254, 255, 2),         # 507/2 = 253.5 -> 254; 513 -> 510; 3/2 -> 2
               128: (126, 255, 130),      # 251/2 = 125.5 -> 126; 761 -> 510; 259/2 = 129.5 -> 130
               160: (0, 252, 255),        # -5 -> 0; 505/2 = 252.5 -> 252; 515 -> 510
               224: (0, 0, 252),          # 503/2 = 251.5 -> 252
               255: (0, 0, 128)}
    for j, bgr in by_hand.items():
        assert tuple(int(v) for v in lut[j]) == bgr, j
    assert np.array_equal(lut[:, 0], lut[::-1, 2])                    # B and R are mirror images
    assert np.array_equal(lut[:, 1], lut[::-1, 1])
    assert not jet_lut() is lut                                       # a fresh array each time


class NeverRead:
    def __getattr__(self, name):
        raise AssertionError("the capture was touched: %s" % name)


@pytest.mark.parametrize("bad", [dict(ingest="rgb"), dict(heatmap_constant=0), dict(heatmap_constant=-5.0), dict(heatmap_constant=np.nan),
                                 dict(heatmap_constant=np.inf), dict(alpha=-0.1), dict(alpha=np.inf), dict(alpha=np.nan),
                                 dict(lut=np.zeros((256, 3), np.int32)), dict(lut=np.zeros((255, 3), np.uint8)),
                                 dict(lut=np.zeros((256, 4), np.uint8)), dict(chunk_frames=0), dict(resize_info={"w": 0, "h": 4})])
def test_heatmap_frames_refuses_bad_arguments_before_anything_is_opened(bad, monkeypatch):
    from evenvizion_amd import heatmap, runtime

    def no_context(*a, **k):
        raise AssertionError("a context was opened")

    monkeypatch.setattr(runtime, "get_context", no_context)
    kw = dict(resize_info={"w": 8, "h": 4})
    kw.update(bad)
    ri = kw.pop("resize_info")
    with pytest.raises(ValueError):
        heatmap.heatmap_frames(NeverRead(), {1: np.eye(3)}, ri, **kw)
