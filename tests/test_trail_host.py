"""Host side of the trail (evh_trail_fixed_plane, include/evhip.h): the colour step of tests/trail_checks.py over all 2^24
colours, its literal restatement against the vectorised one, the rectangle of change_frame_location against the recorded
corner dictionary, and the refusals of the Python arguments."""
import json
import os

import numpy as np
import pytest

import trail_checks as T
import warp_checks as W
from evenvizion_amd import stabilization as S

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the colour step over every colour ---------------------------------------------------------------------------------------------
def test_tables_are_the_fixed_point_reciprocals():
    assert T.S_TAB[0] == 0 and T.H_TAB[0] == 0 and T.S_TAB[255] == 4096 and T.S_TAB[1] == 255 << 12
    assert T.H_TAB[1] == 122880 and T.H_TAB[255] == 482                  # 737280 / 1530 = 481.88
    assert T.S_TAB[2] == 522240 and T.H_TAB[4] == 30720                  # exact quotients stay exact
    assert T.C6 == np.float32(6.0) / np.float32(180.0) and T.K255 == np.float32(1.0) / np.float32(255.0)


def test_hsv_ranges_over_every_colour():
    frame = T.every_colour()[0]
    for rows in range(0, 4096, 1024):
        h, s, v = T.to_hsv(frame[rows:rows + 1024])
        assert h.min() == 0 and h.max() <= 179 and s.min() == 0 and s.max() <= 255 and v.min() >= 0 and v.max() <= 255
    # grays have no hue and no saturation; the primaries sit at 0, 60 and 120
    assert [tuple(int(a) for a in T.to_hsv(np.array(p, np.uint8))) for p in ((7, 7, 7), (0, 0, 255), (0, 255, 0), (255, 0, 0))] == \
        [(0, 0, 7), (0, 255, 255), (60, 255, 255), (120, 255, 255)]


def test_keep_lowers_the_largest_channel_by_two():
    frame, kept, _, value = T.every_colour()
    assert np.array_equal(value, frame.max(axis=-1))
    assert np.array_equal(kept.max(axis=-1), np.maximum(value - 2, 0))


def test_every_colour_is_black_after_128_steps():
    """keep strictly lowers the largest channel (the test above), so the number of steps to black follows colour by colour
    from the colours below: steps(p) = 1 + steps(keep(p)), filled in order of the largest channel."""
    frame, kept, _, value = T.every_colour()
    assert (kept.max(axis=-1) < np.maximum(value, 1)).all()
    code = lambda p: p[..., 0].astype(np.int64) | p[..., 1].astype(np.int64) << 8 | p[..., 2].astype(np.int64) << 16
    nxt = code(kept).reshape(-1)                                        # pixel i of the frame holds the colour with code i
    assert np.array_equal(code(frame).reshape(-1), np.arange(1 << 24))
    steps = np.full(1 << 24, -1, np.int64)
    steps[0] = 0
    order = value.reshape(-1)
    for m in range(256):
        sel = np.flatnonzero(order == m)
        sel = sel[sel != 0]
        assert (steps[nxt[sel]] >= 0).all()
        steps[sel] = 1 + steps[nxt[sel]]
    assert steps.min() == 0 and steps.max() <= 128
    assert steps.max() == 128 and steps[255] == 128                     # (255, 0, 0) takes all of them


def test_show_is_the_constant_below_two_and_keep_above():
    frame, kept, shown, value = T.every_colour()
    dim = value < 2
    assert dim.sum() == 8 and (shown[dim] == np.array(T.DARK, np.uint8)).all()
    assert np.array_equal(T.show(np.zeros(3, np.uint8)), np.array(T.DARK, np.uint8))
    assert np.array_equal(T.from_hsv(*T.DARK_HSV), np.array(T.DARK, np.uint8))       # h = 222 wraps into sector 1
    assert np.array_equal(shown[~dim], kept[~dim])
    assert not kept[dim].any()
    assert tuple(T.show(np.array(T.WHITE, np.uint8))) == (253, 253, 253)


# ---- the trail: a pixel at a time == whole canvases ------------------------------------------------------------------------------
def small_sequence():
    rng = np.random.default_rng(41)
    n, sw, sh, dw, dh = 6, 5, 4, 13, 11
    frames = rng.integers(0, 256, (n, sh, sw, 3), dtype=np.uint8)
    frames[1, 0, 0] = 255
    frames[2, 1, 1] = (1, 0, 1)
    mats = [W.translation(2, 1), W.translation(6, 5), np.full((3, 3), np.nan), W.translation(-2, 8), W.translation(10.5, -1.25),
            np.array([[1.1, 0.05, 3], [-0.04, 0.95, 2], [1e-3, -2e-3, 1]])]
    rects = np.array([[2, 1, 7, 5], [6, 5, 11, 9], [0, 0, 12, 10], [-2, 8, 3, 12], [4, 4, 3, 9], [5, 5, 5, 5]], np.int32)
    canvas = rng.integers(0, 256, (dh, dw, 3), dtype=np.uint8)
    return frames, np.stack(mats), canvas, rects


@pytest.mark.parametrize("with_rects", [True, False])
def test_literal_trail_equals_the_vectorised_one(with_rects):
    frames, mats, canvas, rects = small_sequence()
    rects = rects if with_rects else None
    want_pictures, want_canvas = T.trail_literal(frames, mats, canvas, (-1, -1), rects)
    pictures, after = T.trail(frames, mats, canvas, (-1, -1), rects)
    assert np.array_equal(pictures, want_pictures) and np.array_equal(after, want_canvas)
    assert (pictures[2] != pictures[1]).any()                           # a frame that covers nothing still dims
    if with_rects:
        assert (pictures[0, 1, 2:8] == 253).all() and (pictures[4] != 253).any()
        plain = T.trail(frames, mats, canvas, (-1, -1), None)
        assert np.array_equal(plain[1], after)                          # the outline never reaches the carried canvas
        assert (plain[0] != pictures).any()


# ---- the rectangle ---------------------------------------------------------------------------------------------------------------
def test_frame_outline_is_change_frame_locations_rectangle():
    with open(os.path.join(HERE, "golden", "stabilization_goldens.json")) as f:
        g = json.load(f)
    case = [c for c in g["cases"] if c["name"] == "all"][0]
    corner, w, h = case["corner_dict"], g["resize_info"]["w"], g["resize_info"]["h"]
    shape = [s["panorama_shape"] for s in case["shapes"] if s["width"] == w][0]
    for k in range(1, 13):
        H = np.array(g["sup"][str(k)], np.float64).reshape(3, 3)
        v = np.dot(H, [0, 0, 1])
        x_offset, y_offset = int(v[0] / v[2]), int(v[1] / v[2])
        assert (x_offset, y_offset) == S.translate_offset(H)
        x0, y0, x1, y1 = S.frame_outline(abs(corner["min_x"]), abs(corner["min_y"]), x_offset, y_offset, w, h)
        # the four cv2.line calls (stabilization.py:76-96): their end points, and the paste of stabilize_view inside them
        assert (x0, y0) == (np.abs(corner["min_x"]) + x_offset, np.abs(corner["min_y"]) + y_offset)
        assert (x1, y1) == (np.abs(corner["min_x"]) + x_offset + w, np.abs(corner["min_y"]) + y_offset + h)
        assert 0 <= x0 and 0 <= y0 and x1 < shape[1] and y1 < shape[0]  # the recorded canvas holds it whole
    assert S.frame_outline(3, 4, -3, -4, 400, 224) == (0, 0, 400, 224)


# ---- refusals of the Python arguments, before anything is opened ---------------------------------------------------------------------
class NoCapture:
    def __getattr__(self, name):
        raise AssertionError("the capture was touched before the arguments were checked")


@pytest.mark.parametrize("kw", [dict(trail=True, mode="each"), dict(trail=True, mode="mosaic"),
                                dict(trail=True, border=True, placement="warp"), dict(trail=True, border="yes"), dict(trail=True, border=1),
                                dict(border=True)])
def test_stabilized_frames_refuses_before_the_device(kw):
    sup = {1: np.eye(3)}
    with pytest.raises(ValueError):
        next(S.stabilized_frames(NoCapture(), sup, {"w": 8, "h": 6}, **dict(dict(mode="history", placement="translate"), **kw)))


def test_comparison_frames_refuses_before_the_device():
    sup = {1: np.eye(3)}
    for kw in (dict(placement="warp", border=True), dict(height=0), dict(canvas_border=(0, 0, 256)), dict(canvas_border=(1, 2))):
        with pytest.raises(ValueError):
            next(S.comparison_frames(NoCapture(), sup, {"w": 8, "h": 6}, **kw))
    assert S.comparison_size(1170, 658, 895, 254, 300) == ((int(1170 * (300 / 658.0)), int(895 * (300 / 254.0))), 300)
    assert S.comparison_size(1170, 658, 895, 254, 300)[0][0] == 533


def test_stabilize_help_lists_the_trail_and_the_comparison(capsys):
    from evenvizion_amd import stabilize
    with pytest.raises(SystemExit):
        stabilize.main(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    for word in ("--comparison", "--trail", "PNG", "never drawn"):
        assert word in text, word
    with pytest.raises(SystemExit):
        stabilize.main(["--trail", "1", "--mode", "each"])
