"""Host side of the stabilised view: the numpy restatement of evh_warp_fixed_plane (tests/warp_checks.py) against plain
copies and pastes, evenvizion_amd.stabilization's canvas geometry against the reference-recorded fixture
(tests/golden/stabilization_goldens.json, written by make_stabilization_goldens.py), the translate offsets, the PPM writer."""
import json
import os

import numpy as np
import pytest

import warp_checks as W
from evenvizion_amd import stabilization as S

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def stab_goldens():
    with open(os.path.join(HERE, "golden", "stabilization_goldens.json")) as f:
        g = json.load(f)
    g["sup"] = {int(k): np.array(v, np.float64).reshape(3, 3) for k, v in g["sup"].items()}
    return g


def paste(canvas, frame, x, y):
    """frame's pixels onto canvas with its upper left corner at canvas pixel (x, y), clipped to the canvas"""
    h, w = frame.shape[:2]
    ch, cw = canvas.shape[:2]
    x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, cw), min(y + h, ch)
    if x1 > x0 and y1 > y0:
        canvas[y0:y1, x0:x1] = frame[y0 - y:y1 - y, x0 - x:x1 - x]
    return canvas


FRAMES = np.random.default_rng(11).integers(0, 256, (5, 17, 23, 3), dtype=np.uint8)
OFFSETS = [(0, 0), (5, -3), (-4, 6), (12, 9), (3, 2)]           # overlapping, two of them cut by the canvas edge


@pytest.mark.parametrize("gray", [False, True])
def test_identity_copies(gray):
    src = FRAMES[0, ..., 0] if gray else FRAMES[0]
    val, cov = W.warp_frame(src, np.eye(3), 23, 17)
    assert cov.all() and np.array_equal(val, src)
    val, cov = W.warp_frame(src, np.eye(3), 23, 17, inverse_map=True)
    assert cov.all() and np.array_equal(val, src)


@pytest.mark.parametrize("origin", [(0, 0), (-7, -5), (4, 2)])
@pytest.mark.parametrize("offset", [(5, -3), (-4, 6), (0, 0)])
def test_integer_translation_pastes(origin, offset):
    dw, dh = 40, 30
    val, cov = W.warp_frame(FRAMES[1], W.translation(*offset), dw, dh, origin)
    got = np.where(cov[..., None], val, 0).astype(np.uint8)
    want = paste(np.zeros((dh, dw, 3), np.uint8), FRAMES[1], offset[0] - origin[0], offset[1] - origin[1])
    assert np.array_equal(got, want)
    assert np.array_equal(cov, paste(np.zeros((dh, dw), bool), np.ones((17, 23), bool), offset[0] - origin[0], offset[1] - origin[1]))


def test_mosaic_is_the_sequential_paste_and_history_its_prefixes():
    dw, dh, origin = 36, 28, (-6, -4)
    background = np.random.default_rng(12).integers(0, 256, (dh, dw, 3), dtype=np.uint8)
    mats = np.stack([W.translation(*o) for o in OFFSETS])
    want = background.copy()
    prefixes = []
    for f, (x, y) in zip(FRAMES, OFFSETS):
        paste(want, f, x - origin[0], y - origin[1])
        prefixes.append(want.copy())
    assert np.array_equal(W.warp_canvases(FRAMES, mats, "mosaic", dw, dh, origin, background), want)
    history = W.warp_canvases(FRAMES, mats, "history", dw, dh, origin, background)
    for k in range(len(FRAMES)):
        assert np.array_equal(history[k], prefixes[k])
        assert np.array_equal(history[k], W.warp_canvases(FRAMES[:k + 1], mats[:k + 1], "mosaic", dw, dh, origin, background))
    each = W.warp_canvases(FRAMES, mats, "each", dw, dh, origin, background)
    for k, (x, y) in enumerate(OFFSETS):
        assert np.array_equal(each[k], paste(background.copy(), FRAMES[k], x - origin[0], y - origin[1]))


@pytest.mark.parametrize("M", [np.zeros((3, 3)), np.full((3, 3), np.nan), np.ones((3, 3)), np.eye(3) * 1e300, np.eye(3) * 1e-300])
def test_degenerate_matrices_cover_nothing(M):
    assert not W.warp_frame(FRAMES[0], M, 9, 7, (-2, -2))[1].any()


def shifted(goldens, case):
    d = {k: goldens["sup"][k].copy() for k in range(case["first"], case["last"] + 1)}
    for m in d.values():
        m[0][2] -= case["shift"][0] * m[2][2]
        m[1][2] -= case["shift"][1] * m[2][2]
    return d


def test_reference_system_and_panorama_shape_match_the_reference(stab_goldens):
    assert len(stab_goldens["cases"]) >= 6
    for case in stab_goldens["cases"]:
        corner = S.get_reference_system(shifted(stab_goldens, case))
        assert corner == case["corner_dict"], case["name"]
        assert all(type(v) is int for v in corner.values())
        for s in case["shapes"]:
            assert S.panorama_shape(corner, s["frame_shape"]) == s["panorama_shape"], (case["name"], s["width"])
            assert S.panorama_shape(corner, tuple(s["frame_shape"]) + (3,)) == s["panorama_shape"]


def test_translate_offsets_of_every_frame(stab_goldens):
    sup, ri = stab_goldens["sup"], stab_goldens["resize_info"]
    assert sorted(sup) == list(range(1, 122))
    ox, oy, dw, dh, matrix_of = S._placement(sup, ri, "translate", 1.0, 1170, 658, 1 << 30)
    corner = S.get_reference_system(sup)
    assert [dh, dw] == S.panorama_shape(corner, (ri["h"], ri["w"])) and (ox, oy) == (-abs(corner["min_x"]), -abs(corner["min_y"]))
    for k in range(1, 122):
        v = np.dot(sup[k], [0, 0, 1])
        want = (int(v[0] / v[2]), int(v[1] / v[2]))
        assert S.translate_offset(sup[k]) == want
        assert np.array_equal(matrix_of(k), [1, 0, want[0], 0, 1, want[1], 0, 0, 1])
    assert np.isnan(matrix_of(500)).all()                         # a frame without a matrix leaves the canvas alone


def test_fixed_plane_bounds(stab_goldens):
    sup, ri = stab_goldens["sup"], stab_goldens["resize_info"]
    w, h = ri["w"], ri["h"]
    assert S.fixed_plane_bounds({1: np.eye(3)}, ri) == (0, 0, w + 1, h + 1)
    assert S.fixed_plane_bounds({1: np.eye(3), 2: None, 3: np.full((3, 3), np.nan)}, ri, scale=0.5) == (0, 0, w // 2 + 1, h // 2 + 1)
    ox, oy, dw, dh = S.fixed_plane_bounds(sup, ri)
    lo, hi = np.full(2, np.inf), np.full(2, -np.inf)
    for m in sup.values():
        for x, y in ((0, 0), (w, 0), (0, h), (w, h)):
            p = np.dot(m, [x, y, 1.0])
            lo, hi = np.minimum(lo, p[:2] / p[2]), np.maximum(hi, p[:2] / p[2])
    assert (ox, oy) == (int(np.floor(lo[0])), int(np.floor(lo[1])))
    assert (ox + dw - 1, oy + dh - 1) == (int(np.ceil(hi[0])), int(np.ceil(hi[1])))
    with pytest.raises(ValueError):
        S.fixed_plane_bounds(sup, ri, max_pixels=dw * dh - 1)
    with pytest.raises(ValueError):
        S.fixed_plane_bounds({1: None}, ri)
    with pytest.raises(ValueError):                                # the horizon x = 10 crosses the frame
        S.fixed_plane_bounds({1: [[1, 0, 0], [0, 1, 0], [-0.1, 0, 1]]}, ri)


def read_ppm(path):
    """A binary P6 file with maxval 255 -> u8[h,w,3] in the file's RGB order."""
    data = open(path, "rb").read()
    magic, w, h, maxval = data.split(None, 4)[:4]
    assert magic == b"P6" and maxval == b"255"
    header = len(data) - int(w) * int(h) * 3
    assert data[header - 1:header].isspace()
    return np.frombuffer(data, np.uint8, int(w) * int(h) * 3, header).reshape(int(h), int(w), 3)


def test_ppm_round_trip(tmp_path):
    img = np.random.default_rng(13).integers(0, 256, (7, 5, 3), dtype=np.uint8)
    path = str(tmp_path / "000001.ppm")
    S.write_ppm(path, img)
    raw = open(path, "rb").read()
    assert raw.startswith(b"P6\n5 7\n255\n") and len(raw) == 11 + 7 * 5 * 3
    assert raw[11:14] == bytes(img[0, 0, ::-1])                   # P6 is RGB, the frames are BGR
    assert np.array_equal(read_ppm(path)[:, :, ::-1], img)
    with pytest.raises(ValueError):
        S.write_ppm(path, img[..., 0])


def test_stabilize_help_says_what_is_not_drawn(capsys):
    from evenvizion_amd import stabilize
    with pytest.raises(SystemExit):
        stabilize.main(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    for word in ("--mode", "--placement", "--scale", "--path_to_homography_dict", "--path_to_video", "--experiment_name",
                 "no text", "no border", "no dimming"):
        assert word in text, word
