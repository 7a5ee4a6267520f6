"""evenvizion_amd.stabilization.stabilized_frames on the reference video with its recorded homography dictionary."""
import itertools
import json
import os

import numpy as np
import pytest

import warp_checks as W
from evenvizion_amd import capture
from evenvizion_amd import stabilization as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MP4 = os.path.join(ROOT, "tests", "golden", "ref_test_video.mp4")
GOLD = os.path.join(ROOT, "tests", "golden", "ref_dict_with_homography_matrix.json")


class First:
    """The first n frames of a capture, with whatever ways of reading it offers."""

    def __init__(self, cap, n):
        self.cap, self.left = cap, n
        self.width, self.height, self.bgr_mode = cap.width, cap.height, cap.bgr_mode

    def read(self):
        if self.left == 0:
            return False, None
        self.left -= 1
        return self.cap.read()

    def read_yuv420_into(self, y, cb, cr):
        if self.left == 0:
            return False
        self.left -= 1
        return self.cap.read_yuv420_into(y, cb, cr)


@pytest.fixture(scope="module")
def recorded():
    from evenvizion_amd.processing.utils import read_homography_dict, superposition_dict
    hd, ri = read_homography_dict(GOLD)
    return superposition_dict(hd), ri


def first_frames(n):
    cap = capture.VideoCapture(MP4)
    frames = [cap.read()[1] for _ in range(n)]
    assert all(f is not None for f in frames)
    return np.stack(frames)


def test_translate_history_is_the_reference_paste(recorded):
    import torch
    from evenvizion_amd import runtime
    sup, ri = recorded
    n, w, h = 12, ri["w"], ri["h"]
    frames = first_frames(n)
    small = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    ctx = runtime.get_context(64, 64)
    ctx.resize_area(torch.from_numpy(frames).cuda(), small)
    ctx.synchronize()
    small = small.cpu().numpy()
    with open(os.path.join(ROOT, "tests", "golden", "stabilization_goldens.json")) as f:
        case = [c for c in json.load(f)["cases"] if c["name"] == "all"][0]
    shape = [s["panorama_shape"] for s in case["shapes"] if s["width"] == w][0]
    corner = case["corner_dict"]
    canvas = np.zeros(tuple(shape) + (3,), np.uint8)
    gen = S.stabilized_frames(capture.VideoCapture(MP4), sup, ri, mode="history", placement="translate", chunk_frames=5)
    got = list(itertools.islice(gen, n))
    gen.close()
    assert [k for k, _ in got] == list(range(1, n + 1))
    for k, picture in got:
        v = np.dot(np.asarray(sup[k], np.float64), [0, 0, 1])
        x, y = abs(corner["min_x"]) + int(v[0] / v[2]), abs(corner["min_y"]) + int(v[1] / v[2])
        canvas[y:y + h, x:x + w] = small[k - 1]                          # stabilize_view's paste (stabilization.py:162-165)
        assert list(picture.shape[:2]) == shape and picture.dtype == np.uint8
        assert np.array_equal(picture, canvas), k


def test_warp_mosaic_does_not_depend_on_the_chunks(recorded):
    sup, ri = recorded
    n = 24
    pictures = []
    for chunk in (5, 32):
        got = list(S.stabilized_frames(First(capture.VideoCapture(MP4), n), sup, ri, mode="mosaic", placement="warp",
                                       chunk_frames=chunk))
        assert len(got) == 1 and got[0][0] == n
        pictures.append(got[0][1])
    ox, oy, dw, dh = S.fixed_plane_bounds(sup, ri)
    assert pictures[0].shape == (dh, dw, 3) and pictures[0].any()
    assert np.array_equal(pictures[0], pictures[1])
    # and it is the warp of the full-size frames through H_sup . diag(kx, ky, 1)
    m = 6
    frames = first_frames(m)
    K = np.diag([ri["w"] / frames.shape[2], ri["h"] / frames.shape[1], 1.0])
    mats = [np.dot(np.dot(np.eye(3), np.asarray(sup[k + 1], np.float64)), K) for k in range(m)]
    got = list(S.stabilized_frames(First(capture.VideoCapture(MP4), m), sup, ri, mode="mosaic", placement="warp", chunk_frames=4))
    assert np.array_equal(got[0][1], W.warp_canvases(frames, mats, "mosaic", dw, dh, (ox, oy)))


def test_planes_and_bgr_frames_give_the_same_pictures(recorded):
    sup, ri = recorded
    n = 12
    runs = {}
    for ingest in ("auto", "bgr"):
        runs[ingest] = list(S.stabilized_frames(First(capture.VideoCapture(MP4), n), sup, ri, mode="history", placement="warp",
                                                scale=0.5, chunk_frames=5, ingest=ingest))
    assert [k for k, _ in runs["auto"]] == list(range(1, n + 1)) == [k for k, _ in runs["bgr"]]
    for (_, a), (_, b) in zip(runs["auto"], runs["bgr"]):
        assert a.any() and np.array_equal(a, b)
    # a frame without a matrix leaves the canvas as it was
    holes = {k: (None if k == 3 else np.full((3, 3), np.nan) if k == 4 else v) for k, v in sup.items()}
    got = list(S.stabilized_frames(First(capture.VideoCapture(MP4), 5), holes, ri, mode="history", placement="warp", scale=0.5))
    assert np.array_equal(got[2][1], got[1][1]) and np.array_equal(got[3][1], got[1][1]) and not np.array_equal(got[4][1], got[1][1])
