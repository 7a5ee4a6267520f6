"""The steady view end to end on the device: steady.steady_frames over a crafted jittered pan equals the numpy restatement
(tests/steady_checks.py) driven by the same tables, steady_jpegs gives the files of those pictures, and the command line writes
steady.avi and steady_report.json for the recorded video."""
import json
import os

import numpy as np
import pytest

import steady_checks as C
from evenvizion_amd import steady, synthetic
from evenvizion_amd.pictures import encode_jpeg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MP4 = os.path.join(ROOT, "tests", "golden", "ref_test_video.mp4")
GOLD = os.path.join(ROOT, "tests", "golden", "ref_dict_with_homography_matrix.json")
N, W, H = 12, 96, 64
PATH = dict(radius=3, sigma=None, max_zoom=1.5)


@pytest.fixture(scope="module")
def pan():
    """A pan of 3 pixels per frame with a jitter of up to 2 pixels and half a degree: frame k shows a textured canvas through the
    pose G_k, which is its matrix into the fixed plane.  -> (frames u8[N,H,W,3], {frame_no: G}, resize_info)"""
    rng = np.random.Generator(np.random.PCG64(11))
    canvas = synthetic.make_canvas(rng, W + 3 * N, H)
    frames, sup = [], {}
    for k in range(1, N + 1):
        a = np.deg2rad(rng.uniform(-0.5, 0.5))
        G = np.array([[np.cos(a), -np.sin(a), 3.0 * k + rng.uniform(-2, 2)], [np.sin(a), np.cos(a), rng.uniform(-2, 2)], [0, 0, 1.0]])
        gray = synthetic.warp_canvas(canvas, G, W, H)
        frames.append(np.stack([gray, np.roll(gray, 2, axis=1), 255 - gray], -1))
        sup[k] = G
    return np.ascontiguousarray(np.stack(frames)), sup, {"w": W, "h": H}


def cap(frames):
    return synthetic.SyntheticCapture(list(frames))


def restated(frames, sup, ri, zoom, fill, feather_px, scale=1.0):
    """The pictures from the whole video as one chunk: the tables of steady_taps, the restatement of the entry."""
    B = steady.smooth_path(sup, ri, zoom=zoom, **PATH)
    tap_frame, tap_M = steady.steady_taps(B, sup, ri, (W, H), 1, len(frames), fill, scale)
    dw, dh = steady.output_size((W, H), scale)
    return C.steady_frames(frames, tap_frame, tap_M, dw, dh, int(round(feather_px * 32)))


@pytest.mark.parametrize("fill,feather_px,chunk,scale", [(2, 4, 8, 1.0), (1, 0, 5, 1.0), (2, 8, 12, 0.5), (0, 8, 4, 1.0)])
def test_pictures_equal_the_restatement_driven_by_the_same_tables(pan, fill, feather_px, chunk, scale):
    frames, sup, ri = pan
    report = {}
    got = list(steady.steady_frames(cap(frames), sup, ri, zoom=1.05, fill=fill, feather_px=feather_px, scale=scale, chunk_frames=chunk,
                                    report=report, **PATH))
    want, tap_of, counts = restated(frames, sup, ri, 1.05, fill, feather_px, scale)
    assert [k for k, _ in got] == list(range(1, N + 1))
    for (k, picture), w in zip(got, want):
        print("frame %d: differing bytes %d of %d" % (k, (picture != w).sum(), w.size))
        assert np.array_equal(picture, w)
    assert fill == 0 or (tap_of > 1).any()                               # the neighbours did fill something
    px = float(want[0].shape[0] * want[0].shape[1])
    for k in range(1, N + 1):
        f = report["frames"][k]
        assert (f["uncovered"], f["own"], f["filled"]) == (counts[k - 1, 0] / px, counts[k - 1, 1] / px, counts[k - 1, 2:].sum() / px)
    assert 0 < report["jitter_after"] < report["jitter_before"]


def test_jpegs_are_the_files_of_those_pictures(pan):
    frames, sup, ri = pan
    kw = dict(zoom="auto", fill=2, feather_px=4, chunk_frames=8, **PATH)
    pictures = [p for _, p in steady.steady_frames(cap(frames), sup, ri, **kw)]
    files = list(steady.steady_jpegs(cap(frames), sup, ri, quality=85, subsampling="420", **kw))
    assert [k for k, _ in files] == list(range(1, N + 1))
    assert [f for _, f in files] == encode_jpeg(np.stack(pictures), 85, "420")


def test_auto_zoom_below_its_cap_leaves_nothing_to_fill(pan):
    frames, sup, ri = pan
    report = {}
    got = list(steady.steady_frames(cap(frames), sup, ri, zoom="auto", fill=0, chunk_frames=8, report=report, **PATH))
    assert 1.0 < report["zoom"] < PATH["max_zoom"] and not report["zoom_capped"]
    assert [report["frames"][k]["uncovered"] for k in range(1, N + 1)] == [0.0] * N
    assert all(report["frames"][k]["own"] == 1.0 for k in range(1, N + 1))
    want, _, counts = restated(frames, sup, ri, report["zoom"], 0, 8)
    assert (counts[:, 0] == 0).all() and all(np.array_equal(p, w) for (_, p), w in zip(got, want))
    out = steady.steady_report(report)
    assert out["jitter_after"] < out["jitter_before"] and out["mean_shares"] == dict(uncovered=0.0, own=1.0, filled=0.0)


def test_command_line_writes_the_video_and_the_report(tmp_path, monkeypatch):
    from evenvizion_amd import stabilize
    monkeypatch.chdir(tmp_path)
    folder = stabilize.main(["--path_to_homography_dict", GOLD, "--path_to_video", MP4, "--experiment_name", "run", "--steady", "1",
                             "--steady_radius", "8", "--steady_fill", "1", "--scale", "0.25", "--format", "mjpeg"])
    assert sorted(os.listdir(folder)) == ["steady.avi", "steady_report.json"]
    report = json.load(open(os.path.join(folder, "steady_report.json")))
    n = len(report["frames"])
    assert n > 100 and sorted(int(k) for k in report["frames"]) == list(range(1, n + 1))
    assert report["radius"] == 8 and report["fill"] == 1 and report["scale"] == 0.25 and 1.0 <= report["zoom"] <= 1.25
    assert report["jitter_after"] < report["jitter_before"]
    for f in report["frames"].values():
        assert abs(f["uncovered"] + f["own"] + f["filled"] - 1.0) < 1e-12
    data = open(os.path.join(folder, "steady.avi"), "rb").read()
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI " and data.count(b"00dc") >= n
