"""The drivers of evh_jpeg_encode: stabilized_jpegs and surface_jpegs yield exactly jpeg_checks.encode of the pictures
stabilized_frames and surface_frames yield, and python -m evenvizion_amd.stabilize --format jpeg | mjpeg writes those bytes.
Six synthetic frames of 400 x 224 that pan by 4 pixels a frame."""
import json
import os

import numpy as np
import pytest

import jpeg_checks as J
from evenvizion_amd import stabilization as S
from evenvizion_amd import stabilize, surface, synthetic
from evenvizion_amd.pictures import quant_tables

pytestmark = pytest.mark.gpu
N, W, H, STEP = 6, 400, 224, 4


@pytest.fixture(scope="module")
def pan(tmp_path_factory):
    """-> (frames u8[N,H,W,3], superposition dictionary, resize_info, path of the frames, path of the dictionary)"""
    from evenvizion_amd.processing.utils import read_homography_dict, superposition_dict
    gray = synthetic.make_pan_stream(7, N, W, H, step=STEP)
    frames = np.ascontiguousarray(np.stack([gray, np.roll(gray, 2, axis=2), 255 - gray], -1))
    folder = tmp_path_factory.mktemp("pan")
    video, path = str(folder / "pan.npy"), str(folder / "dict.json")
    np.save(video, frames)
    d = {str(k): {"H": [[1, 0, STEP], [0, 1, 0], [0, 0, 1]]} for k in range(2, N + 1)}
    d["resize_info"] = {"w": W, "h": H}
    with open(path, "w") as f:
        json.dump(d, f)
    hd, ri = read_homography_dict(path)
    return frames, superposition_dict(hd), ri, video, path


@pytest.fixture(scope="module")
def encoded():
    """jpeg_checks.encode, each distinct picture once."""
    memo = {}

    def files(pictures, quality, sub):
        out = []
        for p in pictures:
            key = (p.tobytes(), p.shape, quality, sub)
            if key not in memo:
                memo[key] = J.encode(p, quant_tables(quality), sub)
            out.append(memo[key])
        return out
    return files


def cap(frames):
    return synthetic.SyntheticCapture(list(frames))


@pytest.mark.parametrize("mode,trail,placement,quality,sub", [("each", False, "warp", 90, "420"), ("history", False, "warp", 75, "444"),
                                                              ("history", True, "translate", 90, "420"), ("mosaic", False, "warp", 90, "420")])
def test_stabilized_jpegs_are_the_encoded_pictures(pan, encoded, mode, trail, placement, quality, sub):
    frames, sup, ri = pan[:3]
    kw = dict(mode=mode, placement=placement, trail=trail, chunk_frames=4)
    pictures = list(S.stabilized_frames(cap(frames), sup, ri, **kw))
    got = list(S.stabilized_jpegs(cap(frames), sup, ri, quality=quality, subsampling=sub, **kw))
    assert [k for k, _ in got] == [k for k, _ in pictures] == ([N] if mode == "mosaic" else list(range(1, N + 1)))
    assert all(p.any() for _, p in pictures)
    assert [f for _, f in got] == encoded([p for _, p in pictures], quality, sub)
    P = J.parse(got[-1][1])
    assert (P["sof"]["h"], P["sof"]["w"]) == pictures[-1][1].shape[:2]


def test_bad_formats_are_refused_before_anything_is_read(pan):
    frames, sup, ri = pan[:3]
    for kw in (dict(quality=0), dict(quality=101), dict(subsampling="422")):
        with pytest.raises(ValueError):
            S.stabilized_jpegs(None, sup, ri, **kw)
        with pytest.raises(ValueError):
            surface.surface_jpegs(None, sup, ri, **kw)


def test_surface_jpegs_are_the_encoded_pictures(pan, encoded):
    frames, sup, ri = pan[:3]
    kw = dict(surface="cylinder", focal=500.0, mode="history", chunk_frames=4)
    pictures = list(surface.surface_frames(cap(frames), sup, ri, **kw))
    got = list(surface.surface_jpegs(cap(frames), sup, ri, quality=90, subsampling="420", **kw))
    assert [k for k, _ in got] == [k for k, _ in pictures] == list(range(1, N + 1))
    assert [f for _, f in got] == encoded([p for _, p in pictures], 90, "420")


def run(tmp_path, monkeypatch, pan, name, *extra):
    monkeypatch.chdir(tmp_path)
    folder = stabilize.main(["--path_to_homography_dict", pan[4], "--path_to_video", pan[3], "--experiment_name", name] + list(extra))
    return folder, sorted(os.listdir(folder))


def test_command_line_formats(pan, encoded, tmp_path, monkeypatch):
    frames, sup, ri = pan[:3]
    pictures = [p for _, p in S.stabilized_frames(cap(frames), sup, ri, mode="history", placement="translate")]
    # no --format: the PPM files as before, and nothing else
    folder, names = run(tmp_path, monkeypatch, pan, "plain")
    assert names == ["%06d.ppm" % k for k in range(1, N + 1)]
    for k, p in enumerate(pictures):
        want = b"P6\n%d %d\n255\n" % (p.shape[1], p.shape[0]) + np.ascontiguousarray(p[:, :, ::-1]).tobytes()
        assert open(os.path.join(folder, names[k]), "rb").read() == want
    files = encoded(pictures, 75, "444")
    folder, names = run(tmp_path, monkeypatch, pan, "jpeg", "--format", "jpeg", "--quality", "75", "--subsampling", "444")
    assert names == ["%06d.jpg" % k for k in range(1, N + 1)]
    assert [open(os.path.join(folder, n), "rb").read() for n in names] == files
    folder, names = run(tmp_path, monkeypatch, pan, "mjpeg", "--format", "mjpeg", "--quality", "75", "--subsampling", "444", "--fps", "12.5")
    assert names == ["stabilized.avi"]
    J.check_avi(open(os.path.join(folder, "stabilized.avi"), "rb").read(), files, pictures[0].shape[1], pictures[0].shape[0], 12.5)
    # the one picture of a mosaic
    mosaic = [p for _, p in S.stabilized_frames(cap(frames), sup, ri, mode="mosaic", placement="translate")]
    folder, names = run(tmp_path, monkeypatch, pan, "mosaic", "--format", "jpeg", "--mode", "mosaic")
    assert names == ["%06d.jpg" % N]
    assert open(os.path.join(folder, names[0]), "rb").read() == encoded(mosaic, 90, "420")[0]
    for bad in (["--quality", "75"], ["--format", "jpeg", "--comparison", "1"], ["--format", "jpeg", "--quality", "0"]):
        with pytest.raises(SystemExit):
            run(tmp_path, monkeypatch, pan, "bad", *bad)


def test_command_line_surface_and_plate(pan, encoded, tmp_path, monkeypatch):
    frames, sup, ri = pan[:3]
    model = surface.surface_model(sup, ri, surface="cylinder", focal=500.0, scale=1.0)
    pictures = [p for _, p in surface.surface_frames(cap(frames), sup, ri, surface="cylinder", focal=model.focal, mode="history")]
    folder, names = run(tmp_path, monkeypatch, pan, "surface", "--surface", "cylinder", "--focal", "500", "--format", "jpeg")
    assert names == ["%06d.jpg" % k for k in range(1, N + 1)] + ["surface_report.json"]
    assert [open(os.path.join(folder, n), "rb").read() for n in names[:N]] == encoded(pictures, 90, "420")
    plate = S.background_plate(cap(frames), sup, ri, placement="translate").plate
    folder, names = run(tmp_path, monkeypatch, pan, "plate", "--plate", "1", "--format", "mjpeg")
    assert names == ["plate.jpg", "plate_count.png"]
    assert open(os.path.join(folder, "plate.jpg"), "rb").read() == encoded([plate], 90, "420")[0]
