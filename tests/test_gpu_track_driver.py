"""evenvizion_amd.tracking.recover_homography_dict and the command line's --recover_tracking on the device: a capture on which
descriptor matching finds nothing gets a matrix for every pair, within the bound the host run of the same frames reaches."""
import json
import os

import numpy as np
import pytest

import track_families as F

pytestmark = pytest.mark.gpu

# The host run of capture_frames(41, 6): seeds and rows from tests/track_checks.py (radius 2, cell 16, border 8, min_eig 0.5; levels 3,
# radius 7, 20 iterations, forward-backward 0.5 px; 146..160 rows per pair), solved pair by pair with the oracle's compute_homography and
# matrix_superposition (solver_families.scan_mirror): the frame corners through the superposition miss the truth by 0.020, 0.016,
# 0.036, 0.042, 0.044 px.  The device tracks the same rows (test_gpu_track.py holds it to equality); 0.05 px are the digits its
# exact-mode solver may differ in.
HOST_WORST = 0.0444
BOUND = HOST_WORST + 0.05
CORNERS = np.array([(0, 0), (399, 0), (0, 223), (399, 223)], np.float64)


def corner_errors(homography_dict, step):
    from evenvizion_amd.processing.utils import superposition_dict
    per_frame = {int(k): v for k, v in homography_dict.items() if k != "resize_info"}
    sup = superposition_dict(per_frame)
    return {k: float(np.abs(F.apply(np.asarray(sup[k], np.float64), CORNERS) - (CORNERS + (k - 1) * np.asarray(step))).max())
            for k in per_frame}


def test_a_capture_without_corners_gets_every_matrix(tmp_path, monkeypatch):
    from evenvizion_amd import tracking
    from evenvizion_amd._lib import PAIR_NO_DESCRIPTORS, PAIR_OK
    from evenvizion_amd.processing.video_processing import get_homography_dict
    from evenvizion_amd.synthetic import SyntheticCapture
    frames, M = F.capture_frames(41, 6)
    assert int(frames.max()) - int(frames.min()) <= 20
    with pytest.raises(AttributeError):                       # the reference's end of such a video: no matrix for the first pair
        get_homography_dict(SyntheticCapture(list(frames)), resize_width=400, features_type_list=["ORB"], ingest="bgr")
    recovered, report = tracking.recover_homography_dict(SyntheticCapture(list(frames)), {"resize_info": {"w": 400, "h": 224}}, ingest="bgr")
    assert sorted(report) == [2, 3, 4, 5, 6] and recovered["resize_info"] == {"h": 224, "w": 400}
    for k in range(2, 7):                                     # the premise: the first pass has nothing for any pair
        assert report[k]["first_status"] == PAIR_NO_DESCRIPTORS, report[k]
        assert report[k]["final_status"] == PAIR_OK and report[k]["tracked"] >= 100 and 2 * report[k]["seeds"] >= 24 * 13, report[k]
        assert report[k]["flags"]["tracked"] == report[k]["tracked"] and sum(report[k]["flags"].values()) == report[k]["seeds"]
        assert np.asarray(recovered[k]["H"]).shape == (3, 3)
    errors = corner_errors(recovered, M[:2, 2])
    print("corner errors by frame: %s (bound %.4f)" % ({k: round(v, 4) for k, v in errors.items()}, BOUND))
    assert max(errors.values()) <= BOUND
    # the rows themselves, through the other door
    rows = tracking.track_rows(SyntheticCapture(list(frames)), {"w": 400, "h": 224}, ingest="bgr")
    assert sorted(rows) == [2, 3, 4, 5, 6]
    for k in range(2, 7):
        r = rows[k]["rows"]
        assert len(r) == report[k]["tracked"] and rows[k]["seeds"] == report[k]["seeds"]
        assert np.abs(r[:, 2:] - r[:, :2] - M[:2, 2]).max() <= 0.5
    # the command line on such a video: the reference's end without the flag, the two new files alone with it
    from evenvizion_amd import component
    np.save(tmp_path / "low.npy", frames)
    monkeypatch.chdir(tmp_path)
    base = ["--path_to_video", str(tmp_path / "low.npy"), "--features", "ORB"]
    with pytest.raises(AttributeError):
        component.main(base + ["--experiment_name", "plain"])
    folder = component.main(base + ["--experiment_name", "tracked", "--recover_tracking", "1"])
    assert sorted(os.listdir(folder)) == ["dict_with_homography_matrix_recovered.json", "tracking_report.json"]
    with open(os.path.join(folder, "dict_with_homography_matrix_recovered.json")) as f:
        assert json.load(f)["6"]["H"] == recovered[6]["H"]


def test_planes_at_the_working_size_take_the_plane_route():
    """A capture that delivers 4:2:0 planes at the working size: nothing is resized, so the tracker is handed the packed planes
    themselves (gathered as (prev, cur) rows, the seeds on every second of them).  The result equals the BGR route's on the frames
    the planes convert to."""
    from evenvizion_amd import tracking
    from evenvizion_amd._lib import PAIR_NO_DESCRIPTORS, PAIR_OK
    from evenvizion_amd.synthetic import SyntheticCapture, SyntheticYuvCapture, yuv420_to_bgr_host
    frames, M = F.capture_frames(45, 4, hi=115)               # luma 100..115: 17 levels of gray once converted
    neutral = np.full((112, 200), 128, np.uint8)
    planes = [(np.ascontiguousarray(f[..., 0]), neutral, neutral) for f in frames]
    bgr = [yuv420_to_bgr_host(*p) for p in planes]
    assert int(np.max(bgr)) - int(np.min(bgr)) <= 20
    first = {"resize_info": {"w": 400, "h": 224}}
    by_planes = tracking.recover_homography_dict(SyntheticYuvCapture(planes), first, ingest="yuv420")
    by_bgr = tracking.recover_homography_dict(SyntheticCapture(bgr), first, ingest="bgr")
    assert by_planes[1] == by_bgr[1] and sorted(by_planes[1]) == [2, 3, 4]
    for k in (2, 3, 4):
        assert by_planes[1][k]["first_status"] == PAIR_NO_DESCRIPTORS and by_planes[1][k]["final_status"] == PAIR_OK
        assert by_planes[1][k]["tracked"] >= 50, by_planes[1][k]
        assert np.asarray(by_planes[0][k]["H"]).tobytes() == np.asarray(by_bgr[0][k]["H"]).tobytes(), k
    errors = corner_errors(by_planes[0], M[:2, 2])
    print("corner errors by frame, planes: %s" % {k: round(v, 4) for k, v in errors.items()})       # reported; equality above is the check
    rows = tracking.track_rows(SyntheticYuvCapture(planes), {"w": 400, "h": 224}, ingest="yuv420")
    assert [len(rows[k]["rows"]) for k in (2, 3, 4)] == [by_planes[1][k]["tracked"] for k in (2, 3, 4)]


def test_pairs_before_the_first_failure_are_the_first_passs(tmp_path, monkeypatch):
    from evenvizion_amd import component, tracking
    from evenvizion_amd._lib import PAIR_OK
    from evenvizion_amd.processing.video_processing import get_homography_dict
    from evenvizion_amd.synthetic import SyntheticCapture
    frames, M = F.capture_frames(43, 6, textured=(0, 1, 2, 3))
    first = get_homography_dict(SyntheticCapture(list(frames)), resize_width=400, features_type_list=["ORB"], ingest="bgr")
    recovered, report = tracking.recover_homography_dict(SyntheticCapture(list(frames)), first, ingest="bgr")
    assert sorted(report) == [5, 6] and report[6]["final_status"] == PAIR_OK and report[6]["first_status"] != PAIR_OK
    for k in (2, 3, 4):
        assert np.asarray(recovered[k]["H"]).tobytes() == np.asarray(first[k]["H"]).tobytes(), k
    assert np.asarray(first[6]["H"]).tobytes() == np.asarray(first[5]["H"]).tobytes()             # what the first pass does: repeat
    pair = np.asarray(recovered[6]["H"])
    assert np.isfinite(pair).all() and pair.tobytes() != np.asarray(first[6]["H"]).tobytes()
    # the command line: the new files only on request, the old ones byte for byte
    np.save(tmp_path / "mixed.npy", frames)
    monkeypatch.chdir(tmp_path)
    base = ["--path_to_video", str(tmp_path / "mixed.npy"), "--features", "ORB"]
    plain = component.main(base + ["--experiment_name", "plain"])
    folder = component.main(base + ["--experiment_name", "tracked", "--recover_tracking", "1"])
    old = sorted(os.listdir(plain))
    assert sorted(os.listdir(folder)) == sorted(old + ["dict_with_homography_matrix_recovered.json", "tracking_report.json"])
    for name in old:
        with open(os.path.join(plain, name), "rb") as a, open(os.path.join(folder, name), "rb") as b:
            assert a.read() == b.read(), name
    with open(os.path.join(folder, "dict_with_homography_matrix_recovered.json")) as f:
        written = json.load(f)
    with open(os.path.join(folder, "tracking_report.json")) as f:
        assert sorted(json.load(f)) == ["5", "6"]
    assert list(written) == ["2", "3", "4", "5", "6", "resize_info"] and written["6"]["H"] == recovered[6]["H"]
