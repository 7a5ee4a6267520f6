"""evh_rows_moving_filter off the device: the numpy restatement (moving_checks) against a literal per-row, per-pixel loop, what the
filter is for on the panning scene, and the argument handling of moving.refine_homography_dict and of the command line."""
import collections

import numpy as np
import pytest

import moving_checks as MC
import plate_checks as P
import warp_checks as W
from evenvizion_amd import moving as M


def literal_hit(frame, m, plate, count, X, Y, origin, min_cover, threshold):
    """One canvas pixel, in Python floats and ints: is it a hit for this frame?"""
    dh, dw = count.shape
    sh, sw = frame.shape[:2]
    if not (0 <= X < dw and 0 <= Y < dh) or count[Y, X] < min_cover:
        return False
    a = [float(v) for v in W.adjugate(m)]
    px, py = float(X + origin[0]), float(Y + origin[1])
    tx, ty, tw = (a[0] * px + a[1] * py) + a[2], (a[3] * px + a[4] * py) + a[5], (a[6] * px + a[7] * py) + a[8]
    try:
        U, V = round(tx / tw * 32), round(ty / tw * 32)         # Python rounds halves to even
    except (ZeroDivisionError, ValueError, OverflowError):
        return False
    if not (0 <= U <= 32 * (sw - 1) and 0 <= V <= 32 * (sh - 1)):
        return False
    sx, fx, sy, fy = U >> 5, U & 31, V >> 5, V & 31
    f = frame.astype(np.int64).reshape(sh, sw, -1)
    tap = lambda y, x, wgt: f[y, x] * wgt if wgt else 0
    s = (tap(sy, sx, (32 - fx) * (32 - fy)) + tap(sy, min(sx + 1, sw - 1), fx * (32 - fy)) + tap(min(sy + 1, sh - 1), sx, (32 - fx) * fy)
         + tap(min(sy + 1, sh - 1), min(sx + 1, sw - 1), fx * fy) + 512) >> 10
    g = lambda v: int(v[0]) if len(v) == 1 else (int(v[0]) * 1868 + int(v[1]) * 9617 + int(v[2]) * 4899 + 8192) >> 14
    return abs(g(s) - g(np.atleast_1d(plate[Y, X]))) > threshold


def literal_point(x, y, frame, m, plate, count, origin, radius, min_hits, row_scale, min_cover, threshold):
    m = [float(v) for v in np.asarray(m).reshape(9)]
    px, py = float(np.float32(x)) * row_scale[0], float(np.float32(y)) * row_scale[1]
    tx, ty, tw = (m[0] * px + m[1] * py) + m[2], (m[3] * px + m[4] * py) + m[5], (m[6] * px + m[7] * py) + m[8]
    try:
        cx, cy = round(tx / tw), round(ty / tw)
    except (ZeroDivisionError, ValueError, OverflowError):
        return False
    if not (abs(cx) <= 1 << 30 and abs(cy) <= 1 << 30):
        return False
    hits = sum(literal_hit(frame, m, plate, count, cx - origin[0] + i, cy - origin[1] + j, origin, min_cover, threshold)
               for j in range(-radius, radius + 1) for i in range(-radius, radius + 1))
    return hits >= min_hits


def small_case(gray, projective, seed=3):
    rng = np.random.default_rng(seed)
    n, sh, sw, dw, dh, origin = 4, 9, 13, 30, 20, (-3, -2)
    frames = rng.integers(0, 256, (n, sh, sw) if gray else (n, sh, sw, 3)).astype(np.uint8)
    mats = np.stack([W.translation(2 + 3 * k, 1 + 2 * k) for k in range(n)])
    if projective:
        mats = mats + rng.normal(0, 1, mats.shape) * np.array([[0.05, 0.05, 0.5], [0.05, 0.05, 0.5], [1e-3, 1e-3, 0]])
    plate, count, _ = P.plate(frames, mats, dw, dh, origin)
    cap = 40
    rows = np.zeros((n - 1, cap, 4), np.float32)
    rows[..., 0::2] = rng.uniform(-2, sw + 2, (n - 1, cap, 2))
    rows[..., 1::2] = rng.uniform(-2, sh + 2, (n - 1, cap, 2))
    rows[0, 3] = [np.nan, 1, 2, 3]
    rows[1, 4] = [1e30, 1, -0.0, 3]
    counts = np.array([cap, 17, 33], np.int32)
    status1 = np.zeros(n - 1, np.int32)
    return frames, mats, plate, count, origin, rows, counts, status1, cap


@pytest.mark.parametrize("gray", [True, False])
@pytest.mark.parametrize("projective", [False, True])
@pytest.mark.parametrize("radius,min_hits,min_cover,threshold,min_keep,row_scale",
                         [(0, 1, 1, 16, 0, (1.0, 1.0)), (1, 1, 2, 0, 8, (1.0, 1.0)), (1, 9, 1, 16, 8, (1.0, 1.0)),
                          (2, 3, 2, 40, 30, (0.9, 1.1)), (0, 1, 1, 255, 8, (1.0, 1.0))])
def test_restatement_equals_the_literal_loop(gray, projective, radius, min_hits, min_cover, threshold, min_keep, row_scale):
    frames, mats, plate, count, origin, rows, counts, status1, cap = small_case(gray, projective)
    npairs = len(counts)
    sent = np.full((npairs, cap, 4), -7.0, np.float32)
    got_rows, got_counts, got_moving, got_flags = MC.rows_filter(
        frames, mats, plate, count, origin, rows, counts, status1, sent, np.full(npairs, -5, np.int32), np.full(npairs, -5, np.int32),
        np.full((npairs, cap), 99, np.uint8), threshold=threshold, min_cover=min_cover, radius=radius, min_hits=min_hits,
        row_scale=row_scale, frame_step=1, min_keep=min_keep)
    seen = 0
    for p in range(npairs):
        n = int(counts[p])
        kw = dict(plate=plate, count=count, origin=origin, radius=radius, min_hits=min_hits, row_scale=row_scale,
                  min_cover=min_cover, threshold=threshold)
        a = [literal_point(r[0], r[1], frames[p + 1], mats[p + 1], **kw) for r in rows[p, :n]]
        b = [literal_point(r[2], r[3], frames[p], mats[p], **kw) for r in rows[p, :n]]
        flags = [int(x) | int(y) << 1 for x, y in zip(a, b)]
        assert got_flags[p, :n].tolist() == flags and (got_flags[p, n:] == 99).all()
        moving = sum(1 for f in flags if f)
        seen += moving
        assert got_moving[p] == moving
        want = [r for r, f in zip(rows[p, :n], flags) if not f] if n - moving >= min_keep else list(rows[p, :n])
        assert got_counts[p] == len(want)
        assert np.array_equal(got_rows[p, :len(want)].view(np.uint32), np.array(want, np.float32).reshape(-1, 4).view(np.uint32))
        assert (got_rows[p, len(want):] == -7.0).all()
    if threshold == 255:
        assert seen == 0
    elif threshold == 0:
        assert seen > 0


def test_pairs_that_are_not_ok_or_empty_are_passed_over():
    frames, mats, plate, count, origin, rows, counts, status1, cap = small_case(False, False)
    counts = np.array([0, -4, cap + 9], np.int32)
    status1 = np.array([0, 0, 3], np.int32)
    out = MC.rows_filter(frames, mats, plate, count, origin, rows, counts, status1, np.full((3, cap, 4), -7.0, np.float32),
                         np.full(3, -5, np.int32), np.full(3, -5, np.int32), np.full((3, cap), 99, np.uint8))
    assert (out[0] == -7.0).all() and out[1].tolist() == [0, -4, cap + 9] and out[2].tolist() == [0, 0, 0] and (out[3] == 99).all()


def test_the_filter_drops_the_square_and_keeps_the_background_of_the_panning_scene():
    B, frames, mats, squares = P.panning_scene()
    plate, count, _ = P.plate(frames, mats, 60, 40, min_cover=2, threshold=0)
    rows, counts, background, cap = MC.scene_rows()
    out_rows, out_counts, moving, flags = MC.rows_filter(
        frames, mats, plate, count, (0, 0), rows, counts, np.zeros(8, np.int32), np.zeros_like(rows), np.zeros(8, np.int32),
        np.zeros(8, np.int32), np.zeros((8, cap), np.uint8), threshold=0, min_cover=2, radius=0, min_hits=1, min_keep=4)
    for p in range(8):
        assert 35 <= len(background[p]) <= 37 and counts[p] == len(background[p]) + 16
        assert moving[p] == 16 and out_counts[p] == len(background[p])
        assert np.array_equal(out_rows[p, :out_counts[p]], background[p])


class NoCapture:
    def __getattr__(self, name):
        raise AssertionError("the capture was touched before the arguments were checked")


Plate = collections.namedtuple("Plate", "plate count origin frame_nos masks")
GOOD_DICT = {2: {"H": np.eye(3).tolist()}, "resize_info": {"w": 8, "h": 6}}
GOOD_PLATE = Plate(np.zeros((16, 18, 3), np.uint8), np.zeros((16, 18), np.uint8), (0, 0), [1, 2], None)


@pytest.mark.parametrize("kw", [dict(placement="paste"), dict(placement=None), dict(ingest="nv12"), dict(ingest=None), dict(scale=0),
                                dict(scale=float("nan")), dict(scale=-1.0), dict(placement="translate", scale=2.0),
                                dict(threshold=-1), dict(threshold=256), dict(threshold=1.5), dict(min_cover=0), dict(min_cover=256),
                                dict(radius=-1), dict(radius=8), dict(min_hits=0), dict(radius=1, min_hits=10), dict(min_keep=-1),
                                dict(nfeatures=0), dict(chunk_frames=1), dict(features_type_list=["KAZE"]), dict(features_type_list=["SIFT", "ORB"]), dict(features_type_list=None),
                                dict(homography_dict={2: {"H": None}}), dict(homography_dict={"resize_info": {"w": 8, "h": 6}}),
                                dict(homography_dict=None), dict(plate=None), dict(plate=GOOD_PLATE._replace(count=np.zeros((3, 3), np.uint8))),
                                dict(plate=GOOD_PLATE._replace(plate=np.zeros((16, 18), np.uint8)))])
def test_refine_refuses_before_the_capture_is_touched(kw, monkeypatch):
    monkeypatch.setattr(M, "superposition_dict", lambda d: pytest.fail("the device was touched before the arguments were checked"))
    args = dict(homography_dict=GOOD_DICT, plate=GOOD_PLATE)
    args.update(kw)
    with pytest.raises(ValueError):
        M.refine_homography_dict(NoCapture(), **args)


def host_superposition(per_frame):
    sup, S = {1: np.eye(3).tolist()}, np.eye(3)
    for k, v in per_frame.items():
        S = np.dot(np.asarray(v["H"], np.float64), S)
        sup[k] = S.tolist()
    return sup


def test_refine_refuses_a_plate_of_another_canvas_after_the_first_frame_only(monkeypatch):
    class OneFrame:
        width, height, bgr_mode = 8, 6, None
        reads = 0

        def read(self):
            self.reads += 1
            assert self.reads == 1, "a further frame was read before the canvas was compared"
            return True, np.zeros((6, 8, 3), np.uint8)
    monkeypatch.setattr(M, "superposition_dict", host_superposition)
    d = {k: {"H": W.translation(2, 1).tolist()} for k in range(2, 5)}
    d["resize_info"] = {"w": 8, "h": 6}
    for plate, placement in ((GOOD_PLATE, "translate"),                                        # the canvas is 17 x 24 there
                             (GOOD_PLATE._replace(plate=np.zeros((9, 14, 3), np.uint8), count=np.zeros((9, 14), np.uint8),
                                                  origin=(1, 0)), "warp")):                    # the shape fits, the origin does not
        cap = OneFrame()
        with pytest.raises(ValueError, match="placement or scale"):
            M.refine_homography_dict(cap, d, plate, placement=placement, ingest="bgr")
        assert cap.reads == 1


def test_component_parses_the_moving_options(capsys):
    from evenvizion_amd import component
    a = component.parser().parse_args([])
    assert (a.reject_moving, a.moving_threshold, a.moving_radius, a.moving_min_cover, a.plate_frames) == (0, 16, 1, 2, 64)
    a = component.parser().parse_args(["--reject_moving", "1", "--moving_threshold", "0", "--moving_radius", "7",
                                       "--moving_min_cover", "255", "--plate_frames", "255"])
    assert (a.reject_moving, a.moving_threshold, a.moving_radius, a.moving_min_cover, a.plate_frames) == (1, 0, 7, 255, 255)
    for bad in (["--reject_moving", "2"], ["--moving_threshold", "256"], ["--moving_threshold", "-1"], ["--moving_radius", "8"],
                ["--moving_min_cover", "0"], ["--plate_frames", "0"], ["--plate_frames", "256"], ["--moving_radius", "x"]):
        with pytest.raises(SystemExit):
            component.parser().parse_args(bad)
    with pytest.raises(ValueError, match="one video"):
        component.main(["--reject_moving", "1", "--features", "ORB", "--path_to_videos", "synthetic:4:64x48:1", "synthetic:4:64x48:2"])
    with pytest.raises(ValueError, match="--features ORB"):
        component.main(["--reject_moving", "1", "--path_to_video", "synthetic:4:64x48:1"])
    capsys.readouterr()
    with pytest.raises(SystemExit):
        component.main(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    for word in ("--reject_moving", "--moving_threshold", "--moving_radius", "--moving_min_cover", "--plate_frames",
                 "dict_with_homography_matrix_refined.json", "moving_rows.json"):
        assert word in text, word
