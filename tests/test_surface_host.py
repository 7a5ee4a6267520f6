"""evenvizion_amd.surface on the host: the rotation model, the tables and bounds of the fixed cylinder and sphere, the surface
coordinates, the refusals of surface_frames and the command line -- and tests/surface_checks.py held against warp_checks."""
import math

import numpy as np
import pytest

import surface_checks as SC
import warp_checks as W
from evenvizion_amd import surface as F
from evenvizion_amd.registration import pair_maps

SIZE = (400, 224)


def rot_y(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float64)


def rot_x(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], np.float64)


def rot_z(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float64)


def pan_dictionary(focal, size, angles, tilt=0.0, roll=0.0):
    """{frame_no: S_k}: the superposed matrices of a camera that only turns -- S_k = K . R_k . K^-1 divided by its [2][2], as the
    reference's composition leaves it -- and the rotations R_k themselves (rays of frame k -> rays of frame 1)."""
    K = F.camera_matrix(focal, F._centre(size, None))
    R0 = np.dot(rot_x(tilt), rot_z(roll))
    Rs = [np.dot(R0.T, np.dot(rot_y(a), R0)) for a in angles]
    sup = {}
    for k, R in enumerate(Rs):
        S = np.dot(np.dot(K, R), np.linalg.inv(K))
        sup[k + 1] = S / S[2][2]
    return sup, Rs


# ---- the focal length and the rotations -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("focal", [300.0, 450.0, 900.0])
@pytest.mark.parametrize("step", [0.5, 1.0, 2.0])
def test_estimate_focal_on_noiseless_pans(focal, step):
    sup, _ = pan_dictionary(focal, SIZE, step * np.arange(30), tilt=4.0)
    got = F.estimate_focal(pair_maps(sup), SIZE)
    print("focal %.1f step %.1f: estimated %.4f" % (focal, step, got))
    assert abs(got - focal) <= 0.02 * focal


def test_estimate_focal_skips_what_it_cannot_use():
    sup, _ = pan_dictionary(450.0, SIZE, 2.0 * np.arange(10))
    maps = pair_maps(sup)
    maps[3] = np.full((3, 3), np.nan)
    maps[4] = np.diag([1.0, -1.0, 1.0])                                  # det < 0: a mirror is no camera motion
    assert abs(F.estimate_focal(maps, SIZE) - 450.0) <= 9.0
    assert abs(F.estimate_focal(list(maps.values()), SIZE, centre=(199.5, 111.5)) - 450.0) <= 9.0
    with pytest.raises(ValueError):
        F.estimate_focal({2: np.full((3, 3), np.nan), 3: np.zeros((3, 3)), 4: None}, SIZE)
    with pytest.raises(ValueError):
        F.estimate_focal({}, SIZE)


def test_rotations_are_rotations_and_compose_to_the_camera_path():
    angles = 5.0 * np.arange(41)                                          # 200 degrees
    sup, Rs = pan_dictionary(48.0, (64, 36), angles, tilt=10.0, roll=5.0)
    centre = F._centre((64, 36), None)
    pairs = F.rotations(pair_maps(sup), 48.0, centre)
    assert sorted(pairs) == list(range(2, 42))
    for Q, residual in pairs.values():
        assert np.linalg.norm(np.dot(Q.T, Q) - np.eye(3)) < 1e-12 and abs(np.linalg.det(Q) - 1) < 1e-12
        assert residual < 1e-9
    R_sup = F.superposed_rotations(pairs)
    assert sorted(R_sup) == list(range(1, 42)) and np.array_equal(R_sup[1], np.eye(3))
    for k, R in R_sup.items():
        assert np.linalg.norm(np.dot(R.T, R) - np.eye(3)) < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12
        assert np.abs(R - Rs[k - 1]).max() < 1e-9, k
    # a wrong focal length leaves a residual: that is what the report shows
    assert min(r for _, r in F.rotations(pair_maps(sup), 96.0, centre).values()) > 1e-3


def test_both_choices_for_a_missing_pair():
    sup, Rs = pan_dictionary(300.0, SIZE, 3.0 * np.arange(6))
    sup[4] = None                                                        # pairs 4 and 5 have no map
    maps = pair_maps(sup)
    centre = F._centre(SIZE, None)
    pairs = F.rotations(maps, 300.0, centre)
    assert pairs[4] is None and pairs[5] is None and pairs[3] is not None and pairs[6] is not None
    assert F.rotations({2: np.diag([1.0, -1.0, 1.0]), 3: np.zeros((3, 3))}, 300.0, centre) == {2: None, 3: None}
    repeat = F.superposed_rotations(pairs, none_processing=True, first=1)
    still = F.superposed_rotations(pairs, none_processing=False, first=1)
    for R_sup in (repeat, still):
        for R in R_sup.values():
            assert np.linalg.norm(np.dot(R.T, R) - np.eye(3)) < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12
        assert np.abs(R_sup[3] - Rs[2]).max() < 1e-9
    assert np.abs(repeat[4] - Rs[3]).max() < 1e-9 and np.abs(repeat[5] - Rs[4]).max() < 1e-9      # the 3 degree step goes on
    assert np.array_equal(still[4], still[3]) and np.array_equal(still[5], still[3])              # the camera stands still
    assert np.abs(repeat[6] - Rs[5]).max() < 1e-9 and np.abs(still[6] - Rs[3]).max() < 1e-9
    assert sorted(F.superposed_rotations(pairs)) == [1, 2, 3, 4, 5, 6]                          # first defaults to first key - 1
    assert list(F.superposed_rotations({})) == [1]


# ---- tables ---------------------------------------------------------------------------------------------------------------------------
def test_surface_tables_against_the_formulas():
    scale_px, ox, oy, dw, dh = 20.0, -7, -5, 126, 11
    x, y = np.arange(dw) + ox, np.arange(dh) + oy
    cols, rows = F.surface_tables("cylinder", scale_px, ox, oy, dw, dh)
    assert cols.shape == (dw, 2) and rows.shape == (dh,) and cols.dtype == rows.dtype == np.float64
    assert np.array_equal(cols[:, 0], np.sin(x / scale_px)) and np.array_equal(cols[:, 1], np.cos(x / scale_px))
    assert np.array_equal(rows, y / scale_px)
    cols_s, rows_s = F.surface_tables("sphere", scale_px, ox, oy, dw, dh)
    assert np.array_equal(cols_s, cols) and np.array_equal(rows_s, np.tan(y / scale_px))
    cols_p, rows_p = F.surface_tables("plane", 1.0, ox, oy, dw, dh)
    want = SC.plane_tables(dw, dh, (ox, oy))
    assert np.array_equal(cols_p, want[0]) and np.array_equal(rows_p, want[1])
    F.surface_tables("sphere", scale_px, 0, -31, 4, 63)                   # |phi| <= 31 / 20 < pi / 2
    for bad in (dict(oy=-32), dict(oy=0, dh=33)):
        with pytest.raises(ValueError):
            F.surface_tables("sphere", scale_px, **dict(dict(ox=0, oy=-31, dw=4, dh=63), **bad))
    for args in (("torus", 20.0, 0, 0, 4, 4), ("cylinder", 0.0, 0, 0, 4, 4), ("cylinder", math.nan, 0, 0, 4, 4), ("cylinder", 20.0, 0, 0, 0, 4)):
        with pytest.raises(ValueError):
            F.surface_tables(*args)


# ---- bounds ---------------------------------------------------------------------------------------------------------------------------
def bounds_of(total, kind="cylinder", step=5.0, tilt=0.0, **kw):
    size, focal = (64, 36), 48.0
    _, Rs = pan_dictionary(focal, size, np.arange(0.0, total + 1e-9, step), tilt=tilt)
    return F.surface_bounds({k + 1: R for k, R in enumerate(Rs)}, focal, None, size, kind, **kw)


@pytest.mark.parametrize("kind", ["cylinder", "sphere"])
def test_surface_bounds_of_three_pans(kind):
    half = math.atan(32.5 / 48.0)                                        # the frame's half width seen from its centre, pixel 64
    left = math.atan(31.5 / 48.0)
    for total in (30.0, 200.0):
        ox, oy, dw, dh, scale_px = bounds_of(total, kind)
        assert scale_px == 48.0
        assert ox == math.floor(-left * 48.0) and ox + dw - 1 == math.ceil((math.radians(total) + half) * 48.0)
        assert oy < 0 < oy + dh - 1 and abs(oy + (oy + dh - 1)) <= 2      # about the equator, a pixel for y = 0 .. 36 about 17.5
    assert bounds_of(200.0, kind)[2] > bounds_of(30.0, kind)[2] + 140    # 170 degrees more, 48 pixels per radian
    full = int(round(2 * math.pi * 48.0))
    assert bounds_of(400.0, kind)[2] == full == 302                     # clipped to the full turn
    assert bounds_of(355.0, kind)[2] == full                            # 355 degrees and a frame's width close the surface too
    assert bounds_of(400.0, kind, scale=0.5)[2] == int(round(2 * math.pi * 24.0)) and bounds_of(400.0, kind, scale=0.5)[4] == 24.0
    # backwards: the pan unwraps the other way
    _, Rs = pan_dictionary(48.0, (64, 36), -5.0 * np.arange(41))
    ox, _, dw, _, _ = F.surface_bounds({k + 1: R for k, R in enumerate(Rs)}, 48.0, None, (64, 36), kind)
    assert ox == math.floor((-math.radians(200.0) - left) * 48.0) and ox + dw - 1 == math.ceil(half * 48.0)


def test_surface_bounds_refusals():
    up = {1: np.eye(3), 2: rot_x(80.0), 3: rot_x(90.0)}                  # the camera tilts up to the cylinder's axis
    with pytest.raises(ValueError, match="axis"):
        F.surface_bounds(up, 48.0, None, (64, 36), "cylinder")
    ox, oy, dw, dh, _ = F.surface_bounds(up, 48.0, None, (64, 36), "sphere")      # the sphere has a place for it
    assert abs(oy) <= math.ceil(math.pi / 2 * 48.0) - 1 and oy + dh - 1 <= math.ceil(math.pi / 2 * 48.0) - 1
    F.surface_tables("sphere", 48.0, ox, oy, dw, dh)
    with pytest.raises(ValueError, match="max_pixels"):
        bounds_of(200.0, max_pixels=1000)
    with pytest.raises(ValueError):
        F.surface_bounds({1: None}, 48.0, None, (64, 36), "cylinder")
    with pytest.raises(ValueError):
        F.surface_bounds({1: np.eye(3)}, 48.0, None, (64, 36), "plane")
    for kw in (dict(focal=0.0), dict(focal=math.nan), dict(scale=0.0)):
        with pytest.raises(ValueError):
            F.surface_bounds({1: np.eye(3)}, kw.get("focal", 48.0), None, (64, 36), "cylinder", scale=kw.get("scale", 1.0))


def test_frame_matrix_takes_a_ray_to_full_size_pixels():
    R = np.dot(rot_y(33.0), rot_x(7.0))
    A = F.frame_matrix(R, 48.0, None, (1280, 720), (64, 36)).reshape(3, 3)
    ray = np.dot(R, [0.25, -0.125, 1.0])                                 # frame k sees it at ((.25, -.125) * 48 + centre) resized pixels
    p = np.dot(A, ray)
    assert np.allclose(p[:2] / p[2], [(0.25 * 48 + 31.5) * 20, (-0.125 * 48 + 17.5) * 20], atol=1e-9) and p[2] > 0
    assert np.dot(A, -ray)[2] < 0                                        # the antipode: the same pixel, behind the camera


# ---- coordinates ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cylinder", "sphere"])
def test_surface_coordinates_and_back_across_200_degrees(kind):
    size, focal = (64, 36), 48.0
    centre = F._centre(size, None)
    _, Rs = pan_dictionary(focal, size, 5.0 * np.arange(41), tilt=10.0, roll=5.0)
    R_sup = {k + 1: R for k, R in enumerate(Rs)}
    rng = np.random.default_rng(5)
    pts = np.column_stack([rng.uniform(0, 63, 50), rng.uniform(0, 35, 50)])
    centres = []
    for k in R_sup:
        c = F.surface_coordinates(pts, k, R_sup, focal, centre, kind)
        back = F.surface_to_frame(c, k, R_sup, focal, centre, kind)
        assert np.abs(back - pts).max() < 1e-9, k
        centres.append(F.surface_coordinates([centre], k, R_sup, focal, centre, kind)[0][0])
    assert np.all(np.diff(centres) > 0) and centres[-1] > math.pi * focal       # unwrapped: past the half turn and still growing
    _, flat = pan_dictionary(focal, size, 5.0 * np.arange(41))                 # about the cylinder's own axis: theta is the pan angle
    last = F.surface_coordinates([centre], 41, {k + 1: R for k, R in enumerate(flat)}, focal, centre, kind)[0]
    assert abs(last[0] - math.radians(200.0) * focal) < 1e-9 and abs(last[1]) < 1e-9
    # the same world direction has the same coordinates from every frame that sees it
    ray = np.dot(Rs[20], [0.1, 0.05, 1.0])
    seen = []
    for k in (19, 20, 21, 22):
        p = np.dot(Rs[k].T, ray)
        seen.append(F.surface_coordinates([[p[0] / p[2] * focal + centre[0], p[1] / p[2] * focal + centre[1]]], k + 1, R_sup, focal, centre, kind)[0])
    assert np.abs(np.array(seen) - seen[0]).max() < 1e-9
    assert np.isnan(F.surface_to_frame(F.surface_coordinates([centre], 41, R_sup, focal, centre, kind), 1, R_sup, focal, centre, kind)).all()
    with pytest.raises(ValueError):
        F.surface_coordinates(pts, 99, R_sup, focal, centre, kind)
    with pytest.raises(ValueError):
        F.surface_coordinates(pts, 1, R_sup, focal, centre, "plane")


# ---- surface_checks against warp_checks: the plane is the special case --------------------------------------------------------------
def test_the_restatement_on_plane_tables_is_warp_checks():
    rng = np.random.default_rng(6)
    f = rng.integers(0, 256, (17, 23, 3), dtype=np.uint8)
    cols, rows = SC.plane_tables(37, 29, (-6, -4))
    for M in (np.eye(3), W.translation(4.25, -2.5), np.array([[1.1, 0.2, 3.0], [-0.1, 0.9, 2.0], [1e-3, -2e-3, 1.0]])):
        want, cov = W.warp_frame(f, M, 37, 29, (-6, -4), inverse_map=True)
        got, cov2, tw = SC.ray_frame(f, M, cols, rows)
        assert (tw > 0).all() and cov.any() and np.array_equal(cov, cov2) and np.array_equal(got[cov], want[cov])
        assert np.array_equal(SC.ray_canvases(f[None], [M], cols, rows, "mosaic"),
                              W.warp_canvases(f[None], [M], "mosaic", 37, 29, (-6, -4), None, True))
    # the sign of tw: minus the matrix is the same plane map and covers nothing here
    assert not SC.ray_frame(f, -np.eye(3), cols, rows)[1].any() and W.warp_frame(f, -np.eye(3), 37, 29, (-6, -4), True)[1].any()


# ---- refusals of surface_frames, before anything is opened --------------------------------------------------------------------------
class NoCapture:
    def __getattr__(self, name):
        raise AssertionError("the capture was touched before the arguments were checked")


@pytest.mark.parametrize("kw", [dict(surface="plane"), dict(surface="torus"), dict(surface=None), dict(mode="trail"), dict(focal=0),
                                dict(focal=-3.0), dict(focal=math.nan), dict(focal=math.inf), dict(focal="48"), dict(scale=0),
                                dict(scale=-1.0), dict(scale=math.inf), dict(scale=None), dict(ingest="planes")])
def test_surface_frames_refuses_before_the_capture(kw):
    sup, _ = pan_dictionary(48.0, (64, 36), 5.0 * np.arange(4))
    with pytest.raises(ValueError):
        next(iter(F.surface_frames(NoCapture(), sup, {"w": 64, "h": 36}, **kw)))


# ---- the model and its report ---------------------------------------------------------------------------------------------------------
def test_surface_model_and_report():
    import json
    sup, _ = pan_dictionary(48.0, (64, 36), 5.0 * np.arange(41))
    sup[7] = None
    model = F.surface_model(sup, {"w": 64, "h": 36}, "cylinder")
    assert model.estimated and abs(model.focal - 48.0) <= 0.96 and model.kind == "cylinder"
    report = json.loads(json.dumps(F.surface_report(model)))
    assert report["focal_estimated"] is True and report["fit_residual"]["7"] is None and report["fit_residual"]["8"] is None
    assert report["fit_residual"]["9"] < 1e-3 and report["fit_residual_median"] < 1e-3
    assert report["canvas"]["dw"] == model.bounds[2] and report["canvas"]["closed"] is False
    given = F.surface_model(sup, {"w": 64, "h": 36}, "sphere", focal=48.0)
    assert not given.estimated and given.focal == 48.0 and F.surface_report(given)["fit_residual_median"] < 1e-9


# ---- the command line -----------------------------------------------------------------------------------------------------------------
def test_stabilize_parser_knows_the_surfaces(capsys):
    from evenvizion_amd import stabilize
    args = stabilize.parser().parse_args(["--surface", "cylinder", "--focal", "312.5", "--mode", "mosaic"])
    assert args.surface == "cylinder" and args.focal == 312.5
    args = stabilize.parser().parse_args([])
    assert args.surface is None and args.focal is None                   # without --surface nothing changes
    for argv in (["--surface", "plane"], ["--surface", "cylinder", "--trail", "1"], ["--surface", "sphere", "--plate", "1"],
                 ["--surface", "sphere", "--comparison", "1"], ["--focal", "300"], ["--surface", "sphere", "--focal", "-1"]):
        with pytest.raises(SystemExit):
            stabilize.main(argv)
    with pytest.raises(SystemExit):
        stabilize.main(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    for word in ("--surface", "--focal", "surface_report.json"):
        assert word in text, word
