"""The restatement of evh_mask_components (tests/components_checks.py) against hand-written expectations, link_objects on crafted
boxes, the refusals of moving_objects and of the command line, and evh_mask_components_work_bytes through the library.  No GPU."""
import numpy as np
import pytest

import components_checks as K


def grid(*rows):
    return np.array([[c == "#" for c in r] for r in rows], np.uint8)


def one(o, **fields):
    return {k: o[k] for k in fields} == fields


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def test_ring():
    m = grid("#####",
             "#...#",
             "#...#",
             "#...#",
             "#####")
    for c in (4, 8):
        labels, objects = K.components(m, c)
        assert np.array_equal(labels, m.astype(np.int32))
        assert K.table(objects) == [(0, 0, 4, 4, 16, 0, 32, 32)]          # x0 y0 x1 y1 area first sx sy


def test_two_diagonal_pixels():
    m = grid("#.",
             ".#")
    labels, objects = K.components(m, 4)
    assert labels.tolist() == [[1, 0], [0, 2]] and K.table(objects) == [(0, 0, 0, 0, 1, 0, 0, 0), (1, 1, 1, 1, 1, 3, 1, 1)]
    labels, objects = K.components(m, 8)
    assert labels.tolist() == [[1, 0], [0, 1]] and K.table(objects) == [(0, 0, 1, 1, 2, 0, 1, 1)]
    m = grid(".#",
             "#.")
    assert K.components(m, 4)[0].tolist() == [[0, 1], [2, 0]] and K.components(m, 8)[0].tolist() == [[0, 1], [1, 0]]


def test_u_whose_arms_meet_below_its_first_pixel():
    m = grid(".#..#",
             ".#..#",
             "##..#",
             ".####")
    labels, objects = K.components(m, 4)
    assert np.array_equal(labels, m.astype(np.int32))                  # one component although the scan meets the right arm apart
    assert K.table(objects) == [(0, 0, 4, 3, 11, 1, 1 + 1 + 0 + 1 + 4 * 3 + 1 + 2 + 3 + 4, 0 + 1 + 2 + 2 + 0 + 1 + 2 + 3 * 4)]


def test_spiral():
    m = grid("#######",
             "......#",
             "#####.#",
             "#...#.#",
             "#.###.#",
             "#.....#",
             "#######")
    labels, objects = K.components(m, 4)
    assert np.array_equal(labels, m.astype(np.int32)) and len(objects) == 1
    assert one(objects[0], x0=0, y0=0, x1=6, y1=6, area=int(m.sum()), first=0)
    # its complement under 4-connectivity: the channel, one component winding the other way; under 8 likewise
    labels, objects = K.components(1 - m, 4)
    assert len(objects) == 1 and one(objects[0], first=7, area=49 - int(m.sum()))


def test_opening_removes_a_bridge_and_splits_a_blob():
    m = grid("###....###",
             "##########",
             "###....###")
    assert len(K.components(m, 4)[1]) == 1
    opened = K.opening(m != 0, 1)
    assert np.array_equal(opened, grid("###....###",
                                       "###....###",
                                       "###....###") != 0)
    labels, objects = K.components(m, 8, open_radius=1)
    assert labels.tolist() == [[1, 1, 1, 0, 0, 0, 0, 2, 2, 2]] * 3
    assert K.table(objects) == [(0, 0, 2, 2, 9, 0, 9, 9), (7, 0, 9, 2, 9, 7, 72, 9)]
    # the canvas edge counts as background: a 3 x 3 block survives radius 1, a 2-wide strip along the edge does not
    assert not K.opening(grid("##", "##", "##", "##") != 0, 1).any()
    assert K.opening(np.ones((3, 3), bool), 1).all() and not K.opening(np.ones((3, 3), bool), 2).any()
    assert np.array_equal(K.opening(m != 0, 0), m != 0)


def test_min_area_removes_the_first_component_and_renumbers_the_rest():
    m = grid("#..##.",
             "...##.",
             "#....#",
             "#....#")
    labels, objects = K.components(m, 4)
    assert [o["area"] for o in objects] == [1, 4, 2, 2] and labels[0].tolist() == [1, 0, 0, 2, 2, 0]
    labels, objects = K.components(m, 4, min_area=2)
    assert labels.tolist() == [[0, 0, 0, 1, 1, 0], [0, 0, 0, 1, 1, 0], [2, 0, 0, 0, 0, 3], [2, 0, 0, 0, 0, 3]]
    assert [o["first"] for o in objects] == [3, 12, 17]
    labels, objects = K.components(m, 4, min_area=5)
    assert not labels.any() and objects == []


def test_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    m = (np.random.default_rng(1).random((30, 40)) < 0.5).astype(np.uint8)
    for c, structure in ((4, None), (8, np.ones((3, 3), int))):
        want, k = ndi.label(m, structure)
        labels, objects = K.components(m, c)
        assert len(objects) == k and np.array_equal(labels, want)       # scipy numbers in raster order of the first pixel too
    opened = ndi.binary_opening(m, np.ones((3, 3), bool))              # scipy's border value is 0, as the contract's
    assert np.array_equal(K.opening(m != 0, 1), opened)


# ---- tracks ---------------------------------------------------------------------------------------------------------------------------
def boxes(*b):
    return [{"box_plane": x} for x in b]


def test_link_objects():
    from evenvizion_amd.moving import _iou, link_objects
    assert _iou((0, 0, 9, 9), (0, 0, 9, 9)) == 1.0 and _iou((0, 0, 9, 9), (10, 0, 19, 9)) == 0.0
    assert _iou((0, 0, 9, 9), (5, 0, 14, 9)) == 50 / 150
    # a split: the larger overlap continues the track, the other half opens one
    assert link_objects({1: boxes((0, 0, 19, 9)), 2: boxes((12, 0, 19, 9), (0, 0, 10, 9))}) == [[(1, 0), (2, 1)], [(2, 0)]]
    # a merge: the track with the larger overlap goes on, the other closes
    assert link_objects({1: boxes((0, 0, 5, 9), (8, 0, 19, 9)), 2: boxes((0, 0, 19, 9)), 3: boxes((0, 0, 19, 9))}) == \
        [[(1, 0)], [(1, 1), (2, 0), (3, 0)]]
    # a tie: the lower track takes the lower object
    assert link_objects({1: boxes((0, 0, 9, 9), (0, 0, 9, 9)), 2: boxes((0, 0, 9, 9), (0, 0, 9, 9))}) == [[(1, 0), (2, 0)], [(1, 1), (2, 1)]]
    assert link_objects({1: boxes((0, 0, 9, 9)), 2: boxes((5, 0, 14, 9), (-5, 0, 4, 9))}) == [[(1, 0), (2, 0)], [(2, 1)]]
    # a gap closes a track: frame 2 has no match, so frame 3 opens a new one; an empty frame closes all
    assert link_objects({1: boxes((0, 0, 9, 9)), 2: boxes((50, 50, 59, 59)), 3: boxes((0, 0, 9, 9))}) == [[(1, 0)], [(2, 0)], [(3, 0)]]
    assert link_objects({1: boxes((0, 0, 9, 9)), 2: [], 3: boxes((0, 0, 9, 9))}) == [[(1, 0)], [(3, 0)]]
    assert link_objects({}) == [] and link_objects({4: []}) == []
    # frames in ascending order whatever the dictionary's; min_iou bounds a match
    assert link_objects({3: boxes((2, 0, 11, 9)), 1: boxes((0, 0, 9, 9)), 2: boxes((1, 0, 10, 9))}) == [[(1, 0), (2, 0), (3, 0)]]
    far = {1: boxes((0, 0, 9, 9)), 2: boxes((8, 0, 17, 9))}                # IoU 20 / 180
    assert link_objects(far) == [[(1, 0), (2, 0)]] and link_objects(far, min_iou=0.2) == [[(1, 0)], [(2, 0)]]
    for bad in (-0.1, 1.5, None, True):
        with pytest.raises(ValueError):
            link_objects(far, min_iou=bad)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
class NoCapture:
    def __getattr__(self, name):
        raise AssertionError("the capture was touched before the arguments were checked")


@pytest.mark.parametrize("kw", [dict(max_frames=0), dict(max_frames=256), dict(max_frames=2.5), dict(min_cover=0), dict(min_cover=256),
                                dict(threshold=-1), dict(threshold=256), dict(placement="paste"), dict(placement=None), dict(ingest="nv12"),
                                dict(scale=0), dict(scale=float("nan")), dict(scale="2"), dict(placement="translate", scale=2.0),
                                dict(connectivity=6), dict(connectivity=True), dict(connectivity=None), dict(open_radius=-1),
                                dict(open_radius=4), dict(open_radius=1.0), dict(min_area=0), dict(min_area=2.5), dict(max_objects=0),
                                dict(max_objects=65536), dict(max_objects=None), dict(min_iou=2), dict(min_iou=None)])
def test_moving_objects_refuses_before_the_capture_is_touched(kw):
    from evenvizion_amd.moving import moving_objects
    with pytest.raises(ValueError):
        moving_objects(NoCapture(), {1: np.eye(3)}, {"w": 8, "h": 6}, **kw)


def test_stabilize_parses_the_object_options(capsys):
    from evenvizion_amd import stabilize
    a = stabilize.parser().parse_args([])
    assert (a.plate_objects, a.object_connectivity, a.object_open, a.object_min_area, a.object_max) == (0, None, None, None, None)
    a = stabilize.parser().parse_args(["--plate", "1", "--plate_objects", "1", "--object_connectivity", "4", "--object_open", "2",
                                       "--object_min_area", "7", "--object_max", "12"])
    assert (a.plate_objects, a.object_connectivity, a.object_open, a.object_min_area, a.object_max) == (1, 4, 2, 7, 12)
    for bad in (["--plate_objects", "1"], ["--plate", "1", "--plate_objects", "2"], ["--plate", "1", "--object_open", "1"],
                ["--plate", "1", "--object_max", "3"], ["--plate", "1", "--plate_objects", "1", "--object_connectivity", "6"],
                ["--plate", "1", "--plate_objects", "1", "--object_open", "4"], ["--plate", "1", "--plate_objects", "1", "--object_open", "-1"],
                ["--plate", "1", "--plate_objects", "1", "--object_min_area", "0"], ["--plate", "1", "--plate_objects", "1", "--object_max", "0"],
                ["--plate", "1", "--plate_objects", "1", "--object_max", "65536"], ["--plate", "1", "--plate_objects", "1", "--trail", "1"]):
        with pytest.raises(SystemExit):
            stabilize.main(bad)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        stabilize.main(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    for word in ("--plate_objects", "--object_connectivity", "--object_open", "--object_min_area", "--object_max", "moving_objects.json"):
        assert word in text, word


# ---- the size of the work buffer -----------------------------------------------------------------------------------------------------
def test_work_bytes():
    from evenvizion_amd._lib import component_dtype, mask_components_work_bytes as wb
    assert component_dtype().itemsize == 40 and component_dtype().names == K.FIELDS
    for dw, dh, n in ((1, 1, 1), (9, 7, 300), (778, 287, 64), (1536, 864, 64), (65535, 32767, 1), (46340, 46340, 65535), (3, 5, 65535)):
        got = wb(dw, dh, n)
        assert 8 * dw * dh <= got <= 8 * dw * dh * n + (1 << 20), (dw, dh, n)
        assert got % (8 * dw * dh) == 0                                # whole masks: one i32 of area and one of ordinal per pixel
    assert wb(9, 7, 300) == 8 * 9 * 7 * 300 and wb(1536, 864, 64) < 8 * 1536 * 864 * 64     # groups of masks above 256 MiB
    assert wb(1536, 864, 64) == wb(1536, 864, 65535)                   # and then independent of nmasks
    for dw, dh, n in ((0, 5, 1), (5, 0, 1), (-1, 5, 1), (5, 5, -1), (5, 5, 65536), (65536, 32768, 1), (1 << 31, 1, 1), (5, 5, 0)):
        assert wb(dw, dh, n) == 0, (dw, dh, n)
