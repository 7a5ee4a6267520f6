"""The background plate without a device: the numpy restatement of evh_plate_fixed_plane (tests/plate_checks.py) against a literal
per-pixel loop, what the plate is for (a panning scene loses its moving object), the frame selection, and the refusals of
background_plate and the command line before anything is opened."""
import numpy as np
import pytest

import plate_checks as P
import warp_checks as W
from evenvizion_amd import stabilization as S


def literal(frames, mats, dw, dh, origin, background, inverse_map, min_cover, threshold):
    """The header's four steps, pixel by pixel, with sorted()."""
    frames = np.asarray(frames)
    n = len(frames)
    cn = 3 if frames.ndim == 4 else 1
    warped = [W.warp_frame(frames[k], mats[k], dw, dh, origin, inverse_map) for k in range(n)]
    plate = np.zeros((dh, dw, cn), np.uint8)
    count = np.zeros((dh, dw), np.uint8)
    masks = np.zeros((n, dh, dw), np.uint8)
    bg = np.zeros((dh, dw, cn), np.uint8) if background is None else np.asarray(background).reshape(dh, dw, cn)

    def gray(p):
        return int(p[0]) if cn == 1 else (int(p[0]) * 1868 + int(p[1]) * 9617 + int(p[2]) * 4899 + 8192) >> 14
    for y in range(dh):
        for x in range(dw):
            cover = [k for k in range(n) if warped[k][1][y, x]]
            samples = [warped[k][0][y, x].reshape(cn) for k in cover]
            count[y, x] = len(cover)
            if len(cover) < min_cover:
                plate[y, x] = bg[y, x]
                continue
            for c in range(cn):
                plate[y, x, c] = sorted(int(s[c]) for s in samples)[(len(cover) - 1) >> 1]
            for k, s in zip(cover, samples):
                masks[k, y, x] = 255 if abs(gray(s) - gray(plate[y, x])) > threshold else 0
    return (plate if cn == 3 else plate[..., 0]), count, masks


def scattered(seed, n, gray):
    """n frames of 7 x 5 scattered over a 13 x 9 canvas: integer pastes, fractional shifts and one projective frame"""
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (n, 5, 7) if gray else (n, 5, 7, 3), dtype=np.uint8)
    mats = [W.translation(int(rng.integers(-2, 9)), int(rng.integers(-2, 6))) for _ in range(n)]
    if n > 2:
        mats[1] = W.translation(2.25, 1.5)
        mats[2] = np.array([[1.1, 0.1, 1.0], [-0.05, 0.9, 2.0], [1e-3, -2e-3, 1.0]])
    return frames, np.stack(mats)


@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("n,min_cover,threshold", [(1, 1, 0), (2, 1, 16), (5, 2, 16), (6, 3, 0), (9, 1, 255), (12, 12, 40)])
def test_restatement_equals_the_literal_loop(gray, n, min_cover, threshold):
    frames, mats = scattered(100 + n, n, gray)
    bg = np.random.default_rng(7).integers(0, 256, (9, 13) if gray else (9, 13, 3), dtype=np.uint8)
    for background in (None, bg):
        got = P.plate(frames, mats, 13, 9, (-1, -1), background, False, min_cover, threshold)
        want = literal(frames, mats, 13, 9, (-1, -1), background, False, min_cover, threshold)
        for g, w, name in zip(got, want, ("plate", "count", "masks")):
            assert g.dtype == np.uint8 and g.shape == w.shape and np.array_equal(g, w), name
    assert got[1].max() >= min(n, 2) and got[1].min() == 0              # pixels under several frames and under none


@pytest.mark.parametrize("n", [1, 3, 7, 11])
def test_odd_counts_give_numpys_median(n):
    rng = np.random.default_rng(n)
    frames = rng.integers(0, 256, (n, 9, 13, 3), dtype=np.uint8)
    plate, count, _ = P.plate(frames, np.stack([np.eye(3)] * n), 13, 9)
    assert (count == n).all()
    assert np.array_equal(plate, np.median(frames, axis=0).astype(np.uint8))


def test_even_counts_take_the_lower_middle_value_and_no_frames_the_background():
    frames = np.array([10, 200, 30, 100], np.uint8).reshape(4, 1, 1)
    plate, count, masks = P.plate(frames, np.stack([np.eye(3)] * 4), 1, 1, threshold=69)
    assert plate[0, 0] == 30 and count[0, 0] == 4 and masks[:, 0, 0].tolist() == [0, 255, 0, 255]
    bg = np.full((2, 3, 3), 9, np.uint8)
    plate, count, masks = P.plate(np.zeros((0, 4, 4, 3), np.uint8), np.zeros((0, 9)), 3, 2, background=bg)
    assert np.array_equal(plate, bg) and not count.any() and masks.shape == (0, 2, 3)
    assert P.gray(np.array([255, 255, 255])) == 255 and P.gray(np.array([0, 0, 255])) == (4899 * 255 + 8192) >> 14


def test_plate_removes_the_moving_object_of_a_panning_scene():
    P.check_panning_scene(lambda f, m, dw, dh, **kw: P.plate(f, m, dw, dh, **kw),
                          lambda f, m, dw, dh: W.warp_canvases(f, m, "mosaic", dw, dh))


@pytest.mark.parametrize("n_frames,max_frames,first,step,length", [
    (1, 64, 1, 1, 1), (64, 64, 1, 1, 64), (65, 64, 1, 2, 33), (121, 64, 1, 2, 61), (255, 255, 1, 1, 255), (256, 255, 1, 2, 128),
    (1000, 64, 1, 16, 63), (1000, 255, 1, 4, 250), (7, 1, 1, 7, 1)])
def test_plate_frame_numbers(n_frames, max_frames, first, step, length):
    got = S.plate_frame_numbers(n_frames, max_frames)
    assert got == list(range(first, n_frames + 1, step)) and len(got) == length <= max_frames
    assert got[0] == 1 and got[-1] <= n_frames and got[-1] + step > n_frames
    assert step == max(1, -(-n_frames // max_frames))
    with pytest.raises(ValueError):
        S.plate_frame_numbers(0, 64)
    with pytest.raises(ValueError):
        S.plate_frame_numbers(10, 0)


class NoCapture:
    def __getattr__(self, name):
        raise AssertionError("the capture was touched before the arguments were checked")


@pytest.mark.parametrize("kw", [dict(max_frames=0), dict(max_frames=256), dict(max_frames=-1), dict(min_cover=0), dict(min_cover=256),
                                dict(threshold=-1), dict(threshold=256), dict(placement="paste"), dict(placement=None),
                                dict(ingest="nv12"), dict(ingest=None)])
def test_background_plate_refuses_before_the_capture_is_touched(kw):
    with pytest.raises(ValueError):
        S.background_plate(NoCapture(), {1: np.eye(3)}, {"w": 8, "h": 6}, **kw)


def test_background_plate_refuses_max_bytes_after_the_first_frame_only():
    class OneFrame:
        width, height, bgr_mode = 8, 6, None
        reads = 0

        def read(self):
            self.reads += 1
            assert self.reads == 1, "a further frame was read before max_bytes was checked"
            return True, np.zeros((6, 8, 3), np.uint8)
    cap = OneFrame()
    with pytest.raises(ValueError, match="max_bytes"):
        S.background_plate(cap, {k: W.translation(k, 0) for k in range(1, 5)}, {"w": 8, "h": 6}, placement="translate",
                           ingest="bgr", masks=True, max_bytes=4 * 8 * 6 * 3)
    assert cap.reads == 1


def test_stabilize_parses_the_plate_options(capsys):
    from evenvizion_amd import stabilize
    a = stabilize.parser().parse_args([])
    assert (a.plate, a.plate_frames, a.plate_min_cover, a.plate_masks, a.plate_threshold) == (0, 64, 1, 0, 16)
    a = stabilize.parser().parse_args(["--plate", "1", "--plate_frames", "200", "--plate_min_cover", "3", "--plate_masks", "1",
                                       "--plate_threshold", "0"])
    assert (a.plate, a.plate_frames, a.plate_min_cover, a.plate_masks, a.plate_threshold) == (1, 200, 3, 1, 0)
    for bad in (["--plate", "2"], ["--plate", "1", "--plate_frames", "256"], ["--plate", "1", "--plate_frames", "0"],
                ["--plate", "1", "--plate_min_cover", "0"], ["--plate", "1", "--plate_threshold", "256"],
                ["--plate", "1", "--plate_masks", "2"], ["--plate", "1", "--trail", "1"], ["--plate", "1", "--comparison", "1"]):
        with pytest.raises(SystemExit):
            stabilize.main(bad)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        stabilize.main(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    for word in ("--plate", "--plate_frames", "--plate_min_cover", "--plate_masks", "--plate_threshold", "plate.ppm"):
        assert word in text, word


def test_write_png_takes_gray_pictures(tmp_path):
    import struct
    import zlib
    from evenvizion_amd.matching_pictures import write_png
    g = np.arange(35, dtype=np.uint8).reshape(5, 7) * 7
    path = str(tmp_path / "g.png")
    write_png(path, g, gray=True)
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[12:16] == b"IHDR"
    assert struct.unpack(">IIBBBBB", data[16:29]) == (7, 5, 8, 0, 0, 0, 0)          # 8-bit grayscale
    at = data.index(b"IDAT")
    size = struct.unpack(">I", data[at - 4:at])[0]
    rows = np.frombuffer(zlib.decompress(data[at + 4:at + 4 + size]), np.uint8).reshape(5, 8)
    assert not rows[:, 0].any() and np.array_equal(rows[:, 1:], g)
    for bad, kw in ((np.zeros((5, 7, 2), np.uint8), {}), (g, {}), (np.zeros((5, 7, 3), np.uint8), dict(gray=True))):
        with pytest.raises(ValueError):
            write_png(path, bad, **kw)
