"""Multi-band blending without a device: the restatement (tests/bands_checks.py) held against the identities include/evhip.h draws
from the contract of evh_blend_bands_*, the sizing helpers, the refusals of the drivers and of the command line, and what the band
blend is for -- on a crafted pair of frames it removes SEAM's exposure step and keeps the texture FEATHER loses."""
import numpy as np
import pytest

import bands_checks as N
import blend_checks as BC
import surface_checks as SC
import warp_checks as W
from evenvizion_amd import blend as B

SW, SH, DW, DH, ORIGIN = 32, 24, 45, 37, (-7, -5)


def frames_of(seed, n=5, gray=False):
    return np.random.default_rng(seed).integers(0, 256, (n, SH, SW) if gray else (n, SH, SW, 3), dtype=np.uint8)


def matrices():
    """frame pixel -> plane point: an integer and a fractional translation, two projective matrices, NaN"""
    return np.stack([W.translation(-3, -2), W.translation(4.37, 6.81),
                     np.array([[1.05, 0.08, 2.3], [-0.06, 0.97, 9.1], [6e-4, -3e-4, 1.0]]),
                     np.array([[0.9, -0.12, 11.6], [0.1, 1.1, -3.2], [-8e-4, 5e-4, 1.0]]), np.full((3, 3), np.nan)])


GAINS = np.array([[3072, 4096, 5120], [5000, 3900, 4100], [4096, 4096, 4096], [2048, 8192, 4097], [1, 2, 3]], np.uint16)


def test_level_sizes_and_the_sizing_helpers():
    from evenvizion_amd import _lib
    assert N.level_sizes(45, 37, 5) == [(45, 37), (23, 19), (12, 10), (6, 5), (3, 3), (2, 2)]
    for dw, dh, cn, levels in ((45, 37, 1, 0), (45, 37, 3, 5), (64, 48, 3, 8), (1, 1, 1, 8), (1600, 900, 3, 5), (46340, 46340, 3, 8)):
        assert _lib.bands_state_elems(dw, dh, cn, levels) == N.state_elems(dw, dh, cn, levels)
        assert _lib.bands_frame_ws_bytes(dw, dh, cn, levels) == N.frame_ws_bytes(dw, dh, cn, levels)
    for bad in ((0, 4, 3, 1), (4, 0, 3, 1), (4, 4, 2, 1), (4, 4, 3, -1), (4, 4, 3, 9)):
        assert _lib.bands_state_elems(*bad) == -1 and _lib.bands_frame_ws_bytes(*bad) == -1


@pytest.mark.parametrize("gray", [False, True])
def test_labels_are_seams_choice_and_no_levels_are_seam(gray):
    """(b): the labels name the frame whose sample SEAM keeps, and levels = 0 under them is SEAM byte for byte"""
    f, mats = frames_of(1, gray=gray), matrices()
    for feather in (0, 40, 65535):
        best, label = N.labels_plane(mats, SW, SH, DW, DH, ORIGIN, feather)
        seam, state = BC.blend(f, mats, DW, DH, ORIGIN, BC.SEAM, feather, GAINS)
        assert np.array_equal(best, state[..., -1].astype(np.uint32))
        assert ((label == N.NOBODY) == (best == 0)).all() and (label[best > 0] < 4).all()
        got, _ = N.bands_plane(f, mats, DW, DH, ORIGIN, label, 0, gains=GAINS)
        assert np.array_equal(got, seam)
    # calls that carry the state equal one call, and the earliest frame holds among equal weights
    head = N.labels_plane(mats[:2], SW, SH, DW, DH, ORIGIN, 40)
    tail = N.labels_plane(mats[2:], SW, SH, DW, DH, ORIGIN, 40, first_label=2, best=head[0], label=head[1])
    whole = N.labels_plane(mats, SW, SH, DW, DH, ORIGIN, 40)
    assert np.array_equal(tail[0], whole[0]) and np.array_equal(tail[1], whole[1])
    twice = N.labels_plane(np.stack([W.translation(2, 3)] * 2), SW, SH, DW, DH, ORIGIN, 40)[1]
    assert set(twice.reshape(-1).tolist()) == {0, N.NOBODY}


@pytest.mark.parametrize("levels", [0, 1, 3, 5])
def test_one_frame_under_its_own_labels_is_the_warp_entrys_picture(levels):
    """(a), to the border of the frame: the round-up of W keeps every weight with support positive"""
    f = frames_of(2)
    for m in matrices()[:4]:
        val, cov = W.warp_frame(f[0], m, DW, DH, ORIGIN)
        label = np.where(cov, 0, N.NOBODY).astype(np.uint16)
        got, state = N.bands_plane(f[:1], m[None], DW, DH, ORIGIN, label, levels)
        assert cov.any() and np.array_equal(got[cov], val[cov]) and (got[~cov] == 0).all()
        gain = np.array([[5000, 3900, 65535]], np.uint16)
        got, _ = N.bands_plane(f[:1], m[None], DW, DH, ORIGIN, label, levels, gains=gain)
        want = np.minimum(255, (val.astype(np.int64) * gain[0].astype(np.int64) + 2048) >> 12)
        assert np.array_equal(got[cov], want[cov])


@pytest.mark.parametrize("levels", [0, 2, 5, 8])
def test_constant_frames_blend_to_the_constant(levels):
    """(c): any labels that give every pixel to one of the frames"""
    f = np.zeros((4, SH, SW, 3), np.uint8)
    f[...] = [137, 0, 255]
    label = np.random.default_rng(3).integers(0, 4, (DH, DW)).astype(np.uint16)
    gain = np.tile(np.array([[5000, 3900, 3000]], np.uint16), (4, 1))
    got, state = N.bands_plane(f, matrices()[:4], DW, DH, ORIGIN, label, levels, gains=gain)
    want = np.minimum(255, (np.array([137, 0, 255]) * gain[0].astype(np.int64) + 2048) >> 12)
    assert (got == want).all()
    top = N.split(state, DW, DH, 3, levels)[0]
    assert (top[..., 3] == 65536).all()                    # the masks partition the canvas


def test_carried_state_frame_order_and_the_state_layout():
    """(d)"""
    f, mats = frames_of(4), matrices()
    label = N.labels_plane(mats, SW, SH, DW, DH, ORIGIN, 40)[1]
    pos = N.plane_positions(mats, SW, SH, DW, DH, ORIGIN)
    whole = N.bands(f, pos, label, 3, gains=GAINS)
    assert whole[1].size == N.state_elems(DW, DH, 3, 3)
    _, head = N.bands(f[:2], pos[:2], label, 3, gains=GAINS[:2])
    tail = N.bands(f[2:], pos[2:], label, 3, first_label=2, gains=GAINS[2:], state=head)
    assert np.array_equal(tail[0], whole[0]) and np.array_equal(tail[1], whole[1])
    other = N.bands(f, pos, label, 3, gains=GAINS, order=[3, 0, 4, 2, 1])
    assert np.array_equal(other[0], whole[0]) and np.array_equal(other[1], whole[1])
    # no frames: the picture of the incoming state
    again = N.bands(f[:0], [], label, 3, state=whole[1])
    assert np.array_equal(again[0], whole[0]) and np.array_equal(again[1], whole[1])
    assert not np.array_equal(whole[0], N.bands(f, pos, label, 0, gains=GAINS)[0])      # the levels act


def test_ray_form_with_plane_tables_is_the_plane_form():
    """(e)"""
    f = frames_of(5)
    inv = np.stack([np.linalg.inv(m) if np.isfinite(m).all() else m for m in matrices()])
    cols, rows = SC.plane_tables(DW, DH, ORIGIN)
    assert all((SC.ray_frame(f[k], inv[k], cols, rows)[2] > 0).all() for k in range(4))
    la = N.labels_plane(inv, SW, SH, DW, DH, ORIGIN, 40, inverse_map=True)
    lb = N.labels_ray(inv, cols, rows, SW, SH, 40)
    assert np.array_equal(la[0], lb[0]) and np.array_equal(la[1], lb[1])
    a = N.bands_plane(f, inv, DW, DH, ORIGIN, la[1], 4, inverse_map=True, gains=GAINS)
    b = N.bands_ray(f, inv, cols, rows, la[1], 4, gains=GAINS)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- what it is for ---------------------------------------------------------------------------------------------------------------------
def test_bands_remove_the_exposure_step_and_keep_the_texture():
    """Canvas 96 x 48; two gray frames of 64 x 48 at x = 0 and x = 32, cut from a checkerboard 120 +- 20; the second one is shifted
    by one pixel and carries a gain of 4915 / 4096 = 1.2; the seam lies at x = 48, the middle of the overlap, on every row;
    levels = 4.  SEAM and FEATHER (16 pixels) are blend_checks' own.  SEAM's rule puts its seam at x = 48 only on the rows 16 .. 31
    (nearer the top and bottom both frames are equally near their border and the earlier one holds), so the SEAM picture with the
    seam at x = 48 everywhere is put together from blend_checks' SEAM of either frame alone.  Figures of the restatement, all
    rows: jump 24.00 / 0.84 / 2.50 and texture 41.14 / 4.20 / 38.29 for SEAM / FEATHER / bands."""
    dw, dh, sw, sh = 96, 48, 64, 48
    yy, xx = np.mgrid[0:dh, 0:dw + 2]
    scene = (120 + 20 * np.where((xx + yy) & 1, 1, -1)).astype(np.uint8)
    frames = np.stack([scene[:, 0:sw], scene[:, 33:33 + sw]])
    mats = np.stack([W.translation(0, 0), W.translation(32, 0)])
    gains = np.array([[4096] * 3, [4915] * 3], np.uint16)
    label = np.where(np.arange(dw)[None, :] < 48, 0, 1).astype(np.uint16).repeat(dh, 0)
    own = N.labels_plane(mats, sw, sh, dw, dh, (0, 0), 16 * 32)[1]
    assert np.array_equal(own[16:32], label[16:32])
    alone = [BC.blend(frames[k:k + 1], mats[k:k + 1], dw, dh, (0, 0), BC.SEAM, 16 * 32, gains[k:k + 1])[0] for k in range(2)]
    seam = np.where(label == 0, alone[0], alone[1]).astype(np.float64)
    assert np.array_equal(seam[16:32], BC.blend(frames, mats, dw, dh, (0, 0), BC.SEAM, 16 * 32, gains)[0][16:32])
    feather = BC.blend(frames, mats, dw, dh, (0, 0), BC.FEATHER, 16 * 32, gains)[0].astype(np.float64)
    got = N.bands_plane(frames, mats, dw, dh, (0, 0), label, 4, gains=gains)[0].astype(np.float64)

    def jump(p):
        return abs(p[:, 48:52].mean() - p[:, 44:48].mean())

    def texture(p):
        return np.abs(np.diff(p[:, 44:52], axis=1)).mean()

    print("jump: seam %.2f feather %.2f bands %.2f; texture: seam %.2f feather %.2f bands %.2f"
          % (jump(seam), jump(feather), jump(got), texture(seam), texture(feather), texture(got)))
    assert jump(got) <= jump(seam) / 4
    assert texture(got) >= 0.8 * texture(seam)
    assert texture(got) >= 4 * texture(feather)


# ---- the drivers' refusals --------------------------------------------------------------------------------------------------------------
class Untouched:
    """A capture that must not be read"""
    def __getattr__(self, name):
        raise AssertionError("the capture was touched: %s" % name)


@pytest.mark.parametrize("kw", [dict(bands=-1), dict(bands=9), dict(bands=2.0), dict(bands=True), dict(feather_px=-1), dict(scale=0),
                                dict(surface="torus"), dict(surface="cylinder", placement="translate"), dict(focal=300.0),
                                dict(chunk_frames=0), dict(ingest="rgb"), dict(gains=np.zeros((3, 3)))])
def test_blended_mosaic_in_bands_refuses_before_it_touches_the_capture(kw):
    with pytest.raises(ValueError):
        B.blended_mosaic(Untouched(), {1: np.eye(3).tolist()}, {"w": 8, "h": 8}, blend="bands", **kw)


def test_a_label_mask_names_at_most_65535_frames():
    with pytest.raises(ValueError):
        B.blended_mosaic(Untouched(), {1: np.eye(3).tolist(), 65537: np.eye(3).tolist()}, {"w": 8, "h": 8}, blend="bands")
    with pytest.raises(ValueError):
        B.seam_labels({1: np.eye(3).tolist(), 65537: np.eye(3).tolist()}, {"w": 8, "h": 8}, (8, 8))


@pytest.mark.parametrize("kw", [dict(frame_size=(0, 8)), dict(frame_size=(8, 8), feather_px=-1), dict(frame_size=(8, 8), placement="paste"),
                                dict(frame_size=(8, 8), surface="torus"), dict(frame_size=(8, 8), scale=0)])
def test_seam_labels_refuses_bad_arguments(kw):
    with pytest.raises(ValueError):
        B.seam_labels({1: np.eye(3).tolist()}, {"w": 8, "h": 8}, **kw)


@pytest.mark.parametrize("argv", [["--blend", "bands"], ["--mode", "mosaic", "--blend", "bands", "--bands", "9"],
                                  ["--mode", "mosaic", "--blend", "bands", "--bands", "-1"],
                                  ["--mode", "mosaic", "--blend", "feather", "--bands", "3"], ["--mode", "mosaic", "--bands", "3"],
                                  ["--mode", "mosaic", "--blend", "feather", "--bands", "5"], ["--mode", "mosaic", "--bands", "5"],
                                  ["--mode", "mosaic", "--blend", "bands", "--plate", "1"]])
def test_command_line_refusals(argv, capsys):
    from evenvizion_amd import stabilize
    with pytest.raises(SystemExit) as e:
        stabilize.main(argv + ["--path_to_video", "/nonexistent/video.mp4"])
    assert e.value.code == 2
    assert "usage" in capsys.readouterr().err
