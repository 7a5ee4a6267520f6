"""The blended mosaic without a device: the restatement (tests/blend_checks.py) held against the identities include/evhip.h draws
from the contract of evh_blend_*, and the host side of evenvizion_amd.blend -- pairs, the gain solve, the quantisation, the
refusals of blended_mosaic and of the command line."""
import numpy as np
import pytest

import blend_checks as BC
import surface_checks as SC
import warp_checks as W
from evenvizion_amd import blend as B

SW, SH, DW, DH, ORIGIN = 37, 23, 53, 41, (-7, -5)


def frames_of(seed, n=5, gray=False):
    return np.random.default_rng(seed).integers(0, 256, (n, SH, SW) if gray else (n, SH, SW, 3), dtype=np.uint8)


def matrices():
    """frame pixel -> plane point: an integer and a fractional translation, two projective matrices, NaN"""
    return np.stack([W.translation(-3, -2), W.translation(4.37, 6.81),
                     np.array([[1.05, 0.08, 2.3], [-0.06, 0.97, 9.1], [6e-4, -3e-4, 1.0]]),
                     np.array([[0.9, -0.12, 11.6], [0.1, 1.1, -3.2], [-8e-4, 5e-4, 1.0]]), np.full((3, 3), np.nan)])


def covers(mats, n=5):
    return np.stack([BC.position(mats[k], SW, SH, DW, DH, ORIGIN)[2] for k in range(n)])


def test_position_and_taps_are_warp_checks():
    f, mats = frames_of(1), matrices()
    for k in range(5):
        U, V, cov = BC.position(mats[k], SW, SH, DW, DH, ORIGIN)
        val, cov_w = W.warp_frame(f[k], mats[k], DW, DH, ORIGIN)
        assert np.array_equal(cov, cov_w) and np.array_equal(SC.taps(f[k], U, V, cov)[cov], val[cov])
    cov = covers(mats)
    assert cov[:4].all(axis=(1, 2)).sum() == 0 and cov[:4].any(axis=(1, 2)).all() and not cov[4].any()
    assert (cov.sum(axis=0) == 1).any() and (cov.sum(axis=0) >= 3).any() and (cov.sum(axis=0) == 0).any()


@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("mode", [BC.FEATHER, BC.SEAM])
def test_a_pixel_one_frame_covers_holds_the_warp_entrys_byte(mode, gray):
    f, mats = frames_of(2, gray=gray), matrices()
    once = covers(mats).sum(axis=0) == 1
    want = W.warp_canvases(f, mats, "mosaic", DW, DH, ORIGIN)
    for F in (0, 1, 40, 65535):
        got, _ = BC.blend(f, mats, DW, DH, ORIGIN, mode, F)
        assert np.array_equal(got[once], want[once]), F


@pytest.mark.parametrize("mode", [BC.FEATHER, BC.SEAM])
def test_equal_values_blend_to_that_value(mode):
    f, mats = np.full((5, SH, SW, 3), 137, np.uint8), matrices()
    f[..., 1], f[..., 2] = 0, 255
    got, _ = BC.blend(f, mats, DW, DH, ORIGIN, mode, 40)
    any_cover = covers(mats).any(axis=0)
    assert (got[any_cover] == [137, 0, 255]).all() and (got[~any_cover] == 0).all()


@pytest.mark.parametrize("mode", [BC.FEATHER, BC.SEAM])
def test_no_gains_are_gains_of_one_and_chunks_are_one_call(mode):
    f, mats = frames_of(3), matrices()
    bg = frames_of(4, 1)[0][:1, :1].repeat(DH, 0).repeat(DW, 1)
    whole, state = BC.blend(f, mats, DW, DH, ORIGIN, mode, 40, background=bg)
    ones, state1 = BC.blend(f, mats, DW, DH, ORIGIN, mode, 40, gains=np.full((5, 3), 4096), background=bg)
    assert np.array_equal(whole, ones) and (state == state1).all()
    _, head = BC.blend(f[:3], mats[:3], DW, DH, ORIGIN, mode, 40)
    tail, state2 = BC.blend(f[3:], mats[3:], DW, DH, ORIGIN, mode, 40, state=head, background=bg)
    assert np.array_equal(whole, tail) and (state == state2).all()


@pytest.mark.parametrize("mode", [BC.FEATHER, BC.SEAM])
def test_ray_form_with_plane_tables_is_the_plane_form(mode):
    f = frames_of(5)
    inv = np.stack([np.linalg.inv(m) if np.isfinite(m).all() else m for m in matrices()])     # plane point -> frame pixel
    cols, rows = SC.plane_tables(DW, DH, ORIGIN)
    tw = np.stack([SC.ray_frame(f[k], inv[k], cols, rows)[2] for k in range(4)])
    assert (tw > 0).all()
    a = BC.blend(f, inv, DW, DH, ORIGIN, mode, 40, inverse_map=True)
    b = BC.blend_ray(f, inv, cols, rows, mode, 40)
    assert np.array_equal(a[0], b[0]) and (a[1] == b[1]).all()


def test_seam_keeps_the_earliest_of_equal_weights():
    f = frames_of(6, 2)
    mats = np.stack([W.translation(2, 3)] * 2)
    got, _ = BC.blend(f, mats, DW, DH, ORIGIN, BC.SEAM, 40)
    assert np.array_equal(got, W.warp_canvases(f[:1], mats[:1], "mosaic", DW, DH, ORIGIN))


def test_weight_is_symmetric_under_mirroring_the_frame():
    rng = np.random.default_rng(7)
    U = rng.integers(0, 32 * (SW - 1) + 1, (DH, DW)).astype(np.float64)
    V = rng.integers(0, 32 * (SH - 1) + 1, (DH, DW)).astype(np.float64)
    cov = np.ones((DH, DW), bool)
    for F in (0, 1, 40, 65535):
        w = BC.weight(U, V, cov, SW, SH, F)
        assert np.array_equal(w, BC.weight(32 * (SW - 1) - U, V, cov, SW, SH, F))
        assert np.array_equal(w, BC.weight(U, 32 * (SH - 1) - V, cov, SW, SH, F))
        assert w.min() >= 1 and w.max() <= F + 1
    assert (BC.weight(U, V, cov, SW, SH, 0) == 1).all()
    assert BC.weight(np.array([[0.0]]), np.array([[50.0]]), np.array([[True]]), SW, SH, 99)[0, 0] == 1       # on the border


def test_picture_of_a_handed_in_state_cannot_wrap():
    st = np.empty((1, 4, 2), object)
    den = (1 << 44) - 1
    st[0, :, 1] = den
    st[0, :, 0] = [(1 << 62) - 1, 255 * (den << 12) - (den << 11), 255 * (den << 12) - (den << 11) - 1, 0]
    assert BC.picture(st, BC.FEATHER).tolist() == [[64, 255, 254, 0]]          # 2^62 / 2^56
    assert BC.picture(st, BC.SEAM).tolist() == [[255, 255, 255, 0]]


# ---- the gain solve --------------------------------------------------------------------------------------------------------------------
def chain_stats(n, gamma, seed, strides=(1, 2)):
    """Pairs of a chain of n frames that show the same scene under exact gains gamma: N pixels of mean m per pair."""
    rng = np.random.default_rng(seed)
    pairs = B.exposure_pairs(n, strides)
    stats = np.zeros((len(pairs), 7), np.float64)
    for p, (i, j) in enumerate(pairs):
        N = float(rng.integers(900, 1100))
        m = rng.uniform(80, 120, 3)
        stats[p, 0], stats[p, 1:4], stats[p, 4:7] = N, N * gamma[i] * m, N * gamma[j] * m
    return pairs, stats


def test_equal_means_give_gains_of_one():
    pairs, stats = chain_stats(9, np.ones(9), 11)
    g = B.solve_gains(pairs, stats, 9)
    assert g.shape == (9, 3) and np.abs(g - 1.0).max() <= 1e-12
    assert np.abs(B.solve_gains(pairs, stats, 9, per_channel=False) - 1.0).max() <= 1e-12


def gradient(g, pairs, stats, c, sigma_n, sigma_g):
    """d gain_cost / d g, and the diagonal of the normal equations"""
    grad, diag = np.zeros(len(g)), np.zeros(len(g))
    for (i, j), s in zip(pairs, stats):
        N, a, b = s[0], s[1 + c] / s[0], s[4 + c] / s[0]
        r = g[i] * a - g[j] * b
        grad[i] += 2 * N * (r * a / sigma_n ** 2 - (1 - g[i]) / sigma_g ** 2)
        grad[j] += 2 * N * (-r * b / sigma_n ** 2 - (1 - g[j]) / sigma_g ** 2)
        diag[i] += N * (a * a / sigma_n ** 2 + 1 / sigma_g ** 2)
        diag[j] += N * (b * b / sigma_n ** 2 + 1 / sigma_g ** 2)
    return grad, diag


def test_the_gradient_of_the_cost_vanishes_at_the_solution():
    """The gradient is 2 (A g - rhs) of the normal equations.  A backward-stable solve leaves |A g - rhs|_inf <= c n eps |A|_inf
    |g|_inf with a modest c (4 here); A is symmetric positive definite, so |a_ij| <= max diagonal and |A|_inf <= n max diagonal:
    |gradient|_inf <= 8 n^2 eps max_diag max|g|.  Against that, the gradient at gains of 1 is some 1e5 here."""
    n, sigma_n, sigma_g = 12, 10.0, 0.1
    gamma = np.random.default_rng(12).uniform(0.75, 1.25, n)
    pairs, stats = chain_stats(n, gamma, 13, (1, 3))
    g = B.solve_gains(pairs, stats, n, sigma_n, sigma_g)
    for c in range(3):
        grad, diag = gradient(g[:, c], pairs, stats, c, sigma_n, sigma_g)
        bound = 8 * n * n * np.finfo(np.float64).eps * diag.max() * np.abs(g[:, c]).max()
        print("channel %d: |gradient| %.3e, bound %.3e, at ones %.3e" % (c, np.abs(grad).max(), bound,
                                                                          np.abs(gradient(np.ones(n), pairs, stats, c, sigma_n, sigma_g)[0]).max()))
        assert np.abs(grad).max() <= bound
        assert np.abs(gradient(np.ones(n), pairs, stats, c, sigma_n, sigma_g)[0]).max() > 1e6 * bound
        eps = 1e-6          # and the cost itself rises in every direction tried
        base = BC.gain_cost(g[:, c], pairs, stats, c, sigma_n, sigma_g)
        for k in range(n):
            for sign in (-1, 1):
                moved = g[:, c].copy()
                moved[k] += sign * eps
                assert BC.gain_cost(moved, pairs, stats, c, sigma_n, sigma_g) >= base


def test_a_weak_prior_leaves_the_corrected_frames_equal():
    """Frame k shows the scene times gamma_k, so the corrected products h_k = g_k gamma_k should agree.  In h the data term is
    sum_p N m^2 / sigma_n^2 (h_i - h_j)^2 = h' L h with L the Laplacian of the pair graph under those weights, and the normal
    equations read L h = r, r_i = deg_i (1 - g_i) / (sigma_g^2 gamma_i), deg_i = the sum of N over the pairs of frame i.  r sums
    to what L cannot see, so |h - mean h|_2 <= |r|_2 / lambda_2(L) and any two h differ by at most twice that.  |1 - g_i| is
    bounded without the solution: the optimum costs no more than g = 1 / gamma (no data cost, prior cost P0), and each prior term
    alone is at most the whole, so (1 - g_i)^2 <= P0 sigma_g^2 / deg_i.  Everything in the bound comes from the inputs; the
    ratio of prior to data weight, sigma_n^2 / (sigma_g^2 m^2), is what makes it small."""
    n, sigma_n, sigma_g = 8, 1.0, 100.0
    gamma = np.random.default_rng(14).uniform(0.75, 1.25, n)
    pairs, stats = chain_stats(n, gamma, 15)
    g = B.solve_gains(pairs, stats, n, sigma_n, sigma_g)
    for c in range(3):
        L, deg, P0 = np.zeros((n, n)), np.zeros(n), 0.0
        for (i, j), s in zip(pairs, stats):
            N = s[0]
            m = s[1 + c] / N / gamma[i]
            wgt = N * m * m / sigma_n ** 2
            L[i, i] += wgt; L[j, j] += wgt; L[i, j] -= wgt; L[j, i] -= wgt
            deg[i] += N; deg[j] += N
            P0 += N * ((1 - 1 / gamma[i]) ** 2 + (1 - 1 / gamma[j]) ** 2) / sigma_g ** 2
        slack = np.sqrt(P0 * sigma_g ** 2 / deg)                          # |1 - g_i| <= slack_i
        r = deg * slack / (sigma_g ** 2 * gamma)
        bound = 2 * np.linalg.norm(r) / np.linalg.eigvalsh(L)[1]
        h = g[:, c] * gamma
        print("channel %d: spread of g gamma %.3e, bound %.3e" % (c, h.max() - h.min(), bound))
        assert bound < 1e-4 and h.max() - h.min() <= bound
        assert abs(h.mean() - 1) < 0.3                                    # the prior still fixes the level near 1


def test_pairs_below_min_pixels_and_frames_alone():
    pairs = [(0, 1), (1, 2), (2, 3)]
    stats = np.array([[1000, 100000, 0, 0, 120000, 0, 0], [63, 6300, 0, 0, 63000, 0, 0], [0, 0, 0, 0, 0, 0, 0]], np.int64)
    g = B.solve_gains(pairs, stats, 5)
    assert (g[2:] == 1.0).all() and (g[:, 1:] == 1.0).all() and g[0, 0] > 1.0 > g[1, 0]
    assert B.solve_gains([], np.zeros((0, 7)), 0).shape == (0, 3)
    with pytest.raises(ValueError, match="4096"):
        B.solve_gains([], np.zeros((0, 7)), 4097)
    with pytest.raises(ValueError):
        B.solve_gains([(0, 5)], np.zeros((1, 7)), 5)
    with pytest.raises(ValueError):
        B.solve_gains([(0, 1)], np.zeros((2, 7)), 5)


def test_quantise_gains():
    got = B.quantise_gains([0, 1 / 8192, 1, 15.9999, 16, 100])
    assert got.dtype == np.uint16 and got.tolist() == [1, 1, 4096, 65535, 65535, 65535]
    assert B.quantise_gains(np.array([[0.75, 1.25, 3 / 8192]])).tolist() == [[3072, 5120, 2]]      # 1.5 rounds to even


def test_exposure_pairs():
    assert B.exposure_pairs(0) == [] and B.exposure_pairs(1) == []
    assert B.exposure_pairs(2) == [(0, 1)]
    got = B.exposure_pairs(17)
    assert got == [(k, k + 1) for k in range(16)] + [(k, k + 4) for k in range(13)] + [(0, 16)]
    assert B.exposure_pairs(5, (2,)) == [(0, 2), (1, 3), (2, 4)]
    for bad in ((0,), (1, 1), (1.5,), (True,)):
        with pytest.raises(ValueError):
            B.exposure_pairs(5, bad)
    with pytest.raises(ValueError):
        B.exposure_pairs(-1)


class Untouched:
    """A capture that must not be read"""
    def __getattr__(self, name):
        raise AssertionError("the capture was touched: %s" % name)


@pytest.mark.parametrize("kw", [dict(blend="median"), dict(feather_px=-1), dict(feather_px=2048), dict(feather_px=True),
                                dict(gains=np.zeros((3, 3))), dict(gains=np.ones((3, 2))), dict(gains=np.full((1, 3), np.nan)),
                                dict(placement="paste"), dict(scale=0), dict(surface="torus"),
                                dict(surface="cylinder", placement="translate"), dict(focal=300.0), dict(surface="sphere", focal=-1.0),
                                dict(chunk_frames=0), dict(ingest="rgb")])
def test_blended_mosaic_refuses_before_it_touches_the_capture(kw):
    with pytest.raises(ValueError):
        B.blended_mosaic(Untouched(), {1: np.eye(3).tolist()}, {"w": 8, "h": 8}, **kw)


@pytest.mark.parametrize("kw", [dict(strides=(0,)), dict(step=0), dict(step=65), dict(lo=9, hi=8), dict(hi=256), dict(ingest="rgb"),
                                dict(chunk_frames=0)])
def test_exposure_stats_refuses_before_it_touches_the_capture(kw):
    with pytest.raises(ValueError):
        B.exposure_stats(Untouched(), {1: np.eye(3).tolist(), 2: np.eye(3).tolist()}, {"w": 8, "h": 8}, **kw)


@pytest.mark.parametrize("argv", [["--blend", "feather"], ["--blend", "seam", "--mode", "each"], ["--mode", "mosaic", "--exposure", "1"],
                                  ["--mode", "mosaic", "--feather", "8"], ["--mode", "mosaic", "--blend", "median"],
                                  ["--mode", "mosaic", "--blend", "feather", "--feather", "-1"],
                                  ["--mode", "mosaic", "--blend", "feather", "--plate", "1"]])
def test_command_line_refusals(argv, capsys):
    from evenvizion_amd import stabilize
    with pytest.raises(SystemExit) as e:
        stabilize.main(argv + ["--path_to_video", "/nonexistent/video.mp4"])
    assert e.value.code == 2
    assert "usage" in capsys.readouterr().err
