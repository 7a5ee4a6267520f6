"""The steady view without a GPU: the numpy restatement of evh_steady_frames against plain statements, the properties of
steady.smooth_path (each derivable, held to 1e-9 pixels at the frame corners), steady.steady_taps, and the driver's loop against
a recording context over scripted captures."""
import numpy as np
import pytest

import frames_checks as F
import steady_checks as S
import warp_checks as W
from evenvizion_amd import runtime, steady

TOL = 1e-9
WH = (64.0, 48.0)
INFO = {"w": 64, "h": 48}


# ---- the restatement against plain statements ------------------------------------------------------------------------------------------
def frames_of(seed, n, w, h, gray=False):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w) if gray else (n, h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("gray", [False, True])
def test_restatement_identity_and_integer_translation(gray):
    f = frames_of(1, 2, 13, 9, gray)
    eye = np.eye(3).reshape(9)
    pic, of, counts = S.steady_frames(f, [[1], [0]], [[eye], [eye]], 13, 9)
    assert np.array_equal(pic[0], f[1]) and np.array_equal(pic[1], f[0]) and (of == 1).all() and counts.tolist() == [[0, 117]] * 2
    # output pixel (x, y) shows frame pixel (x - 4, y + 2): the frame pasted at (4, -2), clipped, over the background
    bg = frames_of(2, 1, 20, 12, gray)[0]
    pic, of, counts = S.steady_frames(f, [[0]], [[W.translation(-4, 2).reshape(9)]], 20, 12, 0, bg)
    want = bg.copy()
    want[0:7, 4:17] = f[0][2:9, 0:13]
    assert np.array_equal(pic[0], want)
    assert (of[0][0:7, 4:17] == 1).all() and of[0].sum() == 7 * 13 and counts.tolist() == [[240 - 91, 91]]
    # a tap that is no frame of the chunk covers nothing; without a background the picture is black
    pic, of, counts = S.steady_frames(f, [[2, -1]], [[eye, eye]], 13, 9)
    assert not pic.any() and not of.any() and counts.tolist() == [[117, 0, 0]]


@pytest.mark.parametrize("feather", [1, 33, 256, 8160])
def test_restatement_feather(feather):
    f = frames_of(3, 2, 37, 21)
    eye, paste = np.eye(3).reshape(9), W.translation(-5, -3).reshape(9)       # tap 0 pasted at (5, 3), tap 1 the identity
    pic, of, _ = S.steady_frames(f, [[0, 1]], [[paste, eye]], 37, 21, feather)
    d = S.edge_distance(paste, 37, 21, 37, 21)
    first = np.zeros((21, 37), np.uint8)
    first[3:, 5:] = f[0][:18, :32, 0] * 0 + 1
    assert np.array_equal(of[0], np.where(first == 1, 1, 2))
    # d in 1/32 pixels from the plain statement: a pixel n whole pixels inside tap 0's frame has d = 32 n
    x, y = np.meshgrid(np.arange(37), np.arange(21))
    plain_d = 32 * np.minimum(np.minimum(x - 5, 36 - (x - 5)), np.minimum(y - 3, 20 - (y - 3)))
    own = first == 1
    assert np.array_equal(d[own], plain_d[own])
    v0 = np.zeros_like(f[1])
    v0[3:, 5:] = f[0][:18, :32]
    assert np.array_equal(pic[0][~own], f[1][~own])                                   # outside tap 0: the second tap alone
    assert np.array_equal(pic[0][own & (d == 0)], f[1][own & (d == 0)])               # d = 0: wholly the second tap's byte
    assert np.array_equal(pic[0][own & (d >= feather)], v0[own & (d >= feather)])     # d >= feather: the first tap's byte
    band = own & (d < feather)
    mixed = (v0.astype(np.int64) * d[..., None] + f[1].astype(np.int64) * (feather - d[..., None]) + (feather >> 1)) // feather
    assert np.array_equal(pic[0][band], mixed[band].astype(np.uint8))
    # without a second tap the band stays the first tap's, over any background
    bg = frames_of(4, 1, 37, 21)[0]
    pic, of, _ = S.steady_frames(f, [[0, -1]], [[paste, eye]], 37, 21, feather, bg)
    assert np.array_equal(pic[0][own], v0[own]) and np.array_equal(pic[0][~own], bg[~own])


# ---- smooth_path ----------------------------------------------------------------------------------------------------------------------------
def translation(dx, dy=0.0):
    return np.array([[1.0, 0.0, dx], [0.0, 1.0, dy], [0.0, 0.0, 1.0]])


def corners_of(M):
    q, tw = steady.project(M, steady.rectangle(*WH))
    assert np.all(tw > 0)
    return q


def zoomed(zoom):
    """The corners of the zoom alone, from its plain statement: c + (p - c) / zoom."""
    c = np.array(WH) / 2
    return c + (steady.rectangle(*WH) - c) / zoom


def weights(radius, sigma=None):
    s = radius / 2.0 if sigma is None else sigma
    return {j: np.exp(-j * j / (2.0 * s * s)) for j in range(-radius, radius + 1)}


@pytest.mark.parametrize("zoom", [1.0, 1.1])
def test_static_camera_and_radius_zero_give_the_zoom_alone(zoom):
    still = {k: np.eye(3) for k in range(1, 12)}
    for B in steady.smooth_path(still, INFO, radius=4, zoom=zoom).values():
        assert np.abs(corners_of(B) - zoomed(zoom)).max() <= TOL
    moving = {k: translation(3.0 * k + np.sin(k), np.cos(2.0 * k)) for k in range(1, 12)}
    for B in steady.smooth_path(moving, INFO, radius=0, zoom=zoom).values():
        assert np.array_equal(corners_of(B), corners_of(steady.zoom_matrix(zoom, *WH)))
        assert np.abs(corners_of(B) - zoomed(zoom)).max() <= TOL


def test_constant_velocity_is_left_alone_where_the_window_is_whole():
    n, radius = 25, 5
    sup = {k: translation(2.5 * k, -0.75 * k) for k in range(1, n + 1)}
    B = steady.smooth_path(sup, INFO, radius=radius, zoom=1.05)
    for k in range(1 + radius, n + 1 - radius):
        assert np.abs(corners_of(B[k]) - zoomed(1.05)).max() <= TOL
    assert np.abs(corners_of(B[1]) - zoomed(1.05)).max() > 1.0          # a cut window leans towards the frames it still has


@pytest.mark.parametrize("period,radius,sigma", [(7.0, 6, None), (4.0, 3, 2.0), (12.5, 8, 3.0)])
def test_sinusoidal_jitter_is_attenuated_by_the_windows_response(period, radius, sigma):
    n, amp = 60, np.array([3.0, -1.5])
    jitter = {k: amp * np.sin(2 * np.pi * k / period + np.array([0.0, 0.7])) for k in range(1, n + 1)}
    sup = {k: translation(4.0 * k + jitter[k][0], jitter[k][1]) for k in jitter}
    g = weights(radius, sigma)
    response = sum(g[j] * np.cos(2 * np.pi * j / period) for j in g) / sum(g.values())
    B = steady.smooth_path(sup, INFO, radius=radius, sigma=sigma, zoom=1.0)
    for k in range(1 + radius, n + 1 - radius):
        # in the frame's own pixels the steady rectangle is the frame moved back by what the smoothing takes off its jitter ...
        assert np.abs(corners_of(B[k]) - (steady.rectangle(*WH) + (response - 1.0) * jitter[k])).max() <= TOL
        # ... so in the fixed plane it follows the pan with the jitter times the window's frequency response
        plane = corners_of(np.dot(sup[k], B[k]))
        assert np.abs(plane - (steady.rectangle(*WH) + [4.0 * k, 0.0] + response * jitter[k])).max() <= TOL
    assert abs(response) < 0.6


def inside(B, tolerance=steady.INSIDE_TOLERANCE):
    ok = True
    for M in B.values():                                 # the pixel centres (0, 0) .. (w - 1, h - 1) of the picture, inside the frame's
        q, tw = steady.project(M, steady.rectangle(WH[0] - 1, WH[1] - 1))
        ok = ok and bool(np.all(tw > 0) and np.all(q >= -tolerance) and np.all(q[:, 0] <= WH[0] - 1 + tolerance) and
                         np.all(q[:, 1] <= WH[1] - 1 + tolerance))
    return ok


def jittered_pan(n=40, amp=2.0, seed=5):
    rng = np.random.default_rng(seed)
    out = {}
    for k in range(1, n + 1):
        a = np.deg2rad(rng.uniform(-0.5, 0.5))
        R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
        out[k] = np.dot(translation(3.0 * k + rng.uniform(-amp, amp), rng.uniform(-amp, amp)), R)
    return out


def test_auto_zoom_is_the_least_that_keeps_every_rectangle_inside():
    sup = jittered_pan()
    report = {}
    B = steady.smooth_path(sup, INFO, radius=6, zoom="auto", max_zoom=1.5, report=report)
    z, below = report["zoom"], report["zoom_fails_at"]
    assert 1.0 < z < 1.5 and not report["zoom_capped"] and inside(B)
    assert 1.0 <= below < z and z - below <= (1.5 - 1.0) / 2 ** steady.BISECTIONS * 1.0000001          # one bisection step less ...
    assert not inside(steady.smooth_path(sup, INFO, radius=6, zoom=below))                              # ... does not fit
    assert all(np.array_equal(B[k], M) for k, M in steady.smooth_path(sup, INFO, radius=6, zoom=z).items())
    # a static camera needs no zoom at all
    report = {}
    steady.smooth_path({k: np.eye(3) for k in range(1, 9)}, INFO, radius=3, zoom="auto", report=report)
    assert report["zoom"] == 1.0 and report["zoom_fails_at"] is None and not report["zoom_capped"]
    # and a cap that does not suffice is reported, not exceeded
    report = {}
    B = steady.smooth_path(jittered_pan(amp=6.0), INFO, radius=6, zoom="auto", max_zoom=1.02, report=report)
    assert report["zoom"] == 1.02 and report["zoom_capped"] and not inside(B)


def test_a_nan_neighbour_drops_out_without_moving_the_others_weights():
    n, radius, bad = 15, 3, 9
    shift = {k: np.array([2.0 * k + 1.5 * np.sin(1.3 * k), np.cos(0.9 * k)]) for k in range(1, n + 1)}
    sup = {k: translation(*shift[k]) for k in shift}
    sup[bad] = np.full((3, 3), np.nan)
    report = {}
    B = steady.smooth_path(sup, INFO, radius=radius, zoom=1.0, report=report)
    g = weights(radius)
    for k in range(1, n + 1):
        if k == bad:
            assert np.array_equal(B[k], np.eye(3))                      # no usable matrix: the frame comes out as it went in
            continue
        window = [j for j in range(k - radius, k + radius + 1) if 1 <= j <= n and j != bad]
        mean = sum(g[j - k] * (shift[j] - shift[k]) for j in window) / sum(g[j - k] for j in window)
        assert np.abs(corners_of(B[k]) - (steady.rectangle(*WH) + mean)).max() <= TOL
    assert report["no_matrix"] == [bad] and report["fallback"] == []
    # a neighbour that puts a corner behind the camera drops out the same way
    sup[bad] = np.array([[1, 0, 0], [0, 1, 0], [-2.0 / WH[0], 0, 1.0]])           # tw = 1 - 2 x / w: negative at the right corners
    B2 = steady.smooth_path(sup, INFO, radius=radius, zoom=1.0)
    for k in range(1, n + 1):
        if abs(k - bad) > radius:
            assert np.array_equal(B2[k], B[k])
        elif k != bad:
            assert np.abs(corners_of(B2[k]) - corners_of(B[k])).max() <= TOL


def test_a_mean_that_is_not_convex_falls_back_and_is_listed():
    # the picture of the rectangle under the neighbour's matrix is convex, its corner-wise mean with the rectangle is not
    Q = np.array([[158.0, 5.0], [61.0, -90.0], [88.0, 125.0], [137.0, 117.0]])
    N = steady.four_point(steady.rectangle(*WH), Q)
    assert np.abs(corners_of(N) - Q).max() <= 1e-9
    mean = (steady.rectangle(*WH) + Q) / 2
    a, b = np.roll(mean, -1, 0) - mean, np.roll(mean, -2, 0) - np.roll(mean, -1, 0)
    turn = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    assert (turn > 1).any() and (turn < -1).any()
    report = {}
    B = steady.smooth_path({1: np.eye(3), 2: N}, INFO, radius=1, sigma=1e6, zoom=1.1, report=report)
    assert 1 in report["fallback"] and np.array_equal(B[1], steady.zoom_matrix(1.1, *WH))
    # all four corners of the mean in one point: the system is singular
    half_turn = np.array([[-1.0, 0, WH[0]], [0, -1.0, WH[1]], [0, 0, 1.0]])
    report = {}
    B = steady.smooth_path({1: np.eye(3), 2: half_turn}, INFO, radius=1, sigma=1e6, zoom=1.0, report=report)
    assert report["fallback"] == [1, 2] and np.array_equal(B[1], np.eye(3))


def test_path_jitter_and_argument_refusals():
    i = np.arange(10.0)
    assert steady.path_jitter(np.stack([i * i, 0 * i], axis=1)) == 2.0                 # second difference of i^2
    assert steady.path_jitter(np.stack([3 * i, -i], axis=1)[:, None, :].repeat(4, axis=1)) == 0.0
    assert steady.path_jitter(np.zeros((2, 4, 2))) == 0.0
    wobble = np.stack([np.where(i % 2 == 0, 1.0, -1.0), 0 * i], axis=1)               # +1, -1, +1, ...: second difference 4
    assert steady.path_jitter(wobble) == 4.0
    sup = jittered_pan(20)
    B = steady.smooth_path(sup, INFO, radius=5, zoom=1.0)
    before = steady.path_jitter(steady.corner_trajectories(sup, INFO))
    after = steady.path_jitter(steady.corner_trajectories(sup, INFO, B))
    assert 0 < after < 0.5 * before
    for kw in (dict(radius=-1), dict(radius=1.5), dict(sigma=0.0), dict(zoom=0.0), dict(zoom="most"), dict(max_zoom=0.9),
               dict(zoom=float("nan"))):
        with pytest.raises(ValueError):
            steady.smooth_path(sup, INFO, **kw)


# ---- steady_taps ----------------------------------------------------------------------------------------------------------------------------
def test_taps_order_maps_and_what_is_left_out():
    n, fill = 9, 2
    sup = jittered_pan(n)
    B = steady.smooth_path(sup, INFO, radius=3, zoom=1.1)
    frame_size, scale = (128, 72), 0.5                                    # working size 64 x 48: K = diag(1/2, 2/3, 1)
    K, Kinv, D = np.diag([0.5, 48 / 72.0, 1.0]), np.diag([2.0, 72 / 48.0, 1.0]), np.diag([2.0, 2.0, 1.0])
    first, count = 3, 5                                                   # the chunk holds frames 3 .. 7 of 1 .. 9
    tap_frame, tap_M = steady.steady_taps(B, sup, INFO, frame_size, first, count, fill, scale)
    assert tap_frame.dtype == np.int32 and tap_frame.shape == (5, 5) and tap_M.shape == (5, 5, 9) and tap_M.dtype == np.float64
    for i in range(count):
        k = first + i
        want = [k] + [j if first <= j < first + count else None for j in (k - 1, k + 1, k - 2, k + 2)]       # k, k-1, k+1, k-2, k+2
        assert tap_frame[i].tolist() == [-1 if j is None else j - first for j in want]
        for t, j in enumerate(want):
            if j is None:
                assert np.isnan(tap_M[i, t]).all()
                continue
            M = np.linalg.multi_dot([Kinv, np.linalg.inv(sup[j]), sup[k], B[k], K, D])
            got = tap_M[i, t].reshape(3, 3)
            assert np.abs(got / got[2, 2] - M / M[2, 2]).max() <= 1e-9
            assert t > 0 or np.abs(got - np.linalg.multi_dot([Kinv, B[k], K, D])).max() <= 1e-12
    # the ends of the video: frame 1 has nothing before it, frame 9 nothing after it, even with room in the chunk
    tap_frame, _ = steady.steady_taps(B, sup, INFO, frame_size, 1, 9, fill, scale)
    assert tap_frame[0].tolist() == [0, -1, 1, -1, 2] and tap_frame[8].tolist() == [8, 7, -1, 6, -1]
    assert steady.steady_taps(B, sup, INFO, frame_size, 4, 3, 0, scale)[0].tolist() == [[0], [1], [2]]
    # a neighbour without a matrix is no tap; a frame without one has the identity and no taps but its own
    holed = dict(sup)
    holed[5] = None
    Bh = steady.smooth_path(holed, INFO, radius=3, zoom=1.1)
    tap_frame, tap_M = steady.steady_taps(Bh, holed, INFO, frame_size, 3, 5, fill, scale)
    assert tap_frame[2].tolist() == [2, -1, -1, -1, -1] and np.abs(tap_M[2, 0].reshape(3, 3) - D).max() <= 1e-15
    assert tap_frame[1].tolist() == [1, 0, -1, -1, 3] and tap_frame[3].tolist() == [3, -1, 4, 1, -1]
    # a denominator that changes its sign over the output rectangle: tw = 1 - 2 x / w between frame 6 and the others
    bent = dict(sup)
    bent[6] = np.dot(sup[6], np.array([[1, 0, 0], [0, 1, 0], [2.0 / WH[0], 0, 1.0]]))
    Bb = steady.smooth_path(sup, INFO, radius=3, zoom=1.0)
    tap_frame, _ = steady.steady_taps(Bb, bent, INFO, frame_size, 3, 5, fill, scale)
    assert tap_frame[2].tolist() == [2, 1, -1, 0, 4] and tap_frame[4].tolist() == [4, -1, -1, 2, -1]
    assert steady.tap_order(3) == [-1, 1, -2, 2, -3, 3] and steady.output_size((1280, 720), 0.25) == (320, 180)


# ---- the driver against a recording context -----------------------------------------------------------------------------------------------
def _ids(frames):
    while frames.dim() > 1:
        frames = frames[:, 0]
    return [int(v) for v in frames]


class Recorder:
    """Stands in for libevhip: notes every steady_frames call and leaves the position of each picture's own frame in the
    picture's first byte."""

    def __init__(self):
        self.calls = []

    def order_torch_after(self):
        pass

    def steady_frames(self, frames, tap_frame, tap_M, out, feather=0, background=None, tap_of=None, counts=None, size=None):
        import torch
        ids = _ids(frames)
        assert tap_M.shape == tap_frame.shape + (9,) and out.shape[0] == tap_frame.shape[0]
        self.calls.append(("steady", ids, tuple(frames.shape[1:]), size, tap_frame.tolist(), feather, tap_M[:, 0, 2].tolist()))
        out.zero_()
        out.reshape(out.shape[0], -1)[:, 0] = torch.tensor([ids[t[0]] for t in tap_frame.tolist()], dtype=torch.uint8)
        counts.zero_()
        counts[:, 1] = out[0].numel() // (1 if out.dim() == 3 else 3)

    def jpeg_encode(self, pictures, tables, subsampling):
        return [bytes([int(p.reshape(-1)[0])]) for p in pictures]


@pytest.fixture
def rec(monkeypatch):
    import torch
    fake = Recorder()
    monkeypatch.setattr(runtime, "device", lambda: torch.device("cpu"))
    monkeypatch.setattr(runtime, "get_context", lambda *a, **k: fake)
    runtime.release_staging()
    yield fake
    runtime.release_staging()


def expected_calls(total, chunk, fill):
    """[(positions of the chunk's frames, first row, the rows' taps)] from the plain statement of the loop: chunks share 2 fill
    frames; a chunk gives its frames from `fill` (the first: from 0) to n - fill, the last one the rest as well."""
    spans = F.spans(total, chunk, 2 * fill)
    offsets = [s * d for d in range(1, fill + 1) for s in (-1, 1)]
    out = []
    for i, (start, n) in enumerate(spans):
        lo = 0 if i == 0 else fill
        hi = max(lo, n - fill)
        parts = [(lo, hi)] + ([(hi, n)] if i == len(spans) - 1 else [])
        for a, b in parts:
            if b > a:
                rows = [[r] + [r + o if 0 <= r + o < n else -1 for o in offsets] for r in range(a, b)]
                out.append((list(range(start, start + n)), a, rows))
    return out


CHUNK = 6


@pytest.mark.parametrize("form", ["bgr", "gray", "planes"])
@pytest.mark.parametrize("fill", [0, 2])
@pytest.mark.parametrize("total", [5, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 3, CHUNK + 4, CHUNK + 5, 2 * CHUNK - 4, 2 * CHUNK, 3 * CHUNK - 7])
def test_driver_gives_every_frame_once_with_its_neighbours(rec, total, fill, form):
    cap, ingest = F.make(form, total)
    sup = {f: translation(f) for f in range(1, total + 1)}                 # frame f sits f pixels to the right
    report = {}
    got = [(no, p.copy()) for no, p in steady.steady_frames(cap, sup, {"w": F.W0, "h": F.H0}, radius=2, zoom=1.0, fill=fill,
                                                            feather_px=3, chunk_frames=CHUNK, ingest=ingest, report=report)]
    assert [no for no, _ in got] == list(range(1, total + 1))              # exactly once, in order -- the tail included
    assert [int(p.reshape(-1)[0]) for _, p in got] == list(range(total))
    shape = {"bgr": (F.H0, F.W0, 3), "gray": (F.H0, F.W0), "planes": (F.W0 * F.H0 * 3 // 2,)}[form]
    assert all(p.shape == ((F.H0, F.W0) if form == "gray" else (F.H0, F.W0, 3)) for _, p in got)
    want = expected_calls(total, CHUNK, fill)
    assert len(rec.calls) == len(want) and sum(len(rows) for _, _, rows in want) == total
    for call, (ids, first_row, rows) in zip(rec.calls, want):
        assert call[:6] == ("steady", ids, shape, (F.W0, F.H0) if form == "planes" else None, rows, 96)
    assert cap.i == total and sorted(report["frames"]) == list(range(1, total + 1))
    assert all(f == dict(uncovered=0.0, own=1.0, filled=0.0) for f in report["frames"].values())
    out = steady.steady_report(report)
    assert out["zoom"] == 1.0 and out["fill"] == fill and out["mean_shares"]["own"] == 1.0 and len(out["frames"]) == total
    assert out["jitter_before"] == 0.0


def test_driver_jpegs_and_a_frame_without_matrix(rec):
    total, fill = CHUNK + 4, 2
    sup = {f: translation(f) for f in range(1, total + 1)}
    sup[4] = None
    report = {}
    files = list(steady.steady_jpegs(F.make("bgr", total)[0], sup, {"w": F.W0, "h": F.H0}, radius=1, zoom=1.0, fill=fill,
                                     chunk_frames=CHUNK, ingest="bgr", report=report))
    assert files == [(k + 1, bytes([k])) for k in range(total)]
    first = rec.calls[0]
    assert first[4][3] == [3, -1, -1, -1, -1] and first[6][3] == 0.0       # frame 4: the identity, no taps but its own
    assert first[4][2] == [2, 1, -1, 0, 4] and first[4][1] == [1, 0, 2, -1, -1]
    assert steady.steady_report(report)["frames_without_matrix"] == [4]


class NoCapture:
    def __getattr__(self, name):
        raise AssertionError("the capture was touched: %s" % name)


@pytest.mark.parametrize("kw", [dict(fill=-1), dict(fill=8), dict(fill=1.5), dict(feather_px=-1), dict(feather_px=256), dict(scale=0),
                                dict(chunk_frames=4), dict(chunk_frames=0, fill=0), dict(ingest="nv12"), dict(radius=-1),
                                dict(zoom="least"), dict(sigma=-1.0), dict(max_zoom=0.5)])
def test_driver_refuses_before_the_capture_is_touched(rec, kw):
    sup = {f: translation(f) for f in range(1, 4)}
    with pytest.raises(ValueError):
        next(steady.steady_frames(NoCapture(), sup, {"w": F.W0, "h": F.H0}, **kw))
    with pytest.raises(ValueError):
        steady.steady_jpegs(NoCapture(), sup, {"w": F.W0, "h": F.H0}, **kw)
    with pytest.raises(ValueError):
        steady.steady_jpegs(NoCapture(), sup, {"w": F.W0, "h": F.H0}, quality=0)
    assert rec.calls == []


def test_a_video_too_short_for_its_fill_is_refused(rec):
    """Chunks that share 2 * fill frames have at least 2 * fill + 1: a shorter video never fills one, and says so."""
    sup = {f: translation(f) for f in range(1, 5)}
    with pytest.raises(ValueError, match="4 frames"):
        list(steady.steady_frames(F.make("bgr", 4)[0], sup, {"w": F.W0, "h": F.H0}, fill=2, chunk_frames=CHUNK, ingest="bgr"))
    assert rec.calls == []


def test_command_line_refusals(capsys):
    from evenvizion_amd import stabilize
    for flag, extra in (("trail", ["--trail", "1"]), ("comparison", ["--comparison", "1"]), ("plate", ["--plate", "1"]),
                        ("surface", ["--surface", "cylinder"]), ("blend", ["--mode", "mosaic", "--blend", "seam"])):
        with pytest.raises(SystemExit) as e:
            stabilize.main(["--steady", "1", "--path_to_video", "/nonexistent/video.mp4"] + extra)
        assert e.value.code == 2 and ("not with --%s" % flag) in capsys.readouterr().err
    for extra in (["--steady_fill", "2"], ["--steady", "1", "--steady_fill", "8"], ["--steady", "1", "--steady_zoom", "wide"],
                  ["--steady", "1", "--steady_feather", "300"], ["--steady", "1", "--steady_radius", "-2"]):
        with pytest.raises(SystemExit) as e:
            stabilize.main(["--path_to_video", "/nonexistent/video.mp4"] + extra)
        assert e.value.code == 2 and "steady" in capsys.readouterr().err
