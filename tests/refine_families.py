"""Crafted pairs with a known true map, for the direct-alignment tests (host and GPU).

A scene is a sum of six sinusoids with periods of 18 to 30 pixels (smooth enough for central differences over two pixels,
textured in every direction) plus uniform noise of +-2 per frame.  cur samples the scene at its own pixels, prev at the pixels
the true map M_true sends them from: prev(M_true . x) = cur(x) up to the noise and the rounding to bytes, so M_true minimises
the residual.  The start is M_true with the images of the four corners pushed by 1.0 .. 1.5 pixels in random directions.

    pair(seed, w, h, channels)      -> (prev, cur, M_true, M_start)
    CASES                           -> the (seed, w, h, channels) of the convergence tests
    shift_pair(seed, dx, dy)        -> (prev, cur, M_true) of 96 x 64 under a pure shift, to be started from the identity
    SHIFTS                          -> the (seed, dx, dy) of the pyramid tests
"""
import numpy as np

SIZES = ((37, 29), (64, 48), (96, 64))
# Seeds: on frames this small the minimiser of the noisy residual itself lies up to 0.49 px from the true map (37 x 29, seed 128 of
# the 40 scanned per size: the perspective terms are barely constrained), so the seeds kept are those at which the restatement
# ends within 0.125 px, half the bar of the tests (worst of the twelve: 0.083 px, seed 122).  Odd seeds have three channels.
CASES = [(seed, w, h, 3 if seed % 2 else 1) for (w, h), seeds in zip(SIZES, ((111, 122, 126, 137), (141, 142, 145, 152),
                                                                              (183, 187, 196, 206))) for seed in seeds]
SHIFTS = [(1, -4.0, 4.5), (3, 4.5, -6.0), (5, 5.0, 3.0), (8, -6.0, -4.0)]


def homography_from_points(src, dst):
    """the 3x3 with [2][2] = 1 that takes four points to four points"""
    A, b = [], []
    for (x, y), (u, v) in zip(src, dst):
        A.append([x, y, 1, 0, 0, 0, -u * x, -u * y]); b.append(u)
        A.append([0, 0, 0, x, y, 1, -v * x, -v * y]); b.append(v)
    return np.append(np.linalg.solve(np.array(A, np.float64), np.array(b, np.float64)), 1.0).reshape(3, 3)


def apply(M, pts):
    p = np.dot(M, np.vstack([np.asarray(pts, np.float64).T, np.ones(len(pts))]))
    return (p[:2] / p[2]).T


def corners(w, h):
    return np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]], np.float64)


def scene(rng, channels):
    """-> f(u, v): float64 [..., channels] in about 40 .. 215"""
    waves = []
    for _ in range(6):
        period, angle = rng.uniform(18, 30), rng.uniform(0, np.pi)
        k = 2 * np.pi / period
        waves.append((k * np.cos(angle), k * np.sin(angle), rng.uniform(0, 2 * np.pi, channels), rng.uniform(14, 21, channels)))

    def f(u, v):
        out = np.full(u.shape + (channels,), 128.0)
        for ku, kv, phase, amp in waves:
            out += amp * np.sin((ku * u + kv * v)[..., None] + phase)
        return out
    return f


def render(f, rng, Minv, w, h, channels):
    """the scene at Minv . (pixel), with the noise, as bytes"""
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    den = Minv[2, 0] * x + Minv[2, 1] * y + Minv[2, 2]
    u = (Minv[0, 0] * x + Minv[0, 1] * y + Minv[0, 2]) / den
    v = (Minv[1, 0] * x + Minv[1, 1] * y + Minv[1, 2]) / den
    img = np.clip(np.rint(f(u, v) + rng.integers(-2, 3, (h, w, channels))), 0, 255).astype(np.uint8)
    return img[..., 0] if channels == 1 else img


def pair(seed, w, h, channels=1):
    rng = np.random.default_rng(seed)
    f = scene(rng, channels)
    c = corners(w, h)
    M_true = homography_from_points(c, c + rng.uniform(-3, 3, (4, 2)))
    angle, push = rng.uniform(0, 2 * np.pi, 4), rng.uniform(1.0, 1.5, 4)
    M_start = homography_from_points(c, apply(M_true, c) + (push * np.array([np.cos(angle), np.sin(angle)])).T)
    cur = render(f, rng, np.eye(3), w, h, channels)
    prev = render(f, rng, np.linalg.inv(M_true), w, h, channels)
    return prev, cur, M_true, M_start


def shift_pair(seed, dx, dy, w=96, h=64, channels=1):
    rng = np.random.default_rng(seed)
    f = scene(rng, channels)
    M_true = np.array([[1, 0, dx], [0, 1, dy], [0, 0, 1]], np.float64)
    return render(f, rng, np.linalg.inv(M_true), w, h, channels), render(f, rng, np.eye(3), w, h, channels), M_true
