"""Crafted frame pairs with a known true map, for the tracker (evh_track_points) and its restatement (track_checks.py).

    noise_field(seed, w, h, sigma)              -> f64[h,w]: Gaussian-filtered white noise on a torus (filtered in the spectrum)
    shift_pair(seed, dx, dy, ...)               -> (prev, cur, M_true): cur(a) = prev(a + (dx, dy)), the shift made in the spectrum
    projective_pair(seed, ...)                  -> (prev, cur, M_true, M_guess)
    grid_points(w, h, nx, ny, margin)           -> f32[nx*ny,2]
    capture_frames(seed, n, step)               -> BGR frames of the low-contrast family panning by `step` per frame, and the true maps

M_true maps pixels of the current frame to pixels of the previous frame, as d_M does."""
import numpy as np

LOW = dict(sigma=2.0, lo=100, hi=120, w=128, h=96)          # cannot hold a FAST corner: the gray values span 20 levels
FULL = dict(sigma=4.0, lo=0, hi=255, w=128, h=96)
LOW_SHIFTS = [(11, 3.25, -2.5), (12, -1.75, 0.5), (13, 0.25, 2.25)]       # (seed, dx, dy)
FULL_SHIFTS = [(21, 9.5, 6.25), (22, -9.5, 6.25)]
PAD = 32                                                   # the torus is larger than the frame by this much on every side


def noise_field(seed, w, h, sigma):
    rng = np.random.default_rng(seed)
    spectrum = np.fft.fft2(rng.standard_normal((h, w)))
    fy, fx = np.fft.fftfreq(h)[:, None], np.fft.fftfreq(w)[None, :]
    return spectrum * np.exp(-2.0 * (np.pi * sigma) ** 2 * (fx * fx + fy * fy))       # still in the spectrum


def _shifted(spectrum, dx, dy):
    """The field moved by (dx, dy): out(x) = field(x - d), exact for the band the Gaussian leaves."""
    h, w = spectrum.shape
    fy, fx = np.fft.fftfreq(h)[:, None], np.fft.fftfreq(w)[None, :]
    return np.real(np.fft.ifft2(spectrum * np.exp(-2j * np.pi * (fx * dx + fy * dy))))


def _to_gray(field, lo, hi, ref):
    a, b = ref.min(), ref.max()
    return np.clip(np.rint(lo + (field - a) * ((hi - lo) / (b - a))), 0, 255).astype(np.uint8)


def shift_pair(seed, dx, dy, sigma, lo, hi, w, h):
    """cur(a) = prev(a + (dx, dy)): a point a of the current frame is found at a + (dx, dy) in the previous one."""
    S = noise_field(seed, w + 2 * PAD, h + 2 * PAD, sigma)
    cur_f, prev_f = _shifted(S, 0.0, 0.0), _shifted(S, dx, dy)
    cut = (slice(PAD, PAD + h), slice(PAD, PAD + w))
    M = np.array([[1, 0, dx], [0, 1, dy], [0, 0, 1]], np.float64)
    return _to_gray(prev_f[cut], lo, hi, cur_f), _to_gray(cur_f[cut], lo, hi, cur_f), M


def _bilinear(field, x, y):
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    fx, fy = x - x0, y - y0
    return (field[y0, x0] * (1 - fx) * (1 - fy) + field[y0, x0 + 1] * fx * (1 - fy) + field[y0 + 1, x0] * (1 - fx) * fy
            + field[y0 + 1, x0 + 1] * fx * fy)


def projective_pair(seed, sigma=4.0, lo=0, hi=255, w=128, h=96):
    """prev is the field itself, cur(a) = field(M_true a) by bilinear taps on the smooth field (sigma 4: the taps are within a
    hundredth of a gray level of the field).  M_guess is M_true with its translation off by (2.5, -1.5) and no perspective."""
    S = noise_field(seed, w + 2 * PAD, h + 2 * PAD, sigma)
    field = _shifted(S, 0.0, 0.0)
    c, s = 1.02 * np.cos(np.deg2rad(2.0)), 1.02 * np.sin(np.deg2rad(2.0))
    M = np.array([[c, -s, 3.0], [s, c, -4.0], [1e-4, -5e-5, 1.0]], np.float64)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    tw = M[2, 0] * xs + M[2, 1] * ys + M[2, 2]
    bx, by = (M[0, 0] * xs + M[0, 1] * ys + M[0, 2]) / tw, (M[1, 0] * xs + M[1, 1] * ys + M[1, 2]) / tw
    cur = _bilinear(field, bx + PAD, by + PAD)
    guess = np.array([[c, -s, 3.0 + 2.5], [s, c, -4.0 - 1.5], [0, 0, 1.0]], np.float64)
    return _to_gray(field[PAD:PAD + h, PAD:PAD + w], lo, hi, field), _to_gray(cur, lo, hi, field), M, guess


def grid_points(w, h, nx=7, ny=5, margin=16):
    xs, ys = np.linspace(margin, w - 1 - margin, nx), np.linspace(margin, h - 1 - margin, ny)
    return np.array([(np.rint(x * 4) / 4, np.rint(y * 4) / 4) for y in ys for x in xs], np.float32)


def apply(M, pts):
    p = np.asarray(pts, np.float64)
    q = np.concatenate([p, np.ones((len(p), 1))], 1) @ np.asarray(M, np.float64).reshape(3, 3).T
    return q[:, :2] / q[:, 2:]


def capture_frames(seed, n, step=(1.75, -0.5), sigma=2.0, lo=100, hi=120, w=400, h=224, textured=()):
    """n BGR frames of one field panning by `step` per frame -> (frames u8[n,h,w,3], M_true per pair).  Frames whose index is in
    `textured` use the field at full contrast with blocks of hard edges laid over it (FAST finds corners there)."""
    S = noise_field(seed, w + 2 * PAD, h + 2 * PAD, sigma)
    ref = _shifted(S, 0.0, 0.0)
    rng = np.random.default_rng(seed + 1)
    blocks = rng.integers(0, 256, ((h + 2 * PAD) // 8 + 1, (w + 2 * PAD) // 8 + 1)).astype(np.float64)
    frames = []
    for k in range(n):
        f = _shifted(S, -k * step[0], -k * step[1])
        if k in textured:
            # the blocks pan with the field, by whole pixels
            ox, oy = int(round(k * step[0])), int(round(k * step[1]))
            ys, xs = np.mgrid[0:h, 0:w]
            g = blocks[(ys + PAD + oy) // 8, (xs + PAD + ox) // 8]
            gray = np.clip(np.rint(g), 0, 255).astype(np.uint8)
        else:
            gray = _to_gray(f[PAD:PAD + h, PAD:PAD + w], lo, hi, ref)
        frames.append(np.repeat(gray[..., None], 3, 2))
    M = np.array([[1, 0, step[0]], [0, 1, step[1]], [0, 0, 1]], np.float64)        # frame k shows the field at x + k * step
    return np.stack(frames), M
