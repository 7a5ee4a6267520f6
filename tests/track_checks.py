"""numpy restatement of evh_track_points and evh_track_seeds (include/evhip.h): plain integers (int64 arrays, Python ints) and one
IEEE float64 operation at a time, in the order the header states, so the device must agree with it for equality.

    gray_frame(frame)                                         -> u8[h,w], cvtColor's weights on BGR, the byte on gray frames
    pyramid(gray, levels)                                     -> the levels that exist, level l = 2x2 means of level l-1
    down(P), up(P)                                            -> a 1/32-pixel position one level coarser / finer
    sample(img, X, Y)                                         -> the un-shifted bilinear sum at 1/32-pixel positions (arrays)
    first_guess(A0, M)                                        -> B0 of a point under a guess matrix
    track_run(tmpl_pyr, search_pyr, A0, B0, radius, iters, min_eig)
                                                              -> (flag, B, err, steps): one direction of the tracker
    track_points(frames, pts, npts, mats, ...)                -> (rows, counts, flags, err) as the entry writes them
    track_seeds(frames, radius, cell, border, min_eig, pt_cap) -> (pts, npts)
"""
import numpy as np

TRACKED, BAD_POINT, NO_WINDOW, LEFT_FRAME, FLAT, HIGH_ERROR, FB_FAILED = range(7)
FLAGS = ("tracked", "bad_point", "no_window", "left_frame", "flat", "high_error", "fb_failed")
NO_ERR = 0xFFFFFFFF           # d_err of a point that did not reach the level-0 window
GUESS_MAX = 1 << 24           # a guess further out than this many 1/32 pixels is taken for no guess
MAX_LEVELS, MAX_RADIUS, MAX_ITERS, MAX_SEED_RADIUS = 4, 10, 64, 3


def gray_frame(frame):
    f = np.asarray(frame)
    if f.ndim == 2:
        return f.astype(np.uint8)
    f = f.astype(np.int64)
    return ((f[..., 0] * 1868 + f[..., 1] * 9617 + f[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def pyramid(gray, levels):
    """Level 0 always; level l only with both sides >= 2 (an odd last column or row of level l-1 is dropped)."""
    out = [np.asarray(gray, np.uint8)]
    for _ in range(1, levels):
        g = out[-1].astype(np.int64)
        h, w = g.shape[0] >> 1, g.shape[1] >> 1
        if w < 2 or h < 2:
            break
        g = g[:2 * h, :2 * w]
        out.append(((g[0::2, 0::2] + g[0::2, 1::2] + g[1::2, 0::2] + g[1::2, 1::2] + 2) >> 2).astype(np.uint8))
    return out


def down(P):
    return (int(P) - 16) >> 1            # Python's >> on a negative int is the arithmetic shift


def up(P):
    return 2 * int(P) + 16


def sample(img, X, Y):
    """S(img, X, Y) for int64 arrays of positions in 1/32 pixels, all defined (the caller has checked the window): a tap of weight 0
    is not read -- its index is only clamped to keep numpy's gather inside the array, and its product is 0."""
    h, w = img.shape
    x, fx, y, fy = X >> 5, X & 31, Y >> 5, Y & 31
    assert (x >= 0).all() and (y >= 0).all() and ((x < w - 1) | ((x == w - 1) & (fx == 0))).all() \
        and ((y < h - 1) | ((y == h - 1) & (fy == 0))).all()
    x1, y1 = np.minimum(x + 1, w - 1), np.minimum(y + 1, h - 1)
    s = img.astype(np.int64)
    return s[y, x] * ((32 - fx) * (32 - fy)) + s[y, x1] * (fx * (32 - fy)) + s[y1, x] * ((32 - fx) * fy) + s[y1, x1] * (fx * fy)


def inside(img, X, Y, reach):
    """Is the (2*reach+1)^2 window of whole-pixel offsets around (X, Y) defined on img?"""
    h, w = img.shape
    return X - 32 * reach >= 0 and X + 32 * reach <= 32 * (w - 1) and Y - 32 * reach >= 0 and Y + 32 * reach <= 32 * (h - 1)


def start_point(x, y, w, h):
    """-> A0 or None (BAD_POINT).  x, y: float32 values as the entry reads them."""
    x, y = np.float64(np.float32(x)), np.float64(np.float32(y))
    if not (np.isfinite(x) and np.isfinite(y)):
        return None
    ax, ay = np.rint(32.0 * x), np.rint(32.0 * y)
    if not (0 <= ax <= 32 * (w - 1) and 0 <= ay <= 32 * (h - 1)):
        return None
    return int(ax), int(ay)


def first_guess(A0, M):
    """evh_warp_fixed_plane's (U, V) for A = M (inverse_map) at (X, Y) = A0 / 32; A0 itself without a matrix, with a guess that is
    not finite, or with one beyond GUESS_MAX."""
    if M is None:
        return A0
    a = np.asarray(M, np.float64).reshape(9)
    with np.errstate(all="ignore"):
        X, Y = np.float64(A0[0]) / 32.0, np.float64(A0[1]) / 32.0
        tx = (a[0] * X + a[1] * Y) + a[2]
        ty = (a[3] * X + a[4] * Y) + a[5]
        tw = (a[6] * X + a[7] * Y) + a[8]
        U, V = np.rint(tx / tw * 32.0), np.rint(ty / tw * 32.0)
    if not (abs(U) <= GUESS_MAX and abs(V) <= GUESS_MAX):          # NaN and +-inf fail
        return A0
    return int(U), int(V)


def _offsets(reach):
    j, i = np.meshgrid(np.arange(-reach, reach + 1, dtype=np.int64), np.arange(-reach, reach + 1, dtype=np.int64), indexing="ij")
    return i, j            # [row = j, column = i]


def min_eigenvalue(Gxx, Gxy, Gyy):
    gxx, gxy, gyy = np.float64(Gxx), np.float64(Gxy), np.float64(Gyy)
    dd = gxx - gyy
    return ((gxx + gyy) - np.sqrt(dd * dd + 4.0 * (gxy * gxy))) * 0.5


def level_run(tmpl, search, A, B, r, iters, min_eig=None):
    """One level.  -> (flag, B, err, steps); flag != TRACKED: B is the B handed in.  min_eig: None above level 0."""
    Ax, Ay = A
    B_in = (int(B[0]), int(B[1]))
    if not inside(tmpl, Ax, Ay, r + 1):
        return NO_WINDOW, B_in, NO_ERR, 0
    i, j = _offsets(r + 1)
    T = sample(tmpl, Ax + 32 * i, Ay + 32 * j)                       # [2r+3, 2r+3]
    gx = (T[1:-1, 2:] - T[1:-1, :-2]).reshape(-1)
    gy = (T[2:, 1:-1] - T[:-2, 1:-1]).reshape(-1)
    T = T[1:-1, 1:-1].reshape(-1)
    n = (2 * r + 1) ** 2
    Gxx, Gxy, Gyy = int((gx * gx).sum()), int((gx * gy).sum()), int((gy * gy).sum())
    assert Gxx < 2 ** 48 and Gyy < 2 ** 48
    gxx, gxy, gyy = np.float64(Gxx), np.float64(Gxy), np.float64(Gyy)
    det = gxx * gyy - gxy * gxy
    if not det > 0:
        return FLAT, B_in, NO_ERR, 0
    if min_eig is not None and min_eigenvalue(Gxx, Gxy, Gyy) < (np.float64(min_eig) * np.float64(n)) * 4194304.0:
        return FLAT, B_in, NO_ERR, 0
    i, j = _offsets(r)
    i, j = i.reshape(-1), j.reshape(-1)
    Bx, By = B_in
    steps = 0
    while True:
        if not inside(search, Bx, By, r):
            return LEFT_FRAME, B_in, NO_ERR, steps
        d = sample(search, Bx + 32 * i, By + 32 * j) - T
        err = int(np.abs(d).sum())
        if steps == iters:
            break
        bx, by = np.float64(int((d * gx).sum())), np.float64(int((d * gy).sum()))
        dx = (gyy * bx - gxy * by) / det
        dy = (gxx * by - gxy * bx) / det
        sx = int(min(max(np.rint(-64.0 * dx), -32.0 * r), 32.0 * r))
        sy = int(min(max(np.rint(-64.0 * dy), -32.0 * r), 32.0 * r))
        if sx == 0 and sy == 0:
            break
        Bx, By, steps = Bx + sx, By + sy, steps + 1
    return TRACKED, (Bx, By), err, steps


def track_run(tmpl_pyr, search_pyr, A0, B0, radius, iters, min_eig):
    """The template around A0 in tmpl_pyr followed into search_pyr from the guess B0 -> (flag, B, err, steps over all levels)."""
    top = len(tmpl_pyr) - 1
    A = [(int(A0[0]), int(A0[1]))]
    for _ in range(top):
        A.append((down(A[-1][0]), down(A[-1][1])))
    B = (int(B0[0]), int(B0[1]))
    for _ in range(top):
        B = (down(B[0]), down(B[1]))
    total = 0
    for l in range(top, 0, -1):
        _, B, _, steps = level_run(tmpl_pyr[l], search_pyr[l], A[l], B, radius, iters)      # a level that fails is skipped
        total += steps
        B = (up(B[0]), up(B[1]))
    flag, B, err, steps = level_run(tmpl_pyr[0], search_pyr[0], A[0], B, radius, iters, min_eig)
    return flag, B, err, total + steps


def track_point(cur_pyr, prev_pyr, xy, M, radius, iters, min_eig, fb_max32, max_err):
    """-> (flag, A0 or None, B, err)"""
    h, w = cur_pyr[0].shape
    A0 = start_point(xy[0], xy[1], w, h)
    if A0 is None:
        return BAD_POINT, None, None, NO_ERR
    flag, B, err, _ = track_run(cur_pyr, prev_pyr, A0, first_guess(A0, M), radius, iters, min_eig)
    if flag != TRACKED:
        return flag, A0, None, NO_ERR
    if max_err >= 0 and err > max_err * (2 * radius + 1) ** 2 * 1024:
        return HIGH_ERROR, A0, B, err
    if fb_max32 >= 0:
        back, A1, _, _ = track_run(prev_pyr, cur_pyr, B, A0, radius, iters, min_eig)
        if back != TRACKED or max(abs(A1[0] - A0[0]), abs(A1[1] - A0[1])) > fb_max32:
            return FB_FAILED, A0, B, err
    return TRACKED, A0, B, err


def track_points(frames, pts, npts, mats=None, frame_step=1, levels=3, radius=7, iters=20, min_eig=0.0, fb_max32=-1, max_err=-1,
                 row_cap=None, fill=0xFF):
    """frames u8[n,h,w(,3)], pts f32[npairs,pt_cap,2], npts i32[npairs], mats f64[npairs,9] or None -> (rows f32[npairs,row_cap,4],
    counts i32[npairs], flags u8[npairs,pt_cap], err u32[npairs,pt_cap]); what the entry leaves alone holds `fill` bytes."""
    pts = np.asarray(pts, np.float32)
    npairs, pt_cap = pts.shape[:2]
    row_cap = pt_cap if row_cap is None else row_cap
    rows = np.full(npairs * row_cap * 16, fill, np.uint8).view(np.float32).reshape(npairs, row_cap, 4)
    counts = np.zeros(npairs, np.int32)
    flags = np.full((npairs, pt_cap), fill, np.uint8)
    err = np.full(npairs * pt_cap * 4, fill, np.uint8).view(np.uint32).reshape(npairs, pt_cap)
    pyrs = {}
    for p in range(npairs):
        for f in (p * frame_step, p * frame_step + 1):
            if f not in pyrs:
                pyrs[f] = pyramid(gray_frame(frames[f]), levels)
        prev, cur = pyrs[p * frame_step], pyrs[p * frame_step + 1]
        k = 0
        for q in range(min(max(int(npts[p]), 0), pt_cap)):
            M = None if mats is None else np.asarray(mats, np.float64).reshape(-1, 9)[p]
            flag, A0, B, e = track_point(cur, prev, pts[p, q], M, radius, iters, min_eig, fb_max32, max_err)
            flags[p, q], err[p, q] = flag, e
            if flag == TRACKED:
                rows[p, k] = (A0[0] / 32.0, A0[1] / 32.0, B[0] / 32.0, B[1] / 32.0)
                k += 1
        counts[p] = k
    return rows, counts, flags, err


def seed_field(gray, radius):
    """lambda f64[h,w] of the (2*radius+1)^2 window around every pixel that has one (NaN elsewhere), from exact integer sums."""
    g = np.asarray(gray).astype(np.int64)
    h, w = g.shape
    lam = np.full((h, w), np.nan)
    m = radius + 1
    if h <= 2 * m or w <= 2 * m:
        return lam
    gx, gy = np.zeros_like(g), np.zeros_like(g)
    gx[:, 1:-1] = g[:, 2:] - g[:, :-2]
    gy[1:-1, :] = g[2:, :] - g[:-2, :]
    k = 2 * radius + 1

    def box(a):
        c = np.zeros((h + 1, w + 1), np.int64)
        c[1:, 1:] = a.cumsum(0).cumsum(1)
        return c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]            # [h-k+1, w-k+1]: windows by their top-left pixel

    Gxx, Gxy, Gyy = box(gx * gx), box(gx * gy), box(gy * gy)
    full = min_eigenvalue(Gxx, Gxy, Gyy)
    lam[m:h - m, m:w - m] = full[1:-1, 1:-1]                               # windows whose gradients are all defined
    return lam


def track_seeds(frames, radius=2, cell=16, border=8, min_eig=0.0, pt_cap=1024, fill=0xFF):
    """-> (pts f32[nframes,pt_cap,2], npts i32[nframes]); slots past the seeds hold `fill` bytes."""
    frames = np.asarray(frames)
    nframes = len(frames)
    pts = np.full(nframes * pt_cap * 8, fill, np.uint8).view(np.float32).reshape(nframes, pt_cap, 2)
    npts = np.zeros(nframes, np.int32)
    n = (2 * radius + 1) ** 2
    bar = (np.float64(min_eig) * np.float64(n)) * 4.0
    for f in range(nframes):
        lam = seed_field(gray_frame(frames[f]), radius)
        h, w = lam.shape
        k = 0
        for y0 in range(border, h - border, cell):
            for x0 in range(border, w - border, cell):
                part = lam[y0:min(y0 + cell, h - border), x0:min(x0 + cell, w - border)]
                at = int(np.argmax(part))                                  # the first of equals in raster order
                best = part.reshape(-1)[at]
                if best >= bar:
                    if k < pt_cap:
                        pts[f, k] = (x0 + at % part.shape[1], y0 + at // part.shape[1])
                    k += 1
        npts[f] = k
    return pts, npts
