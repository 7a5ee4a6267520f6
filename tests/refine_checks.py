"""numpy restatement of evh_pair_refine (include/evhip.h) on top of warp_checks / residual_checks: direct alignment of a pair,
inverse-compositional Gauss-Newton with Levenberg damping on the photometric residual.  Where the header is unclear, this file
is the definition.  The cost is evh_pair_residual's integers; the normal sums exist twice, as exact Python integers (the
yardstick of the device's rounding) and as float64 sums (what the loop here runs on: the device's sums differ from them by
rounding only, so its accepted steps may differ in the last bits, not in kind).

    cost(prev, cur, M)                       -> (covered, ssd), Python ints: residual_checks.residual's COVERED and SSD
    better(a, b)                             -> cost a is better than cost b: ssd_a * covered_b < ssd_b * covered_a, exactly
    jacobian(prev, cur, M, clip)             -> (J int64[n,8], r int64[n]) over the covered, interior pixels with |r| <= clip
    normal_exact(J, r)                       -> (sums: 45 Python ints, abs_sums: 45 Python ints, the sums of the absolute terms)
    normal_float(J, r)                       -> f64[45]: each product one rounded double multiplication, numpy's sum
    solve_step(N, lam)                       -> (delta f64[8], Ah f64[8,8]) or (None, reason)
    try_matrix(M, delta, w, h)               -> M_try f64[3,3] (not checked for finiteness)
    delta_of(M, M_try, w, h)                 -> the delta a trial was made from, in exact rational arithmetic
    refine(prev, cur, M_in, iters, clip)     -> (M_out f64[3,3], info dict)
    refine_levels(prev, cur, M_in, levels, iters, clip) -> the same, coarse to fine on block-mean pyramids
    level_map(w, h, lw, lh)                  -> S f64[3,3]: pixel of the level -> pixel of the full frame
"""
from fractions import Fraction

import numpy as np

import residual_checks as R
import warp_checks as W

MIN_PIXELS = 64
REFINED, UNCHANGED, NOTHING_COVERED, TOO_FEW, DEGENERATE = range(5)
PAIRS = [(i, j) for i in range(8) for j in range(i, 8)]       # sums 0..35: the upper triangle of J'J, row by row


def cost(prev, cur, M):
    s = R.residual(prev, cur, M)[0]
    return s[R.COVERED], s[R.SSD]


def better(a, b):
    """a, b: (covered, ssd) in Python ints"""
    return a[1] * b[0] < b[1] * a[0]


def jacobian(prev, cur, M, clip=255):
    prev, cur = np.asarray(prev), np.asarray(cur)
    h, w = cur.shape[:2]
    val, cov = W.warp_frame(prev, M, w, h, (0, 0), inverse_map=True)
    g = R.gray_of(cur).astype(np.int64)
    r = g - R.gray_of(val).astype(np.int64)
    use = cov & (np.abs(r) <= int(clip))
    use[[0, -1], :] = False
    use[:, [0, -1]] = False
    ys, xs = np.nonzero(use)                                   # row-major: ascending y, then x
    if h < 3 or w < 3:
        ys, xs = ys[:0], xs[:0]
    gx = g[ys, np.minimum(xs + 1, w - 1)] - g[ys, np.maximum(xs - 1, 0)]
    gy = g[np.minimum(ys + 1, h - 1), xs] - g[np.maximum(ys - 1, 0), xs]
    X, Y = 2 * xs - (w - 1), 2 * ys - (h - 1)
    s = gx * X + gy * Y
    J = np.stack([gx * X, gx * Y, gx, gy * X, gy * Y, gy, -X * s, -Y * s], axis=1).astype(np.int64).reshape(-1, 8)
    assert w > 4096 or h > 4096 or J.size == 0 or np.abs(J).max() < 2 ** 53
    return J, r[ys, xs]


def normal_exact(J, r):
    Jo, ro = J.astype(object), r.astype(object)
    cols = [Jo[:, i] * Jo[:, j] for i, j in PAIRS] + [Jo[:, i] * ro for i in range(8)]
    sums = [int(sum(c.tolist())) for c in cols] + [len(r)]
    abs_sums = [int(sum(abs(v) for v in c.tolist())) for c in cols] + [len(r)]
    return sums, abs_sums


def normal_float(J, r):
    Jf, rf = J.astype(np.float64), r.astype(np.float64)
    out = [np.sum(Jf[:, i] * Jf[:, j]) for i, j in PAIRS] + [np.sum(Jf[:, i] * rf) for i in range(8)] + [float(len(r))]
    return np.array(out, np.float64)


def scaled_system(N, lam):
    """-> (Ah, bh, d) or a reason"""
    N = np.asarray(N, np.float64)
    if N[44] < MIN_PIXELS:
        return TOO_FEW
    A = np.zeros((8, 8))
    for k, (i, j) in enumerate(PAIRS):
        A[i, j] = A[j, i] = N[k]
    d = np.sqrt(np.diag(A))
    if not (d > 0).all():
        return DEGENERATE
    return A / np.outer(d, d) + lam * np.eye(8), N[36:44] / d, d


def ldl_solve(A, b):
    """8x8 LDL' in double, as the device runs it"""
    n = len(b)
    L, D = np.eye(n), np.zeros(n)
    for j in range(n):
        D[j] = A[j, j] - np.sum(L[j, :j] * L[j, :j] * D[:j])
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - np.sum(L[i, :j] * L[j, :j] * D[:j])) / D[j]
    y = np.array(b, np.float64)
    for i in range(n):
        y[i] -= np.sum(L[i, :i] * y[:i])
    y /= D
    for i in range(n - 1, -1, -1):
        y[i] -= np.sum(L[i + 1:, i] * y[i + 1:])
    return y


def solve_step(N, lam):
    sysm = scaled_system(N, lam)
    if isinstance(sysm, int):
        return None, sysm
    Ah, bh, d = sysm
    with np.errstate(all="ignore"):
        delta = -4.0 * ldl_solve(Ah, bh) / d
    if not np.isfinite(delta).all():
        return None, DEGENERATE
    return delta, Ah


def centre(w, h):
    return np.array([[2, 0, -(w - 1)], [0, 2, -(h - 1)], [0, 0, 1]], np.float64)


def try_matrix(M, delta, w, h):
    D = np.asarray(delta, np.float64)
    P = np.array([[1 + D[0], D[1], D[2]], [D[3], 1 + D[4], D[5]], [D[6], D[7], 1]])
    Cinv = np.array([[.5, 0, (w - 1) / 2], [0, .5, (h - 1) / 2], [0, 0, 1]])
    Q = np.dot(np.dot(Cinv, P), centre(w, h))
    with np.errstate(all="ignore"):
        T = np.dot(np.asarray(M, np.float64).reshape(3, 3), W.adjugate(Q).reshape(3, 3))
        return T / T[2, 2]


def _frac(M):
    return [[Fraction(float(v)) for v in row] for row in np.asarray(M, np.float64).reshape(3, 3)]


def _mul(A, B):
    return [[sum(A[i][k] * B[k][j] for k in range(3)) for j in range(3)] for i in range(3)]


def _inv(A):
    (a, b, c), (d, e, f), (g, h, i) = A
    adj = [[e * i - f * h, c * h - b * i, b * f - c * e], [f * g - d * i, a * i - c * g, c * d - a * f], [d * h - e * g, b * g - a * h, a * e - b * d]]
    det = a * adj[0][0] + b * adj[1][0] + c * adj[2][0]
    return [[v / det for v in row] for row in adj]


def delta_of(M, M_try, w, h):
    """M_try ~ M Q^-1, Q = C^-1 P C  =>  P ~ C M_try^-1 M C^-1, normalised by [2][2]; exact in rationals, rounded once."""
    C = _frac(centre(w, h))
    P = _mul(_mul(C, _mul(_inv(_frac(M_try)), _frac(M))), _inv(C))
    P = [[v / P[2][2] for v in row] for row in P]
    return np.array([float(P[0][0] - 1), float(P[0][1]), float(P[0][2]), float(P[1][0]), float(P[1][1] - 1), float(P[1][2]),
                     float(P[2][0]), float(P[2][1])])


def refine(prev, cur, M_in, iters=8, clip=255):
    """-> (M_out, info).  M_out IS M_in's array (same bytes) unless a step was accepted."""
    M_in = np.asarray(M_in, np.float64).reshape(3, 3)
    h, w = np.asarray(cur).shape[:2]
    c_in = cost(prev, cur, M_in)
    info = dict(status=UNCHANGED, evals=1, accepted=0, covered_in=c_in[0], ssd_in=c_in[1], covered_out=c_in[0], ssd_out=c_in[1], n_in=0)
    if c_in[0] == 0:
        info["status"] = NOTHING_COVERED
        return M_in, info
    M, c, N, lam = M_in, c_in, normal_float(*jacobian(prev, cur, M_in, clip)), 1e-3
    info["n_in"] = int(N[44])
    for _ in range(int(iters)):
        delta, why = solve_step(N, lam)
        T = try_matrix(M, delta, w, h) if delta is not None else None
        if T is None or not np.isfinite(T).all():
            if not info["accepted"]:
                info["status"] = why if delta is None else DEGENERATE
            break
        c_try = cost(prev, cur, T)
        info["evals"] += 1
        if c_try[0] > 0 and 10 * c_try[0] >= 9 * c_in[0] and better(c_try, c):
            M, c, N, lam = T, c_try, normal_float(*jacobian(prev, cur, T, clip)), max(lam / 10.0, 1e-9)
            info["accepted"] += 1
            info["status"] = REFINED
        else:
            lam = 10.0 * lam
    info["covered_out"], info["ssd_out"] = c
    return M, info


def level_map(w, h, lw, lh):
    fx, fy = w / lw, h / lh
    return np.array([[fx, 0, (fx - 1) / 2], [0, fy, (fy - 1) / 2], [0, 0, 1]], np.float64)


def block_mean(img, f):
    """u8[h,w(,c)] -> u8[h//f, w//f(,c)], the rounded mean of f x f blocks (what an area resize by an integer factor gives)"""
    img = np.asarray(img)
    h, w = img.shape[0] // f, img.shape[1] // f
    b = img[:h * f, :w * f].astype(np.int64).reshape((h, f, w, f) + img.shape[2:])
    return ((2 * b.sum(axis=(1, 3)) + f * f) // (2 * f * f)).astype(np.uint8)


def refine_levels(prev, cur, M_in, levels=3, iters=8, clip=255):
    """Coarse to fine: level l = levels-1 .. 0 works on frames downsized by 2^l, on M_l = S^-1 M S.  -> (M_out, infos)"""
    h, w = np.asarray(cur).shape[:2]
    M, infos = np.asarray(M_in, np.float64).reshape(3, 3), []
    for l in range(int(levels) - 1, -1, -1):
        p, c = (prev, cur) if l == 0 else (block_mean(prev, 2 ** l), block_mean(cur, 2 ** l))
        S = level_map(w, h, c.shape[1], c.shape[0])
        Ml, info = refine(p, c, np.linalg.solve(S, np.dot(M, S)), iters, clip)
        infos.append(info)
        if info["accepted"]:
            M = np.dot(np.dot(S, Ml), np.linalg.inv(S))
            M = M / M[2, 2]
    return M, infos


def corner_error(M, M_true, w, h):
    """the largest distance, in pixels, between where the two maps send the frame's four corners"""
    c = np.array([[0, 0, 1], [w - 1, 0, 1], [0, h - 1, 1], [w - 1, h - 1, 1]], np.float64).T
    a, b = np.dot(np.asarray(M).reshape(3, 3), c), np.dot(np.asarray(M_true).reshape(3, 3), c)
    return float(np.hypot(a[0] / a[2] - b[0] / b[2], a[1] / a[2] - b[1] / b[2]).max())
