"""Seeded adversarial point sets for the homography solver (RANSAC draw, inlier test, iteration bound, refit, LM) and a
float64 reference that does not go through the oracle.  Shared by tests/test_oracle_solver_edges.py (CPU) and
tests/test_gpu_solver_edges.py (device).

Rows are float32 (ax, ay, bx, by): H maps a -> b, as in cv2.findHomography(a, b).  Every family function returns a list of
(name, rows) and names, in its docstring, the branch it is built to reach.  The sets are deterministic: the assertions that
depend on the draw (which branch a set reaches, how many subsets are rejected) are checked on the oracle by the CPU module.
"""
import math

import numpy as np

THR = 3.0
CONF = 0.995
MAX_ITERS = 2000


def _f32(a, b):
    return np.ascontiguousarray(np.c_[a, b], dtype=np.float32)


def proj(H, a):
    """float64 projection of a f64[n,2] by H"""
    a = np.asarray(a, np.float64)
    p = a @ H[:, :2].T + H[:, 2]
    return p[:, :2] / p[:, 2:]


def _h(rng, scale=1.0, persp=1e-5):
    th = np.deg2rad(rng.uniform(-3, 3))
    s = rng.uniform(0.95, 1.05)
    H = np.array([[s * np.cos(th), -s * np.sin(th), rng.uniform(-20, 20) * scale],
                  [s * np.sin(th), s * np.cos(th), rng.uniform(-20, 20) * scale],
                  [rng.uniform(-persp, persp), rng.uniform(-persp, persp), 1.0]])
    return H


def _outliers(rng, b, frac, lo=0.0, hi=1280.0):
    b = b.copy()
    k = int(round(len(b) * frac))
    if k:
        b[rng.choice(len(b), k, replace=False)] = rng.uniform(lo, hi, (k, 2))
    return b


# ---- F1 -------------------------------------------------------------------------------------------------------------------
def f1_collinear():
    """F1 collinear-heavy: integer grids and points on 2-3 lines with a few generic points, so that most 4-subsets hold a
    collinear triple through the last drawn point (haveCollinearPoints) and get_subset's attempt loop runs long.
    'f1_rare': every a row but one lies on one line, and the rows on it are shuffled along the b line, so the only subsets
    checkSubset accepts are (line, line, line, that point) with the three line rows in the same order on both sides: the
    draw runs out of its 10000 attempts (stats[1]) although valid subsets exist."""
    rng = np.random.default_rng(101)
    out = []
    g = np.array([(x, y) for x in range(0, 400, 40) for y in range(0, 300, 50)], np.float64)      # 10 x 6 grid
    H = _h(rng)
    b = proj(H, g) + rng.normal(0, 0.2, g.shape)
    out.append(("f1_grid", _f32(g, _outliers(rng, b, 0.15))))
    g2 = np.array([(x, y) for x in range(8) for y in range(8)], np.float64) * 16 + 100              # 8 x 8 exact grid
    out.append(("f1_grid_exact", _f32(g2, proj(np.array([[1, 0, 7], [0, 1, -5], [0, 0, 1.0]]), g2))))
    for nl in (2, 3):
        pts = []
        for k in range(nl):
            t = rng.uniform(0, 600, 40)
            d = np.array([np.cos(k * 1.1 + 0.3), np.sin(k * 1.1 + 0.3)])
            pts.append(np.array([200.0 + 50 * k, 150.0]) + t[:, None] * d)
        pts.append(rng.uniform(0, 640, (4, 2)))                                                     # a few generic points
        a = np.vstack(pts)
        H = _h(rng)
        out.append(("f1_lines%d" % nl, _f32(a, _outliers(rng, proj(H, a) + rng.normal(0, 0.3, a.shape), 0.1))))
    n = 1500
    t = np.arange(n, dtype=np.float64)
    a = np.c_[10 + t * 0.5, 20 + t * 0.25]                                                          # exact in float32
    perm = rng.permutation(n)
    b = np.c_[30 + perm * 0.5, 20 + perm * 0.5]
    a[n // 2] = (300.0, 600.0)
    b[n // 2] = (700.0, 100.0)
    out.append(("f1_rare", _f32(a, b)))
    return out


# ---- F2 -------------------------------------------------------------------------------------------------------------------
def f2_duplicates():
    """F2 duplicates: 30-90 % of the rows repeat earlier rows exactly.  A subset holding two copies of one point has
    dx = dy = 0 against the last point (or the same triple twice) and is rejected as collinear."""
    rng = np.random.default_rng(202)
    out = []
    for frac, m in ((0.3, 60), (0.6, 40), (0.9, 12)):
        a = rng.uniform(0, 1280, (m, 2))
        H = _h(rng, persp=3e-5)
        b = _outliers(rng, proj(H, a) + rng.normal(0, 0.3, a.shape), 0.15)
        base = _f32(a, b)
        nd = int(round(m * frac / (1 - frac)))
        rows = np.vstack([base, base[rng.integers(0, m, nd)]])
        out.append(("f2_dup%d" % int(frac * 100), rows[rng.permutation(len(rows))]))
    return out


# ---- F3 -------------------------------------------------------------------------------------------------------------------
def f3_orientation():
    """F3 orientation: a mirrored H (det < 0), where all four triangle signs flip and checkSubset accepts negative == 4; and a
    set whose rows follow H for one half and a mirrored H for the other, where mixed subsets have mixed signs and are
    rejected."""
    rng = np.random.default_rng(303)
    out = []
    M = np.diag([-1.0, 1.0, 1.0])
    for k in range(2):
        a = rng.uniform(0, 1280, (80, 2))
        H = np.array([[1, 0, 1280.0], [0, 1, 0], [0, 0, 1]]) @ M @ _h(rng, persp=2e-5)
        out.append(("f3_mirror%d" % k, _f32(a, _outliers(rng, proj(H, a) + rng.normal(0, 0.3, a.shape), 0.2 * k))))
    a = rng.uniform(0, 1280, (120, 2))
    H1 = _h(rng)
    H2 = np.array([[1, 0, 1280.0], [0, 1, 0], [0, 0, 1]]) @ M @ H1
    b = np.where((np.arange(120) % 2 == 0)[:, None], proj(H1, a), proj(H2, a))
    out.append(("f3_half_mirrored", _f32(a, b)))
    b = np.where((np.arange(120) < 84)[:, None], proj(H1, a), proj(H2, a))
    out.append(("f3_70_30_mirrored", _f32(a, b)))
    return out


# ---- F4 -------------------------------------------------------------------------------------------------------------------
def boundary_expected(rows, H):
    """is_inlier's float32 evaluation of every row under float32(H): err <= (float)(thr * thr)."""
    Hf = np.asarray(H, np.float64).reshape(9).astype(np.float32)
    M = rows[:, :2].astype(np.float32); m = rows[:, 2:].astype(np.float32)
    one = np.float32(1)
    ww = one / ((Hf[6] * M[:, 0] + Hf[7] * M[:, 1]) + one)
    dx = ((Hf[0] * M[:, 0] + Hf[1] * M[:, 1]) + Hf[2]) * ww - m[:, 0]
    dy = ((Hf[3] * M[:, 0] + Hf[4] * M[:, 1]) + Hf[5]) * ww - m[:, 1]
    err = dx * dx + dy * dy
    return err, err <= np.float32(THR * THR)


F4_H = np.array([[1.0, 0.0, 5.0], [0.0, 1.0, -3.0], [0.0, 0.0, 1.0]])


def f4_boundary():
    """F4 inlier boundary: rows exactly on a translation (integer coordinates: every projection is exact in float32) plus
    rows displaced by 3 (1 +- k 2^-20) px, axis-aligned and diagonal, so that is_inlier's `err <= 9` decides each of them by
    the float32 evaluation: err == 9 exactly (kept only by <=), one ulp either side, and diagonal sums that round onto 9.
    The expected mask is boundary_expected(rows, F4_H)."""
    rng = np.random.default_rng(404)
    out = []
    for m, nb in ((40, 24), (200, 48)):
        a = rng.integers(0, 48, (m, 2)).astype(np.float64)
        a = np.unique(a, axis=0)[:m]
        b = proj(F4_H, a)
        ea, eb = [], []
        for k in range(nb):
            p = rng.integers(0, 48, 2).astype(np.float64)
            q = proj(F4_H, p[None])[0]
            kind = k % 6
            if kind < 3:                           # axis-aligned: 3 exactly, 3 (1 + j 2^-20), 3 (1 - j 2^-20)
                d = np.float32(3.0) if kind == 0 else np.float32(3.0 * (1 + (1 if kind == 1 else -1) * (1 + k // 6) * 2.0 ** -20))
                sgn = 1 if k % 4 < 2 else -1
                if k % 2:
                    t = (q[0] + sgn * float(d), q[1])
                else:
                    t = (q[0], q[1] + sgn * float(d))
            else:                                  # diagonal: dx = dy ~ 3 / sqrt(2) (1 +- j 2^-20)
                e = 3.0 / math.sqrt(2.0) * (1 + (kind - 4) * (1 + k // 6) * 2.0 ** -20)
                t = (q[0] + e, q[1] - e)
            ea.append(p); eb.append(t)
        a2 = np.vstack([a, np.array(ea)]); b2 = np.vstack([b, np.array(eb)])
        perm = rng.permutation(len(a2))
        out.append(("f4_boundary_%d" % len(a2), _f32(a2[perm], b2[perm])))
    return out


# ---- F5 -------------------------------------------------------------------------------------------------------------------
def num_iters64(n, good, max_iters=MAX_ITERS, conf=CONF):
    """RANSACUpdateNumIters in float64 (numpy, the same chain as the operator) -> (bound, num / denom)."""
    ep = (n - good) / n
    num = math.log(max(1.0 - conf, 2.2250738585072014e-308))
    denom = 1.0 - (1.0 - ep) ** 4
    if denom < 2.2250738585072014e-308:
        return 0, float("inf")
    denom = math.log(denom)
    x = num / denom
    if denom >= 0 or -num >= max_iters * (-denom):
        return max_iters, x
    return int(np.rint(x)), x


def f5_search(nmax=1200, max_iters=MAX_ITERS):
    """(n, good) pairs, n <= nmax, whose log(1 - conf) / log(1 - (1 - eps)^4) lies closest to a half-integer (rint decides
    the bound), and those where -num >= max_iters * (-denom) holds with the nearest equality.  Distances are computed at 50
    digits (mpmath), independently of libm."""
    import mpmath
    mpmath.mp.dps = 50
    lnum = mpmath.log(mpmath.mpf(1) - mpmath.mpf(CONF))
    half, edge = [], []
    for n in range(5, nmax + 1):
        for good in range(4, n + 1):
            w = good / n
            if w < 0.2:
                continue
            x = math.log(1 - CONF) / math.log(1 - w ** 4) if w < 1 else 0.0
            if 1.0 < x < 300 and abs(x - math.floor(x) - 0.5) < 2e-5:
                half.append((n, good))
            r = -math.log(1 - CONF) / (-math.log(1 - w ** 4)) / max_iters if w < 1 else 0.0
            if abs(r - 1) < 1e-4:
                edge.append((n, good))

    def dist_half(p):
        n, good = p
        w = mpmath.mpf(good) / n
        x = lnum / mpmath.log(1 - w ** 4)
        return float(abs(x - mpmath.floor(x) - mpmath.mpf("0.5")))

    def dist_edge(p):
        n, good = p
        w = mpmath.mpf(good) / n
        return float(abs(-lnum - max_iters * -mpmath.log(1 - w ** 4)))
    half.sort(key=dist_half)
    edge.sort(key=dist_edge)
    return [(p, dist_half(p)) for p in half[:4]], [(p, dist_edge(p)) for p in edge[:3]]


# found by f5_search(1200) (tests/test_oracle_solver_edges.py::test_f5_pairs_are_the_closest re-derives the first entries)
F5_HALF = [(1171, 1068), (571, 431), (1142, 862), (256, 207)]
F5_EDGE = [(1142, 259), (1045, 237), (948, 215)]


def f5_iteration_boundary():
    """F5 iteration-count boundary: exact inliers on a generic H plus far outliers, with (n, inlier count) taken from F5_HALF
    (num / denom within ~1e-7 of a half-integer: rint picks the bound) and F5_EDGE (-num ~ maxIters * -denom)."""
    rng = np.random.default_rng(505)
    out = []
    for tag, pairs in (("half", F5_HALF), ("edge", F5_EDGE)):
        for n, good in pairs:
            a = rng.uniform(0, 1280, (n, 2)).astype(np.float32).astype(np.float64)
            H = _h(rng, persp=1e-5)
            b = proj(H, a).astype(np.float32).astype(np.float64)
            k = n - good
            far = rng.uniform(-2e4, 2e4, (k, 2)) + 3e4 * np.sign(rng.uniform(-1, 1, (k, 2)))
            idx = rng.choice(n, k, replace=False)
            b[idx] = far
            out.append(("f5_%s_%d_%d" % (tag, n, good), _f32(a, b)))
    return out


# ---- F6 -------------------------------------------------------------------------------------------------------------------
def f6_conditioning():
    """F6 conditioning: 4K coordinates with 1e4 offsets, 1-2 px clusters, strong perspective (w over 0.2-5), a horizon through
    the source centroid (h33 = 0 in the normalised frame: the h33 = 1 refit of the tolerance mode has no solution, its 8x8
    system is singular -- the LDL^T / 1e12 fall-back), a near-affine H (h31, h32 ~ 1e-9), and n = 4..8 exactly."""
    rng = np.random.default_rng(606)
    out = []
    for off in (0.0, 1e4):
        a = rng.uniform(0, 1, (300, 2)) * [3840, 2160] + off
        H = np.array([[1, 0, off], [0, 1, off], [0, 0, 1.0]]) @ _h(rng, persp=2e-6) @ np.array([[1, 0, -off], [0, 1, -off], [0, 0, 1.0]])
        out.append(("f6_4k_off%g" % off, _f32(a, _outliers(rng, proj(H, a) + rng.normal(0, 0.3, a.shape), 0.1, off, off + 3840))))
    for wdt in (1.0, 2.0):
        c = rng.uniform(200, 1000, 2)
        a = c + rng.uniform(0, wdt, (60, 2))
        H = _h(rng)
        out.append(("f6_cluster%g" % wdt, _f32(a, proj(H, a) + rng.normal(0, 0.05, a.shape))))
    a = rng.uniform(0, 1280, (150, 2))
    H = np.array([[1.0, 0.1, 30], [0.05, 1.0, 10], [4.8 / 1280, 0.0, 0.2]])               # w from 0.2 to 5
    out.append(("f6_perspective", _f32(a, _outliers(rng, proj(H, a) + rng.normal(0, 0.2, a.shape), 0.1))))
    # horizon through the source centroid: w = ax - c, dyadic w and integer coordinates keep every row exact in float32
    c = 100.0
    ws = np.array([0.5, 1, 2, 4, 8, 16])
    ys = np.arange(-6, 7, 3.0)
    a = np.array([(c + s * w, y) for w in ws for s in (-1, 1) for y in ys])
    Hh = np.array([[1.0, 0, 0], [0, 1.0, 0], [1.0, 0, -c]])
    out.append(("f6_horizon", _f32(a, proj(Hh, a))))
    Hh2 = np.array([[2.0, 1.0, 0], [0, 1.0, 4.0], [1.0, 0.5, -c]])                        # w = ax + ay/2 - c
    a2 = np.array([(c + s * w - 0.5 * y, y) for w in ws for s in (-1, 1) for y in ys])
    out.append(("f6_horizon_tilted", _f32(a2, proj(Hh2, a2))))
    a = rng.uniform(0, 1920, (200, 2))
    H = np.array([[1.01, 0.02, 12], [-0.01, 0.99, -7], [1e-9, -1e-9, 1.0]])
    out.append(("f6_near_affine", _f32(a, _outliers(rng, proj(H, a) + rng.normal(0, 0.3, a.shape), 0.1))))
    for n in (4, 5, 6, 7, 8):
        a = rng.uniform(0, 1280, (n, 2))
        H = _h(rng, persp=2e-5)
        b = proj(H, a) + rng.normal(0, 0.3, a.shape)
        if n >= 6:
            b[-1] += 200.0
        out.append(("f6_n%d" % n, _f32(a, b)))
    return out


# ---- F7 -------------------------------------------------------------------------------------------------------------------
F7_SIZES = (63, 64, 65, 511, 512, 513, 1023, 1024, 1025)


def f7_sizes(sizes=F7_SIZES, seed=707):
    """F7 sizes at the kernel switches: n = 63/64/65 (the 64-row tile), 511/512/513 (LM's passes on four waves from 512 inlier
    rows), 1023-1025, filled with F1-F4 content: grid rows (collinear triples), 30 % duplicates, a mirrored H, rows at the
    3 px boundary and outliers."""
    rng = np.random.default_rng(seed)
    out = []
    M = np.array([[-1.0, 0, 1280], [0, 1, 0], [0, 0, 1]])
    for n in sizes:
        H = (M if n % 2 else np.eye(3)) @ np.array([[1.0, 0, 5], [0, 1, -3], [0, 0, 1]])
        ng = int(n * 0.35)
        side = int(math.ceil(math.sqrt(ng)))
        grid = np.array([(x, y) for x in range(side) for y in range(side)], np.float64)[:ng] * 7 + 40
        gen = rng.integers(0, 1280, (int(n * 0.25), 2)).astype(np.float64)
        a = np.vstack([grid, gen])
        b = proj(H, a)
        nb = int(n * 0.05)
        sel = rng.choice(len(a), nb, replace=False)
        d = np.float32(3.0) * (1 + rng.integers(-2, 3, nb) * 2.0 ** -20)
        ab = a[sel]; bb = proj(H, ab) + np.c_[d, np.zeros(nb)]
        no = int(n * 0.08)
        ao = rng.uniform(0, 1280, (no, 2)); bo = rng.uniform(0, 1280, (no, 2))
        rows = _f32(np.vstack([a, ab, ao]), np.vstack([b, bb, bo]))
        nd = n - len(rows)
        rows = np.vstack([rows, rows[rng.integers(0, len(rows), nd)]])
        out.append(("f7_n%d" % n, rows[rng.permutation(n)]))
    return out


# ---- F8 -------------------------------------------------------------------------------------------------------------------
def f8_gate():
    """F8 compute_homography's gate `s < 0.7 n`: exact inliers on a translation plus far outliers with s = 0.7 n exactly
    (7 of 10, 14 of 20, 21 of 30: OK) and one inlier less (LOW_INLIER_RATIO)."""
    rng = np.random.default_rng(808)
    out = []
    for n, s in ((10, 7), (10, 6), (20, 14), (20, 13), (30, 21), (30, 20)):
        a = rng.integers(0, 640, (n, 2)).astype(np.float64)
        b = proj(F4_H, a)
        b[s:] = rng.uniform(2000, 4000, (n - s, 2))
        out.append(("f8_%d_of_%d" % (s, n), _f32(a, b)))
    return out


FAMILIES = {"F1": f1_collinear, "F2": f2_duplicates, "F3": f3_orientation, "F4": f4_boundary, "F5": f5_iteration_boundary,
            "F6": f6_conditioning, "F7": f7_sizes, "F8": f8_gate}


def all_sets():
    out = []
    for fam, fn in FAMILIES.items():
        out += [(fam, name, rows) for name, rows in fn()]
    return out


# ---- float64 reference ----------------------------------------------------------------------------------------------------
def dlt64(a, b):
    """The refit without the oracle: normalised DLT (centroid, mean absolute deviation per axis, as findHomography's
    runKernel normalises) solved by float64 SVD; None when a scale is zero."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    cM = a.mean(0); cm = b.mean(0)
    sM = np.abs(a - cM).sum(0); sm = np.abs(b - cm).sum(0)
    if (sM < 2.2e-16).any() or (sm < 2.2e-16).any():
        return None
    sM = len(a) / sM; sm = len(a) / sm
    X = (a - cM) * sM; x = (b - cm) * sm
    n = len(a)
    L = np.zeros((2 * n, 9))
    L[0::2, 0:2] = X; L[0::2, 2] = 1; L[0::2, 6:8] = -x[:, :1] * X; L[0::2, 8] = -x[:, 0]
    L[1::2, 3:5] = X; L[1::2, 5] = 1; L[1::2, 6:8] = -x[:, 1:] * X; L[1::2, 8] = -x[:, 1]
    h = np.linalg.svd(L)[2][-1].reshape(3, 3)
    T1 = np.array([[sM[0], 0, -cM[0] * sM[0]], [0, sM[1], -cM[1] * sM[1]], [0, 0, 1]])
    T2i = np.array([[1 / sm[0], 0, cm[0]], [0, 1 / sm[1], cm[1]], [0, 0, 1]])
    H = T2i @ h @ T1
    return H / H[2, 2]


def cost(H, a, b):
    """sum ||proj(H, a) - b||^2 in float64"""
    r = proj(np.asarray(H, np.float64), a) - np.asarray(b, np.float64)
    return float((r * r).sum())


def cost_floor(b):
    """below this the float64 evaluation of cost() is noise: n * (1e-12 (1 + max |b|))^2"""
    return len(b) * (1e-12 * (1.0 + float(np.abs(b).max(initial=0.0)))) ** 2


def normalised_jtj_cond(H, a):
    """Conditioning of the LM problem at H, judged in float64: J^T J of findHomography's refinement (eight parameters,
    h33 = 1, raw pixel coordinates: what the 8x8 solves of both modes see) normalised to a unit diagonal (Marquardt's
    scaling, so that units do not count) -> its largest / smallest eigenvalue."""
    a = np.asarray(a, np.float64)
    h = (np.asarray(H, np.float64) / H[2, 2]).reshape(9)
    w = a @ h[6:8] + 1
    xi = (a @ h[0:2] + h[2]) / w; yi = (a @ h[3:5] + h[5]) / w
    J = np.zeros((2 * len(a), 8))
    J[0::2, 0:2] = a / w[:, None]; J[0::2, 2] = 1 / w; J[0::2, 6:8] = -a * (xi / w)[:, None]
    J[1::2, 3:5] = a / w[:, None]; J[1::2, 5] = 1 / w; J[1::2, 6:8] = -a * (yi / w)[:, None]
    A = J.T @ J
    d = 1 / np.sqrt(np.diag(A))
    ev = np.linalg.eigvalsh(A * d[:, None] * d[None, :])
    return float(ev[-1] / max(ev[0], 1e-300))


WELL_CONDITIONED = 1e5      # normalised_jtj_cond at or below this: the BAR_* constants of test_fast_solver_mode apply (its
                            # frames: ~5e2; 1-2 px clusters ~1e13, 4K at a 1e4 offset ~2e6)


# measured multiple of the threshold within which every mask row lies from the final H (see the modules' checks)
MASK_RADIUS = 1.5


def check_solution(H, mask, rows, tag=""):
    """The float64 checks of one found H against its mask rows: finite; LM did not end above its seed (the float64 SVD refit
    on the same rows); every mask row within MASK_RADIUS * thr of the final H.  Returns (cost(H), cost(refit64))."""
    assert H is not None and np.isfinite(H).all(), tag
    sel = mask.astype(bool)
    a = rows[sel, :2].astype(np.float64); b = rows[sel, 2:].astype(np.float64)
    c = cost(H, a, b)
    if sel.sum() <= 4:
        return c, c
    Hr = dlt64(a, b)
    cr = cost(Hr, a, b) if Hr is not None and np.isfinite(Hr).all() else float("inf")
    assert c <= cr * (1 + 1e-7) + cost_floor(b), (tag, c, cr)
    d = np.sqrt(((proj(H, a) - b) ** 2).sum(1))
    assert d.max() <= MASK_RADIUS * THR, (tag, float(d.max()))
    return c, cr


# ---- the stream scan ------------------------------------------------------------------------------------------------------
def scan_pairs(kcap):
    """Crafted pairs for the stream scan: (rows, status1) with every row count <= kcap, status1 mixing 0 with phase-1 failure
    codes (1 no descriptors, 2 few matches, 3 no provisional H), one pair with no rows, one that fails the 0.7 gate."""
    sets = dict((name, rows) for _, name, rows in all_sets())
    empty = np.zeros((0, 4), np.float32)
    plan = [("f3_mirror1", 0), ("f4_boundary_64", 0), ("f2_dup60", 2), ("f8_7_of_10", 0), (None, 0), ("f6_4k_off0", 1),
            ("f1_lines3", 0), ("f8_6_of_10", 0), ("f7_n513", 3), ("f5_half_256_207", 0), ("f6_horizon", 0), ("f1_grid", 0)]
    out = [(empty if name is None else sets[name], st) for name, st in plan]
    assert all(len(r) <= kcap for r, _ in out)
    return out


def scan_mirror(rows_list, status1, state=None, return_state=False, force=False):
    """The scan of evo_stream_gray_ex (oracle/evz_homography.cpp) over given pair rows, from O.compute_homography and
    O.matrix_superposition: a pair whose phase-1 status is not OK, or whose compute_homography fails, repeats the previous
    H (none_H_processing); a failing pair with no previous H ends the scan (NaN H, its status for every later pair).
    state = (Hsup, Hprev) carries the scan across calls, as the device's state_in / state_out do."""
    from oracle import oracle as O
    n = len(rows_list)
    Hs = np.zeros((n, 3, 3)); sts = np.zeros(n, np.int32)
    if state is None:
        Hsup = Hprev = None; first, have_prev = True, False
    else:
        Hsup, Hprev = state; first, have_prev = False, True
    for p in range(n):
        st = int(status1[p])
        if st == O.OK:
            r = rows_list[p]
            st, H = O.compute_homography(r[:, :2], r[:, 2:], None if first else Hsup, force_max_iters=force)
        if st != O.OK:
            if not have_prev:
                sts[p:] = st; Hs[p:] = np.nan
                break
            H = Hprev
        sts[p] = st; Hs[p] = H
        Hsup = O.matrix_superposition(H, Hsup, first)
        Hprev = H; have_prev = True; first = False
    if return_state:
        return Hs, sts, (Hsup, Hprev)
    return Hs, sts
