"""numpy restatement of evh_canvas_refine (include/evhip.h) on top of warp_checks, residual_checks and refine_checks: a frame aligned
against a canvas of another size that has holes, and of the loop evenvizion_amd.registration.anchor_superposition runs with it.
Where the header is unclear, this file is the definition.

    sample(canvas, M, w, h, count, min_cover)          -> (values u8[h,w(,c)], covered bool[h,w]): the warp's coverage AND valid
    cost(canvas, cur, M, count, min_cover)             -> (covered, ssd), Python ints
    jacobian(canvas, cur, M, clip, count, min_cover)   -> (J int64[n,8], r int64[n]) over the covered, interior pixels with |r| <= clip
    refine(canvas, cur, M_in, iters, clip, count, min_cover) -> (M_out f64[3,3], info dict), refine_checks.refine's loop
    anchor(frames, S, bounds, iters, clip, group, blend, feather, min_overlap, margin) -> (S' list, info list): the driver's loop,
                                                           the painting taken from blend_checks

With canvas = the previous frame and count None every function equals refine_checks' (tests/test_canvas_refine_host.py).
"""
import numpy as np

import blend_checks as B
import refine_checks as RC
import residual_checks as R
import warp_checks as W


def sample(canvas, M, w, h, count=None, min_cover=1):
    """The canvas at M . (x, y, 1) for every pixel of a w x h frame: evh_warp_fixed_plane's sample with inverse_map, and the
    validity rule: every tap of non-zero weight needs count >= min_cover at its pixel, a tap of weight 0 is not asked."""
    canvas = np.asarray(canvas)
    dh, dw = canvas.shape[:2]
    val, cov = W.warp_frame(canvas, M, w, h, (0, 0), inverse_map=True)
    if count is None:
        return val, cov
    count = np.asarray(count)
    assert count.shape == (dh, dw) and count.dtype == np.uint8
    U, V, cov2 = B.position(M, dw, dh, w, h, (0, 0), True)          # the same operands in the same order as warp_frame
    assert np.array_equal(cov, cov2)
    Ui, Vi = np.where(cov, U, 0).astype(np.int64), np.where(cov, V, 0).astype(np.int64)
    sx, fx, sy, fy = Ui >> 5, Ui & 31, Vi >> 5, Vi & 31
    sx1, sy1 = np.minimum(sx + 1, dw - 1), np.minimum(sy + 1, dh - 1)
    ok = count >= int(min_cover)
    valid = ok[sy, sx] & ((fx == 0) | ok[sy, sx1]) & ((fy == 0) | ok[sy1, sx]) & ((fx == 0) | (fy == 0) | ok[sy1, sx1])
    return val, cov & valid


def cost(canvas, cur, M, count=None, min_cover=1):
    cur = np.asarray(cur)
    h, w = cur.shape[:2]
    val, cov = sample(canvas, M, w, h, count, min_cover)
    d = np.where(cov, R.gray_of(cur).astype(np.int64) - R.gray_of(val).astype(np.int64), 0)
    return int(cov.sum()), int((d * d).sum())


def jacobian(canvas, cur, M, clip=255, count=None, min_cover=1):
    """refine_checks.jacobian with the canvas sample in the place of the previous frame's"""
    cur = np.asarray(cur)
    h, w = cur.shape[:2]
    val, cov = sample(canvas, M, w, h, count, min_cover)
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
    return J, r[ys, xs]


def refine(canvas, cur, M_in, iters=8, clip=255, count=None, min_cover=1):
    """refine_checks.refine's loop, word for word, on the cost and the Jacobian above.  M_out IS M_in's array unless a step was
    accepted."""
    M_in = np.asarray(M_in, np.float64).reshape(3, 3)
    h, w = np.asarray(cur).shape[:2]
    c_in = cost(canvas, cur, M_in, count, min_cover)
    info = dict(status=RC.UNCHANGED, evals=1, accepted=0, covered_in=c_in[0], ssd_in=c_in[1], covered_out=c_in[0], ssd_out=c_in[1], n_in=0)
    if c_in[0] == 0:
        info["status"] = RC.NOTHING_COVERED
        return M_in, info
    M, c, N, lam = M_in, c_in, RC.normal_float(*jacobian(canvas, cur, M_in, clip, count, min_cover)), 1e-3
    info["n_in"] = int(N[44])
    for _ in range(int(iters)):
        delta, why = RC.solve_step(N, lam)
        T = RC.try_matrix(M, delta, w, h) if delta is not None else None
        if T is None or not np.isfinite(T).all():
            if not info["accepted"]:
                info["status"] = why if delta is None else RC.DEGENERATE
            break
        c_try = cost(canvas, cur, T, count, min_cover)
        info["evals"] += 1
        if c_try[0] > 0 and 10 * c_try[0] >= 9 * c_in[0] and RC.better(c_try, c):
            M, c, N, lam = T, c_try, RC.normal_float(*jacobian(canvas, cur, T, clip, count, min_cover)), max(lam / 10.0, 1e-9)
            info["accepted"] += 1
            info["status"] = RC.REFINED
        else:
            lam = 10.0 * lam
    info["covered_out"], info["ssd_out"] = c
    return M, info


def canvas_pair(seed, w, h, channels=1, scale=1.5, holes=4):
    """A refine_families scene seen twice: as a canvas of int(scale w) x int(scale h) at its own pixels, and as a frame of w x h
    whose pixel x looks at canvas pixel M_true . x (the frame sits near the middle of the canvas, its corners pushed by up to 3
    pixels).  count is 1 except in `holes` blocks of 3 x 3 zeros; the start is M_true with the images of the frame's corners pushed
    by 1.0 .. 1.5 pixels, as in refine_families.pair.  -> (canvas, frame, count, M_true, M_start)"""
    import refine_families as F
    rng = np.random.default_rng(seed)
    f = F.scene(rng, channels)
    dw, dh = int(scale * w), int(scale * h)
    c = F.corners(w, h)
    M_true = F.homography_from_points(c, c + np.array([(dw - w) // 2, (dh - h) // 2], np.float64) + rng.uniform(-3, 3, (4, 2)))
    angle, push = rng.uniform(0, 2 * np.pi, 4), rng.uniform(1.0, 1.5, 4)
    M_start = F.homography_from_points(c, F.apply(M_true, c) + (push * np.array([np.cos(angle), np.sin(angle)])).T)
    frame = F.render(f, rng, M_true, w, h, channels)
    canvas = F.render(f, rng, np.eye(3), dw, dh, channels)
    count = np.ones((dh, dw), np.uint8)
    for _ in range(holes):
        x, y = int(rng.integers(0, dw - 2)), int(rng.integers(0, dh - 2))
        count[y:y + 3, x:x + 3] = 0
    return canvas, frame, count, M_true, M_start


def normalised(M):
    with np.errstate(all="ignore"):
        return M / M[2, 2]


def anchor(frames, S, bounds, iters=8, clip=255, group=1, blend=B.FEATHER, feather=1024, min_overlap=0.25, margin=32):
    """The driver's loop on the host.  frames u8[n,h,w(,c)]; S: n matrices f64[3,3] (NaN = missing), frame pixel -> plane point;
    bounds = (ox, oy, dw, dh) of the plane before the margin.  T takes plane points to canvas pixels, D is the running
    correction: frame k starts at T D S_k / [2][2]; the first group is taken as it stands, every later one refined against the
    canvas picture where the blend's state has a weight; a result is kept when REFINED and covered_in >= min_overlap w h; after a
    group D is chosen so that T D S_last = M'_last; S'_k = T^-1 M'_k / [2][2]; a missing S_k repeats the running S'.
    -> ([S'_k], [info dict with `used` and `overlap`])"""
    frames = np.asarray(frames)
    n, h, w = frames.shape[:3]
    ox, oy, dw, dh = bounds[0] - margin, bounds[1] - margin, bounds[2] + 2 * margin, bounds[3] + 2 * margin
    T, Tinv = W.translation(-ox, -oy), W.translation(ox, oy)
    D, state, picture, running = np.eye(3), None, None, None
    out, infos = [], []
    for g0 in range(0, n, group):
        ks = list(range(g0, min(g0 + group, n)))
        start = [normalised(np.dot(np.dot(T, D), S[k])) if np.isfinite(S[k]).all() else np.full((3, 3), np.nan) for k in ks]
        kept = []
        for k, M0 in zip(ks, start):
            info = dict(status=RC.UNCHANGED, evals=0, accepted=0, covered_in=0, ssd_in=0, covered_out=0, ssd_out=0, n_in=0)
            M1 = M0
            if g0 > 0:
                count = (state[..., -1] > 0).astype(np.uint8)
                M1, info = refine(picture, frames[k], M0, iters, clip, count, 1)
            info["used"] = bool(info["status"] == RC.REFINED and info["covered_in"] >= min_overlap * w * h)
            info["overlap"] = info["covered_in"] / float(w * h)
            kept.append(M1 if info["used"] else M0)
            infos.append(info)
        valid = [i for i, M in enumerate(kept) if np.isfinite(M).all()]
        if valid:
            last = valid[-1]
            D = normalised(np.dot(np.dot(Tinv, kept[last]), np.linalg.inv(S[ks[last]])))
        for M in kept:
            if np.isfinite(M).all():
                running = normalised(np.dot(Tinv, M))
            out.append(running)
        picture, state = B.blend(frames[ks], np.stack(kept), dw, dh, (0, 0), blend, feather, None, state)
    return out, infos
