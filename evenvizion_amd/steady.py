"""Steady view -- the video itself, at its own size, on a smoothed camera path.

Every other picture of the stabilised view lives on a fixed plane or surface that grows with the pan.  Here frame k is shown
through B_k, a homography from steady-view pixels to pixels of frame k (working size), chosen so that the frame's corners follow
the Gaussian mean of their neighbours' corners; the wedges the frame then leaves uncovered at its borders are filled from the
temporally nearest frames through their own matrices, and the join is feathered (evh_steady_frames, include/evhip.h).

    smooth_path(sup, resize_info, radius, sigma, zoom, max_zoom)     {frame_no: B}, float64, no device
    steady_taps(B, sup, resize_info, frame_size, first, count, fill, out_scale)
                                                                     the entry's tables for one chunk, float64, no device
    path_jitter(trajectories)                                        RMS second difference of corner trajectories
    steady_frames(capture, sup, resize_info, ...)                    generator of (frame_no, picture)
    steady_jpegs(capture, sup, resize_info, ...)                     generator of (frame_no, JPEG file)
    steady_report(report)                                            what steady_report.json holds
"""
import numpy as np

from . import runtime
from .frames import DeviceLadder, FrameReader, check_ingest
from .stabilization import _frames_of, _matrix

MAX_FILL = 7                  # 1 + 2 * fill taps, at most the entry's 16
MAX_FEATHER_PX = 255          # the entry's 8160 / 32
INSIDE_TOLERANCE = 1e-9       # pixels a steady rectangle may stand outside its frame and still count as inside
BISECTIONS = 32


def rectangle(w, h):
    """The corners of a w x h frame, in the order every quadrilateral here keeps: f64[4,2]."""
    return np.array([[0, 0], [w, 0], [w, h], [0, h]], np.float64)


def zoom_matrix(zoom, w, h):
    """Steady pixel p -> c + (p - c) / zoom about the centre c = (w/2, h/2): zoom > 1 shows less of the frame, larger."""
    s = 1.0 / float(zoom)
    return np.array([[s, 0, (w / 2.0) * (1 - s)], [0, s, (h / 2.0) * (1 - s)], [0, 0, 1]], np.float64)


def project(M, points):
    """points f64[n,2] through the 3x3 M -> (f64[n,2], the denominators f64[n])."""
    p = np.asarray(points, np.float64)
    with np.errstate(all="ignore"):
        t = np.dot(np.column_stack([p, np.ones(len(p))]), np.asarray(M, np.float64).T)
        return t[:, :2] / t[:, 2:3], t[:, 2]


def four_point(src, dst):
    """The exact homography (h22 = 1) taking the four points src to dst, by the 8x8 system; numpy.linalg.LinAlgError when singular."""
    A, b = np.zeros((8, 8)), np.zeros(8)
    for i, ((x, y), (u, v)) in enumerate(zip(np.asarray(src, np.float64), np.asarray(dst, np.float64))):
        A[2 * i] = [x, y, 1, 0, 0, 0, -u * x, -u * y]
        A[2 * i + 1] = [0, 0, 0, x, y, 1, -v * x, -v * y]
        b[2 * i], b[2 * i + 1] = u, v
    return np.append(np.linalg.solve(A, b), 1.0).reshape(3, 3)


def is_convex(quad, least=0.0):
    """A quadrilateral f64[4,2] whose four turns all go the same way, none of them straight: every cross product of consecutive
    sides is above `least` in size (an area; smooth_path asks for 1e-9 of the frame's, so that corners which only rounding keeps
    apart count as collapsed)."""
    q = np.asarray(quad, np.float64)
    a, b = np.roll(q, -1, axis=0) - q, np.roll(q, -2, axis=0) - np.roll(q, -1, axis=0)
    turn = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    return bool(np.all(np.isfinite(turn)) and (np.all(turn > least) or np.all(turn < -least)))


def _numbered(superposition_homography_dict):
    """{int frame number: f64[3,3] or None} of a dictionary's frames."""
    return {int(k): _matrix(superposition_homography_dict[k]) for k in _frames_of(superposition_homography_dict)}


def _relative(S_to, S_from):
    """inv(S_to) . S_from, or None where that is not finite."""
    if S_to is None or S_from is None:
        return None
    try:
        with np.errstate(all="ignore"):
            R = np.dot(np.linalg.inv(S_to), S_from)
    except np.linalg.LinAlgError:
        return None
    return R if np.all(np.isfinite(R)) else None


def check_path_arguments(radius, sigma, zoom, max_zoom):
    if int(radius) != radius or radius < 0:
        raise ValueError("radius must be a whole number of frames, 0 or more")
    if sigma is not None and not (np.isfinite(sigma) and sigma > 0):
        raise ValueError("sigma must be positive")
    if not (np.isfinite(max_zoom) and max_zoom >= 1):
        raise ValueError("max_zoom must be at least 1")
    if not (isinstance(zoom, str) and zoom == "auto"):
        if isinstance(zoom, str) or not (np.isfinite(zoom) and zoom > 0):
            raise ValueError("zoom must be 'auto' or a positive number")


def window_weights(radius, sigma=None):
    """exp(-j^2 / 2 sigma^2) for j = -radius .. radius, not normalised; sigma defaults to radius / 2."""
    j = np.arange(-int(radius), int(radius) + 1, dtype=np.float64)
    if radius == 0:
        return np.ones(1)
    s = float(radius) / 2.0 if sigma is None else float(sigma)
    return np.exp(-(j * j) / (2.0 * s * s))


def mean_quadrilaterals(superposition_homography_dict, resize_info, radius=15, sigma=None):
    """{frame_no: f64[4,2] or None}: per frame k with a usable matrix, the Gaussian mean of the corners of the frames
    |j - k| <= radius, each taken to frame k's pixels through inv(S_k) . S_j.  The window is cut at the ends of the video and
    renormalised; a neighbour whose relative matrix is not finite, or that puts a corner at tw <= 0, has weight 0.  None: frame k
    has no usable matrix."""
    S = _numbered(superposition_homography_dict)
    rect = rectangle(float(resize_info["w"]), float(resize_info["h"]))
    g = window_weights(radius, sigma)
    out = {}
    for k in sorted(S):
        if S[k] is None or _relative(S[k], S[k]) is None:
            out[k] = None
            continue
        total, weight = np.zeros((4, 2)), 0.0
        for j in range(k - int(radius), k + int(radius) + 1):
            R = np.eye(3) if j == k else _relative(S[k], S.get(j))
            if R is None:
                continue
            q, tw = project(R, rect)
            if not (np.all(tw > 0) and np.all(np.isfinite(q))):
                continue
            total += g[j - k + int(radius)] * q
            weight += g[j - k + int(radius)]
        out[k] = total / weight
    return out


def rectangles_inside(paths, zoom, w, h, tolerance=INSIDE_TOLERANCE):
    """Does every steady rectangle, at this zoom, lie inside its own frame?  paths: {frame_no: P or None}, P without zoom.
    The rectangles are those of the pixel centres, (0, 0) .. (w - 1, h - 1), of the picture and of the frame: what evh_steady_frames
    covers, so that a picture inside its frame has no pixel left to fill."""
    Z, rect = zoom_matrix(zoom, w, h), rectangle(w - 1, h - 1)
    for P in paths.values():
        if P is None:
            continue
        q, tw = project(np.dot(P, Z), rect)
        if not (np.all(tw > 0) and np.all(q >= -tolerance) and np.all(q[:, 0] <= w - 1 + tolerance) and
                np.all(q[:, 1] <= h - 1 + tolerance)):
            return False
    return True


def smooth_path(superposition_homography_dict, resize_info, radius=15, sigma=None, zoom=1.0, max_zoom=1.25, report=None):
    """{frame_no: B f64[3,3]}: B maps steady-view pixels to pixels of that frame, in working-size coordinates.

    Per frame, in the frame's own coordinates (no plane horizon, no drift): mean_quadrilaterals gives where the frame's corners
    should be; P_k is the exact four-point homography from the rectangle to that quadrilateral, and B_k = P_k . zoom_matrix(zoom).
    zoom="auto": the smallest zoom in 1 .. max_zoom, by bisection, at which every steady rectangle lies inside its own frame
    (rectangles_inside, to INSIDE_TOLERANCE); max_zoom itself where even that does not suffice.  A frame whose mean quadrilateral is not convex or
    whose system is singular gets the zoom alone; radius=0 gives the zoom alone to every frame; a frame without a usable matrix
    gets the identity (it comes out as it went in).  report: a dict that receives zoom, zoom_fails_at (the largest zoom the
    bisection saw fail, or None), zoom_capped, radius, sigma, fallback (frames that got the zoom alone for their quadrilateral)
    and no_matrix (frames that got the identity)."""
    check_path_arguments(radius, sigma, zoom, max_zoom)
    w, h = float(resize_info["w"]), float(resize_info["h"])
    rect = rectangle(w, h)
    paths, fallback, no_matrix = {}, [], []
    for k, quad in mean_quadrilaterals(superposition_homography_dict, resize_info, radius, sigma).items():
        if quad is None:
            paths[k] = None
            no_matrix.append(k)
            continue
        paths[k] = np.eye(3)
        if radius == 0:
            continue
        try:
            if not is_convex(quad, 1e-9 * w * h):
                raise np.linalg.LinAlgError("not convex")
            P = four_point(rect, quad)
            if not np.all(np.isfinite(P)):
                raise np.linalg.LinAlgError("not finite")
            paths[k] = P
        except np.linalg.LinAlgError:
            fallback.append(k)
    fails_at, capped = None, False
    if isinstance(zoom, str):
        lo, hi = 1.0, float(max_zoom)
        if rectangles_inside(paths, lo, w, h):
            zoom = lo
        elif not rectangles_inside(paths, hi, w, h):
            zoom, fails_at, capped = hi, hi, True
        else:
            for _ in range(BISECTIONS):
                mid = 0.5 * (lo + hi)
                if rectangles_inside(paths, mid, w, h):
                    hi = mid
                else:
                    lo = mid
            zoom, fails_at = hi, lo
    Z = zoom_matrix(zoom, w, h)
    if report is not None:
        report.update(zoom=float(zoom), zoom_fails_at=fails_at, zoom_capped=capped, radius=int(radius),
                      sigma=None if radius == 0 else float(radius / 2.0 if sigma is None else sigma), fallback=fallback,
                      no_matrix=no_matrix)
    return {k: np.eye(3) if P is None else np.dot(P, Z) for k, P in paths.items()}


def path_jitter(trajectories):
    """The RMS second difference of corner trajectories f64[n, corners, 2] (or [n, 2]): sqrt of the mean, over the inner frames
    and the corners, of |c[i-1] - 2 c[i] + c[i+1]|^2.  0 for fewer than three frames."""
    c = np.asarray(trajectories, np.float64)
    if len(c) < 3:
        return 0.0
    d = c[:-2] - 2.0 * c[1:-1] + c[2:]
    return float(np.sqrt(np.mean(np.sum(d * d, axis=-1))))


def corner_trajectories(superposition_homography_dict, resize_info, B=None):
    """The corners of every frame with a usable matrix in the fixed plane, f64[n,4,2]: of the frame itself, or with B of its
    steady rectangle.  Frames whose corners are not finite are left out."""
    S = _numbered(superposition_homography_dict)
    rect = rectangle(float(resize_info["w"]), float(resize_info["h"]))
    out = []
    for k in sorted(S):
        if S[k] is None:
            continue
        q, tw = project(S[k] if B is None else np.dot(S[k], B[k]), rect)
        if np.all(np.isfinite(q)) and (np.all(tw > 0) or np.all(tw < 0)):
            out.append(q)
    return np.array(out).reshape(-1, 4, 2)


def output_size(frame_size, out_scale):
    return max(1, int(round(frame_size[0] * float(out_scale)))), max(1, int(round(frame_size[1] * float(out_scale))))


def tap_order(fill):
    """The offsets of taps 1 ..: -1, +1, -2, +2, ... up to `fill` on each side."""
    return [s * d for d in range(1, int(fill) + 1) for s in (-1, 1)]


def steady_taps(B, superposition_homography_dict, resize_info, frame_size, first, count, fill, out_scale=1.0):
    """The tables of evh_steady_frames for the chunk of frames first .. first + count - 1 (frame numbers, from 1), one row per
    frame -> (tap_frame i32[count, 1 + 2 fill], tap_M f64[count, 1 + 2 fill, 9]).

    Frames are full size (frame_size = (w0, h0)): with K = diag(w / w0, h / h0, 1), as stabilization._placement scales, and
    D = diag(1 / out_scale, 1 / out_scale, 1), tap 0 of frame k is the frame itself (index k - first) through
    inv(K) . B_k . K . D, and taps 1 .. are frames k-1, k+1, k-2, k+2, ... through inv(K) . inv(S_j) . S_k . B_k . K . D.  A tap is -1
    (its matrix NaN) when its frame lies outside the video or the chunk, when its matrix is not finite, or when its denominator
    -- the sign taken from the centre of the output rectangle -- is not positive at all four corners of the output rectangle.
    A frame without B or without a usable matrix has the identity for B and no taps but its own."""
    S = _numbered(superposition_homography_dict)
    w0, h0 = float(frame_size[0]), float(frame_size[1])
    dw, dh = output_size(frame_size, out_scale)
    K = np.diag([float(resize_info["w"]) / w0, float(resize_info["h"]) / h0, 1.0])
    Kinv = np.diag([w0 / float(resize_info["w"]), h0 / float(resize_info["h"]), 1.0])
    D = np.diag([1.0 / float(out_scale), 1.0 / float(out_scale), 1.0])
    corners = np.array([[0, 0], [dw - 1, 0], [dw - 1, dh - 1], [0, dh - 1]], np.float64)
    centre = np.array([[(dw - 1) / 2.0, (dh - 1) / 2.0]])
    offsets = tap_order(fill)
    tap_frame = np.full((count, 1 + len(offsets)), -1, np.int32)
    tap_M = np.full((count, 1 + len(offsets), 9), np.nan)
    for i in range(count):
        k = int(first) + i
        usable = k in B and S.get(k) is not None
        tail = np.dot(np.dot(B[k] if usable else np.eye(3), K), D)
        tap_frame[i, 0] = i
        tap_M[i, 0] = np.dot(Kinv, tail).reshape(9)
        for t, off in enumerate(offsets if usable else (), 1):
            j = k + off
            if not 0 <= j - int(first) < count:
                continue
            R = _relative(S.get(j), S[k])
            if R is None:
                continue
            with np.errstate(all="ignore"):
                M = np.dot(np.dot(Kinv, R), tail)
            if not np.all(np.isfinite(M)):
                continue
            sign = np.sign(project(M, centre)[1][0])
            if sign == 0 or not np.all(project(M, corners)[1] * sign > 0):
                continue
            tap_frame[i, t] = j - int(first)
            tap_M[i, t] = (M * sign).reshape(9)
    return tap_frame, tap_M


def check_steady_arguments(radius, sigma, zoom, max_zoom, fill, feather_px, scale, chunk_frames, ingest):
    """The refusals of steady_frames and steady_jpegs, before the capture is touched."""
    check_path_arguments(radius, sigma, zoom, max_zoom)
    if int(fill) != fill or not 0 <= fill <= MAX_FILL:
        raise ValueError("fill must lie in 0..%d frames on each side" % MAX_FILL)
    if not (np.isfinite(feather_px) and 0 <= feather_px <= MAX_FEATHER_PX):
        raise ValueError("feather_px must lie in 0..%d pixels" % MAX_FEATHER_PX)
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError("scale must be positive")
    if int(chunk_frames) != chunk_frames or chunk_frames < 2 * fill + 1:
        raise ValueError("chunk_frames must be at least 2 * fill + 1: consecutive chunks share 2 * fill frames")
    check_ingest(ingest)


def _steady_chunks(capture, superposition_homography_dict, resize_info, radius, sigma, zoom, max_zoom, fill, feather_px, scale,
                   chunk_frames, ingest, report):
    """The loop behind steady_frames and steady_jpegs, in the form pictures.jpegs_of_chunks takes: yields (number of the first
    picture, n, the pictures [n,dh,dw(,3)] on the device, None, None), valid until the next step.

    Chunks share 2 * fill frames, so that a frame in the middle of a chunk finds all its neighbours there: a chunk gives the
    pictures of its frames from `fill` (the first chunk: from 0) to n - fill.  Its last `fill` frames are the next chunk's to
    give -- unless there is none, which is only known once the reader has been asked: the video may end exactly where the chunk
    does.  Then they are produced from the chunk that is still on the device, their forward taps cut by steady_taps."""
    import torch
    check_steady_arguments(radius, sigma, zoom, max_zoom, fill, feather_px, scale, chunk_frames, ingest)
    fill, chunk, feather = int(fill), int(chunk_frames), int(round(float(feather_px) * 32))
    report = {} if report is None else report
    B = smooth_path(superposition_homography_dict, resize_info, radius, sigma, zoom, max_zoom, report)
    report.update(fill=fill, feather_px=float(feather_px), scale=float(scale), frames={},
                  jitter_before=path_jitter(corner_trajectories(superposition_homography_dict, resize_info)),
                  jitter_after=path_jitter(corner_trajectories(superposition_homography_dict, resize_info, B)))
    reader = FrameReader(capture, ingest)
    w0, h0 = reader.w0, reader.h0
    dw, dh = output_size((w0, h0), scale)
    ctx = runtime.get_context(64, 64)             # the entry works on caller buffers of any size
    dev = runtime.device()
    ladder = DeviceLadder(dev, chunk, reader.planes, (w0, h0))
    gray = not reader.planes and reader.first.ndim == 2
    out = torch.empty((chunk, dh, dw) + (() if gray else (3,)), dtype=torch.uint8, device=dev)
    counts = torch.zeros((chunk, 2 + 2 * fill), dtype=torch.int32, device=dev)

    def pictures(start, src, size, tables, lo, hi):
        m = hi - lo
        tap_frame = torch.from_numpy(np.ascontiguousarray(tables[0][lo:hi])).to(dev)
        tap_M = torch.from_numpy(np.ascontiguousarray(tables[1][lo:hi])).to(dev)
        ctx.steady_frames(src, tap_frame, tap_M, out[:m], feather=feather, counts=counts[:m], size=size)
        ctx.order_torch_after()
        pixels = counts[:m].cpu().numpy().astype(np.int64)
        for i in range(m):
            report["frames"][start + lo + 1 + i] = dict(uncovered=int(pixels[i, 0]) / float(dw * dh), own=int(pixels[i, 1]) / float(dw * dh),
                                                        filled=int(pixels[i, 2:].sum()) / float(dw * dh))
        return start + lo + 1, m, out[:m], None, None

    chunks = reader.chunks(chunk, 2 * fill)
    current = next(chunks, None)
    if current is None:                           # chunks that share 2 * fill frames have more than that: this video never fills one
        raise ValueError("the video has only %d frames: fill = %d needs at least %d" % (reader.consumed, fill, 2 * fill + 1))
    while current is not None:
        start, frames = current
        n = len(frames)
        # a copy of its own: the reader's buffer is written again before the chunk's last pictures are known to be wanted
        _, src, size = ladder(ctx, torch.from_numpy(frames).to(dev, copy=True))
        tables = steady_taps(B, superposition_homography_dict, resize_info, (w0, h0), start + 1, n, fill, scale)
        lo = 0 if start == 0 else fill
        hi = max(lo, n - fill)
        if hi > lo:
            yield pictures(start, src, size, tables, lo, hi)
        current = next(chunks, None)
        if current is None and n > hi:
            yield pictures(start, src, size, tables, hi, n)


def steady_frames(capture, superposition_homography_dict, resize_info, radius=15, sigma=None, zoom="auto", fill=2, feather_px=8,
                  scale=1.0, chunk_frames=32, ingest="auto", max_zoom=1.25, report=None):
    """Generator of (frame_no, uint8 ndarray [dh,dw,3], or [dh,dw] for a gray capture): every frame of `capture`, exactly once and
    in order (frame_no counts from 1, as the dictionary's keys do), seen from the smoothed camera path of smooth_path(radius,
    sigma, zoom, max_zoom) at `scale` times its own size.  What the frame does not cover is filled from the `fill` frames before
    and after it (nearest first), feathered over feather_px pixels inside the frame's border; what none of them covers is black.
    A frame without a usable matrix comes out as it went in.  Frames are read and uploaded chunk_frames at a time (as 4:2:0
    planes where ingest allows), consecutive chunks sharing 2 * fill frames; a video of at most 2 * fill frames is a ValueError.  report: a dict that receives what steady_report
    formats -- complete once the generator is exhausted.  Bad arguments are refused before the capture is touched."""
    for first, n, pictures, _, _ in _steady_chunks(capture, superposition_homography_dict, resize_info, radius, sigma, zoom, max_zoom,
                                                   fill, feather_px, scale, chunk_frames, ingest, report):
        host = pictures.cpu().numpy()
        for k in range(n):
            yield first + k, host[k]


def steady_jpegs(capture, superposition_homography_dict, resize_info, radius=15, sigma=None, zoom="auto", fill=2, feather_px=8,
                 scale=1.0, chunk_frames=32, ingest="auto", max_zoom=1.25, report=None, quality=90, subsampling="420"):
    """Generator of (frame_no, bytes): the pictures of steady_frames -- same arguments, same pictures -- as baseline JPEG files,
    encoded on the device where the chunk's pictures lie (evh_jpeg_encode): no picture is downloaded, only the files."""
    from .pictures import check_format, jpegs_of_chunks
    check_format(quality, subsampling)
    check_steady_arguments(radius, sigma, zoom, max_zoom, fill, feather_px, scale, chunk_frames, ingest)
    return jpegs_of_chunks(_steady_chunks(capture, superposition_homography_dict, resize_info, radius, sigma, zoom, max_zoom, fill,
                                          feather_px, scale, chunk_frames, ingest, report), False, quality, subsampling)


def steady_report(report):
    """What steady_report.json holds, from the dict steady_frames / steady_jpegs filled: the path (radius, sigma, zoom, whether the
    zoom met its cap), the jitter of the frames' corners in the fixed plane before and after smoothing (path_jitter, working-size
    pixels), the frames that fell back, and per frame the shares of its picture no frame covered, its own frame gave and its
    neighbours filled."""
    frames = report.get("frames", {})
    mean = (lambda name: float(np.mean([f[name] for f in frames.values()])) if frames else 0.0)
    return {"radius": report.get("radius"), "sigma": report.get("sigma"), "zoom": report.get("zoom"),
            "zoom_capped": bool(report.get("zoom_capped", False)), "fill": report.get("fill"), "feather_px": report.get("feather_px"),
            "scale": report.get("scale"), "jitter_before": report.get("jitter_before"), "jitter_after": report.get("jitter_after"),
            "frames_without_matrix": [int(k) for k in report.get("no_matrix", [])],
            "frames_with_zoom_alone": [int(k) for k in report.get("fallback", [])],
            "mean_shares": {name: mean(name) for name in ("uncovered", "own", "filled")},
            "frames": {str(k): frames[k] for k in sorted(frames)}}
