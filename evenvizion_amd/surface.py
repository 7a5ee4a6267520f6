"""Fixed surfaces that do not end at the horizon: the stabilised view of a camera that turns, on a cylinder or a sphere.

The reference's known-issues.md: "The coordinates can't be defined also when camera rotation angle is more than 90 deg.  As a
solution ... we see the transfer to the cylindrical coordinate system."  The fixed plane of stabilization.py is the picture plane
of frame 1; a frame turned by a quarter turn against it has its horizon inside the picture, fixed_plane_bounds refuses it and
the point transform answers n/a.  Here the fixed coordinate system is a surface of viewing rays around the camera of frame 1:

    estimate_focal, rotations, superposed_rotations   the rotation model: every pair map M_k = S_{k-1}^-1 . S_k of
                                                      registration.pair_maps is read as K . Q_k . K^-1 with Q_k in SO(3)
    surface_tables, surface_bounds, frame_matrix      the canvas: which ray a canvas pixel stands for, how large the canvas is,
                                                      and the matrix that takes a ray to a frame's pixels
    surface_frames                                    the frames of a capture placed on the surface by evh_warp_ray_surface
                                                      (include/evhip.h), the canvas carried on the device
    surface_coordinates, surface_to_frame             a frame's pixels in surface coordinates and back -- defined where
                                                      fixed_coordinate_system answers n/a

Rays live in the camera frame of frame 1: x to the right, y down, z along the optical axis.  The cylinder's axis is y:
theta = atan2(x, z) runs along the canvas rows, v = y / hypot(x, z) (cylinder) or phi = atan(v) (sphere, equirectangular) down
its columns; canvas pixel (x, y) is theta = (x + ox) / scale_px and v or phi = (y + oy) / scale_px.  Everything in this module
is host float64 numpy and small; nothing of it is claimed byte for byte.  Only the resampling runs on the device, from tables
built here: no trigonometry there.  A camera that also translates does not fit the model; the fit
residual |N - Q|_F per pair says by how much.
"""
import collections
import math

import numpy as np

from . import runtime
from ._lib import WARP_MODES, WARP_MOSAIC
from .frames import check_ingest, entry_matrix
from .registration import pair_maps
from .stabilization import MAX_PIXELS, _canvas_chunks, _frames_of

KINDS = ("cylinder", "sphere", "plane")
EDGE_SAMPLES = 33             # points per frame edge that surface_bounds looks at
GRID_POINTS = 49              # estimate_focal's geometric grid, 0.25 w .. 16 w: a factor 2^(1/8) per step
AXIS_LIMIT = 1e-6             # a ray closer to the cylinder's axis than this share of its length has no place on the cylinder


def _centre(size, centre):
    if centre is None:
        return (float(size[0]) - 1.0) / 2.0, (float(size[1]) - 1.0) / 2.0
    return float(centre[0]), float(centre[1])


def camera_matrix(focal, centre):
    """K = [[f, 0, cx], [0, f, cy], [0, 0, 1]]: ray -> homogeneous pixel."""
    return np.array([[focal, 0.0, centre[0]], [0.0, focal, centre[1]], [0.0, 0.0, 1.0]], np.float64)


def _camera_inverse(focal, centre):
    return np.array([[1.0 / focal, 0.0, -centre[0] / focal], [0.0, 1.0 / focal, -centre[1] / focal], [0.0, 0.0, 1.0]], np.float64)


def polar(N):
    """The rotation next to N (det N > 0) in the Frobenius norm: U . V^T of its SVD.  Works on [..., 3, 3]."""
    U, _, Vt = np.linalg.svd(N)
    return np.matmul(U, Vt)


def _usable(maps, centre):
    """The finite pair maps with a positive determinant, as f64[n,3,3] (possibly empty).  A 3x3 map and its negative are the same
    map of pixels but have opposite determinants, and the superposed matrices change sign where their [2][2], by which the
    reference divides them, does (a quarter turn): each map is first given the sign that sends the frame's centre in front of
    the camera, (M . (cx, cy, 1))[2] > 0.  What then has det <= 0 is a mirror image, not a camera motion."""
    keep = []
    for M in maps:
        m = entry_matrix(M)
        if not np.isfinite(m).all():
            continue
        m = m * np.sign(np.dot(m[2], [centre[0], centre[1], 1.0]))
        if np.linalg.det(m) > 0:
            keep.append(m)
    return np.stack(keep) if keep else np.zeros((0, 3, 3))


def _normalised(M, focal, centre):
    """N = K^-1 . M . K / cbrt(det M) for M f64[..., 3, 3]: a rotation exactly when M = s . K . Q . K^-1."""
    N = np.matmul(np.matmul(_camera_inverse(focal, centre), M), camera_matrix(focal, centre))
    return N / np.cbrt(np.linalg.det(M))[..., None, None]


def focal_cost(M, focal, centre):
    """sum over the maps M f64[n,3,3] of |N - polar(N)|_F^2."""
    N = _normalised(M, focal, centre)
    return float(((N - polar(N)) ** 2).sum())


def estimate_focal(pair_maps, size, centre=None):
    """The focal length, in pixels of the resized frame of size = (w, h), under which the pair maps are closest to rotations:
    the f that minimises sum |N - polar(N)|_F^2 over the finite maps with det > 0 (N as in `rotations`, the sign of a map as
    _usable fixes it; the others are skipped, ValueError when none is left).  pair_maps: {frame_no: 3x3} as
    registration.pair_maps returns, or a sequence of matrices.
    Search: GRID_POINTS focal lengths in geometric progression from 0.25 w to 16 w, then golden-section refinement between
    the two neighbours of the best one.  Small rotations say little about f (the cost is flat in f as the angle goes to 0)."""
    w = float(size[0])
    centre = _centre(size, centre)
    M = _usable(pair_maps.values() if isinstance(pair_maps, dict) else pair_maps, centre)
    if not len(M):
        raise ValueError("no pair map with a positive determinant: nothing to estimate the focal length from")
    grid = 0.25 * w * 64.0 ** (np.arange(GRID_POINTS) / (GRID_POINTS - 1.0))
    cost = [focal_cost(M, f, centre) for f in grid]
    best = int(np.argmin(cost))
    lo, hi = grid[max(best - 1, 0)], grid[min(best + 1, GRID_POINTS - 1)]
    g = (math.sqrt(5.0) - 1.0) / 2.0
    x1, x2 = hi - g * (hi - lo), lo + g * (hi - lo)
    c1, c2 = focal_cost(M, x1, centre), focal_cost(M, x2, centre)
    for _ in range(60):
        if c1 <= c2:
            hi, x2, c2 = x2, x1, c1
            x1 = hi - g * (hi - lo)
            c1 = focal_cost(M, x1, centre)
        else:
            lo, x1, c1 = x1, x2, c2
            x2 = lo + g * (hi - lo)
            c2 = focal_cost(M, x2, centre)
    return float((lo + hi) / 2.0)


def rotations(pair_maps, focal, centre):
    """{frame_no: (Q f64[3,3] in SO(3), fit residual |N - Q|_F)}, None for a pair map that is not finite or has det <= 0.
    N = K^-1 . M . K / cbrt(det M), Q = polar(N).  M_k takes pixels of frame k to pixels of frame k-1 (registration.pair_maps),
    so Q_k takes rays of frame k to rays of frame k-1.  The residual is 0 for a camera that only rotates and has this K."""
    out = {}
    for k, M in pair_maps.items():
        m = _usable([M], centre)
        if not len(m):
            out[k] = None
            continue
        N = _normalised(m[0], float(focal), centre)
        Q = polar(N)
        out[k] = (Q, float(np.linalg.norm(N - Q)))
    return out


def superposed_rotations(pair_rotations, none_processing=True, first=None):
    """{frame_no: R f64[3,3]}: R_first = I, R_k = polar(R_{k-1} . Q_k) in the dictionary's order -- R_k takes rays of frame k to
    rays of the first frame.  pair_rotations: what `rotations` returns.  A missing pair (None) repeats the previous pair's
    rotation (none_processing, identity before the first) or takes the identity step -- the two choices of the reference's
    none_H_processing.  first: the key of the frame before the first pair (default: the first key - 1)."""
    keys = list(pair_rotations)
    if first is None:
        first = keys[0] - 1 if keys else 1
    out = {first: np.eye(3)}
    R, step = np.eye(3), np.eye(3)
    for k in keys:
        if pair_rotations[k] is not None:
            step = np.asarray(pair_rotations[k][0], np.float64)
            R = polar(np.dot(R, step))
        elif none_processing:
            R = polar(np.dot(R, step))
        out[k] = R
    return out


def _check_kind(kind):
    if kind not in KINDS:
        raise ValueError("kind must be 'cylinder', 'sphere' or 'plane'")


def surface_tables(kind, scale_px, ox, oy, dw, dh):
    """(cols f64[dw,2], rows f64[dh]) for evh_warp_ray_surface: canvas pixel (x, y) is the ray (cols[x,0], rows[y], cols[x,1]).
    cylinder: (sin t, cos t), v;  sphere: (sin t, cos t), tan p;  plane: (X, 1), Y -- with t = (x + ox) / scale_px, v or
    p = (y + oy) / scale_px, X = (x + ox) / scale_px, Y = (y + oy) / scale_px.  "sphere" refuses rows with |p| >= pi / 2."""
    _check_kind(kind)
    scale_px, dw, dh = float(scale_px), int(dw), int(dh)
    if not (scale_px > 0 and math.isfinite(scale_px)) or dw < 1 or dh < 1:
        raise ValueError("scale_px must be positive and finite, dw and dh at least 1")
    t = (np.arange(dw, dtype=np.float64) + float(int(ox))) / scale_px
    v = (np.arange(dh, dtype=np.float64) + float(int(oy))) / scale_px
    if kind == "plane":
        return np.stack([t, np.ones(dw)], axis=1), v
    cols = np.stack([np.sin(t), np.cos(t)], axis=1)
    if kind == "cylinder":
        return cols, v
    if np.abs(v).max() >= math.pi / 2:
        raise ValueError("sphere: a canvas row lies on or beyond a pole (|phi| >= pi / 2)")
    return cols, np.tan(v)


def _wrap(a):
    """a modulo 2 pi into [-pi, pi)."""
    return (np.asarray(a, np.float64) + math.pi) % (2.0 * math.pi) - math.pi


def _angles(rays, kind, what):
    """rays f64[n,3] -> (theta in [-pi, pi], v (cylinder) or phi (sphere))."""
    x, y, z = rays[:, 0], rays[:, 1], rays[:, 2]
    flat = np.hypot(x, z)
    if kind == "cylinder" and (flat < AXIS_LIMIT * np.linalg.norm(rays, axis=1)).any():
        raise ValueError("%s looks along the cylinder's axis: use the sphere" % what)
    with np.errstate(all="ignore"):
        return np.arctan2(x, z), (y / flat if kind == "cylinder" else np.arctan2(y, flat))


def _centre_thetas(R_sup):
    """{frame_no: theta of the frame's optical axis, unwrapped cumulatively along the dictionary's order}"""
    out, prev = {}, None
    for k, R in R_sup.items():
        if R is None:
            continue
        t = float(np.arctan2(R[0][2], R[2][2]))
        prev = t if prev is None else prev + float(_wrap(t - prev))
        out[k] = prev
    return out


def _frame_angles(points, R, theta_c, focal, centre, kind, what):
    """Resized-frame pixels f64[n,2] of a frame with rotation R -> (theta unwrapped relative to theta_c, v or phi)."""
    p = np.asarray(points, np.float64).reshape(-1, 2)
    rays = np.dot(np.column_stack([(p[:, 0] - centre[0]) / focal, (p[:, 1] - centre[1]) / focal, np.ones(len(p))]), np.asarray(R).T)
    t, v = _angles(rays, kind, what)
    return theta_c + _wrap(t - theta_c), v


def surface_bounds(R_sup, focal, centre, size, kind, scale=1.0, max_pixels=MAX_PIXELS):
    """(ox, oy, dw, dh, scale_px) of the canvas that holds every frame; scale_px = focal * scale canvas pixels per radian (one
    canvas pixel per frame pixel at the frame's centre for scale = 1).  R_sup: {frame_no: R or None} from superposed_rotations,
    size = (w, h) of the resized frame.  EDGE_SAMPLES points per frame edge are taken to the surface; the theta of each frame's
    optical axis is unwrapped cumulatively along the frame order and the edge points relative to their frame's axis, so a pan
    beyond 180 degrees keeps growing.  A span of 2 pi or more gives exactly round(2 pi scale_px) columns: sin and cos wrap by
    themselves.  kind "plane" is the fixed plane (stabilization.fixed_plane_bounds) and is refused here.  ValueError: no frame
    with a rotation; "cylinder" and a frame edge that meets the axis; dw * dh > max_pixels."""
    _check_kind(kind)
    if kind == "plane":
        raise ValueError("the plane's canvas is stabilization.fixed_plane_bounds'")
    focal, scale = float(focal), float(scale)
    if not (focal > 0 and math.isfinite(focal) and scale > 0 and math.isfinite(scale)):
        raise ValueError("focal and scale must be positive and finite")
    w, h = float(size[0]), float(size[1])
    centre = _centre(size, centre)
    s = np.linspace(0.0, 1.0, EDGE_SAMPLES)
    edge = np.concatenate([np.column_stack([s * w, 0 * s]), np.column_stack([s * w, 0 * s + h]),
                           np.column_stack([0 * s, s * h]), np.column_stack([0 * s + w, s * h])])
    axes = _centre_thetas(R_sup)
    if not axes:
        raise ValueError("no frame with a rotation: the surface has no extent")
    t_lo = v_lo = math.inf
    t_hi = v_hi = -math.inf
    for k, theta_c in axes.items():
        t, v = _frame_angles(edge, R_sup[k], theta_c, focal, centre, kind, "frame %s" % k)
        t_lo, t_hi, v_lo, v_hi = min(t_lo, t.min()), max(t_hi, t.max()), min(v_lo, v.min()), max(v_hi, v.max())
        for sign in (-1.0, 1.0):              # an end of the axis inside the frame: its edges do not show it
            p = sign * np.asarray(R_sup[k], np.float64)[1]                  # R^T . (0, sign, 0)
            if p[2] > 0 and 0 <= p[0] / p[2] * focal + centre[0] <= w and 0 <= p[1] / p[2] * focal + centre[1] <= h:
                if kind == "cylinder":
                    raise ValueError("frame %s looks along the cylinder's axis: use the sphere" % k)
                t_lo, t_hi = min(t_lo, theta_c - math.pi), max(t_hi, theta_c + math.pi)
                v_lo, v_hi = min(v_lo, sign * math.pi / 2.0), max(v_hi, sign * math.pi / 2.0)
    scale_px = focal * scale
    ox = int(math.floor(t_lo * scale_px))
    dw = int(math.ceil(t_hi * scale_px)) - ox + 1
    if t_hi - t_lo >= 2.0 * math.pi or dw > int(round(2.0 * math.pi * scale_px)):
        dw = max(1, int(round(2.0 * math.pi * scale_px)))
    oy, y1 = int(math.floor(v_lo * scale_px)), int(math.ceil(v_hi * scale_px))
    if kind == "sphere":                      # the rows stay inside the poles
        pole = int(math.ceil(math.pi / 2.0 * scale_px)) - 1
        oy, y1 = max(oy, -pole), min(y1, pole)
    dh = y1 - oy + 1
    if dw * dh > int(max_pixels):
        raise ValueError("the surface is %d x %d pixels, more than max_pixels = %d" % (dw, dh, int(max_pixels)))
    return ox, oy, dw, dh, scale_px


def frame_matrix(R_k, focal, centre, frame_size, resized_size):
    """f64[9], D . K . R_k^T: a ray of the fixed surface -> homogeneous pixels of the full-size frame, what evh_warp_ray_surface
    takes as d_A.  K is the camera of the resized frame (resized_size = (w, h)), D = diag(frame_w / w, frame_h / h, 1) takes
    resized pixels to pixels of the frame as it is decoded (frame_size = (frame_w, frame_h))."""
    D = np.diag([float(frame_size[0]) / float(resized_size[0]), float(frame_size[1]) / float(resized_size[1]), 1.0])
    return np.dot(np.dot(D, camera_matrix(float(focal), _centre(resized_size, centre))), np.asarray(R_k, np.float64).T).reshape(9)


SurfaceModel = collections.namedtuple("SurfaceModel", "kind focal estimated centre pair_rotations rotations bounds")


def surface_model(superposition_homography_dict, resize_info, surface="cylinder", focal=None, scale=1.0, max_pixels=MAX_PIXELS,
                  none_processing=True):
    """Everything surface_frames derives from the dictionary, on the host: SurfaceModel(kind, focal, estimated -- whether the
    focal length was estimated --, centre, pair_rotations {frame_no: (Q, residual) or None}, rotations {frame_no: R},
    bounds (ox, oy, dw, dh, scale_px))."""
    size = (int(resize_info["w"]), int(resize_info["h"]))
    centre = _centre(size, None)
    maps = pair_maps(superposition_homography_dict)
    estimated = focal is None
    focal = estimate_focal(maps, size, centre) if estimated else float(focal)
    pairs = rotations(maps, focal, centre)
    keys = _frames_of(superposition_homography_dict)
    R_sup = superposed_rotations(pairs, none_processing, first=keys[0] if keys else None)
    bounds = surface_bounds(R_sup, focal, centre, size, surface, scale, max_pixels)
    return SurfaceModel(surface, focal, estimated, centre, pairs, R_sup, bounds)


def surface_report(model):
    """A SurfaceModel as plain data (what stabilize --surface writes to surface_report.json): the focal length and whether it
    was estimated, the fit residual |N - Q|_F of every pair (None: the pair had no usable matrix) with its median, the canvas."""
    residual = {str(k): (None if v is None else v[1]) for k, v in model.pair_rotations.items()}
    known = [r for r in residual.values() if r is not None]
    ox, oy, dw, dh, scale_px = model.bounds
    return {"surface": model.kind, "focal": model.focal, "focal_estimated": bool(model.estimated), "centre": list(model.centre),
            "fit_residual": residual, "fit_residual_median": float(np.median(known)) if known else None,
            "canvas": {"ox": ox, "oy": oy, "dw": dw, "dh": dh, "scale_px": scale_px,
                       "closed": dw == int(round(2.0 * math.pi * scale_px))}}


def _check_surface_arguments(surface, focal, mode, scale, ingest):
    if surface == "plane":
        raise ValueError("surface='plane' is stabilization.stabilized_frames: the fixed plane has its own driver")
    if surface not in ("cylinder", "sphere"):
        raise ValueError("surface must be 'cylinder' or 'sphere'")
    if mode not in WARP_MODES:
        raise ValueError("mode must be 'each', 'history' or 'mosaic'")
    if focal is not None and not (isinstance(focal, (int, float)) and focal > 0 and math.isfinite(focal)):
        raise ValueError("focal must be a positive number of pixels, or None to estimate it")
    if not (isinstance(scale, (int, float)) and scale > 0 and math.isfinite(scale)):
        raise ValueError("scale must be positive and finite")
    check_ingest(ingest)


def surface_frames(capture, superposition_homography_dict, resize_info, surface="cylinder", focal=None, mode="history", scale=1.0,
                   chunk_frames=32, ingest="auto", max_pixels=MAX_PIXELS, none_processing=True):
    """Generator of (frame_no, uint8 ndarray [dh,dw,3]): the frames of `capture` placed on the fixed cylinder or sphere on the
    device (evh_warp_ray_surface), in the mould of stabilization.stabilized_frames -- mode, chunk_frames, ingest and the canvas
    carried on the device between chunks as there.  focal: pixels of the resized frame, None = estimate_focal.  scale: canvas
    pixels per frame pixel at a frame's centre.  none_processing: see superposed_rotations.  A frame without a rotation (beyond
    the dictionary) leaves the canvas as it was.  The geometry is surface_model's.  Bad keywords are refused when the function
    is called, before the dictionary is read and the capture is touched; surface="plane" is refused: that is stabilized_frames."""
    _check_surface_arguments(surface, focal, mode, scale, ingest)
    return _surface_frames(capture, superposition_homography_dict, resize_info, surface, focal, mode, scale, chunk_frames, ingest,
                           max_pixels, none_processing)


def surface_jpegs(capture, superposition_homography_dict, resize_info, surface="cylinder", focal=None, mode="history", scale=1.0,
                  chunk_frames=32, ingest="auto", max_pixels=MAX_PIXELS, none_processing=True, quality=90, subsampling="420"):
    """Generator of (frame_no, bytes): the pictures of surface_frames -- same arguments, same canvases -- as baseline JPEG files
    (quality 1..100, subsampling "420" or "444") encoded on the device where the chunk's canvases lie (evh_jpeg_encode): no
    canvas is downloaded, only the files."""
    from .pictures import check_format, jpegs_of_chunks
    _check_surface_arguments(surface, focal, mode, scale, ingest)
    check_format(quality, subsampling)
    return jpegs_of_chunks(_surface_chunks(capture, superposition_homography_dict, resize_info, surface, focal, mode, scale,
                                           chunk_frames, ingest, max_pixels, none_processing), mode == "mosaic", quality, subsampling)


def _surface_chunks(capture, superposition_homography_dict, resize_info, surface, focal, mode, scale, chunk_frames, ingest,
                    max_pixels, none_processing):
    """The chunks behind surface_frames and surface_jpegs: _canvas_chunks with the surface's geometry and entry."""
    import torch
    model = surface_model(superposition_homography_dict, resize_info, surface, focal, scale, max_pixels, none_processing)
    ox, oy, dw, dh, scale_px = model.bounds
    size = (int(resize_info["w"]), int(resize_info["h"]))
    nan = np.full(9, np.nan)

    def setup(w0, h0):
        dev = runtime.device()
        cols, rows = (torch.from_numpy(t).to(dev) for t in surface_tables(surface, scale_px, ox, oy, dw, dh))

        def paint(ctx, frame_no, n, src, src_size, out, canvas):
            mats = [model.rotations.get(frame_no + 1 + k) for k in range(n)]
            mats = np.stack([nan if R is None else frame_matrix(R, model.focal, model.centre, (w0, h0), size) for R in mats])
            mats = torch.from_numpy(mats).to(dev)
            if out is None:
                ctx.warp_ray_surface(src, mats, cols, rows, canvas, mode, background=canvas, size=src_size)
                ctx.order_torch_after()
                return
            ctx.warp_ray_surface(src, mats, cols, rows, out, mode, background=canvas if mode == "history" else None, size=src_size)
            ctx.order_torch_after()
            if mode == "history":
                canvas.copy_(out[n - 1])
        return dw, dh, None, paint

    return _canvas_chunks(capture, mode, chunk_frames, ingest, setup)


def _surface_frames(capture, superposition_homography_dict, resize_info, surface, focal, mode, scale, chunk_frames, ingest,
                    max_pixels, none_processing):
    frame_no = 0
    for first, n, pictures, _, canvas in _surface_chunks(capture, superposition_homography_dict, resize_info, surface, focal, mode,
                                                         scale, chunk_frames, ingest, max_pixels, none_processing):
        frame_no = first + n - 1
        if pictures is not None:
            pictures = pictures.cpu().numpy()
            for k in range(n):
                yield first + k, pictures[k]
    if WARP_MODES[mode] == WARP_MOSAIC:
        yield frame_no, canvas.cpu().numpy()


def surface_coordinates(points, frame_no, R_sup, focal, centre, kind, scale=1.0):
    """Pixels f64[n,2] of the resized frame `frame_no` -> f64[n,2] surface coordinates (scale_px theta, scale_px v) (cylinder)
    or (scale_px theta, scale_px phi) (sphere), scale_px = focal * scale: the object coordinates the reference exists to
    produce, on a surface where every viewing direction has a place -- defined also where fixed_coordinate_system answers n/a.
    theta is unwrapped as in surface_bounds, so a pan beyond a full turn keeps counting; the canvas column of a coordinate X
    is X - ox, modulo dw on a canvas that closes.  ValueError for a frame without a rotation and, on the cylinder, for a point
    on its axis."""
    if kind not in ("cylinder", "sphere"):
        raise ValueError("kind must be 'cylinder' or 'sphere'")
    axes = _centre_thetas(R_sup)
    if frame_no not in axes:
        raise ValueError("frame %s has no rotation" % frame_no)
    scale_px = float(focal) * float(scale)
    t, v = _frame_angles(points, R_sup[frame_no], axes[frame_no], float(focal), centre, kind, "a point of frame %s" % frame_no)
    return np.column_stack([t * scale_px, v * scale_px])


def surface_to_frame(coordinates, frame_no, R_sup, focal, centre, kind, scale=1.0):
    """The inverse of surface_coordinates: surface coordinates f64[n,2] -> pixels f64[n,2] of the resized frame `frame_no`; NaN
    for a direction behind that frame's camera."""
    if kind not in ("cylinder", "sphere"):
        raise ValueError("kind must be 'cylinder' or 'sphere'")
    R = R_sup.get(frame_no)
    if R is None:
        raise ValueError("frame %s has no rotation" % frame_no)
    scale_px = float(focal) * float(scale)
    c = np.asarray(coordinates, np.float64).reshape(-1, 2) / scale_px
    rays = np.column_stack([np.sin(c[:, 0]), c[:, 1] if kind == "cylinder" else np.tan(c[:, 1]), np.cos(c[:, 0])])
    p = np.dot(rays, np.asarray(R, np.float64))            # rows: R^T . ray
    with np.errstate(all="ignore"):
        out = np.column_stack([p[:, 0] / p[:, 2] * float(focal) + centre[0], p[:, 1] / p[:, 2] * float(focal) + centre[1]])
    out[~(p[:, 2] > 0)] = np.nan
    return out
