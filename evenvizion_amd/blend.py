"""The blended mosaic: feathered seams and exposure gains.

stabilized_frames(mode="mosaic") gives every canvas pixel to the last frame that covers it: every frame edge stays as a seam and
every change of the camera's auto-exposure as a step in brightness.  Here the covering frames are reduced on the device
(evh_blend_fixed_plane / evh_blend_ray_surface, include/evhip.h states the arithmetic): "feather" is the mean weighted by each
sample's distance to its frame's nearest edge, cut at the feather width -- a frame fades out towards its border --, "seam" keeps
per pixel the frame whose border is farthest away.  Exposure: evh_pair_exposure sums, for pairs of frames one to sixteen frames
apart, the pixels both see; solve_gains turns the sums into one gain per frame and channel (Brown and Lowe's gain compensation:
overlapping means should agree, gains should stay near 1), a small linear system solved on the host in float64.

    pairs, stats = exposure_stats(capture, sup, resize_info)
    gains = solve_gains(pairs, stats, n_frames)
    canvas = blended_mosaic(capture_again, sup, resize_info, gains=gains)

blend="bands" is multi-band blending (Burt and Adelson; evh_blend_bands_*): seam_labels gives every canvas pixel to the frame
"seam" would take, from the matrices alone, and the Laplacian pyramids of the frames are blended under the Gaussian pyramids of
that label mask -- exposure steps fade over a wide zone, detail changes hands over a narrow one.

Not done here: seam finding by graph cut (the label mask is where one would write), vignetting.
"""
import math

import numpy as np

from . import runtime
from .frames import DeviceLadder, FrameReader, check_ingest, entry_matrix

MAX_SOLVE_FRAMES = 4096        # solve_gains forms the normal equations densely: n x n float64
Q12 = 4096                     # a gain of 1.0 in evh_blend_*'s d_gain
MAX_FEATHER_PX = 65535 / 32.0
MAX_BANDS = 8                  # evh_blend_bands_*: levels 0..8
MAX_LABEL = 65534              # 65535 is "nobody" in a label mask
LABEL_CHUNK = 1024             # matrices per evh_seam_labels_* call


def _whole(value, lo, name):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or int(value) < lo:
        raise ValueError("%s must be an integer of at least %d" % (name, lo))
    return int(value)


def _strides(strides):
    out = tuple(_whole(s, 1, "a stride") for s in strides)
    if len(set(out)) != len(out):
        raise ValueError("strides must not repeat")
    return out


def exposure_pairs(n_frames, strides=(1, 4, 16)):
    """[(k, k + s)] for every stride s and every k with k + s < n_frames, stride by stride: neighbours tie the chain together,
    the longer strides keep its drift down.  Frames are numbered from 0 in the order they are read."""
    n = _whole(n_frames, 0, "n_frames")
    return [(k, k + s) for s in _strides(strides) for k in range(n - s)]


def _host_pair_map(S_i, S_j):
    """S_j^-1 . S_i: pixels of frame i -> pixels of frame j"""
    from .registration import _pair_map
    return _pair_map(S_j, S_i)


def exposure_stats(capture, superposition_homography_dict, resize_info, strides=(1, 4, 16), step=2, lo=8, hi=247, chunk_frames=32,
                   ingest="auto", maps=None):
    """-> (pairs, stats): exposure_pairs of the frames read, and int64[npairs,7] = (pixels, sum a per channel, sum b per channel)
    per pair (evh_pair_exposure): over every step-th pixel of frame i in both directions that frame j covers under the pair's
    map, with all bytes of both inside [lo, hi].  The i-th frame read goes with the i-th entry of the dictionary and is taken to
    the size of resize_info; the map of (i, j) is S_j^-1 . S_i in float64 on the host (NaN, a pair that counts nothing, where an
    entry is missing or singular), or maps[(i, j)] where `maps` is given (a dictionary of 3x3 matrices, pixels of resized frame
    i -> pixels of resized frame j: K . R_j^T . R_i . K^-1 for a surface).  Chunks overlap by the largest stride, so that
    every pair lies inside one."""
    import torch
    check_ingest(ingest)
    strides = _strides(strides)
    step, lo, hi = _whole(step, 1, "step"), _whole(lo, 0, "lo"), _whole(hi, 0, "hi")
    if step > 64 or hi > 255 or lo > hi:
        raise ValueError("step lies in 1..64, lo <= hi in 0..255")
    w, h = int(resize_info["w"]), int(resize_info["h"])
    if w < 1 or h < 1:
        raise ValueError("resize_info must hold a positive w and h")
    S = [entry_matrix(v) for k, v in superposition_homography_dict.items() if k != "resize_info"]
    reach = max(strides) if strides else 0
    chunk = max(_whole(chunk_frames, 1, "chunk_frames"), reach + 1)
    nan = np.full((3, 3), np.nan)
    done_pairs, done_stats = [], []
    if len(S) < 2 or not strides:
        return [], np.zeros((0, 7), np.int64)
    reader = FrameReader(capture, ingest)
    ctx = runtime.get_context(64, 64)             # the entry works on caller buffers of any size
    dev = runtime.device()
    ladder = DeviceLadder(dev, chunk, reader.planes, (reader.w0, reader.h0), (w, h), bgr=True, gray3=True)
    seen = 0                                      # frames [0, seen) lay in earlier chunks: their pairs are done
    for start, frames in reader.chunks(chunk, reach, len(S)):
        n = len(frames)
        mine = [(i, i + s) for s in strides for i in range(start, start + n - s) if i + s >= seen]
        seen = start + n
        if not mine:
            continue
        _, src, _ = ladder(ctx, torch.from_numpy(frames).to(dev))
        M = np.stack([(maps.get((i, j), nan) if maps is not None else _host_pair_map(S[i], S[j])) for i, j in mine])
        local = np.array([(i - start, j - start) for i, j in mine], np.int32)
        got = ctx.pair_exposure(src, torch.from_numpy(local).to(dev), torch.from_numpy(np.asarray(M, np.float64).reshape(-1, 9)).to(dev),
                                step=step, lo=lo, hi=hi)
        ctx.order_torch_after()
        done_pairs += mine
        done_stats.append(got.cpu().numpy())
    rank = {s: r for r, s in enumerate(strides)}
    order = sorted(range(len(done_pairs)), key=lambda p: (rank[done_pairs[p][1] - done_pairs[p][0]], done_pairs[p][0]))
    stats = np.concatenate(done_stats) if done_stats else np.zeros((0, 7), np.int64)
    return [done_pairs[p] for p in order], stats[order]


def surface_pair_maps(model, keys, pairs):
    """{(i, j): K . R_j^T . R_i . K^-1} for exposure_stats(maps=): the pairs of a camera that only rotates, from a
    surface.SurfaceModel.  keys: the dictionary's frame numbers in order (pair indices are positions in it)."""
    from .surface import camera_matrix
    K = camera_matrix(model.focal, model.centre)
    Kinv = np.linalg.inv(K)
    out = {}
    for i, j in pairs:
        Ri, Rj = model.rotations.get(keys[i]), model.rotations.get(keys[j])
        if Ri is not None and Rj is not None:
            out[(i, j)] = np.dot(np.dot(K, np.dot(np.asarray(Rj).T, Ri)), Kinv)
    return out


def solve_gains(pairs, stats, n_frames, sigma_n=10.0, sigma_g=0.1, min_pixels=64, per_channel=True):
    """float64[n_frames,3]: per channel the gains g that minimise
        sum_p N_p * [(g_i abar_p - g_j bbar_p)^2 / sigma_n^2 + ((1 - g_i)^2 + (1 - g_j)^2) / sigma_g^2],
    abar = sum a / N, bbar = sum b / N of pair p = (i, j) (exposure_stats' rows) -- Brown and Lowe's gain compensation -- by the
    normal equations and numpy.linalg.solve.  Pairs with fewer than min_pixels pixels are dropped; a frame in no pair gets gain
    1.  per_channel=False: one gain per frame from the means over the channels, repeated three times.  More than 4096 frames
    are refused: the system is formed densely."""
    n = _whole(n_frames, 0, "n_frames")
    if n > MAX_SOLVE_FRAMES:
        raise ValueError("solve_gains forms an n x n system: more than %d frames are refused (solve a subsampled chain)" % MAX_SOLVE_FRAMES)
    if not (sigma_n > 0 and sigma_g > 0 and math.isfinite(sigma_n) and math.isfinite(sigma_g)):
        raise ValueError("sigma_n and sigma_g must be positive and finite")
    stats = np.asarray(stats).reshape(-1, 7)
    if len(stats) != len(pairs):
        raise ValueError("one row of stats per pair")
    for i, j in pairs:
        if not (0 <= i < n and 0 <= j < n):
            raise ValueError("a pair names a frame outside 0..n_frames-1")
    N = stats[:, 0].astype(np.float64)
    keep = (N >= float(min_pixels)) & (N > 0)
    safe = np.where(N > 0, N, 1.0)
    a, b = stats[:, 1:4].astype(np.float64) / safe[:, None], stats[:, 4:7].astype(np.float64) / safe[:, None]
    if not per_channel:
        colour = 3 if stats[:, [2, 3, 5, 6]].any() else 1
        a = np.repeat(a.sum(axis=1, keepdims=True) / colour, 3, axis=1)
        b = np.repeat(b.sum(axis=1, keepdims=True) / colour, 3, axis=1)
    gains = np.ones((n, 3), np.float64)
    wn, wg = 1.0 / (sigma_n * sigma_n), 1.0 / (sigma_g * sigma_g)
    for c in range(3 if per_channel else 1):
        A, rhs = np.zeros((n, n), np.float64), np.zeros(n, np.float64)
        for p, (i, j) in enumerate(pairs):
            if not keep[p]:
                continue
            A[i, i] += N[p] * (a[p, c] * a[p, c] * wn + wg)
            A[j, j] += N[p] * (b[p, c] * b[p, c] * wn + wg)
            A[i, j] -= N[p] * a[p, c] * b[p, c] * wn
            A[j, i] -= N[p] * a[p, c] * b[p, c] * wn
            rhs[i] += N[p] * wg
            rhs[j] += N[p] * wg
        alone = np.diag(A) == 0
        A[alone, alone] = 1.0
        rhs[alone] = 1.0
        if n:
            gains[:, c] = np.linalg.solve(A, rhs)
    if not per_channel:
        gains[:, 1] = gains[:, 2] = gains[:, 0]
    return gains


def quantise_gains(g):
    """float gains -> uint16 Q12 as evh_blend_* takes them: clip(rint(g * 4096), 1, 65535).  Gains are positive: 0 would erase a
    frame, so the smallest value kept is 1 / 4096; above 16 the format ends."""
    return np.clip(np.rint(np.asarray(g, np.float64) * Q12), 1, 65535).astype(np.uint16)


def _check_mosaic(blend, feather_px, gains, placement, scale, surface, focal, chunk_frames, ingest, bands=5):
    from ._lib import BLEND_MODES
    from .stabilization import check_placement
    if blend not in BLEND_MODES and blend != "bands":
        raise ValueError("blend must be 'feather', 'seam' or 'bands'")
    if isinstance(bands, (bool, np.bool_)) or not isinstance(bands, (int, np.integer)) or not 0 <= int(bands) <= MAX_BANDS:
        raise ValueError("bands must be an integer in 0..%d" % MAX_BANDS)
    if isinstance(feather_px, bool) or not isinstance(feather_px, (int, float)) or not 0 <= feather_px <= MAX_FEATHER_PX:
        raise ValueError("feather_px must lie in 0..%g" % MAX_FEATHER_PX)
    check_placement(placement)
    if surface not in (None, "plane", "cylinder", "sphere"):
        raise ValueError("surface must be None, 'plane', 'cylinder' or 'sphere'")
    on_surface = surface in ("cylinder", "sphere")
    if on_surface and placement != "warp":
        raise ValueError("a surface takes the full-size frames: placement must be 'warp'")
    if focal is not None and not on_surface:
        raise ValueError("focal needs surface='cylinder' or 'sphere'")
    if focal is not None and not (isinstance(focal, (int, float)) and focal > 0 and math.isfinite(focal)):
        raise ValueError("focal must be a positive number of pixels, or None to estimate it")
    if not (isinstance(scale, (int, float)) and scale > 0 and math.isfinite(scale)):
        raise ValueError("scale must be positive and finite")
    _whole(chunk_frames, 1, "chunk_frames")
    check_ingest(ingest)
    if gains is not None:
        gains = np.asarray(gains, np.float64)
        if gains.ndim != 2 or gains.shape[1] != 3 or not np.isfinite(gains).all() or (gains <= 0).any():
            raise ValueError("gains must be positive finite numbers [n_frames,3]")
        gains = quantise_gains(gains)
    return on_surface, int(round(float(feather_px) * 32)), gains


def _geometry(superposition_homography_dict, resize_info, on_surface, surface, focal, placement, scale, w0, h0):
    """Where the frames of a w0 x h0 video go: (dw, dh, the size the frames are resized to or None, matrix_of(frame_no) -> f64[9],
    origin (ox, oy) or None, the ray tables (cols, rows) as numpy or None)."""
    from .stabilization import _placement, MAX_PIXELS
    if on_surface:
        from .surface import frame_matrix, surface_model, surface_tables
        size = (int(resize_info["w"]), int(resize_info["h"]))
        model = surface_model(superposition_homography_dict, resize_info, surface, focal, scale, MAX_PIXELS)
        ox, oy, dw, dh, scale_px = model.bounds
        nan = np.full(9, np.nan)

        def matrix_of(frame_no):
            R = model.rotations.get(frame_no)
            return nan if R is None else frame_matrix(R, model.focal, model.centre, (w0, h0), size)
        return dw, dh, None, matrix_of, None, surface_tables(surface, scale_px, ox, oy, dw, dh)
    ox, oy, dw, dh, matrix_of = _placement(superposition_homography_dict, resize_info, placement, scale, w0, h0, MAX_PIXELS)
    resize_to = (int(resize_info["w"]), int(resize_info["h"])) if placement == "translate" else None
    return dw, dh, resize_to, matrix_of, (ox, oy), None


def _last_frame(superposition_homography_dict):
    keys = [int(k) for k in superposition_homography_dict if k != "resize_info"]
    last = max(keys) if keys else 0
    if last - 1 > MAX_LABEL:
        raise ValueError("a label mask names at most %d frames" % (MAX_LABEL + 1))
    return last


def _device_labels(ctx, dev, n_frames, frame_size, dw, dh, matrix_of, origin, tables, feather):
    """uint16 [dh,dw] on the device: frame number f (from 1) carries label f - 1; the matrices go LABEL_CHUNK at a time, the
    state carried."""
    import torch
    best, label = None, None
    for first in range(0, max(n_frames, 1), LABEL_CHUNK):
        n = max(0, min(LABEL_CHUNK, n_frames - first))
        mats = torch.from_numpy(np.stack([matrix_of(first + 1 + k) for k in range(n)]).reshape(n, 9) if n else np.zeros((0, 9))).to(dev)
        kw = dict(feather=feather, first_label=first, best=best, label=label, state_in=best is not None)
        if tables is None:
            best, label = ctx.seam_labels_fixed_plane(mats, frame_size, origin, (dh, dw), **kw)
        else:
            best, label = ctx.seam_labels_ray_surface(mats, frame_size, tables[0], tables[1], **kw)
        ctx.order_torch_after()        # `mats` is dropped at the next turn: torch may hand its memory out again only behind the call
    return label


def seam_labels(superposition_homography_dict, resize_info, frame_size, feather_px=32, placement="warp", scale=1.0, surface=None,
                focal=None):
    """uint16 [dh,dw]: which frame "seam" gives every pixel of blended_mosaic's canvas to, from the matrices alone -- no video is
    read (evh_seam_labels_*).  The i-th frame read carries label i (from 0), 65535 is a pixel no frame covers.  frame_size: (w, h)
    of the video's frames; everything else as for blended_mosaic."""
    import torch
    on_surface, feather, _ = _check_mosaic("seam", feather_px, None, placement, scale, surface, focal, 1, "auto")
    w0, h0 = _whole(frame_size[0], 1, "frame_size"), _whole(frame_size[1], 1, "frame_size")
    n_frames = _last_frame(superposition_homography_dict)
    dw, dh, resize_to, matrix_of, origin, tables = _geometry(superposition_homography_dict, resize_info, on_surface, surface, focal,
                                                             placement, scale, w0, h0)
    ctx = runtime.get_context(64, 64)
    dev = runtime.device()
    if tables is not None:
        tables = tuple(torch.from_numpy(t).to(dev) for t in tables)
    label = _device_labels(ctx, dev, n_frames, resize_to or (w0, h0), dw, dh, matrix_of, origin, tables, feather)
    return label.cpu().numpy()


class CanvasPainter:
    """A blended canvas that grows group by group, with its coverage: what registration.anchor_superposition aligns frames
    against.  picture: uint8 [dh,dw,3], the blend of everything painted so far (evh_blend_fixed_plane's d_out, the state d_acc
    carried from call to call, no gains); cover: uint8 [dh,dw], 255 where a frame has been painted, 0 elsewhere
    (evh_warp_fixed_plane in mode "mosaic" on frames of 255s with the same matrices over the cover itself: blend and warp share
    one coverage rule, so cover >= 1 is exactly "the picture holds a blended sample here").  No pixel is touched by torch."""

    def __init__(self, dev, dw, dh, blend="feather", feather=1024):
        import torch
        self.blend, self.feather = blend, int(feather)
        self.acc = torch.zeros((dh, dw, 4), dtype=torch.int64, device=dev)
        self.picture = torch.zeros((dh, dw, 3), dtype=torch.uint8, device=dev)
        self.cover = torch.zeros((dh, dw), dtype=torch.uint8, device=dev)
        self.ones, self.carried = None, False

    def paint(self, ctx, src, mats):
        """src: CUDA uint8 [n,h,w,3]; mats: CUDA float64 [n,9], frame pixel -> canvas pixel (NaN: the frame is left out)."""
        import torch
        n, h, w = src.shape[:3]
        if self.ones is None or self.ones.shape[0] < n or tuple(self.ones.shape[1:]) != (h, w):
            self.ones = torch.full((n, h, w), 255, dtype=torch.uint8, device=src.device)
        ctx.blend_fixed_plane(src, mats, (0, 0), out=self.picture, mode=self.blend, feather=self.feather, acc=self.acc,
                              acc_in=self.carried)
        ctx.warp_fixed_plane(self.ones[:n], mats, self.cover, "mosaic", (0, 0), background=self.cover)
        self.carried = True


def blended_mosaic(capture, superposition_homography_dict, resize_info, blend="feather", feather_px=32, gains=None,
                   placement="warp", scale=1.0, surface=None, focal=None, chunk_frames=32, ingest="auto", bands=5):
    """uint8 [dh,dw,3]: all frames of `capture` blended into one canvas on the device, the state carried from chunk to chunk.
    blend "feather": the weighted mean, weights rising over feather_px pixels from a frame's border; "seam": per pixel the frame
    whose border is farthest away; "bands": multi-band blending with pyramid levels 0..bands under the label mask of "seam"
    (seam_labels; first the labels from the matrices, then the frames).  gains: float [n_frames,3] (solve_gains), row i for the
    i-th frame read, or None; frames past its end get 1.  The canvas is the fixed plane's (placement, scale as in
    stabilization.stabilized_frames) or, with surface "cylinder" / "sphere", surface.surface_model's (focal as there).  Bad
    arguments are refused before the capture is touched."""
    import torch
    from .stabilization import _canvas_chunks
    on_surface, feather, q = _check_mosaic(blend, feather_px, gains, placement, scale, surface, focal, chunk_frames, ingest, bands)
    n_frames = _last_frame(superposition_homography_dict) if blend == "bands" else 0
    state = {}

    def chunk_gains(dev, frame_no, n):
        if q is None:
            return None
        g = np.full((n, 3), Q12, np.uint16)
        have = q[frame_no:frame_no + n]
        g[:len(have)] = have
        return torch.from_numpy(g).to(dev)

    def setup(w0, h0):
        dev = runtime.device()
        dw, dh, resize_to, matrix_of, origin, tables = _geometry(superposition_homography_dict, resize_info, on_surface, surface,
                                                                 focal, placement, scale, w0, h0)
        if tables is not None:
            cols, rows = (torch.from_numpy(t).to(dev) for t in tables)
        if blend == "bands":
            from ._lib import bands_state_elems
            ctx = runtime.get_context(64, 64)
            label = _device_labels(ctx, dev, n_frames, resize_to or (w0, h0), dw, dh, matrix_of, origin,
                                   None if tables is None else (cols, rows), feather)
            acc = torch.zeros(bands_state_elems(dw, dh, 3, int(bands)), dtype=torch.int64, device=dev)
        else:
            acc = torch.zeros((dh, dw, 4), dtype=torch.int64, device=dev)

        def paint(ctx, frame_no, n, src, size, out, canvas):
            mats = torch.from_numpy(np.stack([matrix_of(frame_no + 1 + k) for k in range(n)])).to(dev)
            if blend == "bands":
                # a frame past the last label owns no pixel: it adds nothing, and its label may not be named
                n = max(0, min(n, MAX_LABEL + 1 - frame_no))
                if n == 0 and state:
                    return
                common = dict(label=label, levels=int(bands), first_label=frame_no, out=canvas, gains=chunk_gains(dev, frame_no, n),
                              state=acc, state_in=bool(state), size=size)
                src = tuple(p[:n] for p in src) if isinstance(src, (tuple, list)) else src[:n]
                if on_surface:
                    ctx.blend_bands_ray_surface(src, mats[:n], cols, rows, **common)
                else:
                    ctx.blend_bands_fixed_plane(src, mats[:n], origin, **common)
            else:
                common = dict(out=canvas, mode=blend, feather=feather, gains=chunk_gains(dev, frame_no, n), acc=acc,
                              acc_in=bool(state), size=size)
                if on_surface:
                    ctx.blend_ray_surface(src, mats, cols, rows, **common)
                else:
                    ctx.blend_fixed_plane(src, mats, origin, **common)
            ctx.order_torch_after()
            state["carried"] = True
        return dw, dh, resize_to, paint

    canvas = None
    for _, _, _, _, canvas in _canvas_chunks(capture, "mosaic", int(chunk_frames), ingest, setup):
        pass
    if canvas is None:
        raise ValueError("Problem with video! Can't read first frame")
    return canvas.cpu().numpy()
