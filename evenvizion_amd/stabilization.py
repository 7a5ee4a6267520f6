"""Stabilised view -- the geometry of evenvizion/visualization/stabilization.py:100-290 with the frames kept on the device.

The reference shows a frame "in the fixed coordinate system" by pasting the resized frame at int(H_sup . (0, 0, 1)) onto a
canvas that accumulates the frames (stabilize_view, :129-172), i.e. it only translates.  Here a frame is placed by
evh_warp_fixed_plane (include/evhip.h), either way:

    placement="translate"   the reference's paste, byte for byte: the frame resized on the device (evh_resize_area_u8), the
                            reference's canvas (get_reference_system / initialize_background, :100-126, :241-249);
    placement="warp"        the projective warp of the full-size frame through diag(s,s,1) . H_sup . diag(kx,ky,1).

stabilized_frames yields the canvases as arrays.  With trail=True they are the reference's picture of the fixed plane:
earlier frames fade out behind the current one (the HSV dimming of decrease_brightness) and the current frame sits in its
white rectangle (change_frame_location), both by evh_trail_fixed_plane; comparison_frames sets the original beside it inside
the red canvas border, as create_video_comparison does.  The two words of text ("Original",
"EvenVizion") are not drawn: no Hershey glyph table is at hand.  The colour conversions are restated arithmetic, not
cv2.cvtColor compared byte for byte (include/evhip.h says what is claimed).

background_plate takes the registered frames one step further than the reference goes: their per-pixel temporal median is the
scene without what moves through it, and each frame's difference from it a moving-object mask (evh_plate_fixed_plane,
DESIGN.md section 16).
"""
import collections
import math

import numpy as np

from . import runtime
from ._lib import PLATE_MAX_FRAMES, WARP_MODES, WARP_MOSAIC
from .frames import DeviceLadder, FrameReader, check_ingest, entry_matrix

MAX_PIXELS = 1 << 26          # canvas pixels fixed_plane_bounds accepts by default (201 MB of BGR)
CHUNK_BYTES = 512 << 20       # cap of the canvases of one "each" / "history" chunk on the device


def _frames_of(superposition_homography_dict):
    return [k for k in superposition_homography_dict if k != "resize_info"]


def _matrix(H):
    """A frame's matrix as f64[3,3], or None when it has none or it is not finite."""
    m = entry_matrix(H)
    return m if np.all(np.isfinite(m)) else None


def get_reference_system(superposition_homography_dict):
    """{"max_x", "min_x", "max_y", "min_y"} of the frames' upper left corners in the fixed plane, truncated with int() as the
    reference does (stabilization.py:100-126)."""
    x_corner, y_corner = [], []
    for k in _frames_of(superposition_homography_dict):
        v = np.dot(np.asarray(superposition_homography_dict[k], np.float64), [0, 0, 1])
        v = v[:-1] / v[-1]
        x_corner.append(v[0])
        y_corner.append(v[1])
    return {"max_x": int(np.max(x_corner)), "min_x": int(np.min(x_corner)),
            "max_y": int(np.max(y_corner)), "min_y": int(np.min(y_corner))}


def panorama_shape(corner_dict, frame_shape):
    """[h, w] of the reference's canvas for resized frames of frame_shape = (h, w, ...) (stabilization.py:241-244)."""
    return [int(np.abs(corner_dict["min_y"]) + corner_dict["max_y"] + frame_shape[0] + 10),
            int(np.abs(corner_dict["min_x"]) + corner_dict["max_x"] + frame_shape[1] + 10)]


def translate_offset(H):
    """(x_offset, y_offset) of stabilize_view (stabilization.py:159-161): int() of H . (0, 0, 1) after the division."""
    v = np.dot(np.asarray(H, np.float64), [0, 0, 1])
    return int(v[0] / v[2]), int(v[1] / v[2])


def fixed_plane_bounds(superposition_homography_dict, resize_info, scale=1.0, max_pixels=MAX_PIXELS):
    """(ox, oy, dw, dh) of the canvas that holds every warped frame: floor and ceiling of the four corners (0, 0), (w, 0),
    (0, h), (w, h) of the resized frame, times `scale`, under every finite matrix of the dictionary; canvas pixel (x, y) is
    the plane point (x + ox, y + oy).  ValueError when no matrix is finite, a corner lies on or behind a frame's horizon,
    or dw * dh exceeds max_pixels."""
    w, h = float(resize_info["w"]), float(resize_info["h"])
    corners = np.array([[0, 0, 1], [w, 0, 1], [0, h, 1], [w, h, 1]], np.float64).T
    lo, hi = np.array([np.inf, np.inf]), np.array([-np.inf, -np.inf])
    for k in _frames_of(superposition_homography_dict):
        m = _matrix(superposition_homography_dict[k])
        if m is None:
            continue
        with np.errstate(all="ignore"):
            p = np.dot(m, corners)
            if not (np.all(p[2] > 0) or np.all(p[2] < 0)):
                raise ValueError("frame %s: the horizon of its matrix crosses the frame, its picture in the plane is unbounded" % k)
            xy = p[:2] / p[2] * float(scale)
        lo, hi = np.minimum(lo, xy.min(axis=1)), np.maximum(hi, xy.max(axis=1))
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))):
        raise ValueError("no frame with a finite matrix: the fixed plane has no extent")
    ox, oy = int(math.floor(lo[0])), int(math.floor(lo[1]))
    dw, dh = int(math.ceil(hi[0])) - ox + 1, int(math.ceil(hi[1])) - oy + 1
    if dw * dh > int(max_pixels):
        raise ValueError("the fixed plane is %d x %d pixels, more than max_pixels = %d" % (dw, dh, int(max_pixels)))
    return ox, oy, dw, dh


def check_placement(placement):
    if placement not in ("warp", "translate"):
        raise ValueError("placement must be 'warp' or 'translate'")


def _placement(superposition_homography_dict, resize_info, placement, scale, frame_w, frame_h, max_pixels):
    """-> (ox, oy, dw, dh, matrix_of(frame_no) -> f64[9], NaN for a frame that leaves the canvas alone)"""
    w, h = int(resize_info["w"]), int(resize_info["h"])
    nan = np.full(9, np.nan)
    check_placement(placement)
    if placement == "translate":
        if float(scale) != 1.0:
            raise ValueError("placement='translate' is the reference's paste: scale must be 1")
        corner = get_reference_system(superposition_homography_dict)
        dh, dw = panorama_shape(corner, (h, w))
        ox, oy = -int(np.abs(corner["min_x"])), -int(np.abs(corner["min_y"]))

        def matrix_of(frame_no):
            m = _matrix(superposition_homography_dict.get(frame_no))
            if m is None or m[2][2] == 0:
                return nan
            dx, dy = translate_offset(m)
            return np.array([1, 0, dx, 0, 1, dy, 0, 0, 1], np.float64)
    else:
        ox, oy, dw, dh = fixed_plane_bounds(superposition_homography_dict, resize_info, scale, max_pixels)
        S = np.diag([float(scale), float(scale), 1.0])
        K = np.diag([w / frame_w, h / frame_h, 1.0])          # from_original_to_fix: original pixels -> resized pixels

        def matrix_of(frame_no):
            m = _matrix(superposition_homography_dict.get(frame_no))
            return nan if m is None else np.dot(np.dot(S, m), K).reshape(9)
    if dw * dh > int(max_pixels):
        raise ValueError("the canvas is %d x %d pixels, more than max_pixels = %d" % (dw, dh, int(max_pixels)))
    return ox, oy, dw, dh, matrix_of


def _check_trail(mode, placement, trail, border):
    """The refusals of the trail arguments -> whether the frames get their white outline."""
    if not (isinstance(border, bool) or (isinstance(border, str) and border == "auto")):
        raise ValueError("border must be 'auto', True or False")
    if not trail:
        if border is True:
            raise ValueError("border=True needs trail=True: only the trail pictures carry the frame's outline")
        return False
    if mode != "history":
        raise ValueError("trail=True needs mode='history': the trail is the canvas after every frame")
    if border is True and placement == "warp":
        raise ValueError("border=True with placement='warp': a projective outline is not built")
    return placement == "translate" and border is not False


def _canvas_chunks(capture, mode, chunk_frames, ingest, setup, originals=False):
    """The loop behind _chunks and surface.surface_frames: reads and uploads chunk_frames frames at a time and yields (number of
    the chunk's first frame, n, the canvases of the chunk on the device or None for "mosaic", the chunk's full-size BGR frames
    on the device when `originals`, the carried canvas).  What it yields is valid until the next step.
    setup(w0, h0) -> (dw, dh, the size the ladder resizes the frames to or None, paint); paint(ctx, number of the frame before the
    chunk, n, the chunk's source, its size= argument, the chunk's canvases [n,dh,dw,3] or None for "mosaic", the carried canvas)
    enqueues the chunk's work and leaves torch ordered after it."""
    import torch
    reader = FrameReader(capture, ingest)
    w0, h0 = reader.w0, reader.h0
    dw, dh, resize_to, paint = setup(w0, h0)
    ctx = runtime.get_context(64, 64)             # the entries used here work on caller buffers of any size
    dev = runtime.device()
    per_frame = WARP_MODES[mode] != WARP_MOSAIC
    chunk = max(1, int(chunk_frames))
    if per_frame:
        chunk = max(1, min(chunk, CHUNK_BYTES // (dw * dh * 3)))
    canvas = torch.zeros((dh, dw, 3), dtype=torch.uint8, device=dev)
    out = torch.empty((chunk, dh, dw, 3), dtype=torch.uint8, device=dev) if per_frame else None
    ladder = DeviceLadder(dev, chunk, reader.planes, (w0, h0), resize_to, bgr=originals)
    for frame_no, frames in reader.chunks(chunk, 0):
        n = len(frames)
        full, src, size = ladder(ctx, torch.from_numpy(frames).to(dev))
        paint(ctx, frame_no, n, src, size, out[:n] if per_frame else None, canvas)
        yield frame_no + 1, n, (out[:n] if per_frame else None), (full if originals else None), canvas


def _chunks(capture, superposition_homography_dict, resize_info, mode, placement, scale, chunk_frames, ingest, max_pixels,
            trail, border, originals=False):
    """The loop behind stabilized_frames and comparison_frames: _canvas_chunks with the fixed plane's geometry and entries."""
    import torch
    if mode not in WARP_MODES:
        raise ValueError("mode must be 'each', 'history' or 'mosaic'")
    check_ingest(ingest)
    outline = _check_trail(mode, placement, trail, border)
    w, h = int(resize_info["w"]), int(resize_info["h"])

    def setup(w0, h0):
        ox, oy, dw, dh, matrix_of = _placement(superposition_homography_dict, resize_info, placement, scale, w0, h0, max_pixels)
        dev = runtime.device()

        def paint(ctx, frame_no, n, src, size, out, canvas):
            host_mats = np.stack([matrix_of(frame_no + 1 + k) for k in range(n)])
            mats = torch.from_numpy(host_mats).to(dev)
            if trail:
                if frame_no == 0 and placement == "translate":
                    # initialize_background (stabilization.py:245-249): frame 1 at (|min_x|, |min_y|), the plane's origin, undimmed
                    eye = torch.tensor([1, 0, 0, 0, 1, 0, 0, 0, 1], dtype=torch.float64, device=dev)
                    ctx.warp_fixed_plane(src[:1], eye, canvas, "mosaic", (ox, oy), background=canvas, size=size)
                rects = None
                if outline:                           # change_frame_location's corners (stabilization.py:76-94)
                    rects = np.tile(np.array([0, 0, -1, -1], np.int32), (n, 1))
                    for k, m in enumerate(host_mats):
                        if np.isfinite(m[2]) and np.isfinite(m[5]):
                            rects[k] = frame_outline(-ox, -oy, int(m[2]), int(m[5]), w, h)
                    rects = torch.from_numpy(rects).to(dev)
                ctx.trail_fixed_plane(src, mats, canvas, (ox, oy), out=out, rects=rects, size=size)
                ctx.order_torch_after()
            elif out is not None:
                ctx.warp_fixed_plane(src, mats, out, mode, (ox, oy), background=canvas if mode == "history" else None, size=size)
                ctx.order_torch_after()
                if mode == "history":
                    canvas.copy_(out[n - 1])
            else:
                ctx.warp_fixed_plane(src, mats, canvas, mode, (ox, oy), background=canvas, size=size)
                ctx.order_torch_after()
        return dw, dh, (w, h) if placement == "translate" else None, paint

    yield from _canvas_chunks(capture, mode, chunk_frames, ingest, setup, originals)


def frame_outline(abs_min_x, abs_min_y, x_offset, y_offset, w, h):
    """(x0, y0, x1, y1) of the white rectangle change_frame_location draws around a w x h frame (stabilization.py:76-94):
    from (|min_x| + x_offset, |min_y| + y_offset) to that plus (w, h), both ends inclusive."""
    x0, y0 = int(abs_min_x) + int(x_offset), int(abs_min_y) + int(y_offset)
    return x0, y0, x0 + int(w), y0 + int(h)


def stabilized_frames(capture, superposition_homography_dict, resize_info, mode="history", placement="warp", scale=1.0,
                      chunk_frames=32, ingest="auto", max_pixels=MAX_PIXELS, trail=False, border="auto"):
    """Generator of (frame_no, uint8 ndarray [dh,dw,3]): the frames of `capture` (frame_no counts from 1, as the
    dictionary's keys do) placed in the fixed plane on the device.

    mode "history": per frame, the canvas after this frame -- the picture create_video_comparison shows (without its
    drawing); "each": per frame, this frame alone on black; "mosaic": yields once, the last frame_no and the canvas of all
    frames.  placement, scale: see the module text and fixed_plane_bounds.  Frames are read and uploaded chunk_frames at a
    time (as 4:2:0 planes where ingest allows, see video_processing.get_homography_dict) and the canvas stays on the device
    between chunks.  A frame whose matrix is missing, None or not finite leaves the canvas as it was.

    trail=True (mode "history" only): the reference's picture -- earlier frames fade out behind the current one
    (evh_trail_fixed_plane), and with placement "translate" the canvas starts from initialize_background's.  border: "auto" =
    the white rectangle of change_frame_location for "translate", none for "warp"; True = the rectangle ("warp": ValueError,
    a projective outline is not built); False = none.  A frame without a usable matrix gets no rectangle and still dims."""
    frame_no = 0                                  # _chunks refuses bad arguments before it opens anything
    for first, n, pictures, _, canvas in _chunks(capture, superposition_homography_dict, resize_info, mode, placement, scale,
                                                 chunk_frames, ingest, max_pixels, trail, border):
        frame_no = first + n - 1
        if pictures is not None:
            pictures = pictures.cpu().numpy()
            for k in range(n):
                yield first + k, pictures[k]
    if WARP_MODES[mode] == WARP_MOSAIC:
        yield frame_no, canvas.cpu().numpy()


def stabilized_jpegs(capture, superposition_homography_dict, resize_info, mode="history", placement="warp", scale=1.0,
                     chunk_frames=32, ingest="auto", max_pixels=MAX_PIXELS, trail=False, border="auto", quality=90,
                     subsampling="420"):
    """Generator of (frame_no, bytes): the pictures of stabilized_frames -- same arguments, same canvases -- as baseline JPEG
    files (quality 1..100, subsampling "420" or "444"), encoded on the device where the chunk's canvases lie
    (evh_jpeg_encode, include/evhip.h): no canvas is downloaded, only the files.  A file is a pure function of its canvas:
    tests/jpeg_checks.py restates it."""
    from .pictures import check_format, jpegs_of_chunks
    check_format(quality, subsampling)
    return jpegs_of_chunks(_chunks(capture, superposition_homography_dict, resize_info, mode, placement, scale, chunk_frames, ingest,
                                   max_pixels, trail, border), mode == "mosaic", quality, subsampling)


def comparison_size(w0, h0, dw, dh, height=300):
    """((width of the original, width of the fixed plane), height) of the two halves of a comparison picture:
    imutils.resize(image, height=height) gives (int(w * (height / float(h))), height)."""
    return (int(w0 * (height / float(h0))), int(dw * (height / float(dh)))), int(height)


def comparison_frames(capture, superposition_homography_dict, resize_info, placement="translate", height=300,
                      canvas_border=(0, 0, 248), scale=1.0, chunk_frames=32, ingest="auto", max_pixels=MAX_PIXELS, border="auto"):
    """Generator of (frame_no, uint8 ndarray [height, wa + wb, 3]): create_video_comparison's picture (stabilization.py:252-290)
    without its two words of text.  Left the original frame, right the trail picture of stabilized_frames(trail=True), both
    taken to `height` rows by evh_resize_area_u8 (imutils.resize(height=) is INTER_AREA; enlarging is its bilinear emulation),
    the right one then inside the one-pixel rectangle (0, 0)-(W-1, H-1) of colour canvas_border (b, g, r) that create_border
    draws.  Everything stays on the device; the pictures come back a chunk at a time."""
    import torch
    _check_trail("history", placement, True, border)
    height = int(height)
    if height < 1:
        raise ValueError("height must be at least 1")
    colour = [int(v) for v in canvas_border]
    if len(colour) != 3 or min(colour) < 0 or max(colour) > 255:
        raise ValueError("canvas_border is (b, g, r) with bytes")
    ctx = dev = a = b = both = None
    for first, n, pictures, full, _ in _chunks(capture, superposition_homography_dict, resize_info, "history", placement, scale,
                                               chunk_frames, ingest, max_pixels, True, border, originals=True):
        if both is None:
            ctx, dev = runtime.get_context(64, 64), runtime.device()
            (wa, wb), _ = comparison_size(full.shape[2], full.shape[1], pictures.shape[2], pictures.shape[1], height)
            if wa < 1 or wb < 1:
                raise ValueError("height = %d leaves a half of the picture without columns" % height)
            cap = max(1, int(chunk_frames))
            a = torch.empty((cap, height, wa, 3), dtype=torch.uint8, device=dev)
            b = torch.empty((cap, height, wb, 3), dtype=torch.uint8, device=dev)
            both = torch.empty((cap, height, wa + wb, 3), dtype=torch.uint8, device=dev)
            edge = torch.tensor(colour, dtype=torch.uint8, device=dev)
        ctx.resize_area(full.contiguous(), a[:n])
        ctx.resize_area(pictures, b[:n])
        ctx.order_torch_after()
        b[:n, 0, :] = edge
        b[:n, -1, :] = edge
        b[:n, :, 0] = edge
        b[:n, :, -1] = edge
        both[:n, :, :wa] = a[:n]
        both[:n, :, wa:] = b[:n]
        host = both[:n].cpu().numpy()
        for k in range(n):
            yield first + k, host[k]


BackgroundPlate = collections.namedtuple("BackgroundPlate", "plate count origin frame_nos masks")


def plate_frame_numbers(n_frames, max_frames):
    """The frames a plate is taken over: 1, 1 + s, 1 + 2s, ... <= n_frames with s = max(1, ceil(n_frames / max_frames)), at most
    max_frames of them, spread over the whole video."""
    n_frames, max_frames = int(n_frames), int(max_frames)
    if n_frames < 1 or max_frames < 1:
        raise ValueError("n_frames and max_frames must be at least 1")
    return list(range(1, n_frames + 1, max(1, -(-n_frames // max_frames))))


def background_plate(capture, superposition_homography_dict, resize_info, placement="warp", scale=1.0, max_frames=64, min_cover=1,
                     masks=False, threshold=16, ingest="auto", max_pixels=MAX_PIXELS, max_bytes=2 << 30):
    """The scene without its moving objects -> BackgroundPlate(plate u8[dh,dw,3], count u8[dh,dw], origin (ox, oy), frame_nos,
    masks u8[n,dh,dw] or None).

    Canvas and matrices are those of stabilized_frames (placement, scale, max_pixels as there).  Of the frames 1 .. the largest
    key of the dictionary, plate_frame_numbers(., max_frames) are kept (max_frames in 1..255) while the capture is read once,
    uploaded (as 4:2:0 planes where ingest allows) and handed to evh_plate_fixed_plane in one call: plate = per pixel and channel
    the lower median of the frames that cover it where count >= min_cover (1..255), black elsewhere; count = how many of the
    kept frames cover the pixel; masks=True: per kept frame, 255 where it covers the pixel and its gray differs from the plate's
    by more than threshold (0..255) -- what moves, in fixed-plane coordinates.  A kept frame without a usable matrix covers
    nothing; frame_nos lists the frames that were kept (fewer when the capture ends early).  ValueError when frames, plate, count
    and masks together would take more than max_bytes on the device."""
    dev = _plate_on_device(capture, superposition_homography_dict, resize_info, placement, scale, max_frames, min_cover, masks,
                           threshold, ingest, max_pixels, max_bytes)
    dev.ctx.order_torch_after()
    return BackgroundPlate(dev.plate.cpu().numpy(), dev.count.cpu().numpy(), dev.origin, dev.frame_nos,
                           dev.masks.cpu().numpy() if masks else None)


DevicePlate = collections.namedtuple("DevicePlate", "ctx plate count masks origin frame_nos frame_size inputs")


def check_plate_arguments(max_frames, min_cover, threshold, placement, ingest):
    """The refusals background_plate and moving.moving_objects share, before the capture is touched."""
    if not 1 <= int(max_frames) <= PLATE_MAX_FRAMES:
        raise ValueError("max_frames must lie in 1..%d" % PLATE_MAX_FRAMES)
    if not 1 <= int(min_cover) <= 255:
        raise ValueError("min_cover must lie in 1..255")
    if not 0 <= int(threshold) <= 255:
        raise ValueError("threshold must lie in 0..255")
    check_placement(placement)
    check_ingest(ingest)


def _plate_on_device(capture, superposition_homography_dict, resize_info, placement, scale, max_frames, min_cover, masks, threshold,
                     ingest, max_pixels, max_bytes, extra_bytes_per_mask_pixel=0):
    """background_plate up to its launch: the reader, the ladder, _placement and evh_plate_fixed_plane, with plate, count and masks
    left on the device -> DevicePlate (frame_size: the original (w0, h0)).  Nothing is synchronised: whatever follows on the
    context's stream is ordered behind the plate.  inputs holds the tensors the launch reads: the caller keeps the DevicePlate
    until it has ordered or synchronised, so that their memory is not handed out again while the launch runs.  extra_bytes_per_mask_pixel: what the caller will add per mask pixel, counted
    against max_bytes."""
    import torch
    check_plate_arguments(max_frames, min_cover, threshold, placement, ingest)
    reader = FrameReader(capture, ingest)
    planes, w0, h0 = reader.planes, reader.w0, reader.h0
    ox, oy, dw, dh, matrix_of = _placement(superposition_homography_dict, resize_info, placement, scale, w0, h0, max_pixels)
    w, h = int(resize_info["w"]), int(resize_info["h"])
    frame_nos = plate_frame_numbers(max(int(k) for k in _frames_of(superposition_homography_dict)), max_frames)
    n = len(frame_nos)
    resize = placement == "translate" and (w, h) != (w0, h0)
    device_bytes = n * reader.first.size + (n * h0 * w0 * 3 if planes and resize else 0) + (n * h * w * 3 if resize else 0) \
        + dw * dh * (4 + (n if masks else 0) + n * int(extra_bytes_per_mask_pixel))
    if device_bytes > int(max_bytes):
        raise ValueError("%d frames, plate, count and masks take %d bytes on the device, more than max_bytes = %d"
                         % (n, device_bytes, int(max_bytes)))
    host = reader.buffer(n)
    kept = 1
    while kept < n and reader.read_into(host[kept]):       # the capture read once; only the selected frames stay
        if reader.consumed == frame_nos[kept]:
            kept += 1
    n, frame_nos = kept, frame_nos[:kept]
    ctx = runtime.get_context(64, 64)             # the entries used here work on caller buffers of any size
    dev = runtime.device()
    mats = torch.from_numpy(np.stack([matrix_of(k) for k in frame_nos])).to(dev)
    ladder = DeviceLadder(dev, n, planes, (w0, h0), (w, h) if placement == "translate" else None)
    _, src, size = ladder(ctx, torch.from_numpy(host[:n]).to(dev))
    plate = torch.empty((dh, dw, 3), dtype=torch.uint8, device=dev)
    count = torch.empty((dh, dw), dtype=torch.uint8, device=dev)
    pictures = torch.empty((n, dh, dw), dtype=torch.uint8, device=dev) if masks else None
    ctx.plate_fixed_plane(src, mats, plate, (ox, oy), count=count, masks=pictures, threshold=int(threshold),
                          min_cover=int(min_cover), size=size)
    return DevicePlate(ctx, plate, count, pictures, (ox, oy), frame_nos, (w0, h0), (ladder, src, mats))


def write_ppm(path, image):
    """image u8[h,w,3] in BGR order (as the frames are) -> a binary P6 file (RGB, maxval 255)."""
    image = np.asarray(image)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
        raise ValueError("write_ppm takes a uint8 [h, w, 3] image")
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (image.shape[1], image.shape[0]))
        f.write(np.ascontiguousarray(image[:, :, ::-1]).tobytes())

