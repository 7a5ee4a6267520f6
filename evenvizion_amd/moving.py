"""The second pass over a video: matches on moving objects are dropped before the final solve.

The reference's known-issues.md names moving objects as the open problem of the method: key points cling to what moves, and the
homography follows the object instead of the camera.  With a first pass (get_homography_dict) and the background plate taken from
it (stabilization.background_plate) at hand, refine_homography_dict reads the video again and, per chunk, runs the same batch
entry, fetches the rows that entered its final solve (evh_batch_static_rows), drops the rows one of whose points sits on
something that differs from the plate (evh_rows_moving_filter) and solves the remaining rows with the reference's running
superposition (evh_stream_scan).  Rows, flags and counts never leave the device; only the matrices, the statuses and three counts
per pair come back.
"""
import numpy as np

from . import runtime
from ._lib import PAIR_CAPACITY, PAIR_OK
from .frames import DeviceLadder, FrameReader, check_ingest
from .processing.utils import superposition_dict
from .processing.video_processing import CHUNK_FRAMES

MAX_RADIUS = 7      # evh_rows_moving_filter: the window is (2*radius + 1)^2 canvas pixels


def _integer(name, value, lo, hi=None):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < lo or (hi is not None and value > hi):
        raise ValueError("%s must be an integer %s" % (name, ("in %d..%d" % (lo, hi)) if hi is not None else "of at least %d" % lo))
    return int(value)


def _arguments(homography_dict, plate, placement, scale, threshold, min_cover, radius, min_hits, min_keep, nfeatures, chunk_frames,
               features_type_list, ingest):
    """The refusals of refine_homography_dict, before the capture is opened or the device touched
    -> (per-frame dictionary with int keys, resize_info)"""
    from .processing.video_processing import _feature_list
    from .stabilization import check_placement
    check_placement(placement)
    check_ingest(ingest)
    if isinstance(scale, bool) or not isinstance(scale, (int, float, np.integer, np.floating)) or not np.isfinite(scale) or scale <= 0:
        raise ValueError("scale must be a finite positive number")
    if placement == "translate" and float(scale) != 1.0:
        raise ValueError("placement='translate' is the reference's paste: scale must be 1")
    _integer("threshold", threshold, 0, 255)
    _integer("min_cover", min_cover, 1, 255)
    radius = _integer("radius", radius, 0, MAX_RADIUS)
    _integer("min_hits", min_hits, 1, (2 * radius + 1) ** 2)
    _integer("min_keep", min_keep, 0)
    _integer("nfeatures", nfeatures, 1)
    _integer("chunk_frames", chunk_frames, 2)
    if _feature_list(features_type_list) != ["ORB"]:
        raise ValueError('features_type_list must be ["ORB"]: the second pass is built on the fused ORB path only')
    if not isinstance(homography_dict, dict) or "resize_info" not in homography_dict:
        raise ValueError("homography_dict must be the first pass's dictionary, with its resize_info")
    resize_info = homography_dict["resize_info"]
    per_frame = {int(k): v for k, v in homography_dict.items() if k != "resize_info"}
    if not per_frame:
        raise ValueError("homography_dict holds no pair")
    for name in ("plate", "count", "origin"):
        if not hasattr(plate, name):
            raise ValueError("plate must be the BackgroundPlate that background_plate returned")
    p, c = np.asarray(plate.plate), np.asarray(plate.count)
    if p.dtype != np.uint8 or p.ndim != 3 or p.shape[2] != 3 or c.dtype != np.uint8 or c.shape != p.shape[:2]:
        raise ValueError("plate.plate must be u8[dh,dw,3] and plate.count u8[dh,dw]")
    return per_frame, resize_info


def refine_homography_dict(capture, homography_dict, plate, placement="warp", scale=1.0, threshold=16, min_cover=2, radius=1,
                           min_hits=1, min_keep=8, nfeatures=runtime.NFEATURES, chunk_frames=CHUNK_FRAMES,
                           features_type_list=("ORB",), ingest="auto", none_H_processing=True):
    """-> (refined_dict, stats).  capture: the video of the first pass, opened again.  homography_dict: the first pass's result
    ({frame_no: {"H": 3x3}, ..., "resize_info"}, keys int or str).  plate: the BackgroundPlate background_plate returned for the
    same video with the same placement and scale (its superposition must be superposition_dict of homography_dict).

    The superposition and the canvas are formed as background_plate forms them; a canvas whose shape or origin differs from
    the plate's is a ValueError (wrong placement or scale).  Plate and count are uploaded once.  The capture is then read chunk
    by chunk (chunk_frames frames, consecutive chunks overlapping by one frame); per chunk the batch entry get_homography_dict
    runs for ["ORB"] and this ingest, batch_static_rows, rows_moving_filter -- for "warp" on the frames as uploaded, with
    row_scale = (w0 / w, h0 / h) from resized to original pixels; for "translate" on the device-resized frames with (1, 1) --
    and stream_scan with the carried {H_sup, H_prev}.  The matrices that place a frame on the plate are the FIRST pass's: the
    plate was built from them.  threshold, min_cover, radius, min_hits, min_keep: see Context.rows_moving_filter; the default
    min_cover = 2 judges a point only where at least two of the plate's frames met.

    The chunk loop (frames.FrameReader) is synchronous: every chunk is read, uploaded, solved and downloaded before the next is read.  The
    double-buffered pipeline of get_homography_dict is not built here.  A chunk in which a pair reports EVH_PAIR_CAPACITY (more
    tied key points than a frame slot holds) raises RuntimeError naming the frames: the re-run on larger slots of the first
    pass is not built either.  Only features_type_list=["ORB"] is taken (ValueError otherwise): evh_stream_scan solves the
    row blocks of the fused ORB path; on the wider blocks of a multi-type batch it did not reproduce that batch's own solve
    when it was tried (the first pair came back EVH_PAIR_LOW_INLIER_RATIO), so the second pass over such a list is not built.

    refined_dict has the format and the none_H_processing rule of get_homography_dict.  stats[frame_no] = (rows, moving,
    rows_out) for the pair ending at frame_no: the rows that reached the filter, those it found moving, those handed to the
    solve (rows - moving, or rows when fewer than min_keep would have been left); (0, 0, 0) for a pair without rows."""
    import torch
    from .processing.video_processing import _pairs_into, resized_shape
    from .stabilization import MAX_PIXELS, _placement
    per_frame, resize_info = _arguments(homography_dict, plate, placement, scale, threshold, min_cover, radius, min_hits,
                                                  min_keep, nfeatures, chunk_frames, features_type_list, ingest)
    sup = superposition_dict(per_frame)
    reader = FrameReader(capture, ingest)
    first, planes, w0, h0 = reader.first, reader.planes, reader.w0, reader.h0
    if not planes and (first.ndim != 3 or first.shape[2] != 3):
        raise ValueError("frames must be BGR [h,w,3] or decoded planes: the plate is a BGR picture")
    w, h = int(resize_info["w"]), int(resize_info["h"])
    if (w, h) != resized_shape((h0, w0), w):
        raise ValueError("resize_info %dx%d is not what frames of %dx%d resize to" % (w, h, w0, h0))
    ox, oy, dw, dh, matrix_of = _placement(sup, resize_info, placement, scale, w0, h0, max(MAX_PIXELS, int(np.asarray(plate.plate).size)))
    if (dh, dw) != tuple(np.asarray(plate.plate).shape[:2]) or (ox, oy) != (int(plate.origin[0]), int(plate.origin[1])):
        raise ValueError("the canvas of this dictionary is %d x %d at (%d, %d), the plate %d x %d at (%d, %d): another placement or scale"
                         % (dw, dh, ox, oy, plate.plate.shape[1], plate.plate.shape[0], plate.origin[0], plate.origin[1]))
    method, size = ("stream_homography_batch_yuv420", ((w0, h0),)) if planes else ("stream_homography_batch", ())
    chunk = runtime.chunk_frames_for(first.nbytes, max(2, int(chunk_frames)))
    ctx = runtime.get_context(w, h, chunk, nfeatures)
    dev = runtime.device()
    plate_dev = torch.from_numpy(np.ascontiguousarray(plate.plate)).to(dev)
    count_dev = torch.from_numpy(np.ascontiguousarray(plate.count)).to(dev)
    translate = placement == "translate"
    ladder = DeviceLadder(dev, chunk, planes, (w0, h0), (w, h) if translate else None)
    row_scale = (1.0, 1.0) if translate else (w0 / w, h0 / h)
    H_dev = torch.zeros((chunk - 1, 9), dtype=torch.float64, device=dev)
    st_dev = torch.zeros(chunk - 1, dtype=torch.int32, device=dev)
    first_state = torch.zeros(18, dtype=torch.float64, device=dev)      # {H_sup, H_prev} of the first pass's solve, as it ran
    state = torch.zeros(18, dtype=torch.float64, device=dev)            # and of the refined one
    refined, stats = {}, {}
    have_state = False
    buffers = {}                                             # row capacity -> the filter's outputs
    for start, frames in reader.chunks(chunk, 1):            # consecutive chunks overlap by one frame
        frame_no, n = start + 1, len(frames)                 # frames[0] is frame `frame_no`, the newest frame already paired
        npairs = n - 1
        src = torch.from_numpy(frames).to(dev)
        getattr(ctx, method)(src, *size, H_dev, st_dev, state_in=first_state if have_state else None,
                             state_out=first_state, nfeatures=nfeatures, resize_to=(w, h))
        rows, counts, st1 = ctx.batch_static_rows(0, npairs)
        cap = rows.shape[1]
        if cap not in buffers:
            buffers[cap] = (torch.empty((chunk - 1, cap, 4), dtype=torch.float32, device=dev),
                            torch.empty(chunk - 1, dtype=torch.int32, device=dev), torch.empty(chunk - 1, dtype=torch.int32, device=dev))
        out_rows, out_counts, moving = (t[:npairs] for t in buffers[cap])
        _, judged, judged_size = ladder(ctx, src)
        mats = torch.from_numpy(np.stack([matrix_of(k) for k in range(frame_no, frame_no + n)])).to(dev)
        ctx.rows_moving_filter(judged, mats, plate_dev, count_dev, (ox, oy), rows, counts, st1, out_rows, out_counts, moving,
                               threshold=int(threshold), min_cover=int(min_cover), radius=int(radius), min_hits=int(min_hits),
                               row_scale=row_scale, frame_step=1, min_keep=int(min_keep), size=judged_size)
        Hs, sts = ctx.stream_scan(out_rows, out_counts, st1, state_in=state if have_state else None, state_out=state)
        have_state = True
        sts_h, st1_h = sts.cpu().numpy(), st1.cpu().numpy()
        if (sts_h == PAIR_CAPACITY).any() or (st1_h == PAIR_CAPACITY).any() or (st_dev[:npairs].cpu().numpy() == PAIR_CAPACITY).any():
            raise RuntimeError("frames %d..%d: more tied key points than a frame slot holds (EVH_PAIR_CAPACITY); the re-run on "
                               "larger slots is not built for the second pass" % (frame_no, frame_no + npairs))
        n_in, n_out, mov = (np.clip(t.cpu().numpy(), 0, cap) for t in (counts, out_counts, moving))
        for k in range(npairs):
            ok = st1_h[k] == PAIR_OK and n_in[k] > 0
            stats[frame_no + 1 + k] = (int(n_in[k]), int(mov[k]), int(n_out[k])) if ok else (0, 0, 0)
        _pairs_into(refined, frame_no, Hs.cpu().numpy().reshape(-1, 3, 3), sts_h, none_H_processing)
    refined["resize_info"] = {"h": h, "w": w}
    return refined, stats


# ---- the masks as objects: connected components on the device, tracks on the host ----------------------------------------------------
def _objects_arguments(placement, scale, max_frames, min_cover, threshold, connectivity, open_radius, min_area, max_objects, ingest):
    """The refusals of moving_objects, before the capture is touched."""
    from .stabilization import check_plate_arguments
    for name, value in (("max_frames", max_frames), ("min_cover", min_cover), ("threshold", threshold)):
        _integer(name, value, 0)
    check_plate_arguments(max_frames, min_cover, threshold, placement, ingest)
    if isinstance(scale, bool) or not isinstance(scale, (int, float, np.integer, np.floating)) or not np.isfinite(scale) or scale <= 0:
        raise ValueError("scale must be a finite positive number")
    if placement == "translate" and float(scale) != 1.0:
        raise ValueError("placement='translate' is the reference's paste: scale must be 1")
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise ValueError("connectivity must be 4 or 8")
    _integer("open_radius", open_radius, 0, 3)
    _integer("min_area", min_area, 1)
    _integer("max_objects", max_objects, 1, 65535)


def _iou(a, b):
    """Intersection over union of two inclusive boxes (x0, y0, x1, y1); edges count as one unit, as pixels do."""
    w = min(a[2], b[2]) - max(a[0], b[0]) + 1
    h = min(a[3], b[3]) - max(a[1], b[1]) + 1
    if w <= 0 or h <= 0:
        return 0.0
    inter = w * h
    return inter / ((a[2] - a[0] + 1) * (a[3] - a[1] + 1) + (b[2] - b[0] + 1) * (b[3] - b[1] + 1) - inter)


def link_objects(objects_by_frame, min_iou=0.1):
    """Objects linked into tracks by the overlap of their boxes -> a list of tracks, each a list of (frame_no, object index), in
    the order the tracks were opened.  objects_by_frame: {frame_no: [object, ...]}, an object a dict with "box_plane" = (x0, y0,
    x1, y1) inclusive, in plane coordinates.

    Frames are taken in ascending order.  Every pair (open track, object of the frame) whose intersection over union -- the
    track's last box against the object's -- is at least min_iou (and above 0) is a candidate; candidates are taken greedily in
    order of descending IoU, ties to the lower track, then to the lower object index; a track and an object are matched at most
    once.  A track that finds no match in a frame closes (an empty frame closes every track), an object without a match opens
    a new track."""
    if isinstance(min_iou, bool) or not isinstance(min_iou, (int, float, np.integer, np.floating)) or not 0 <= min_iou <= 1:
        raise ValueError("min_iou must lie in 0..1")
    tracks, open_tracks = [], []                   # open_tracks: indices into tracks
    for frame_no in sorted(objects_by_frame):
        objects = objects_by_frame[frame_no]
        boxes = [tuple(o["box_plane"]) for o in objects]
        candidates = []
        for t in open_tracks:
            last_frame, last_index = tracks[t][-1]
            last = tuple(objects_by_frame[last_frame][last_index]["box_plane"])
            for k, box in enumerate(boxes):
                v = _iou(last, box)
                if v > 0 and v >= min_iou:
                    candidates.append((-v, t, k))
        candidates.sort()
        taken_tracks, taken_objects = set(), set()
        for _, t, k in candidates:
            if t in taken_tracks or k in taken_objects:
                continue
            taken_tracks.add(t)
            taken_objects.add(k)
            tracks[t].append((frame_no, k))
        still_open = [t for t in open_tracks if t in taken_tracks]
        for k in range(len(objects)):
            if k not in taken_objects:
                tracks.append([(frame_no, k)])
                still_open.append(len(tracks) - 1)
        open_tracks = sorted(still_open)
    return tracks


def moving_objects(capture, homography_dict, resize_info, placement="warp", scale=1.0, max_frames=64, min_cover=2, threshold=16,
                   connectivity=8, open_radius=1, min_area=25, max_objects=256, ingest="auto", max_pixels=None, max_bytes=2 << 30,
                   min_iou=0.1, labels=False):
    """The moving objects of a video -> a dict {"frames": {frame_no: {"count": K, "truncated": bool, "objects": [...]}},
    "tracks": [[(frame_no, object index), ...], ...], "origin": (ox, oy), "size": (dw, dh), "frame_nos": [...]} and, with
    labels=True, "labels": i32[n,dh,dw] (else the labels never leave the device).

    homography_dict: the SUPERPOSED dictionary, as background_plate takes it.  The reader, the frame ladder, the canvas and the
    frames kept (placement, scale, max_frames, max_pixels, ingest) are background_plate's; the plate with its masks
    (min_cover, threshold) and their labelling (connectivity, open_radius, min_area: Context.mask_components) are one sequence on
    the device, and only the counts and the tables of max_objects rows per frame are downloaded.  An object is a dict:
    "number" (its label), "area", "box_canvas" (x0, y0, x1, y1 inclusive canvas pixels), "box_plane" and "centre_plane"
    ((canvas + origin) / scale, the centre being sum / area), "box_frame" and "centre_frame": the plane points taken to the
    object's own original frame through from_fix_to_original (two decimals, as there).  "truncated": K > max_objects, the
    objects past max_objects are missing from the list (the labels still hold them).  Tracks: link_objects(., min_iou)."""
    import torch
    from .processing.fixed_coordinate_system import from_fix_to_original
    from .stabilization import MAX_PIXELS, _matrix, _plate_on_device
    _objects_arguments(placement, scale, max_frames, min_cover, threshold, connectivity, open_radius, min_area, max_objects, ingest)
    if isinstance(min_iou, bool) or not isinstance(min_iou, (int, float, np.integer, np.floating)) or not 0 <= min_iou <= 1:
        raise ValueError("min_iou must lie in 0..1")
    plate = _plate_on_device(capture, homography_dict, resize_info, placement, scale, max_frames, min_cover, True, threshold, ingest,
                             MAX_PIXELS if max_pixels is None else max_pixels, max_bytes, extra_bytes_per_mask_pixel=12)
    ctx, masks, (ox, oy), frame_nos = plate.ctx, plate.masks, plate.origin, plate.frame_nos
    n, dh, dw = masks.shape
    sheets = torch.empty((n, dh, dw), dtype=torch.int32, device=masks.device)
    table = torch.zeros((n, int(max_objects), 5), dtype=torch.int64, device=masks.device)
    counts = ctx.mask_components(masks, sheets, int(connectivity), int(open_radius), int(min_area), objects=table)
    ctx.order_torch_after()
    counts_h, table_h = counts.cpu().numpy(), ctx.components_table(table)
    s = float(scale)
    frames, points = {}, {}
    for i, frame_no in enumerate(frame_nos):
        found = []
        for k in range(min(int(counts_h[i]), int(max_objects))):
            o = table_h[i, k]
            x0, y0, x1, y1, area = (int(o[f]) for f in ("x0", "y0", "x1", "y1", "area"))
            cx, cy = int(o["sx"]) / area, int(o["sy"]) / area
            found.append({"number": k + 1, "area": area, "box_canvas": (x0, y0, x1, y1),
                          "box_plane": ((x0 + ox) / s, (y0 + oy) / s, (x1 + ox) / s, (y1 + oy) / s),
                          "centre_plane": ((cx + ox) / s, (cy + oy) / s)})
        frames[frame_no] = {"count": int(counts_h[i]), "truncated": int(counts_h[i]) > int(max_objects), "objects": found}
        points[frame_no] = [{"x1": p[0], "y1": p[1]} for o in found
                            for p in (o["box_plane"][:2], o["box_plane"][2:], o["centre_plane"])]
    w0, h0 = plate.frame_size
    mats = {k: _matrix(homography_dict.get(k)) for k in frame_nos if points[k]}
    back = from_fix_to_original(points, mats, (h0, w0), (int(resize_info["h"]), int(resize_info["w"])))
    for frame_no in frame_nos:
        for j, o in enumerate(frames[frame_no]["objects"]):
            a, b, c = (back[frame_no][3 * j + t] for t in range(3))
            o["box_frame"] = (float(a["x1"]), float(a["y1"]), float(b["x1"]), float(b["y1"]))
            o["centre_frame"] = (float(c["x1"]), float(c["y1"]))
    out = {"frames": frames, "tracks": link_objects({k: v["objects"] for k, v in frames.items()}, min_iou), "origin": (ox, oy),
           "size": (int(dw), int(dh)), "frame_nos": list(frame_nos)}
    if labels:
        out["labels"] = sheets.cpu().numpy()
    return out
