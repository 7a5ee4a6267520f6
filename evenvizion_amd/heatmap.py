"""The reference's heat-map visualisation computed on the GPU: the fixed-plane coordinate field, the number it
yields for metrics_file.txt, and the coloured pictures.

`max_movement` reproduces the number heatmap_video_processing returns and evenvizion_component.py writes to
metrics_file.txt ("Maximum movement during the entire video", processing_visualization.py:407-419): for every frame
the superposed H maps each pixel (x, y) of the resized grid; the per-frame maximum coordinate is appended for every
frame EXCEPT the last one of the dict (the reference skips the append when capture.read() fails), and the maximum of
those is returned.

`heatmap_frames` yields the pictures heatmap_frame_processing writes (processing_visualization.py:336-344) before part_line
draws on them: the field's length over heatmap_constant as a colour index, a 256-entry colour table, 0.8 of the colour laid
over the resized frame (evh_heatmap_render; include/evhip.h states the arithmetic).  The frames stay on the device and one
picture of 3*w*h bytes comes back per frame.  The grid lines, arrows and text of part_line and the PNG encoding are drawing
and are not done here.
"""
import numpy as np

from . import runtime
from .frames import DeviceLadder, FrameReader, check_ingest, entry_matrix
from .processing.constants import HEATMAP_CONSTANT


def frame_maxima(superposition_homography_dict, resize_info):
    """{frame_no: 3x3 superposed H} -> (frame numbers, f64 per-frame max coordinate), computed by evh_fixed_plane_field."""
    keys = list(superposition_homography_dict.keys())
    Hs = np.array([np.asarray(superposition_homography_dict[k], np.float64) for k in keys])
    w, h = int(resize_info["w"]), int(resize_info["h"])
    ctx = runtime.get_context(max(w, 64), max(h, 64))
    return keys, ctx.fixed_plane_max(Hs, w, h)


def max_movement(superposition_homography_dict, resize_info, skip_last=True):
    _, m = frame_maxima(superposition_homography_dict, resize_info)
    if skip_last and len(m) > 1:
        m = m[:-1]
    return float(np.max(m))


def jet_lut():
    """u8[256,3], BGR: the 256-entry jet colour map by an integer rule.  Channel k = 1, 2, 3 (B, G, R) of entry j has the
    doubled value v2 = clamp(765 - 2*|4*j - 255*k|, 0, 510) and the value v2 / 2 with halves to even, so entry 0 is
    (128, 0, 0) and entry 255 is (0, 0, 128).

    This is the piecewise-linear jet map sampled at j / 255.  It is NOT claimed to equal OpenCV 3.4.2's COLORMAP_JET byte for
    byte: that table is built from float arrays and may break the half-way cases the other way, and no OpenCV was at hand to
    compare all 256 entries.  For the reference's own colours pass
    lut=cv2.applyColorMap(np.arange(256, dtype=np.uint8), cv2.COLORMAP_JET).reshape(256, 3) to heatmap_frames."""
    j = np.arange(256, dtype=np.int64)[:, None]
    k = np.array([1, 2, 3], np.int64)[None, :]
    v2 = np.clip(765 - 2 * np.abs(4 * j - 255 * k), 0, 510)
    half = v2 // 2
    return (half + ((v2 & 1) & (half & 1))).astype(np.uint8)          # an odd v2 is a half: up only onto an even value


def heatmap_frames(capture, superposition_homography_dict, resize_info, heatmap_constant=HEATMAP_CONSTANT, alpha=0.8, lut=None,
                   saturate=False, chunk_frames=32, ingest="auto"):
    """Generator of (frame_no, uint8 ndarray [h,w,3] BGR): the heat-map picture of every frame, coloured on the device.

    The i-th frame read from `capture` is paired with the i-th entry of the dictionary in the dictionary's order, as
    heatmap_video_processing pairs them; it ends when either runs out.  Frames are read by frames.FrameReader and taken to the working size by
    frames.DeviceLadder (4:2:0 planes where ingest allows, evh_yuv420_to_bgr, evh_resize_area_u8 to
    resize_info's w x h), chunk_frames at a time.  lut: u8[256,3] in BGR order, default jet_lut() (see there for what it is and
    is not).  saturate=False wraps the colour index as the reference's np.uint8 cast does; True holds it at 255.  An entry
    that is None or not finite gives colour index 0 everywhere: the frame plus alpha * lut[0]."""
    check_ingest(ingest)
    if not (np.isfinite(heatmap_constant) and heatmap_constant > 0):
        raise ValueError("heatmap_constant must be finite and positive")
    if not (np.isfinite(alpha) and alpha >= 0):
        raise ValueError("alpha must be finite and not negative")
    if int(chunk_frames) < 1:
        raise ValueError("chunk_frames must be at least 1")
    table = jet_lut() if lut is None else np.asarray(lut)
    if table.dtype != np.uint8 or table.shape != (256, 3):
        raise ValueError("lut must be a uint8 array [256, 3] in BGR order")
    w, h = int(resize_info["w"]), int(resize_info["h"])
    if w < 1 or h < 1:
        raise ValueError("resize_info must hold a positive w and h")
    entries = [(k, entry_matrix(v).reshape(9)) for k, v in superposition_homography_dict.items() if k != "resize_info"]
    return _heatmap_frames(capture, entries, w, h, float(heatmap_constant), float(alpha), table, bool(saturate), int(chunk_frames),
                           ingest)


def _heatmap_frames(capture, entries, w, h, heatmap_constant, alpha, table, saturate, chunk, ingest):
    import torch
    if not entries:
        return
    reader = FrameReader(capture, ingest)
    first = reader.first
    if not reader.planes and (first.ndim not in (2, 3) or (first.ndim == 3 and first.shape[2] != 3)):
        raise ValueError("frames must be BGR [h,w,3] or gray [h,w]")
    ctx = runtime.get_context(64, 64)             # the entries used here work on caller buffers of any size
    dev = runtime.device()
    chunk = max(1, min(chunk, len(entries), runtime.STAGING_BYTES_PER_BUFFER // max(first.nbytes, 1)))      # the host chunk stays bounded
    d_lut = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
    ladder = DeviceLadder(dev, chunk, reader.planes, (reader.w0, reader.h0), (w, h), bgr=True, gray3=True)
    out = torch.empty((chunk, h, w, 3), dtype=torch.uint8, device=dev)
    for done, frames in reader.chunks(chunk, 0, len(entries)):
        n = len(frames)
        _, src, _ = ladder(ctx, torch.from_numpy(frames).to(dev))
        mats = torch.from_numpy(np.stack([m for _, m in entries[done:done + n]])).to(dev)
        ctx.heatmap_render(mats, out[:n], d_lut, frames=src, heatmap_constant=heatmap_constant, alpha=alpha, saturate=saturate)
        ctx.order_torch_after()
        pictures = out[:n].cpu().numpy()
        for k in range(n):
            yield entries[done + k][0], pictures[k]
