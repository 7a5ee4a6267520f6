"""The reference's matching pictures drawn on the GPU: the two resized frames of a pair side by side and one green line per
static match that enters compute_homography (draw_matches, visualization/processing_visualization.py:22-57, written per pair as
matching_vis_{i}.png by video_processing.py:76-81).

`draw_matches` mirrors the reference function for two host frames.  The per-pair pictures of a video come from
get_homography_dict(..., matching_sink=): the frames, the rows and the pictures stay on the device and one picture of 6*w*h
bytes comes back per pair (evh_batch_static_rows + evh_draw_matches; include/evhip.h states the line rule).  `write_png` stores a
picture with the standard library alone.

The lines follow OpenCV 3.4.2's 8-connected LineIterator as include/evhip.h restates it; no OpenCV binary was at hand to compare
pictures with.
"""
import struct
import zlib

import numpy as np

from . import runtime


def draw_matches(image_a, image_b, pts_a, pts_b, color=(0, 255, 0)):
    """image_a, image_b: uint8 BGR frames [h,w,3] of one size; pts_a, pts_b: n points (x, y) each.  -> uint8 [h, 2w, 3]:
    image_a | image_b with a line from int(pts_a[k]) on image_a to int(pts_b[k]) on image_b for every k, as the reference's
    draw_matches gives for frames of equal size.  A point that is not finite or beyond +-32768 drops its line."""
    import torch
    a, b = np.asarray(image_a), np.asarray(image_b)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or b.dtype != np.uint8 or a.shape != b.shape:
        raise ValueError("draw_matches takes two uint8 BGR frames [h,w,3] of one size")
    pa, pb = np.asarray(pts_a, np.float32).reshape(-1, 2), np.asarray(pts_b, np.float32).reshape(-1, 2)
    if len(pa) != len(pb):
        pa, pb = pa[:min(len(pa), len(pb))], pb[:min(len(pa), len(pb))]          # zip() stops at the shorter list
    h, w = a.shape[:2]
    ctx = runtime.get_context(64, 64)                  # the entry works on caller buffers of any size
    dev = runtime.device()
    rows = np.zeros((1, max(len(pa), 1), 4), np.float32)
    rows[0, :len(pa), :2], rows[0, :len(pa), 2:] = pa, pb
    out = torch.empty((1, h, 2 * w, 3), dtype=torch.uint8, device=dev)
    ctx.draw_matches(torch.from_numpy(np.stack([a, b])).to(dev), torch.from_numpy(rows).to(dev),
                     torch.tensor([len(pa)], dtype=torch.int32, device=dev), out, points="reference", color=color)
    ctx.order_torch_after()
    return out[0].cpu().numpy()


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_png(path, bgr, level=1, gray=False):
    """A uint8 BGR picture [h,w,3] as an 8-bit RGB PNG or, with gray=True, a gray picture [h,w] as an 8-bit grayscale PNG (one
    IDAT chunk, filter 0 on every row), written with zlib alone.  The decoded pixels are the picture's; the file's bytes are
    not those cv2.imwrite would write."""
    bgr = np.asarray(bgr)
    gray = bool(gray)
    if bgr.dtype != np.uint8 or bgr.ndim != (2 if gray else 3) or (not gray and bgr.shape[2] != 3) or bgr.shape[0] < 1 \
            or bgr.shape[1] < 1:
        raise ValueError("write_png takes a uint8 BGR picture [h,w,3], or with gray=True a gray picture [h,w]")
    h, w = bgr.shape[:2]
    cn = 1 if gray else 3
    raw = np.zeros((h, 1 + cn * w), np.uint8)                                 # a filter byte (0: none) before every row
    raw[:, 1:] = bgr if gray else bgr[:, :, ::-1].reshape(h, 3 * w)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0 if gray else 2, 0, 0, 0)) +
                _chunk(b"IDAT", zlib.compress(raw.tobytes(), int(level))) + _chunk(b"IEND", b""))
