"""Frames from a capture to the device, for every driver that reads a video: opening (4:2:0 planes where the capture delivers
them, else BGR), the one host copy of a frame, the chunk loop (FrameReader) and the steps between an uploaded chunk and the
entry that consumes it (DeviceLadder: planes to BGR, gray to three channels, the area resize).  DESIGN.md section 18."""
import logging

import numpy as np


def check_ingest(ingest):
    if ingest not in ("auto", "bgr", "yuv420"):
        raise ValueError("ingest must be 'auto', 'bgr' or 'yuv420'")


def first_planes(capture, ingest):
    """The first frame of `capture` as packed I420 bytes, or None when the frames are to be read as BGR.  Planes are taken
    when the capture offers read_yuv420_into(y, cb, cr), declares the conversion the device implements (bgr_mode ==
    BGR_SWSCALE_X86) and its first plane read succeeds -- a capture refuses, by raising capture.CaptureError, BEFORE it consumes a frame (libevcap: odd crop
    offset), so the BGR path then starts from the same first frame.  -> (packed uint8 array or None, w, h)."""
    from .capture import BGR_SWSCALE_X86, CaptureError
    from ._lib import yuv420_size, yuv420_views
    able = callable(getattr(capture, "read_yuv420_into", None)) and getattr(capture, "bgr_mode", None) == BGR_SWSCALE_X86
    if ingest == "bgr" or not able:
        if ingest == "yuv420":
            raise ValueError("ingest='yuv420': the capture does not deliver 4:2:0 planes in the swscale-x86 conversion")
        return None, 0, 0
    w, h = int(capture.width), int(capture.height)
    packed = np.empty((1, yuv420_size(w, h)[0]), np.uint8)
    y, cb, cr = yuv420_views(packed, w, h)
    try:
        ok = capture.read_yuv420_into(y[0], cb[0], cr[0])
    except CaptureError as e:               # the capture's refusal: nothing was consumed; anything else is a bug and propagates
        if ingest == "yuv420":
            raise ValueError("ingest='yuv420': the capture refused to deliver planes (%s)" % e)
        logging.info("capture refused 4:2:0 planes (%s): reading BGR frames", e)
        return None, 0, 0
    if not ok:
        raise ValueError("Problem with video! Can't read first frame")
    return packed[0], w, h


def open_capture(capture, ingest):
    """The first frame of `capture`: planes where first_planes takes them, else read().
    -> (first frame: packed I420 bytes or a BGR array, planes?, w0, h0)"""
    first, w0, h0 = first_planes(capture, ingest)
    if first is not None:
        return first, True, w0, h0
    success, first = capture.read()
    if not success:
        raise ValueError("Problem with video! Can't read first frame")
    first = np.ascontiguousarray(first, np.uint8)
    h0, w0 = first.shape[:2]
    return first, False, w0, h0


def read_frame(capture, planes, slot, w0, h0, number):
    """The capture's next frame (its `number`, 1-based, for the error) into `slot`, a frame of a host staging buffer: the
    one host copy.  -> False when the capture has no further frame."""
    if planes:
        from ._lib import yuv420_views
        y, cb, cr = yuv420_views(slot[None], w0, h0)
        return bool(capture.read_yuv420_into(y[0], cb[0], cr[0]))
    ok, frame = capture.read()
    if not ok:
        return False
    frame = np.asarray(frame, np.uint8)
    if frame.shape != slot.shape:
        raise ValueError("frame %d has shape %s, the first frame %s" % (number, frame.shape, slot.shape))
    slot[...] = frame
    return True


def entry_matrix(H):
    """A dictionary entry as f64[3,3]; None or a wrong size gives NaN (a frame that covers nothing, colour index 0 everywhere)."""
    if H is not None:
        m = np.asarray(H, np.float64)
        if m.size == 9:
            return m.reshape(3, 3)
    return np.full((3, 3), np.nan)


class FrameReader:
    """A capture from its first frame on.  first, planes, w0, h0: what open_capture found; consumed: the frames taken from the
    capture so far (the first one included); exhausted: the capture has said that it has no further frame, and is not asked
    again."""

    def __init__(self, capture, ingest):
        self.capture = capture
        self.first, self.planes, self.w0, self.h0 = open_capture(capture, ingest)
        self.consumed, self.exhausted = 1, False

    def buffer(self, frames):
        """A host buffer of `frames` frames with the first frame in slot 0."""
        host = np.empty((frames,) + self.first.shape, np.uint8)
        host[0] = self.first
        return host

    def read_into(self, slot):
        """The next frame into `slot` -> False when there is none.  A frame of another shape than the first is a ValueError
        naming its 1-based number."""
        if self.exhausted or not read_frame(self.capture, self.planes, slot, self.w0, self.h0, self.consumed + 1):
            self.exhausted = True
            return False
        self.consumed += 1
        return True

    def chunks(self, size, overlap, limit=None):
        """Generator of (start, frames): frames = host[:n], valid until the next step, frames[0] being frame `start` (0-based)
        of the capture.  Consecutive chunks share `overlap` (0 .. size - 1) frames; every chunk has at least one frame no earlier
        chunk had and at least overlap + 1 frames.  No more than `limit` frames are consumed (the first one counts)."""
        if not 0 <= overlap < size:
            raise ValueError("chunks of %d frames cannot share %d" % (size, overlap))
        host = self.buffer(size)
        start, n = 0, 1
        while True:
            while n < size and (limit is None or self.consumed < limit) and self.read_into(host[n]):
                n += 1
            if n <= overlap:
                return
            yield start, host[:n]
            if overlap:
                host[:overlap] = host[n - overlap:n].copy()
            start, n = start + n - overlap, overlap


class DeviceLadder:
    """The steps between an uploaded chunk and the entry that consumes it, with their buffers: decoded planes to BGR
    (evh_yuv420_to_bgr), gray to three channels, the area resize to the working size (evh_resize_area_u8).

    capacity: the frames of the largest chunk; planes, (w0, h0): as FrameReader has them; work: the working size (w, h), or
    None when the entry takes full-size frames.  Planes are converted ahead of a resize (the resize takes BGR), and without
    one when `bgr`; gray frames [n,h,w] become B = G = R when `gray3`.  Only the buffers this rule needs are allocated."""

    def __init__(self, dev, capacity, planes, size0, work=None, bgr=False, gray3=False):
        import torch
        (w0, h0), self.planes, self.size0, self.gray3 = size0, planes, tuple(size0), gray3
        resize = work is not None and tuple(work) != self.size0
        self.bgr = torch.empty((capacity, h0, w0, 3), dtype=torch.uint8, device=dev) if planes and (resize or bgr) else None
        self.small = torch.empty((capacity, work[1], work[0], 3), dtype=torch.uint8, device=dev) if resize else None

    def __call__(self, ctx, frames):
        """frames: a chunk on the device, as uploaded -> (full, src, size): the full-size frames (BGR when they were converted),
        the frames for the entry, and the size= that entry must be given (None unless src is still packed planes)."""
        n = frames.shape[0]
        full = src = frames
        size = self.size0 if self.planes else None
        if self.bgr is not None:
            ctx.yuv420_to_bgr(src, self.bgr[:n], size=size)
            full = src = self.bgr[:n]
            size = None
        elif self.gray3 and src.dim() == 3:
            full = src = src[..., None].expand(-1, -1, -1, 3).contiguous()
        if self.small is not None:
            ctx.resize_area(src, self.small[:n])
            src = self.small[:n]
        return full, src, size
