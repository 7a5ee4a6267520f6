"""Scripted captures for the host-loop tests of the second-pass drivers: every frame carries its 0-based position in the capture
in its first byte, and the capture counts what it was asked for."""
import numpy as np

from evenvizion_amd import capture

W0, H0 = 12, 6          # the frames of every scripted capture; resized_shape gives 8 x 4 for resize_width 8


class Cap:
    """read() delivers n frames of `shape` ([h,w,3] BGR or [h,w] gray); `odd` = {position: another shape}."""

    def __init__(self, n, shape=(H0, W0, 3), odd=None):
        self.n, self.i, self.shape, self.odd = n, 0, shape, dict(odd or {})
        self.calls, self.failed = 0, 0

    def _next(self):
        """The position of the frame this call delivers, or None; counts the call."""
        self.calls += 1
        if self.i >= self.n:
            self.failed += 1
            return None
        self.i += 1
        return self.i - 1

    def read(self):
        i = self._next()
        if i is None:
            return False, None
        f = np.zeros(self.odd.get(i, self.shape), np.uint8)
        f.reshape(-1)[0] = i
        return True, f


class PlaneCap(Cap):
    """The same frames as 4:2:0 planes (the position sits in the first luma byte); refuse: raises CaptureError before a frame
    is consumed, as libevcap does for an odd crop offset."""
    bgr_mode = capture.BGR_SWSCALE_X86

    def __init__(self, n, refuse=False):
        Cap.__init__(self, n)
        self.width, self.height, self.refuse = W0, H0, refuse

    def read_yuv420_into(self, y, cb, cr):
        if self.refuse:
            raise capture.CaptureError("libevcap: odd crop offset")
        i = self._next()
        if i is None:
            return False
        y[...] = 0
        cb[...] = 128
        cr[...] = 128
        y[0, 0] = i
        return True


def make(form, n):
    """A capture of n frames and the ingest that reads it as `form`: "bgr", "gray" or "planes"."""
    if form == "planes":
        return PlaneCap(n), "auto"
    return Cap(n, (H0, W0) if form == "gray" else (H0, W0, 3)), "bgr"


def spans(total, size, overlap):
    """[(position of the first frame, frames)] of the chunks a driver takes `total` frames in."""
    out, start = [], 0
    while min(size, total - start) > overlap:
        n = min(size, total - start)
        out.append((start, n))
        start += n - overlap
    return out
