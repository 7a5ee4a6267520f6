"""Pictures that leave the device compressed: baseline JPEG files encoded by evh_jpeg_encode (include/evhip.h) where the
canvases lie, and a Motion-JPEG AVI writer for a player to open.  Only the files' bytes cross the host link.

    quant_tables(quality)   the Annex K.1 / K.2 tables scaled by the usual rule;
    encode_jpeg(pictures)   a list of files (bytes) for gray [n,h,w] or BGR [n,h,w,3] pictures, arrays or device tensors;
    write_jpeg(path, data)  one file;
    MjpegAviWriter          RIFF "AVI " with one MJPG video stream and an idx1 index, below 2 GiB (no OpenDML).
"""
import struct

import numpy as np

from . import runtime

# T.81 Annex K.1 (luminance) and K.2 (chrominance), natural order
_K1 = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
       18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
       103, 99)
_K2 = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + \
      (99,) * 32
SUBSAMPLINGS = ("420", "444")


def quant_tables(quality):
    """uint16 [2, 64], natural order: (base * s + 50) // 100 clamped to 1..255, s = 5000 // quality below 50, else
    200 - 2 * quality; quality in 1..100."""
    quality = int(quality)
    if not 1 <= quality <= 100:
        raise ValueError("quality must lie in 1..100")
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.stack([np.clip((np.array(b, np.int64) * s + 50) // 100, 1, 255) for b in (_K1, _K2)]).astype(np.uint16)


def check_format(quality, subsampling):
    """The refusals every JPEG writer here shares, before anything is opened."""
    if not 1 <= int(quality) <= 100:
        raise ValueError("quality must lie in 1..100")
    if subsampling not in SUBSAMPLINGS:
        raise ValueError("subsampling must be '420' or '444'")


def encode_jpeg(pictures, quality=90, subsampling="420"):
    """Files (a list of bytes) of pictures [n,h,w] gray or [n,h,w,3] BGR, or of one picture [h,w,3] (a 3-D input whose last extent is 3 is one BGR picture).  numpy arrays are uploaded,
    device tensors -- also strided views of a larger canvas -- are encoded where they lie.  Gray pictures have no chroma to
    sub-sample: they are written 4:4:4 layout-wise (one component)."""
    import torch
    check_format(quality, subsampling)
    if isinstance(pictures, np.ndarray):
        pictures = torch.from_numpy(np.ascontiguousarray(pictures)).to(runtime.device())
    if pictures.dim() == 3 and pictures.shape[-1] == 3:
        pictures = pictures[None]
    ctx = runtime.get_context(64, 64)             # the entry works on caller buffers of any size
    return ctx.jpeg_encode(pictures, quant_tables(quality), "444" if pictures.dim() == 3 else subsampling)


def jpegs_of_chunks(chunks, mosaic, quality, subsampling):
    """The tail of stabilization.stabilized_jpegs and surface.surface_jpegs: every chunk's canvases (stabilization._canvas_chunks)
    encoded where they lie, as (frame_no, bytes); with `mosaic` the carried canvas once, after the last chunk.  Only the files
    come to the host."""
    ctx, tables = runtime.get_context(64, 64), quant_tables(quality)
    frame_no, canvas = 0, None
    for first, n, pictures, _, canvas in chunks:
        frame_no = first + n - 1
        if pictures is not None:
            for k, data in enumerate(ctx.jpeg_encode(pictures, tables, subsampling)):
                yield first + k, data
    if mosaic and canvas is not None:
        yield frame_no, ctx.jpeg_encode(canvas[None], tables, subsampling)[0]


def write_jpeg(path, data):
    with open(path, "wb") as f:
        f.write(data)


class MjpegAviWriter:
    """Motion-JPEG in RIFF "AVI ": hdrl (avih, one strl with strh "vids"/"MJPG" and strf BITMAPINFOHEADER), movi with one "00dc"
    chunk per frame padded to even length, idx1.  The sizes and the frame counts are patched by close().  A frame that would
    take the file past 2 GiB - 1 is refused (ValueError); OpenDML is not written."""
    LIMIT = (1 << 31) - 1

    def __init__(self, path, w, h, fps):
        if not (1 <= int(w) <= 65535 and 1 <= int(h) <= 65535) or not fps > 0:
            raise ValueError("w and h must lie in 1..65535 and fps must be positive")
        self.w, self.h, self.index, self.largest = int(w), int(h), [], 0
        rate, scale = int(round(float(fps) * 1000)), 1000
        avih = struct.pack("<14I", int(round(1e6 / float(fps))), 0, 0, 0x10, 0, 0, 1, 0, self.w, self.h, 0, 0, 0, 0)
        strh = b"vidsMJPG" + struct.pack("<IHHIIIIIIIIHHHH", 0, 0, 0, 0, scale, rate, 0, 0, 0, 0xFFFFFFFF, 0, 0, 0, self.w, self.h)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.w, self.h, 1, 24, b"MJPG", self.w * self.h * 3, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        head = b"RIFF\0\0\0\0AVI LIST" + struct.pack("<I", len(hdrl)) + hdrl
        self.frames_at = (head.index(b"avih") + 8 + 16, head.index(b"strh") + 8 + 32)     # dwTotalFrames, dwLength
        self.largest_at = head.index(b"strh") + 8 + 36                                   # dwSuggestedBufferSize
        self.movi_at = len(head)
        self.f = open(path, "wb")
        self.f.write(head + b"LIST\0\0\0\0movi")
        self.size = self.movi_at + 12

    def write(self, data):
        data = bytes(data)
        padded = len(data) + (len(data) & 1)
        if self.size + 8 + padded + 8 + 16 * (len(self.index) + 1) > self.LIMIT:
            raise ValueError("the AVI file would pass 2 GiB; OpenDML is not written")
        self.index.append((self.size - (self.movi_at + 8), len(data)))       # offset of the chunk from the "movi" tag
        self.f.write(b"00dc" + struct.pack("<I", len(data)) + data + b"\0" * (padded - len(data)))
        self.size += 8 + padded
        self.largest = max(self.largest, len(data))

    def close(self):
        if self.f is None:
            return
        f, self.f = self.f, None
        idx = b"".join(b"00dc" + struct.pack("<III", 0x10, off, n) for off, n in self.index)
        f.write(b"idx1" + struct.pack("<I", len(idx)) + idx)
        total = self.size + 8 + len(idx)
        for at, value in ((4, total - 8), (self.movi_at + 4, self.size - self.movi_at - 8), (self.frames_at[0], len(self.index)),
                          (self.frames_at[1], len(self.index)), (self.largest_at, self.largest)):
            f.seek(at)
            f.write(struct.pack("<I", value))
        f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
