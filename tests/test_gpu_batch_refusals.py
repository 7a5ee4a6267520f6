"""GPU: what the batch entries refuse, and that a refusal writes nothing.

test_gpu_streams_ragged.py::test_refusals_leave_the_outputs_untouched does this for the ragged entries; here the older batch
entries: evh_pair_homography_batch, evh_stream_homography_batch and its _resized / _yuv420 forms,
evh_multi_stream_homography_batch, the _types forms and evh_stream_static_batch.  Every rule an entry enforces is broken once,
and a handful of inputs break two rules of different error classes at once, which pins the order of the checks: NULL
arguments and minimum counts, the mode, max_frames, (row_cap,) the type list, the frame description, the geometry.  The
entries are called through ctypes: the Context wrapper cannot express most of the bad values.  Nothing is launched, so a
64 x 64 context of 4 frame slots is enough.  The codes are literals: they are what the entries returned before the batch
path was folded into evh_batch.hip."""
import ctypes as C

import numpy as np
import pytest
import torch

from evenvizion_amd._lib import Context, Yuv420, yuv420_size

pytestmark = pytest.mark.gpu

W = H = 64
MAXF = 4
HS, SS = -7.25, -9          # sentinels of float and integer outputs
INVALID, CAPACITY = -1, -3

# the argument order of every entry, in the names of `defaults` below
_RANSAC = ["thr", "mi", "conf", "fm"]
_STATE = ["sin", "sout", "H", "st"]
_PACKED = ["w", "h", "cn", "row", "frame"]
ENTRIES = {
    "pair": ("evh_pair_homography_batch", ["frames", "npairs", "mode"] + _PACKED + ["nf"] + _RANSAC + ["H", "st"]),
    "stream": ("evh_stream_homography_batch", ["frames", "n"] + _PACKED + ["nf"] + _RANSAC + _STATE),
    "resized": ("evh_stream_homography_batch_resized", ["frames", "n"] + _PACKED + ["dw", "dh", "nf"] + _RANSAC + _STATE),
    "yuv420": ("evh_stream_homography_batch_yuv420", ["yuv", "n", "w", "h", "dw", "dh", "nf"] + _RANSAC + _STATE),
    "multi": ("evh_multi_stream_homography_batch", ["frames", "S", "F"] + _PACKED + ["nf"] + _RANSAC + _STATE),
    "pair_types": ("evh_pair_homography_batch_types", ["frames", "npairs", "mode"] + _PACKED + ["dw", "dh", "nf", "types", "ntypes"] +
                   _RANSAC + ["H", "st"]),
    "stream_types": ("evh_stream_homography_batch_types", ["frames", "n"] + _PACKED + ["dw", "dh", "nf", "types", "ntypes"] +
                     _RANSAC + _STATE),
    "types_yuv420": ("evh_stream_homography_batch_types_yuv420", ["yuv", "n", "w", "h", "dw", "dh", "nf", "types", "ntypes"] +
                     _RANSAC + _STATE),
    "static": ("evh_stream_static_batch", ["frames", "n"] + _PACKED + ["nf"] + _RANSAC + ["rows", "row_cap", "counts", "st1"]),
}
PACKED_ENTRIES = ("pair", "stream", "resized", "multi", "pair_types", "stream_types", "static")
PLANE_ENTRIES = ("yuv420", "types_yuv420")
TYPES_ENTRIES = ("pair_types", "stream_types", "types_yuv420")


def _cases():
    """(entry, what is wrong, overrides of the valid call, expected code)"""
    out = []
    for e in ENTRIES:
        few = {"pair": dict(npairs=0), "pair_types": dict(npairs=0), "multi": dict(F=1)}.get(e, dict(n=1))
        many = {"pair": dict(npairs=3), "pair_types": dict(npairs=3), "multi": dict(S=3)}.get(e, dict(n=5))
        outs = ("rows", "counts", "st1") if e == "static" else ("H", "st")
        for k in outs:
            out.append((e, "NULL " + k, {k: None}, INVALID))
            out.append((e, "NULL %s, too many frames" % k, dict(many, **{k: None}), INVALID))
        out.append((e, "too few", few, INVALID))
        out.append((e, "more than max_frames", many, CAPACITY))
        out.append((e, "nfeatures above max_features", dict(nf=501), CAPACITY))
        if e in PACKED_ENTRIES:
            out.append((e, "NULL frames", dict(frames=None), INVALID))
            out.append((e, "NULL frames, too many frames", dict(many, frames=None), INVALID))
            out.append((e, "2 channels", dict(cn=2, row=128), INVALID))
            out.append((e, "row_stride below a row", dict(row=63), INVALID))
            out.append((e, "empty frame", dict(w=0), INVALID))
            out.append((e, "too many frames, 2 channels", dict(many, cn=2, row=128), CAPACITY))
            out.append((e, "2 channels, nfeatures above max_features", dict(cn=2, row=128, nf=501), INVALID))
        if e in PLANE_ENTRIES:
            out.append((e, "NULL source", dict(yuv=None), INVALID))
            out.append((e, "NULL source, too many frames", dict(many, yuv=None), CAPACITY))
            out.append((e, "NULL luma plane", dict(yuv=dict(d_y=None)), INVALID))
            out.append((e, "NULL Cb plane", dict(yuv=dict(d_cb=None)), INVALID))
            out.append((e, "NULL Cr plane", dict(yuv=dict(d_cr=None)), INVALID))
            out.append((e, "luma stride below the width", dict(yuv=dict(y_stride=W - 1)), INVALID))
            out.append((e, "chroma stride below a chroma row", dict(yuv=dict(c_stride=W // 2 - 1)), INVALID))
            out.append((e, "chroma pixel stride 3", dict(yuv=dict(c_pixel_stride=3)), INVALID))
            out.append((e, "luma frame stride below a plane", dict(yuv=dict(y_frame_stride=W * H - 1)), INVALID))
            out.append((e, "chroma frame stride below a plane", dict(yuv=dict(c_frame_stride=W * H // 4 - 1)), INVALID))
            out.append((e, "empty frame", dict(w=0), INVALID))
            out.append((e, "too many frames, NULL Cb plane", dict(many, yuv=dict(d_cb=None)), CAPACITY))
        if e in ("pair", "pair_types"):
            out.append((e, "unknown mode", dict(mode=2), INVALID))
            out.append((e, "negative mode", dict(mode=-1), INVALID))
            out.append((e, "stream mode, more than max_frames", dict(mode=1, npairs=4), CAPACITY))
            out.append((e, "unknown mode, too many frames", dict(mode=2, npairs=3), INVALID))
        if e == "multi":
            out.append((e, "no stream", dict(S=0), INVALID))
            out.append((e, "frame count beyond 32 bits", dict(S=65536, F=65536), CAPACITY))
        if e == "resized":
            out.append((e, "working size above the context's", dict(dw=128), CAPACITY))
        if e in TYPES_ENTRIES:
            out.append((e, "empty type list", dict(types=[]), INVALID))
            out.append((e, "NULL type list", dict(types=None, ntypes=1), INVALID))
            out.append((e, "nine types", dict(types=[0] * 9), INVALID))
            out.append((e, "a type twice", dict(types=[0, 0]), INVALID))
            out.append((e, "unknown type", dict(types=[7]), INVALID))
            out.append((e, "SIFT not enabled", dict(types=[1, 0]), INVALID))
            out.append((e, "SURF not enabled", dict(types=[0, 2]), INVALID))
            out.append((e, "too many frames, unknown type", dict(many, types=[7]), CAPACITY))
            out.append((e, "unknown type, nfeatures above max_features", dict(types=[7], nf=501), INVALID))
        if e == "static":
            out.append((e, "row_cap below the capacity", dict(row_cap=-1), INVALID))
            out.append((e, "row_cap above the capacity", dict(row_cap=+1), INVALID))
            out.append((e, "too many frames, wrong row_cap", dict(n=5, row_cap=+1), CAPACITY))
            out.append((e, "wrong row_cap, nfeatures above max_features", dict(row_cap=+1, nf=501), INVALID))
    # types_yuv420 converts the planes before the geometry is configured: its nfeatures refusal comes after a launch
    return [c for c in out if not (c[0] == "types_yuv420" and c[1] == "nfeatures above max_features")]


CASES = _cases()


@pytest.fixture(scope="module")
def box():
    c = Context(device=0, max_w=W, max_h=H, max_features=500, max_frames=MAXF)
    cap = c.lib.evh_orb_capacity(c.h)
    b = dict(ctx=c, cap=cap,
             frames=torch.zeros(MAXF + 2, H, 2 * W, dtype=torch.uint8, device="cuda"),       # room for every size a case names
             packed=torch.zeros(MAXF + 2, yuv420_size(W, H)[0], dtype=torch.uint8, device="cuda"),
             H=torch.empty(MAXF + 2, 9, dtype=torch.float64, device="cuda"), st=torch.empty(MAXF + 2, dtype=torch.int32, device="cuda"),
             sout=torch.empty(MAXF, 18, dtype=torch.float64, device="cuda"),
             rows=torch.empty(MAXF + 1, cap, 4, dtype=torch.float32, device="cuda"),
             counts=torch.empty(MAXF + 1, dtype=torch.int32, device="cuda"), st1=torch.empty(MAXF + 1, dtype=torch.int32, device="cuda"))
    yield b
    c.close()


def _args(b, entry, over):
    c = b["ctx"]
    for k in ("H", "sout", "rows"):
        b[k].fill_(HS)
    for k in ("st", "counts", "st1"):
        b[k].fill_(SS)
    torch.cuda.synchronize()
    p = b["packed"].data_ptr()
    cw, ch = W // 2, H // 2
    yuv = dict(d_y=p, d_cb=p + W * H, d_cr=p + W * H + cw * ch, y_stride=W, c_stride=cw, y_frame_stride=b["packed"].stride(0),
               c_frame_stride=b["packed"].stride(0), c_pixel_stride=1)
    v = dict(frames=b["frames"].data_ptr(), npairs=2, mode=0, n=MAXF, S=2, F=2, w=W, h=H, cn=1, row=W, frame=b["frames"].stride(0),
             dw=W, dh=H, nf=500, types=[0], thr=3.0, mi=2000, conf=0.995, fm=0, sin=None, sout=b["sout"].data_ptr(),
             H=b["H"].data_ptr(), st=b["st"].data_ptr(), rows=b["rows"].data_ptr(), row_cap=b["cap"], counts=b["counts"].data_ptr(),
             st1=b["st1"].data_ptr(), yuv=yuv)
    over = dict(over)
    if isinstance(over.get("yuv"), dict):
        over["yuv"] = dict(yuv, **over["yuv"])
    if "row_cap" in over:
        over["row_cap"] = b["cap"] + over["row_cap"]
    v.update(over)
    keep = []
    if v["types"] is not None:
        t = np.ascontiguousarray(v["types"] or [0], np.int32)      # (an empty list still hands over a pointer)
        keep.append(t)
        v.setdefault("ntypes", len(v["types"]))
        v["types"] = t.ctypes.data_as(C.c_void_p)
    if v["yuv"] is not None:
        y = Yuv420(**v["yuv"])
        keep.append(y)
        v["yuv"] = C.byref(y)
    sym, order = ENTRIES[entry]
    return getattr(c.lib, sym), [c.h] + [v[k] for k in order], keep


@pytest.mark.parametrize("entry,what,over,code", CASES, ids=["%s-%s" % (c[0], c[1].replace(" ", "_")) for c in CASES])
def test_refusal_leaves_the_outputs_untouched(box, entry, what, over, code):
    fn, args, keep = _args(box, entry, over)
    rc = fn(*args)
    box["ctx"].synchronize()
    print("%s, %s: returned %d, expected %d" % (entry, what, rc, code))
    assert rc == code, (entry, what, rc, box["ctx"].lib.evh_last_error_string(box["ctx"].h).decode())
    for k in ("H", "sout", "rows"):
        assert bool((box[k] == HS).all()), (entry, what, k)
    for k in ("st", "counts", "st1"):
        assert bool((box[k] == SS).all()), (entry, what, k)


def test_a_refused_context_still_says_which_entry_refused(box):
    """Every message begins with the name of the entry that was called (the NULL-output refusal of each)."""
    c = box["ctx"]
    for entry, (sym, _) in ENTRIES.items():
        fn, args, keep = _args(box, entry, {"rows" if entry == "static" else "H": None})
        assert fn(*args) == INVALID
        assert c.lib.evh_last_error_string(c.h).decode().startswith(sym + ":"), (sym, c.lib.evh_last_error_string(c.h))
