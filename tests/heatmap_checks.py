"""numpy restatement of evh_heatmap_render (include/evhip.h) from the field onward: every operation below is one IEEE float64
operation on arrays, in the order the header states, so the device must agree with it byte for byte.

    color_index(field, heatmap_constant, saturate)           -> i64[..., h, w], the colour index of field f64[..., h, w, 2]
    blend(c, p, alpha)                                       -> u8, one table byte over one frame byte
    render(field, lut, frames, heatmap_constant, alpha, saturate)
                                                             -> u8[n,h,w,3], what evh_heatmap_render stores
    oracle_field(Hs, w, h)                                   -> f64[n,h,w,2]

The field itself is fma(h0, x, h1*y) + h2 and one division per coordinate; numpy has no fused multiply-add, so a test takes the
field from the reference-captured grids of tests/golden/plane_goldens.json or from the CPU oracle (oracle_field), whose fields
test_oracle_glue.py pins to the reference's bit for bit, and the device's own field is pinned to both by test_gpu_plane.py.
"""
import numpy as np


def color_index(field, heatmap_constant=1000.0, saturate=False):
    field = np.asarray(field, np.float64)
    with np.errstate(all="ignore"):
        u, v = field[..., 0], field[..., 1]
        s = u * u + v * v                                   # each product rounded, then the sum
        r = np.sqrt(s)
        t = 255.0 * (r / np.float64(heatmap_constant))      # a true division, then the product
        ok = np.isfinite(t) & (t >= 0) & (t < 2.0 ** 31)
        i = np.where(ok, t, 0.0).astype(np.int64) & 255     # the cast truncates
        if saturate:
            i = np.where(t >= 255.0, 255, i)                # +inf included; NaN fails the comparison and stays 0
    return i


def blend(c, p, alpha):
    """rint((double)c * alpha + (double)p), halves to even, clamped to [0, 255]."""
    c, p = np.asarray(c, np.float64), np.asarray(p, np.float64)
    with np.errstate(all="ignore"):
        o = np.rint(c * np.float64(alpha) + p)
    return np.clip(o, 0, 255).astype(np.uint8)


def render(field, lut, frames=None, heatmap_constant=1000.0, alpha=0.8, saturate=False):
    field = np.asarray(field, np.float64)
    field = field.reshape((-1,) + field.shape[-3:])
    lut = np.asarray(lut)
    assert lut.dtype == np.uint8 and lut.shape == (256, 3)
    colours = lut[color_index(field, heatmap_constant, saturate)]
    under = np.zeros_like(colours) if frames is None else np.asarray(frames, np.uint8).reshape(colours.shape)
    return blend(colours, under, alpha)


def oracle_field(Hs, w, h):
    from oracle import oracle as O
    return O.fixed_plane_field(np.asarray(Hs, np.float64).reshape(-1, 3, 3), w, h)[0]
