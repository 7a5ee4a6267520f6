"""evh_mask_components restated in plain Python and numpy (include/evhip.h states the contract): opening by the two definitions
as loops, breadth-first flood fill in raster order, numbering by first pixel, the table as exact Python integers.  Slow and
obvious on purpose: it is what the device result must equal."""
from collections import deque

import numpy as np

FIELDS = ("x0", "y0", "x1", "y1", "area", "first", "sx", "sy")


def opening(fg, r):
    """fg: bool [h,w].  E set iff every pixel of the (2r+1)^2 square lies inside and is set; O set iff some pixel of the
    square lies inside and has E set."""
    h, w = fg.shape
    if r == 0:
        return fg.copy()
    E = np.zeros((h, w), bool)
    for y in range(h):
        for x in range(w):
            ok = True
            for j in range(-r, r + 1):
                for i in range(-r, r + 1):
                    yy, xx = y + j, x + i
                    if not (0 <= yy < h and 0 <= xx < w and fg[yy, xx]):
                        ok = False
            E[y, x] = ok
    out = np.zeros((h, w), bool)
    for y in range(h):
        for x in range(w):
            hit = False
            for j in range(-r, r + 1):
                for i in range(-r, r + 1):
                    yy, xx = y + j, x + i
                    if 0 <= yy < h and 0 <= xx < w and E[yy, xx]:
                        hit = True
            out[y, x] = hit
    return out


def neighbours(connectivity):
    if connectivity == 4:
        return ((0, -1), (-1, 0), (1, 0), (0, 1))
    if connectivity == 8:
        return ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))
    raise ValueError("connectivity must be 4 or 8")


def components(mask, connectivity=8, open_radius=0, min_area=1):
    """mask: [h,w], non-zero = set.  -> (labels int32 [h,w], objects: a list of dicts with FIELDS as Python ints, in number
    order).  Components are met in raster order, so they are met in order of their first pixel."""
    fg = opening(np.asarray(mask) != 0, open_radius)
    h, w = fg.shape
    nb = neighbours(connectivity)
    seen = np.zeros((h, w), bool)
    labels = np.zeros((h, w), np.int32)
    objects = []
    for y in range(h):
        for x in range(w):
            if not fg[y, x] or seen[y, x]:
                continue
            seen[y, x] = True
            queue, pixels = deque([(x, y)]), []
            while queue:
                px, py = queue.popleft()
                pixels.append((px, py))
                for i, j in nb:
                    qx, qy = px + i, py + j
                    if 0 <= qx < w and 0 <= qy < h and fg[qy, qx] and not seen[qy, qx]:
                        seen[qy, qx] = True
                        queue.append((qx, qy))
            if len(pixels) < min_area:
                continue
            number = len(objects) + 1
            xs, ys = [p[0] for p in pixels], [p[1] for p in pixels]
            for px, py in pixels:
                labels[py, px] = number
            objects.append({"x0": min(xs), "y0": min(ys), "x1": max(xs), "y1": max(ys), "area": len(pixels), "first": y * w + x,
                            "sx": sum(xs), "sy": sum(ys)})
    return labels, objects


def table(objects):
    """The objects as tuples in FIELDS order."""
    return [tuple(int(o[f]) for f in FIELDS) for o in objects]
