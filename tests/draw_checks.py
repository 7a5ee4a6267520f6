"""Plain Python / numpy restatement of evh_draw_matches (include/evhip.h): the paste of the two frames, Python's int() on the
coordinates, the skip rules and OpenCV 3.4.2's 8-connected LineIterator as the literal err loop.  The closed form the kernel
uses appears here only as `closed_form`, for the host test that compares it with the loop."""
import math

import numpy as np

REFERENCE, OWN_FRAME = 0, 1


def line_pixels(pt1, pt2):
    """The pixels cv2.line(img, pt1, pt2, colour, 1) visits before clipping, in the order of the walk."""
    x1, y1 = pt1
    x2, y2 = pt2
    dx, dy = x2 - x1, y2 - y1
    if dx < 0:                                  # leftToRight: start at the left end
        x1, y1, dx, dy = x2, y2, -dx, -dy
    sy = -1 if dy < 0 else 1
    dy = abs(dy)
    steep = dy > dx                             # the major axis is y
    D, d = (dy, dx) if steep else (dx, dy)
    err = D - 2 * d
    x, y = x1, y1
    out = []
    for _ in range(D + 1):
        out.append((x, y))
        if err < 0:                             # the minor axis steps
            if steep:
                x += 1
            else:
                y += sy
            err += 2 * D
        if steep:                               # the major axis steps, always
            y += sy
        else:
            x += 1
        err -= 2 * d
    return out


def closed_form(pt1, pt2):
    """The same pixels from the minor offset (2*d*k + D - 1) div (2*D) of pixel k."""
    x1, y1 = pt1
    x2, y2 = pt2
    dx, dy = x2 - x1, y2 - y1
    if dx < 0:
        x1, y1, dx, dy = x2, y2, -dx, -dy
    sy = -1 if dy < 0 else 1
    dy = abs(dy)
    steep = dy > dx
    D, d = (dy, dx) if steep else (dx, dy)
    out = []
    for k in range(D + 1):
        m = (2 * d * k + D - 1) // (2 * D) if D > 0 else 0
        out.append((x1 + m, y1 + sy * k) if steep else (x1 + k, y1 + sy * m))
    return out


def ends(row, w, points):
    """(pt1, pt2) of a row (ax, ay, bx, by), or None when the row is skipped."""
    if not all(math.isfinite(float(v)) for v in row):
        return None
    t = [int(float(v)) for v in row]            # toward zero
    if any(v < -32768 or v > 32767 for v in t):
        return None
    ax, ay, bx, by = t
    if points == REFERENCE:
        return (ax, ay), (bx + w, by)
    return (bx, by), (ax + w, ay)


def picture(prev, cur, rows, points=REFERENCE, color=(0, 255, 0)):
    """prev, cur: u8[h,w,3]; rows: the rows that are drawn, f32[n,4] -> u8[h,2w,3]."""
    h, w = prev.shape[:2]
    out = np.concatenate([prev, cur], axis=1).copy()
    for row in rows:
        e = ends(row, w, points)
        if e is None:
            continue
        for x, y in line_pixels(*e):
            if 0 <= x < 2 * w and 0 <= y < h:
                out[y, x] = color
    return out


def draw(frames, rows, counts, status=None, frame_step=1, points=REFERENCE, color=(0, 255, 0)):
    """frames u8[n,h,w,3], rows f32[npairs,cap,4], counts i32[npairs], status i32[npairs] or None -> u8[npairs,h,2w,3]."""
    npairs, cap = rows.shape[:2]
    h, w = frames.shape[1:3]
    out = np.zeros((npairs, h, 2 * w, 3), np.uint8)
    for p in range(npairs):
        n = min(max(int(counts[p]), 0), cap)
        if status is not None and int(status[p]) != 0:
            n = 0
        out[p] = picture(frames[p * frame_step], frames[p * frame_step + 1], rows[p, :n], points, color)
    return out
