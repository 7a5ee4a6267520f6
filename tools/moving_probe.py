"""Stand-alone probe of evh_rows_moving_filter: device time of one launch for
    small    120 pairs x 500 rows on 121 frames of 400x224,
    large     64 pairs x 2000 rows on 65 frames of 1280x720,
at radius 0, 1 and 7, from BGR frames and from 4:2:0 planes.  The frames are windows panning over one random panorama (6 pixels
right per frame, 2 down every second frame, so that chroma samples stay aligned), each with its own block of noise that stands in
for a moving object; plate and count come from evh_plate_fixed_plane over the same frames with min_cover = 2; the rows are random
points of the frames (a on the current frame, b on the previous one, unrelated: only their cost is of interest).  moving_share says
how many rows the filter dropped, judged_share how many of the window pixels went on to be sampled (inside the canvas and counted
at least min_cover times).
Beside it, once per case and radius, the only other route the library offers: evh_plate_fixed_plane with masks for the same frames
(device time of that launch), the download of rows and masks, and the numpy look-up of every window pixel in the masks on the host.
Device time between two events around a run of launches filling a window of seconds, after a warm-up (as tools/plate_probe.py).
usage: python tools/moving_probe.py [seconds per case, default 1] [0 = leave out the host route]"""
import os, sys, time, json
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np, torch
from evenvizion_amd._lib import Context
window = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
host_route = len(sys.argv) < 3 or sys.argv[2] != '0'
ctx = Context(device=0, max_w=64, max_h=64, max_features=500, max_frames=2)
stream = ctx._torch_stream()
rng = np.random.default_rng(17)
res = {}


def timed(launch):
    def run(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ctx.synchronize()
        t = time.perf_counter()
        e0.record(stream)
        for _ in range(reps):
            launch()
        e1.record(stream)
        ctx.synchronize()
        return e0.elapsed_time(e1) * 1e-3, time.perf_counter() - t
    run(2)
    per = run(4)[1] / 4
    reps = max(4, int(window / per))
    dev_s, host_s = run(reps)
    return reps, dev_s / reps * 1e6, host_s / reps * 1e6


for name, w, h, npairs, cap in (('small', 400, 224, 120, 500), ('large', 1280, 720, 64, 2000)):
    n = npairs + 1
    shift = [(6 * k, 2 * (k // 2)) for k in range(n)]
    dw, dh = w + shift[-1][0], h + shift[-1][1]
    cw, ch = w // 2, h // 2
    pano = rng.integers(0, 256, (dh, dw, 3), dtype=np.uint8)
    pano_y, pano_c = rng.integers(0, 256, (dh, dw), dtype=np.uint8), rng.integers(0, 256, (2, dh // 2, dw // 2), dtype=np.uint8)
    bgr = np.empty((n, h, w, 3), np.uint8)
    planes = np.empty((n, w * h + 2 * cw * ch), np.uint8)
    for k, (dx, dy) in enumerate(shift):
        bx, by = int(rng.integers(0, w - 64)) & ~1, int(rng.integers(0, h - 64)) & ~1       # the block of noise of this frame
        bgr[k] = pano[dy:dy + h, dx:dx + w]
        bgr[k, by:by + 64, bx:bx + 64] = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
        y = pano_y[dy:dy + h, dx:dx + w].copy()
        y[by:by + 64, bx:bx + 64] = rng.integers(0, 256, (64, 64), dtype=np.uint8)
        c = pano_c[:, dy // 2:dy // 2 + ch, dx // 2:dx // 2 + cw]
        planes[k] = np.concatenate([y.reshape(-1), c[0].reshape(-1), c[1].reshape(-1)])
    mats = torch.tensor([[1, 0, dx, 0, 1, dy, 0, 0, 1] for dx, dy in shift], dtype=torch.float64, device='cuda')
    rows_h = np.empty((npairs, cap, 4), np.float32)
    rows_h[..., 0::2] = rng.uniform(0, w - 1, (npairs, cap, 2))
    rows_h[..., 1::2] = rng.uniform(0, h - 1, (npairs, cap, 2))
    rows = torch.from_numpy(rows_h).cuda()
    counts = torch.full((npairs,), cap, dtype=torch.int32, device='cuda')
    status1 = torch.zeros(npairs, dtype=torch.int32, device='cuda')
    out_rows, out_counts = torch.zeros_like(rows), torch.zeros_like(counts)
    moving = torch.zeros_like(counts)
    flags = torch.zeros((npairs, cap), dtype=torch.uint8, device='cuda')
    masks = torch.zeros((n, dh, dw), dtype=torch.uint8, device='cuda')
    for kind, src, size in (('bgr', torch.from_numpy(bgr).cuda(), None), ('yuv420', torch.from_numpy(planes).cuda(), (w, h))):
        plate = torch.zeros((dh, dw, 3), dtype=torch.uint8, device='cuda')
        count = torch.zeros((dh, dw), dtype=torch.uint8, device='cuda')
        with_masks = lambda: ctx.plate_fixed_plane(src, mats, plate, (0, 0), count=count, masks=masks, threshold=16, min_cover=2, size=size)
        with_masks()
        ctx.synchronize()
        judged = float((count >= 2).sum().cpu()) / (dw * dh)
        plate_us = timed(with_masks)[1] if host_route else None
        for radius in (0, 1, 7):
            launch = lambda: ctx.rows_moving_filter(src, mats, plate, count, (0, 0), rows, counts, status1, out_rows, out_counts, moving,
                                                    flags, threshold=16, min_cover=2, radius=radius, min_hits=1, min_keep=8, size=size)
            reps, dev_us, host_us = timed(launch)
            key = '%s_%s_r%d' % (name, kind, radius)
            points = 2 * npairs * cap
            res[key] = dict(pairs=npairs, rows_per_pair=cap, frame='%dx%d' % (w, h), canvas='%dx%d' % (dw, dh), radius=radius,
                            launches=reps, device_us_per_launch=round(dev_us, 1), host_us_per_launch=round(host_us, 1),
                            window_pixels_per_launch=points * (2 * radius + 1) ** 2,
                            Gwindow_pixels_per_s=round(points * (2 * radius + 1) ** 2 / dev_us * 1e-3, 2),
                            moving_share=round(float(moving.sum().cpu()) / (npairs * cap), 3), canvas_judged_share=round(judged, 3))
            print(json.dumps({key: res[key]}), flush=True)
            if host_route:
                t0 = time.perf_counter()
                m, r = masks.cpu().numpy(), rows.cpu().numpy()
                t1 = time.perf_counter()
                gone = np.zeros((npairs, cap), bool)
                for cols, first in ((slice(0, 2), 1), (slice(2, 4), 0)):                    # a on frame p + 1, b on frame p
                    f = np.arange(first, first + npairs)[:, None]
                    cx = np.rint(r[..., cols][..., 0].astype(np.float64) + np.array(shift)[f, 0]).astype(np.int64)
                    cy = np.rint(r[..., cols][..., 1].astype(np.float64) + np.array(shift)[f, 1]).astype(np.int64)
                    for j in range(-radius, radius + 1):
                        for i in range(-radius, radius + 1):
                            X, Y = cx + i, cy + j
                            ok = (X >= 0) & (X < dw) & (Y >= 0) & (Y < dh)
                            gone |= ok & (m[f, np.where(ok, Y, 0), np.where(ok, X, 0)] != 0)
                t2 = time.perf_counter()
                agree = bool(np.array_equal(gone, flags.cpu().numpy() != 0))
                route = dict(plate_with_masks_us=round(plate_us, 1), download_ms=round((t1 - t0) * 1e3, 1),
                             numpy_lookup_ms=round((t2 - t1) * 1e3, 1), masks_bytes=masks.numel(), same_rows_flagged=agree)
                route['total_ms'] = round(plate_us * 1e-3 + route['download_ms'] + route['numpy_lookup_ms'], 1)
                route['over_filter'] = round(route['total_ms'] * 1e3 / dev_us, 1)
                res[key + '_host_route'] = route
                print(json.dumps({key + '_host_route': route}), flush=True)
        del src, plate, count
    del masks, rows, out_rows, flags
ctx.close()
print(json.dumps(res))
