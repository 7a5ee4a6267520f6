"""Stand-alone probe of evh_plate_fixed_plane: time per launch and samples per second for
    paste64    64 frames of 400x224 pasted at integer translations along a pan (6 pixels right, 1 down per frame),
    warp64     64 frames of 1280x720 warped (a slow rotation, zoom and drift, so nearly every sample takes four taps),
    paste255   255 frames of 400x224, the most one call takes,
each from BGR frames and from the same frames as 4:2:0 planes, with the per-frame masks and without (the count is always stored).
A sample is one frame evaluated at one canvas pixel -- the float64 map, two divisions and the coverage test, whether the frame
covers the pixel or not; covered_share says how many of them go on to read taps.
For scale, on the same buffers and matrices: evh_warp_fixed_plane EVH_WARP_MOSAIC, which samples a pixel's frames from the last
one down and stops at the first that covers it; and, once per case, the route the entry replaces -- EVH_WARP_EACH into n full
canvases, their download, numpy.median on the host (that median also counts the black of uncovered frames: it is the cost that
is shown, not the same picture).
Device time between two events around a run of launches filling a window of seconds, after a warm-up (as tools/warp_probe.py).
usage: python tools/plate_probe.py [seconds per case, default 1] [0 = leave out the host route]"""
import os, sys, time, json
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np, torch
from evenvizion_amd._lib import Context
window = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
host_route = len(sys.argv) < 3 or sys.argv[2] != '0'
ctx = Context(device=0, max_w=64, max_h=64, max_features=500, max_frames=2)
stream = ctx._torch_stream()
rng = np.random.default_rng(16)
res = {}


def pan(n, step_x, every_y):
    return [[1, 0, step_x * k, 0, 1, k // every_y, 0, 0, 1] for k in range(n)]


def drift(n):
    mats = []
    for k in range(n):
        th = np.deg2rad(-2 + 0.06 * k)
        c, s = 1.02 * np.cos(th), 1.02 * np.sin(th)
        mats.append([c, -s, 40.5 + 2.3 * k, s, c, 30.25 + 0.7 * k, 2e-6, -1e-6, 1])
    return mats


for name, w, h, mats, dw, dh in (('paste64', 400, 224, pan(64, 6, 1), 400 + 6 * 63, 224 + 63),
                                 ('warp64', 1280, 720, drift(64), 1536, 864),
                                 ('paste255', 400, 224, pan(255, 2, 4), 400 + 2 * 254, 224 + 63)):
    n = len(mats)
    bgr = torch.from_numpy(rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)).cuda()
    cw, ch = w // 2, h // 2
    planes = torch.from_numpy(rng.integers(0, 256, (n, w * h + 2 * cw * ch), dtype=np.uint8)).cuda()
    mats = torch.tensor(mats, dtype=torch.float64, device='cuda')
    plate = torch.zeros((dh, dw, 3), dtype=torch.uint8, device='cuda')
    count = torch.zeros((dh, dw), dtype=torch.uint8, device='cuda')
    masks = torch.zeros((n, dh, dw), dtype=torch.uint8, device='cuda')
    mosaic = torch.zeros((dh, dw, 3), dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    cases = {
        'bgr': lambda: ctx.plate_fixed_plane(bgr, mats, plate, (0, 0), count=count),
        'bgr_masks': lambda: ctx.plate_fixed_plane(bgr, mats, plate, (0, 0), count=count, masks=masks),
        'yuv420': lambda: ctx.plate_fixed_plane(planes, mats, plate, (0, 0), count=count, size=(w, h)),
        'yuv420_masks': lambda: ctx.plate_fixed_plane(planes, mats, plate, (0, 0), count=count, masks=masks, size=(w, h)),
        'mosaic_bgr': lambda: ctx.warp_fixed_plane(bgr, mats, mosaic, 'mosaic', (0, 0)),
        'mosaic_yuv420': lambda: ctx.warp_fixed_plane(planes, mats, mosaic, 'mosaic', (0, 0), size=(w, h)),
    }
    for case, launch in cases.items():
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
        covered = float(count.sum(dtype=torch.int64).cpu()) / (n * dw * dh)
        res['%s_%s' % (name, case)] = dict(frames=n, frame='%dx%d' % (w, h), canvas='%dx%d' % (dw, dh), launches=reps,
                                           device_us_per_launch=round(dev_s / reps * 1e6, 1),
                                           host_us_per_launch=round(host_s / reps * 1e6, 1),
                                           samples_per_launch=n * dw * dh, Gsamples_per_s=round(n * dw * dh * reps / dev_s * 1e-9, 2),
                                           canvas_Mpixels_per_s=round(dw * dh * reps / dev_s * 1e-6, 1), covered_share=round(covered, 3))
        print(json.dumps({'%s_%s' % (name, case): res['%s_%s' % (name, case)]}), flush=True)
    for kind in ('bgr', 'yuv420'):
        res['%s_plate_over_mosaic_%s' % (name, kind)] = round(res['%s_%s' % (name, kind)]['device_us_per_launch'] /
                                                              res['%s_mosaic_%s' % (name, kind)]['device_us_per_launch'], 2)
    if host_route and name != 'paste255':
        each = torch.zeros((n, dh, dw, 3), dtype=torch.uint8, device='cuda')
        ctx.warp_fixed_plane(bgr, mats, each, 'each', (0, 0))
        ctx.synchronize()
        t0 = time.perf_counter()
        ctx.warp_fixed_plane(bgr, mats, each, 'each', (0, 0))
        ctx.synchronize()
        t1 = time.perf_counter()
        host = each.cpu().numpy()
        t2 = time.perf_counter()
        np.median(host, axis=0)
        t3 = time.perf_counter()
        res['%s_download_and_numpy' % name] = dict(canvases_bytes=each.numel(), warp_each_ms=round((t1 - t0) * 1e3, 2),
                                                   download_ms=round((t2 - t1) * 1e3, 1), numpy_median_ms=round((t3 - t2) * 1e3, 1),
                                                   total_ms=round((t3 - t0) * 1e3, 1))
        print(json.dumps({'%s_download_and_numpy' % name: res['%s_download_and_numpy' % name]}), flush=True)
        del each, host
    del bgr, planes, masks
ctx.close()
print(json.dumps(res))
