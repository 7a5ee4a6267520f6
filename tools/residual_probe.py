"""Stand-alone probe of evh_pair_residual: time per launch and input bytes per second at 400x224 x 120 pairs and at
1280x720 x 64 pairs, from BGR frames and from the same number of frames as 4:2:0 planes, with the picture (d_out) and without.
Every pair has a small rotation, zoom and shift, so nearly every pixel is covered and interpolated from four taps.
Beside it, on the same BGR buffers and matrices, the route the library offered before this entry: evh_warp_fixed_plane,
EVH_WARP_EACH with inverse_map, into a second set of full BGR pictures, then torch -- the gray weights on both sets, the
difference, its square, and the four sums per pair (this route has no coverage: it sums over the whole frame, which costs it
nothing extra).  The torch work is enqueued on the context's stream, so one pair of events times both routes alike.
Device time between two events around a run of launches long enough for a window of seconds, after a warm-up (as
tools/warp_probe.py does).  Compare with the read rate tools/ubench/bw reports on the same machine.
usage: python tools/residual_probe.py [seconds per case, default 2]"""
import os, sys, time, json
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np, torch
from evenvizion_amd._lib import Context
window = float(sys.argv[1]) if len(sys.argv) > 1 else 2.0
ctx = Context(device=0, max_w=64, max_h=64, max_features=500, max_frames=2)
stream = ctx._torch_stream()
rng = np.random.default_rng(6)
res = {}
for w, h, npairs in ((400, 224, 120), (1280, 720, 64)):
    n = npairs + 1
    bgr = torch.from_numpy(rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)).cuda()
    cw, ch = w // 2, h // 2
    planes = torch.from_numpy(rng.integers(0, 256, (n, w * h + 2 * cw * ch), dtype=np.uint8)).cuda()
    mats = []
    for k in range(npairs):
        th = np.deg2rad(-1 + 0.03 * k)
        c, s = 1.01 * np.cos(th), 1.01 * np.sin(th)
        mats.append([c, -s, 1.5 + 0.01 * k, s, c, -0.75, 2e-6, -1e-6, 1])
    mats = torch.tensor(mats, dtype=torch.float64, device='cuda')
    stats = torch.zeros((npairs, 6), dtype=torch.int64, device='cuda')
    out = torch.zeros((npairs, h, w), dtype=torch.uint8, device='cuda')
    warped = torch.zeros((npairs, h, w, 3), dtype=torch.uint8, device='cuda')
    wts = torch.tensor([1868, 9617, 4899], dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()

    def composed():
        ctx.warp_fixed_plane(bgr[:npairs], mats, warped, 'each', (0, 0), inverse_map=True)
        with torch.cuda.stream(stream):
            gray = lambda t: ((t.to(torch.int32) * wts).sum(-1) + 8192) >> 14
            g_cur, g_reg, g_prev = gray(bgr[1:]), gray(warped), gray(bgr[:npairs])
            d, d0 = (g_cur - g_reg).abs().to(torch.int64), (g_cur - g_prev).abs().to(torch.int64)
            return torch.stack([d.sum((1, 2)), (d * d).sum((1, 2)), d0.sum((1, 2)), (d0 * d0).sum((1, 2))], dim=1)

    cases = {
        'bgr': lambda: ctx.pair_residual(bgr, mats, stats=stats, out=out),
        'bgr_no_out': lambda: ctx.pair_residual(bgr, mats, stats=stats),
        'yuv420': lambda: ctx.pair_residual_yuv420(planes, mats, stats=stats, out=out, size=(w, h)),
        'yuv420_no_out': lambda: ctx.pair_residual_yuv420(planes, mats, stats=stats, size=(w, h)),
        'bgr_composed': composed,
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

        run(3)
        per = run(10)[1] / 10
        reps = max(10, int(window / per))
        dev_s, host_s = run(reps)
        read = planes.numel() if case.startswith('yuv420') else bgr.numel()
        covered = float(stats[:, 0].float().mean()) / (w * h)
        res['%dx%d_%s' % (w, h, case)] = dict(pairs=npairs, launches=reps, device_us_per_launch=round(dev_s / reps * 1e6, 2),
                                              host_us_per_launch=round(host_s / reps * 1e6, 2), input_bytes_per_launch=read,
                                              input_GBps=round(read * reps / dev_s * 1e-9, 1),
                                              pixels_per_us=round(npairs * w * h * reps / dev_s * 1e-6, 1), covered_share=round(covered, 3))
    # the two routes agree where every pixel is covered by both; printed, not asserted: the composed route sums uncovered pixels too
    fused = ctx.pair_residual(bgr, mats)
    comp = composed()
    ctx.synchronize()
    torch.cuda.synchronize()
    res['%dx%d_ssd_fused_over_composed' % (w, h)] = round(float(fused[:, 2].sum().cpu()) / float(comp[:, 1].sum().cpu()), 4)
    res['%dx%d_fused_over_composed' % (w, h)] = round(res['%dx%d_bgr_no_out' % (w, h)]['device_us_per_launch'] /
                                                      res['%dx%d_bgr_composed' % (w, h)]['device_us_per_launch'], 3)
    del bgr, planes, out, warped
ctx.close()
print(json.dumps(res))
