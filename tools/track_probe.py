"""Stand-alone probe of evh_track_points and evh_track_seeds: device time per call at 400x224 x 120 pairs x 400 points and at
1280x720 x 64 pairs x 2000 points (levels 3, radius 7, 20 iterations, forward-backward 0.5 px), from BGR frames and from the same
frames as 4:2:0 planes.  Beside it, on the same buffers, evh_pair_refine with 8 iterations: the only other way to the map of a pair
whose matching failed.  Frames: a smooth random texture shifted by 0.6 px per frame plus noise, as tools/refine_probe.py makes
them; the points are the frames' own seeds, repeated up to the count.  Device time between two events around a run of calls long
enough for a window of seconds, after a warm-up.  The probe reports; it is not a pass bar.
usage: python tools/track_probe.py [seconds per case, default 2]"""
import os, sys, time, json
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np, torch
from evenvizion_amd._lib import Context
window = float(sys.argv[1]) if len(sys.argv) > 1 else 2.0
LEVELS, RADIUS, ITERS, FB, MIN_EIG = 3, 7, 20, 0.5, 0.5
ctx = Context(device=0, max_w=64, max_h=64, max_features=500, max_frames=2)
stream = ctx._torch_stream()
rng = np.random.default_rng(6)
res = {}
for w, h, npairs, npoints in ((400, 224, 120, 400), (1280, 720, 64, 2000)):
    n = npairs + 1
    coarse = torch.from_numpy(rng.uniform(40, 215, (1, 3, h // 8 + 2, (w + n) // 8 + 3)).astype(np.float32)).cuda()
    tex = torch.nn.functional.interpolate(coarse, scale_factor=8, mode='bicubic', align_corners=False)[0]
    shift = 0.6
    frames = []
    for k in range(n):
        x0 = shift * k
        i0, f = int(x0), x0 - int(x0)
        cut = (1 - f) * tex[:, :h, i0:i0 + w] + f * tex[:, :h, i0 + 1:i0 + 1 + w]
        frames.append((cut + torch.randint(-2, 3, cut.shape, device='cuda')).clamp(0, 255).round().to(torch.uint8).permute(1, 2, 0))
    bgr = torch.stack(frames).contiguous()
    y = ((bgr.float() * torch.tensor([0.098, 0.504, 0.257], device='cuda')).sum(-1) + 16).round().clamp(16, 235).to(torch.uint8)
    cw, ch = w // 2, h // 2
    planes = torch.cat([y.reshape(n, -1), torch.full((n, 2 * cw * ch), 128, dtype=torch.uint8, device='cuda')], dim=1).contiguous()
    mats = torch.tensor([[1, 0, -shift + 0.5, 0, 1, -0.4, 0, 0, 1]] * npairs, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    # the seeds of every current frame, repeated up to npoints per pair
    seed_pts, seed_n = ctx.track_seeds(bgr[1:], radius=2, cell=16, border=8, min_eig=MIN_EIG, pt_cap=npoints)
    ctx.synchronize()
    sp, sn = seed_pts.cpu().numpy(), np.minimum(seed_n.cpu().numpy(), npoints)
    assert sn.min() > 0, "a frame without a seed"
    pts = torch.from_numpy(np.stack([sp[p, np.arange(npoints) % sn[p]] for p in range(npairs)])).cuda()
    npts = torch.full((npairs,), npoints, dtype=torch.int32, device='cuda')
    rows = torch.zeros((npairs, npoints, 4), dtype=torch.float32, device='cuda')
    counts = torch.zeros(npairs, dtype=torch.int32, device='cuda')
    flags = torch.zeros((npairs, npoints), dtype=torch.uint8, device='cuda')
    out = torch.zeros((npairs, 9), dtype=torch.float64, device='cuda')
    info = torch.zeros((npairs, 8), dtype=torch.int64, device='cuda')
    torch.cuda.synchronize()
    kw = dict(levels=LEVELS, radius=RADIUS, iters=ITERS, min_eig=MIN_EIG, fb_max=FB, rows=rows, counts=counts, flags=flags)
    cases = {
        'bgr_track': lambda: ctx.track_points(bgr, pts, npts, mats, **kw),
        'bgr_track_no_backward': lambda: ctx.track_points(bgr, pts, npts, mats, **dict(kw, fb_max=None)),
        'yuv420_track': lambda: ctx.track_points_yuv420(planes, pts, npts, mats, size=(w, h), **kw),
        'bgr_seeds': lambda: ctx.track_seeds(bgr[1:], radius=2, cell=16, border=8, min_eig=MIN_EIG, pts=seed_pts, npts=seed_n),
        'bgr_refine_8': lambda: ctx.pair_refine(bgr, mats, iters=8, out=out, info=info),
        'yuv420_refine_8': lambda: ctx.pair_refine_yuv420(planes, mats, iters=8, out=out, info=info, size=(w, h)),
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
        per = run(5)[1] / 5
        reps = max(5, int(window / per))
        dev_s, host_s = run(reps)
        e = dict(pairs=npairs, calls=reps, device_us_per_call=round(dev_s / reps * 1e6, 1), host_us_per_call=round(host_s / reps * 1e6, 1))
        if 'track' in case:
            c, f = counts.cpu().numpy(), flags.cpu().numpy()
            e.update(points=npoints, points_per_us=round(npairs * npoints * reps / dev_s * 1e-6, 2), kept_mean=round(float(c.mean()), 1),
                     flags=np.bincount(f.reshape(-1), minlength=7).tolist(),
                     median_shift=[round(float(v), 3) for v in np.median((rows[0, :c[0], 2:] - rows[0, :c[0], :2]).cpu().numpy(), 0)])
        if case == 'bgr_seeds':
            e.update(seeds_mean=round(float(seed_n.cpu().numpy().mean()), 1))
        res['%dx%d_%s' % (w, h, case)] = e
    for form in ('bgr', 'yuv420'):
        res['%dx%d_%s_track_over_refine' % (w, h, form)] = round(res['%dx%d_%s_track' % (w, h, form)]['device_us_per_call'] /
                                                                 res['%dx%d_%s_refine_8' % (w, h, form)]['device_us_per_call'], 3)
    del bgr, planes, tex, frames
ctx.close()
print(json.dumps(res))
