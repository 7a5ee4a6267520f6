"""Stand-alone probe of evh_pair_refine: device time per call (iters = 8: nine evaluations, nine launches of the solving kernel)
at 400x224 x 120 pairs and at 1280x720 x 64 pairs, from BGR frames and from the same frames as 4:2:0 planes.  Beside it, on the
same buffers and matrices, iters + 1 launches of evh_pair_residual: the floor, the same sampling without the normal sums.
Frames: a smooth random texture shifted by a fraction of a pixel per frame plus noise, the start matrices a fraction of a pixel
off, so that steps are accepted and no pair stops early (the evaluations a call made are reported).  Device time between two
events around a run of calls long enough for a window of seconds, after a warm-up, as tools/residual_probe.py does.
With a video (and its recorded dictionary) it also records the ITF of the dictionary and of the refined ones, levels 1 and 3.
usage: python tools/refine_probe.py [seconds per case, default 2] [video dictionary.json]"""
import os, sys, time, json
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np, torch
from evenvizion_amd._lib import Context
window = float(sys.argv[1]) if len(sys.argv) > 1 else 2.0
ITERS = 8
ctx = Context(device=0, max_w=64, max_h=64, max_features=500, max_frames=2)
stream = ctx._torch_stream()
rng = np.random.default_rng(6)
res = {}
for w, h, npairs in ((400, 224, 120), (1280, 720, 64)):
    n = npairs + 1
    # one smooth texture, wider than the frame; frame k looks at it 0.6 k pixels further right
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
    # current -> previous is x - shift; the start is half a pixel and a small rotation off
    mats = []
    for k in range(npairs):
        th = np.deg2rad(0.05)
        mats.append([np.cos(th), -np.sin(th), -shift + 0.5, np.sin(th), np.cos(th), -0.4, 1e-6, -1e-6, 1])
    mats = torch.tensor(mats, dtype=torch.float64, device='cuda')
    out = torch.zeros((npairs, 9), dtype=torch.float64, device='cuda')
    info = torch.zeros((npairs, 8), dtype=torch.int64, device='cuda')
    stats = torch.zeros((npairs, 6), dtype=torch.int64, device='cuda')
    torch.cuda.synchronize()

    def floor(call, *a, **k):
        def go():
            for _ in range(ITERS + 1):
                call(*a, **k)
        return go

    cases = {
        'bgr_refine': lambda: ctx.pair_refine(bgr, mats, iters=ITERS, out=out, info=info),
        'bgr_residual_x9': floor(ctx.pair_residual, bgr, mats, stats=stats),
        'yuv420_refine': lambda: ctx.pair_refine_yuv420(planes, mats, iters=ITERS, out=out, info=info, size=(w, h)),
        'yuv420_residual_x9': floor(ctx.pair_residual_yuv420, planes, mats, stats=stats, size=(w, h)),
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
        e = dict(pairs=npairs, calls=reps, device_us_per_call=round(dev_s / reps * 1e6, 1), host_us_per_call=round(host_s / reps * 1e6, 1),
                 pixel_evaluations_per_us=round(npairs * w * h * (ITERS + 1) * reps / dev_s * 1e-6, 1))
        if case.endswith('refine'):
            i = info.cpu().numpy()
            e.update(evaluations_mean=round(float(i[:, 1].mean()), 2), accepted_mean=round(float(i[:, 2].mean()), 2),
                     statuses=sorted(set(int(v) for v in i[:, 0])),
                     psnr_in=round(float(np.mean(10 * np.log10(65025.0 * i[:, 3] / np.maximum(i[:, 4], 1)))), 2),
                     psnr_out=round(float(np.mean(10 * np.log10(65025.0 * i[:, 5] / np.maximum(i[:, 6], 1)))), 2))
        res['%dx%d_%s' % (w, h, case)] = e
    for form in ('bgr', 'yuv420'):
        res['%dx%d_%s_refine_over_floor' % (w, h, form)] = round(res['%dx%d_%s_refine' % (w, h, form)]['device_us_per_call'] /
                                                                  res['%dx%d_%s_residual_x9' % (w, h, form)]['device_us_per_call'], 3)
    del bgr, planes, tex, frames
ctx.close()
if len(sys.argv) > 3:
    from evenvizion_amd import capture, registration, runtime
    from evenvizion_amd.processing.utils import read_homography_dict, superposition_dict
    hd, ri = read_homography_dict(sys.argv[3])
    sup = superposition_dict(hd)
    for levels in (1, 3):
        t = time.perf_counter()
        got = registration.refined_homography_dict(lambda: capture.VideoCapture(sys.argv[2]), sup, ri, iters=ITERS, levels=levels)
        b, a = got['report_before'], got['report_after']
        gains = {no: a['frames'][no]['psnr'] - b['frames'][no]['psnr'] for no in b['frames']}
        res['video_levels_%d' % levels] = dict(
            itf_before=round(b['itf'], 3), itf_after=round(a['itf'], 3), pairs=len(gains), pairs_gaining=sum(g > 0 for g in gains.values()),
            pairs_losing=sum(g < 0 for g in gains.values()), least_gain=round(min(gains.values()), 3), largest_gain=round(max(gains.values()), 3),
            largest_gain_at=max(gains, key=gains.get), accepted_mean=round(float(np.mean([i['accepted'] for i in got['info'].values()])), 2),
            seconds_with_both_reports=round(time.perf_counter() - t, 2))
    runtime.reset()
print(json.dumps(res))
