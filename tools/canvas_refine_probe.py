"""Stand-alone probe of evh_canvas_refine: device time per call (iters = 8: nine evaluations, nine launches of the solving kernel) at
400x224 x 120 frames and at 1280x720 x 64 frames, from BGR frames and from the same frames as 4:2:0 planes, without d_count and with
one (valid everywhere, so that both do the same work but for the count reads).  Beside it evh_pair_refine on the same frame
buffers: the same pixels, gradients and sums, the previous frame in the place of the canvas.
Frames: tools/refine_probe.py's -- a smooth random texture shifted by 0.6 pixels per frame plus noise; the canvas is that texture
itself, n pixels wider than a frame, and frame k starts half a pixel and a small rotation off its place in it, so that steps are
accepted and no frame stops early (the evaluations a call made are reported).  Device time between two events around a run of
calls long enough for a window of seconds, after a warm-up.
With a video (and its recorded dictionary) it also runs registration.anchored_homography_dict end to end: seconds, the ITF of the
dictionary and of the anchored one, and the two canvas-score sums.
usage: python tools/canvas_refine_probe.py [seconds per case, default 2] [video dictionary.json [group]]"""
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
for w, h, nframes in ((400, 224, 120), (1280, 720, 64)):
    n = nframes + 1
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
    dw = w + n
    canvas = tex[:, :h, :dw].clamp(0, 255).round().to(torch.uint8).permute(1, 2, 0).contiguous()
    count = torch.full((h, dw), 255, dtype=torch.uint8, device='cuda')
    y = ((bgr.float() * torch.tensor([0.098, 0.504, 0.257], device='cuda')).sum(-1) + 16).round().clamp(16, 235).to(torch.uint8)
    cw, ch = w // 2, h // 2
    planes = torch.cat([y.reshape(n, -1), torch.full((n, 2 * cw * ch), 128, dtype=torch.uint8, device='cuda')], dim=1).contiguous()
    th = np.deg2rad(0.05)
    # current -> previous is x - shift, frame k -> canvas is x + shift k; the starts are half a pixel and a small rotation off
    pair_mats = torch.tensor([[np.cos(th), -np.sin(th), -shift + 0.5, np.sin(th), np.cos(th), -0.4, 1e-6, -1e-6, 1]] * nframes,
                             dtype=torch.float64, device='cuda')
    canvas_mats = torch.tensor([[np.cos(th), -np.sin(th), shift * (k + 1) + 0.5, np.sin(th), np.cos(th), 0.4, 1e-6, -1e-6, 1]
                                for k in range(nframes)], dtype=torch.float64, device='cuda')
    out = torch.zeros((nframes, 9), dtype=torch.float64, device='cuda')
    info = torch.zeros((nframes, 8), dtype=torch.int64, device='cuda')
    torch.cuda.synchronize()
    later, later_planes = bgr[1:], planes[1:]                   # the current frames of pair_refine's pairs
    cases = {
        'bgr_pair_refine': lambda: ctx.pair_refine(bgr, pair_mats, iters=ITERS, out=out, info=info),
        'bgr_canvas_refine': lambda: ctx.canvas_refine(later, canvas, canvas_mats, iters=ITERS, out=out, info=info),
        'bgr_canvas_refine_count': lambda: ctx.canvas_refine(later, canvas, canvas_mats, count=count, min_cover=2, iters=ITERS, out=out, info=info),
        'yuv420_pair_refine': lambda: ctx.pair_refine_yuv420(planes, pair_mats, iters=ITERS, out=out, info=info, size=(w, h)),
        'yuv420_canvas_refine': lambda: ctx.canvas_refine_yuv420(later_planes, canvas, canvas_mats, iters=ITERS, out=out, info=info, size=(w, h)),
        'yuv420_canvas_refine_count': lambda: ctx.canvas_refine_yuv420(later_planes, canvas, canvas_mats, count=count, min_cover=2, iters=ITERS,
                                                                       out=out, info=info, size=(w, h)),
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
        i = info.cpu().numpy()
        res['%dx%d_%s' % (w, h, case)] = dict(
            frames=nframes, calls=reps, device_us_per_call=round(dev_s / reps * 1e6, 1), host_us_per_call=round(host_s / reps * 1e6, 1),
            pixel_evaluations_per_us=round(nframes * w * h * (ITERS + 1) * reps / dev_s * 1e-6, 1),
            evaluations_mean=round(float(i[:, 1].mean()), 2), accepted_mean=round(float(i[:, 2].mean()), 2),
            statuses=sorted(set(int(v) for v in i[:, 0])), covered_share=round(float(i[:, 3].mean()) / (w * h), 4),
            psnr_in=round(float(np.mean(10 * np.log10(65025.0 * i[:, 3] / np.maximum(i[:, 4], 1)))), 2),
            psnr_out=round(float(np.mean(10 * np.log10(65025.0 * i[:, 5] / np.maximum(i[:, 6], 1)))), 2))
    for form in ('bgr', 'yuv420'):
        base = res['%dx%d_%s_pair_refine' % (w, h, form)]['device_us_per_call']
        for case in ('canvas_refine', 'canvas_refine_count'):
            res['%dx%d_%s_%s_over_pair_refine' % (w, h, form, case)] = round(res['%dx%d_%s_%s' % (w, h, form, case)]['device_us_per_call'] / base, 3)
    del bgr, planes, tex, frames, canvas, count, later, later_planes
ctx.close()
if len(sys.argv) > 3:
    from evenvizion_amd import capture, registration, runtime
    from evenvizion_amd.processing.utils import read_homography_dict, superposition_dict
    hd, ri = read_homography_dict(sys.argv[3])
    sup = superposition_dict(hd)
    group = int(sys.argv[4]) if len(sys.argv) > 4 else 1
    t = time.perf_counter()
    got = registration.anchored_homography_dict(lambda: capture.VideoCapture(sys.argv[2]), sup, ri, iters=ITERS, group=group)
    seconds = time.perf_counter() - t
    b, a, info = got['report_before'], got['report_after'], got['info']
    res['video_group_%d' % group] = dict(
        frames=len(info), seconds_with_both_reports=round(seconds, 2), itf_before=round(b['itf'], 3), itf_after=round(a['itf'], 3),
        canvas_score_before=round(got['canvas_score_before'], 2), canvas_score_after=round(got['canvas_score_after'], 2),
        refined=sum(e['status'] == 0 for e in info.values()), used=sum(e['used'] for e in info.values()),
        overlap_mean=round(float(np.mean([e['overlap'] for e in info.values()])), 3),
        accepted_mean=round(float(np.mean([e['accepted'] for e in info.values()])), 2))
    runtime.reset()
print(json.dumps(res))
