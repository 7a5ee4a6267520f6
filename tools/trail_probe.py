"""Stand-alone probe of evh_trail_fixed_plane: time per launch and output bytes per second, 16 frames of 1280x720 (BGR, and
the same frames as 4:2:0 planes) onto a 1600x900 BGR canvas per launch, through the matrices of tools/warp_probe.py, with the
pictures (d_out: 16 canvases stored per launch, plus the carried canvas) and without (the canvas only advances), with a white
rectangle per frame.  Beside it EVH_WARP_HISTORY of evh_warp_fixed_plane on the same buffers: it stores the same 16 canvases
and does no colour step, so the ratio of the two is what the colour step costs.  The canvas is carried from launch to launch,
so after the warm-up it holds what a video leaves: the pixels the last frames covered, dimmed, and black elsewhere.
Device time between two events on the context's stream around a run of launches long enough for a window of seconds, after a
warm-up (as tools/warp_probe.py does).  Compare with the write rate tools/ubench/bw reports on the same machine.
usage: python tools/trail_probe.py [seconds per case, default 2]"""
import os, sys, time, json
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np, torch
from evenvizion_amd._lib import Context
window = float(sys.argv[1]) if len(sys.argv) > 1 else 2.0
n, sw, sh, dw, dh = 16, 1280, 720, 1600, 900
ctx = Context(device=0, max_w=64, max_h=64, max_features=500, max_frames=2)
stream = ctx._torch_stream()
rng = np.random.default_rng(5)
bgr = torch.from_numpy(rng.integers(0, 256, (n, sh, sw, 3), dtype=np.uint8)).cuda()
cw, ch = sw // 2, sh // 2
planes = torch.from_numpy(rng.integers(0, 256, (n, sw * sh + 2 * cw * ch), dtype=np.uint8)).cuda()
mats = []
for k in range(n):
    th = np.deg2rad(-4 + 0.5 * k)
    c, s = 1.1 * np.cos(th), 1.1 * np.sin(th)
    mats.append([c, -s, 80 + 6 * k, s, c, 40 + 2 * k, 2e-5, -1e-5, 1])
mats = torch.tensor(mats, dtype=torch.float64, device='cuda')
rects = torch.tensor([[180 + 6 * k, 100 + 2 * k, 180 + 6 * k + sw, 100 + 2 * k + sh] for k in range(n)], dtype=torch.int32, device='cuda')
out = torch.zeros((n, dh, dw, 3), dtype=torch.uint8, device='cuda')
res = {}
for source, src, size in (('bgr', bgr, None), ('yuv420', planes, (sw, sh))):
    for case in ('trail', 'trail_no_out', 'history'):
        canvas = torch.zeros((dh, dw, 3), dtype=torch.uint8, device='cuda')

        def launch():
            if case == 'history':
                ctx.warp_fixed_plane(src, mats, out, 'history', (-100, -60), background=canvas, size=size)
            else:
                ctx.trail_fixed_plane(src, mats, canvas, (-100, -60), out=out if case == 'trail' else None, rects=rects, size=size)

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
        stored = (out.numel() if case != 'trail_no_out' else 0) + (canvas.numel() if case != 'history' else 0)
        lit = float((canvas != 0).any(dim=-1).float().mean()) if case != 'history' else float((out[-1] != 0).any(dim=-1).float().mean())
        res['%s_%s' % (source, case)] = dict(frames=n, launches=reps, device_us_per_launch=round(dev_s / reps * 1e6, 2),
                                             host_us_per_launch=round(host_s / reps * 1e6, 2), output_bytes_per_launch=stored,
                                             output_GBps=round(stored * reps / dev_s * 1e-9, 1), lit_share_of_canvas=round(lit, 3))
    res['%s_trail_over_history' % source] = round(res['%s_trail' % source]['device_us_per_launch'] /
                                                  res['%s_history' % source]['device_us_per_launch'], 3)
ctx.close()
print(json.dumps(res))
