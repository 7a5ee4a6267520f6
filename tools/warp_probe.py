"""Stand-alone probe of evh_warp_fixed_plane: output bytes per second of EACH and of MOSAIC, 1280x720 frames (BGR, and the
same frames as 4:2:0 planes) onto a 1600x900 BGR canvas, 16 frames per launch through a rotation with zoom and a perspective
row that leaves part of the canvas to the background.  Device time between two events on the context's stream around a run of
launches long enough for a window of seconds, after a warm-up (as tools/resize_probe.py does; the launch's ordering behind
torch's stream is inside the window).  EACH writes 16 canvases per launch, MOSAIC one: its rate counts the one canvas it
stores, and its frames are looked at newest first until one covers the pixel.
Compare with the write rate tools/ubench/bw reports on the same machine (the streaming-store ceiling).
usage: python tools/warp_probe.py [seconds per case, default 2]"""
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
res = {}
for source, src, size in (('bgr', bgr, None), ('yuv420', planes, (sw, sh))):
    for mode in ('each', 'mosaic'):
        out = torch.zeros((n, dh, dw, 3) if mode == 'each' else (dh, dw, 3), dtype=torch.uint8, device='cuda')

        def run(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ctx.synchronize()
            t = time.perf_counter()
            e0.record(stream)
            for _ in range(reps):
                ctx.warp_fixed_plane(src, mats, out, mode, (-100, -60), size=size)
            e1.record(stream)
            ctx.synchronize()
            return e0.elapsed_time(e1) * 1e-3, time.perf_counter() - t

        run(3)
        per = run(10)[1] / 10
        reps = max(10, int(window / per))
        dev_s, host_s = run(reps)
        covered = float((out.reshape(-1, dh, dw, 3)[-1] != 0).any(dim=-1).float().mean())
        res['%s_%s' % (source, mode)] = dict(frames=n, launches=reps, device_us_per_launch=round(dev_s / reps * 1e6, 2),
                                             host_us_per_launch=round(host_s / reps * 1e6, 2), output_bytes_per_launch=out.numel(),
                                             output_GBps=round(out.numel() * reps / dev_s * 1e-9, 1),
                                             covered_share_last_canvas=round(covered, 3))
ctx.close()
print(json.dumps(res))
