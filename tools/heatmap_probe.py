"""Stand-alone probe of evh_heatmap_render: output bytes per second at 400x224 x 121 frames (the reference video at its working
size) and at 1280x720 x 64 frames, each with frames under the colours and without, one launch per call through the matrices of a
slow pan with a perspective row.  Device time between two events on the context's stream around a run of launches long enough
for a window of seconds, after a warm-up (as tools/warp_probe.py does; the launch's ordering behind torch's stream is inside the
window).  Compare with the write rate tools/ubench/bw reports on the same machine (the streaming-store ceiling).
For scale, timed once on the 400x224 x 121 case: the only route to the same pictures without this entry -- evh_fixed_plane_field
with d_field, the download of its 16 bytes per pixel, and the colouring in numpy on the host (frames already on the host).
usage: python tools/heatmap_probe.py [seconds per case, default 2]"""
import os, sys, time, json
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np, torch
from evenvizion_amd._lib import Context
from evenvizion_amd.heatmap import jet_lut
window = float(sys.argv[1]) if len(sys.argv) > 1 else 2.0
ctx = Context(device=0, max_w=64, max_h=64, max_features=500, max_frames=2)
stream = ctx._torch_stream()
rng = np.random.default_rng(6)
lut_host = jet_lut()
lut = torch.from_numpy(lut_host).cuda()


def matrices(n, w):
    """A pan of up to 2 w pixels with a little rotation, zoom and perspective: colour indices from 0 far into the wrap."""
    out = []
    for k in range(n):
        th = np.deg2rad(0.02 * k)
        c, s = (1 + 1e-3 * k) * np.cos(th), (1 + 1e-3 * k) * np.sin(th)
        out.append([c, -s, 2.0 * w * k / n, s, c, 0.3 * w * k / n, 1e-6 * k / n, -2e-6 * k / n, 1])
    return np.array(out, np.float64)


res = {}
for n, w, h in ((121, 400, 224), (64, 1280, 720)):
    Hs = matrices(n, w)
    mats = torch.from_numpy(Hs).cuda()
    frames_host = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    frames = torch.from_numpy(frames_host).cuda()
    out = torch.zeros((n, h, w, 3), dtype=torch.uint8, device='cuda')
    for name, src in (('frames', frames), ('no_frames', None)):

        def run(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ctx.synchronize()
            t = time.perf_counter()
            e0.record(stream)
            for _ in range(reps):
                ctx.heatmap_render(mats, out, lut, frames=src)
            e1.record(stream)
            ctx.synchronize()
            return e0.elapsed_time(e1) * 1e-3, time.perf_counter() - t

        run(3)
        per = run(10)[1] / 10
        reps = max(10, int(window / per))
        dev_s, host_s = run(reps)
        res['%dx%dx%d_%s' % (w, h, n, name)] = dict(launches=reps, device_us_per_launch=round(dev_s / reps * 1e6, 2),
                                                   host_us_per_launch=round(host_s / reps * 1e6, 2),
                                                   output_bytes_per_launch=out.numel(),
                                                   output_GBps=round(out.numel() * reps / dev_s * 1e-9, 1),
                                                   colours_in_last_picture=int(len(torch.unique(out[-1].reshape(-1, 3), dim=0))))
    if (w, h) == (400, 224):
        # the route without the entry, once: field on the device, 16 bytes per pixel down, numpy on the host
        field = torch.empty((n, h, w, 2), dtype=torch.float64, device='cuda')
        ctx.fixed_plane_max(Hs, w, h, field=field)                               # warm-up
        ctx.synchronize()
        t0 = time.perf_counter()
        ctx.fixed_plane_max(Hs, w, h, field=field)
        F = field.cpu().numpy()
        t1 = time.perf_counter()
        with np.errstate(all='ignore'):
            t = 255.0 * (np.sqrt(F[..., 0] * F[..., 0] + F[..., 1] * F[..., 1]) / 1000.0)
            idx = np.where(np.isfinite(t) & (t >= 0) & (t < 2.0 ** 31), t, 0.0).astype(np.int64) & 255
            pictures = np.clip(np.rint(lut_host[idx].astype(np.float64) * 0.8 + frames_host), 0, 255).astype(np.uint8)
        t2 = time.perf_counter()
        ctx.synchronize()
        t3 = time.perf_counter()
        ctx.heatmap_render(mats, out, lut, frames=frames)
        ctx.order_torch_after()
        mine = out.cpu().numpy()
        t4 = time.perf_counter()
        res['400x224x121_field_route'] = dict(field_and_download_ms=round((t1 - t0) * 1e3, 2), numpy_colouring_ms=round((t2 - t1) * 1e3, 2),
                                              entry_and_download_ms=round((t4 - t3) * 1e3, 2),
                                              pictures_equal=bool(np.array_equal(pictures, mine)))
ctx.close()
print(json.dumps(res))
