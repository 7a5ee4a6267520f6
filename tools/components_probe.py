"""Stand-alone probe of evh_mask_components: time per call for the masks of tools/plate_probe.py's two jobs,
    paste64    64 masks of 778x287 (64 frames of 400x224 pasted along a pan),
    warp64     64 masks of 1536x864 (64 frames of 1280x720 warped),
with three contents: the masks evh_plate_fixed_plane itself wrote for random frames (`plate`), random masks at density 0.5
(`random`) and masks that are all foreground (`full`: every pixel of a mask in one component, the worst case for the sums), under
8-connectivity with open_radius 0 and 1, 256 table rows per mask.  Beside each job: the evh_plate_fixed_plane launch that made
the masks, and the route the entry replaces -- the download of the masks plus scipy.ndimage.label on the host (or, where scipy
is not importable, the flood fill of tests/components_checks.py on the first mask, scaled to 64).
Device time between two events around a run of calls filling a window of seconds, after a warm-up (as tools/plate_probe.py).
usage: python tools/components_probe.py [seconds per case, default 1] [0 = leave out the host route]"""
import os, sys, time, json
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np, torch
from evenvizion_amd._lib import Context, mask_components_work_bytes
window = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
host_route = len(sys.argv) < 3 or sys.argv[2] != '0'
ctx = Context(device=0, max_w=64, max_h=64, max_features=500, max_frames=2)
stream = ctx._torch_stream()
rng = np.random.default_rng(18)
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


for name, w, h, mats, dw, dh in (('paste64', 400, 224, pan(64, 6, 1), 400 + 6 * 63, 224 + 63), ('warp64', 1280, 720, drift(64), 1536, 864)):
    n = len(mats)
    bgr = torch.from_numpy(rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)).cuda()
    mats = torch.tensor(mats, dtype=torch.float64, device='cuda')
    plate = torch.zeros((dh, dw, 3), dtype=torch.uint8, device='cuda')
    count = torch.zeros((dh, dw), dtype=torch.uint8, device='cuda')
    own = torch.zeros((n, dh, dw), dtype=torch.uint8, device='cuda')
    reps, dev_us, host_us = timed(lambda: ctx.plate_fixed_plane(bgr, mats, plate, (0, 0), count=count, masks=own))
    res['%s_plate_launch' % name] = dict(masks=n, canvas='%dx%d' % (dw, dh), launches=reps, device_us_per_launch=round(dev_us, 1))
    print(json.dumps({'%s_plate_launch' % name: res['%s_plate_launch' % name]}), flush=True)
    del bgr
    contents = {'plate': own, 'random': torch.from_numpy((rng.random((n, dh, dw)) < 0.5).astype(np.uint8) * 255).cuda(),
                'full': torch.full((n, dh, dw), 255, dtype=torch.uint8, device='cuda')}
    labels = torch.zeros((n, dh, dw), dtype=torch.int32, device='cuda')
    table = torch.zeros((n, 256, 5), dtype=torch.int64, device='cuda')
    nobj = torch.zeros(n, dtype=torch.int32, device='cuda')
    work = torch.zeros(mask_components_work_bytes(dw, dh, n) // 4, dtype=torch.int32, device='cuda')
    for content, masks in contents.items():
        for r in (0, 1):
            reps, dev_us, host_us = timed(lambda: ctx.mask_components(masks, labels, 8, r, 1, objects=table, nobjects=nobj, work=work))
            key = '%s_%s_r%d' % (name, content, r)
            res[key] = dict(masks=n, canvas='%dx%d' % (dw, dh), density=round(float((masks != 0).float().mean().cpu()), 3),
                            objects_per_mask=round(float(nobj.float().mean().cpu()), 1), calls=reps, device_us_per_call=round(dev_us, 1),
                            host_us_per_call=round(host_us, 1), Mpixels_per_s=round(n * dw * dh / dev_us, 1),
                            over_plate_launch=round(dev_us / res['%s_plate_launch' % name]['device_us_per_launch'], 3))
            print(json.dumps({key: res[key]}), flush=True)
    for r in (0, 1):
        res['%s_full_over_random_r%d' % (name, r)] = round(res['%s_full_r%d' % (name, r)]['device_us_per_call'] /
                                                          res['%s_random_r%d' % (name, r)]['device_us_per_call'], 2)
    if host_route:
        for content in ('plate', 'random'):
            ctx.synchronize()
            t0 = time.perf_counter()
            host = contents[content].cpu().numpy()
            t1 = time.perf_counter()
            try:
                from scipy import ndimage
                how = 'scipy.ndimage.label'
                for m in host:
                    ndimage.label(m, np.ones((3, 3), int))
                t2 = time.perf_counter()
                label_ms = (t2 - t1) * 1e3
            except ImportError:
                sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests'))
                import components_checks
                how = 'components_checks.components on one mask, times %d' % n
                components_checks.components(host[0], 8)
                label_ms = (time.perf_counter() - t1) * 1e3 * n
            key = '%s_%s_download_and_host' % (name, content)
            res[key] = dict(mask_bytes=host.size, download_ms=round((t1 - t0) * 1e3, 1), host_labelling=how, host_labelling_ms=round(label_ms, 1),
                            total_ms=round((t1 - t0) * 1e3 + label_ms, 1))
            print(json.dumps({key: res[key]}), flush=True)
    del contents, own, labels, work
ctx.close()
print(json.dumps(res))
