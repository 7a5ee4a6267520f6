"""Stand-alone probe of evh_warp_ray_surface against evh_warp_fixed_plane: 16 frames of 1280x720 (BGR, and the same frames as
4:2:0 planes) onto a 1600x900 BGR canvas per launch, EACH, HISTORY and MOSAIC.
  plane_basis    evh_warp_fixed_plane with inverse_map = 1;
  ray_plane      evh_warp_ray_surface through the plane's tables (X, 1), Y on the same buffers and the same matrices: both
                 kernels then sample the same positions, and the probe asserts that their outputs are equal byte for byte;
  ray_cylinder   evh_warp_ray_surface on a cylinder: the same frames as a pan of 3 degrees per frame with a focal length of
                 1100 pixels, the canvas 1600 columns at 1100 pixels per radian (83 degrees), D . K . R^T per frame.
Device time between two events on the context's stream around a run of launches long enough for a window of seconds, after a
warm-up, as tools/warp_probe.py does.  Compare the output rate with the write rate tools/ubench/bw reports on the same machine.
usage: python tools/surface_probe.py [seconds per case, default 2]"""
import os, sys, time, json
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np, torch
from evenvizion_amd._lib import Context
from evenvizion_amd import surface
window = float(sys.argv[1]) if len(sys.argv) > 1 else 2.0
n, sw, sh, dw, dh = 16, 1280, 720, 1600, 900
origin = (-100, -60)
ctx = Context(device=0, max_w=64, max_h=64, max_features=500, max_frames=2)
stream = ctx._torch_stream()
rng = np.random.default_rng(5)
bgr = torch.from_numpy(rng.integers(0, 256, (n, sh, sw, 3), dtype=np.uint8)).cuda()
cw, ch = sw // 2, sh // 2
planes = torch.from_numpy(rng.integers(0, 256, (n, sw * sh + 2 * cw * ch), dtype=np.uint8)).cuda()
mats = []
for k in range(n):                          # tools/warp_probe.py's frame -> plane maps, inverted: plane -> frame, tw > 0 on the canvas
    th = np.deg2rad(-4 + 0.5 * k)
    c, s = 1.1 * np.cos(th), 1.1 * np.sin(th)
    inv = np.linalg.inv(np.array([[c, -s, 80 + 6 * k], [s, c, 40 + 2 * k], [2e-5, -1e-5, 1]]))
    mats.append((inv / inv[2][2]).reshape(9))
plane_mats = torch.from_numpy(np.stack(mats)).cuda()
tables = {'plane': surface.surface_tables('plane', 1.0, origin[0], origin[1], dw, dh)}
focal = 1100.0
tables['cylinder'] = surface.surface_tables('cylinder', focal, -700, -450, dw, dh)
Ry = lambda a: np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
cyl_mats = torch.from_numpy(np.stack([surface.frame_matrix(Ry(np.deg2rad(3.0 * k - 20)), focal, None, (sw, sh), (sw, sh)) for k in range(n)])).cuda()
tables = {k: (torch.from_numpy(c).cuda(), torch.from_numpy(r).cuda()) for k, (c, r) in tables.items()}
res = {}
for source, src, size in (('bgr', bgr, None), ('yuv420', planes, (sw, sh))):
    for mode in ('each', 'history', 'mosaic'):
        shape = (dh, dw, 3) if mode == 'mosaic' else (n, dh, dw, 3)
        out = torch.zeros(shape, dtype=torch.uint8, device='cuda')
        kept = {}
        cases = (('plane_basis', lambda: ctx.warp_fixed_plane(src, plane_mats, out, mode, origin, inverse_map=True, size=size)),
                 ('ray_plane', lambda: ctx.warp_ray_surface(src, plane_mats, *tables['plane'], out, mode, size=size)),
                 ('ray_cylinder', lambda: ctx.warp_ray_surface(src, cyl_mats, *tables['cylinder'], out, mode, size=size)))
        for name, launch in cases:
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

            out.zero_()
            run(3)
            per = run(10)[1] / 10
            reps = max(10, int(window / per))
            dev_s, host_s = run(reps)
            covered = float((out.reshape(-1, dh, dw, 3)[-1] != 0).any(dim=-1).float().mean())
            kept[name] = out.clone() if name != 'ray_cylinder' else None
            res['%s_%s_%s' % (source, mode, name)] = dict(
                frames=n, launches=reps, device_us_per_launch=round(dev_s / reps * 1e6, 2), host_us_per_launch=round(host_s / reps * 1e6, 2),
                output_bytes_per_launch=out.numel(), output_GBps=round(out.numel() * reps / dev_s * 1e-9, 1),
                covered_share_last_canvas=round(covered, 3))
        assert torch.equal(kept['plane_basis'], kept['ray_plane']), 'the plane tables do not reproduce evh_warp_fixed_plane'
        res['%s_%s_ray_over_basis' % (source, mode)] = round(res['%s_%s_ray_plane' % (source, mode)]['device_us_per_launch'] /
                                                             res['%s_%s_plane_basis' % (source, mode)]['device_us_per_launch'], 3)
        del out, kept
ctx.close()
print(json.dumps(res))
