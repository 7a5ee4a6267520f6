"""Stand-alone probe of evh_blend_bands_* and evh_seam_labels_* (profiles/bands.txt).
  16 frames of 1280x720 (BGR, and the same frames as 4:2:0 planes) onto a 1600x900 BGR canvas, tools/blend_probe.py's buffers and
  matrices, levels = 5, on the plane (inverse_map = 1) and on a cylinder:
    labels          evh_seam_labels_*;
    bands           picture and state written, a gain table, the workspace of all 16 frames;
    bands_ws1       the same with the workspace of one frame (16 groups);
    bands_state     d_out NULL: the state alone, as every chunk but the last of a video;
    feather         evh_blend_* in mode FEATHER on the same buffers;
    each_torch      the route a user has without the entry: EVH_WARP_EACH, then Gaussian and Laplacian pyramids of the 16 canvases and
                    of the 16 label masks by torch conv2d / conv_transpose2d in float32, blended and collapsed (no edge
                    extension of the frames: the pictures differ near frame borders, torch_vs_bands_mean_abs says by how much).
  The probe asserts that the two workspace sizes leave the same picture and the same state.
Device time between two events on the context's stream around a run of launches, after a warm-up, as tools/blend_probe.py does.
usage: python tools/bands_probe.py [seconds per case, default 1] [--no-torch]"""
import os, sys, time, json
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, HERE)
import numpy as np, torch
import torch.nn.functional as TF
from evenvizion_amd._lib import Context, bands_frame_ws_bytes, bands_state_elems
from evenvizion_amd import surface
argv = [a for a in sys.argv[1:] if not a.startswith('--')]
window = float(argv[0]) if argv else 1.0
ctx = Context(device=0, max_w=64, max_h=64, max_features=500, max_frames=2)
stream = ctx._torch_stream()
rng = np.random.default_rng(5)
res = {}


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
    per = run(3)[1] / 3
    reps = max(3, int(window / per))
    dev_s, host_s = run(reps)
    return dict(launches=reps, device_us_per_launch=round(dev_s / reps * 1e6, 2), host_us_per_launch=round(host_s / reps * 1e6, 2))


n, sw, sh, dw, dh, levels = 16, 1280, 720, 1600, 900, 5
origin = (-100, -60)
bgr = torch.from_numpy(rng.integers(0, 256, (n, sh, sw, 3), dtype=np.uint8)).cuda()
cw, ch = sw // 2, sh // 2
planes = torch.from_numpy(rng.integers(0, 256, (n, sw * sh + 2 * cw * ch), dtype=np.uint8)).cuda()
mats = []
for k in range(n):                          # tools/surface_probe.py's plane -> frame maps
    th = np.deg2rad(-4 + 0.5 * k)
    c, s = 1.1 * np.cos(th), 1.1 * np.sin(th)
    inv = np.linalg.inv(np.array([[c, -s, 80 + 6 * k], [s, c, 40 + 2 * k], [2e-5, -1e-5, 1]]))
    mats.append((inv / inv[2][2]).reshape(9))
mats = torch.from_numpy(np.stack(mats)).cuda()
focal = 1100.0
cyl = tuple(torch.from_numpy(t).cuda() for t in surface.surface_tables('cylinder', focal, -dw // 2, -dh // 2, dw, dh))
cams = []
for k in range(n):                          # a pan of 1.5 degrees per frame about the vertical axis
    a = np.deg2rad(-12 + 1.5 * k)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    cams.append(surface.frame_matrix(R, focal, None, (sw, sh), (sw, sh)))
cams = torch.from_numpy(np.stack(cams).reshape(n, 9)).cuda()
gains = torch.from_numpy(rng.integers(3500, 4700, (n, 3)).astype(np.uint16)).cuda()
feather = 64 * 32
elems, unit = bands_state_elems(dw, dh, 3, levels), bands_frame_ws_bytes(dw, dh, 3, levels)
res['state_MB'] = round(elems * 8 / 1e6, 1)
res['frame_ws_MB'] = round(unit / 1e6, 1)
kernel5 = torch.tensor([1., 4., 6., 4., 1.], device='cuda')
kernel5 = (kernel5[:, None] * kernel5[None, :] / 256.0)[None, None].repeat(4, 1, 1, 1)


def torch_pyramids(each, label, out):
    """float32 multi-band blend of the n warped canvases under the label mask"""
    x = torch.cat([each.permute(0, 3, 1, 2).float() * (gains.float() / 4096.0)[:, :, None, None], (label[None] == torch.arange(n, device='cuda')[:, None, None])[:, None].float()], 1)
    gauss = [x]
    for _ in range(levels):
        gauss.append(TF.conv2d(TF.pad(gauss[-1], (2, 2, 2, 2), mode='replicate'), kernel5, stride=2, groups=4))
    num, den = [], []
    for l in range(levels + 1):
        g = gauss[l]
        if l < levels:
            up = TF.conv_transpose2d(gauss[l + 1][:, :3], 4 * kernel5[:3], stride=2, padding=2, output_padding=1, groups=3)
            lap = g[:, :3] - up[:, :, :g.shape[2], :g.shape[3]]
        else:
            lap = g[:, :3]
        num.append((lap * g[:, 3:]).sum(0, keepdim=True))
        den.append(g[:, 3:].sum(0, keepdim=True))
    r = num[levels] / den[levels].clamp_min(1e-6)
    for l in range(levels - 1, -1, -1):
        up = TF.conv_transpose2d(r, 4 * kernel5[:3], stride=2, padding=2, output_padding=1, groups=3)
        r = num[l] / den[l].clamp_min(1e-6) + up[:, :, :num[l].shape[2], :num[l].shape[3]]
    out.copy_(r[0].permute(1, 2, 0).round().clamp(0, 255).to(torch.uint8))


for geo in ('plane', 'cylinder'):
    for source, src, size in (('bgr', bgr, None), ('yuv420', planes, (sw, sh))):
        key = '%s_%s_' % (geo, source)
        out = torch.zeros((dh, dw, 3), dtype=torch.uint8, device='cuda')
        state = torch.zeros(elems, dtype=torch.int64, device='cuda')
        acc = torch.zeros((dh, dw, 4), dtype=torch.int64, device='cuda')
        ws = torch.empty(unit * n, dtype=torch.uint8, device='cuda')
        best = torch.zeros((dh, dw), dtype=torch.int32, device='cuda')
        label = torch.empty((dh, dw), dtype=torch.uint16, device='cuda')
        if geo == 'plane':
            def labels():
                ctx.seam_labels_fixed_plane(mats, (sw, sh), origin, (dh, dw), feather=feather, best=best, label=label, inverse_map=True)

            def bands(ws=ws, out=out):
                ctx.blend_bands_fixed_plane(src, mats, origin, label, levels=levels, out=out, gains=gains, state=state, ws=ws,
                                            inverse_map=True, shape=(dh, dw), size=size)

            def plain():
                ctx.blend_fixed_plane(src, mats, origin, out=out, mode='feather', feather=feather, gains=gains, acc=acc, inverse_map=True,
                                      size=size)

            def each_of(dst):
                ctx.warp_fixed_plane(src, mats, dst, 'each', origin, inverse_map=True, size=size)
        else:
            def labels():
                ctx.seam_labels_ray_surface(cams, (sw, sh), cyl[0], cyl[1], feather=feather, best=best, label=label)

            def bands(ws=ws, out=out):
                ctx.blend_bands_ray_surface(src, cams, cyl[0], cyl[1], label, levels=levels, out=out, gains=gains, state=state, ws=ws,
                                            size=size)

            def plain():
                ctx.blend_ray_surface(src, cams, cyl[0], cyl[1], out=out, mode='feather', feather=feather, gains=gains, acc=acc, size=size)

            def each_of(dst):
                ctx.warp_ray_surface(src, cams, cyl[0], cyl[1], dst, 'each', size=size)
        res[key + 'labels'] = timed(labels)
        res[key + 'labelled_share'] = round(float((label.to(torch.int32) != 65535).float().mean()), 3)
        res[key + 'bands'] = timed(bands)
        kept = (out.clone(), state.clone())
        res[key + 'bands_ws1'] = timed(lambda: bands(ws=ws[:unit]))
        assert torch.equal(out, kept[0]) and torch.equal(state, kept[1]), 'the result depends on the workspace'
        res[key + 'bands_state'] = timed(lambda: bands(out=None))
        res[key + 'feather'] = timed(plain)
        if '--no-torch' not in sys.argv:
            each = torch.zeros((n, dh, dw, 3), dtype=torch.uint8, device='cuda')
            label32 = label.to(torch.int32)

            def each_torch():
                each_of(each)
                ctx.order_torch_after()
                with torch.cuda.stream(stream):
                    torch_pyramids(each, label32, out)
                ctx.order_after_torch()
            res[key + 'each_torch'] = timed(each_torch)
            diff = (out.to(torch.int32) - kept[0].to(torch.int32)).abs()[label32 != 65535]
            res[key + 'torch_vs_bands_mean_abs'] = round(float(diff.float().mean()), 3)
            del each
        del out, state, acc, ws
ctx.close()
print(json.dumps(res, indent=1))
