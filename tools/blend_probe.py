"""Stand-alone probe of evh_blend_fixed_plane / evh_blend_ray_surface and evh_pair_exposure (profiles/blend.txt).
  kernels   16 frames of 1280x720 (BGR, and the same frames as 4:2:0 planes) onto a 1600x900 BGR canvas, tools/surface_probe.py's
            buffers and matrices:
              plate_basis     evh_plate_fixed_plane without count and masks -- the existing kernel that also samples every frame at
                              every pixel (and does more per sample: LDS, radix select);
              blend_*         FEATHER and SEAM, on the plane (inverse_map = 1) and through the plane's tables of the ray form, with a
                              gain table, writing picture and state; the probe asserts that plane and ray form agree;
              mosaic          EVH_WARP_MOSAIC, for scale: it stops at the first covering frame;
              each_torch      the route the entry replaces: EVH_WARP_EACH, then the weighted sum in torch (int64);
  exposure  evh_pair_exposure with step 1 and 2 beside evh_pair_residual on the same buffers: 120 pairs of 400x224 and 64 pairs of
            1280x720, neighbours under a small translation;
  video     tests/golden/ref_test_video.mp4 with its recorded dictionary: the solved gains' range, the pairs used, and the mean
            absolute gray difference across the frame-edge pixels of the mosaic -- canvas neighbours of which one lies inside a
            frame's footprint and the other outside, both covered by some frame -- for EVH_WARP_MOSAIC and for feather + exposure.
Device time between two events on the context's stream around a run of launches, after a warm-up, as tools/surface_probe.py does.
usage: python tools/blend_probe.py [seconds per case, default 1] [--no-video]"""
import os, sys, time, json
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, HERE)
import numpy as np, torch
from evenvizion_amd._lib import Context
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
    run(3)
    per = run(5)[1] / 5
    reps = max(5, int(window / per))
    dev_s, host_s = run(reps)
    return dict(launches=reps, device_us_per_launch=round(dev_s / reps * 1e6, 2), host_us_per_launch=round(host_s / reps * 1e6, 2))


# ---- kernels ----
n, sw, sh, dw, dh = 16, 1280, 720, 1600, 900
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
cols, rows = (torch.from_numpy(t).cuda() for t in surface.surface_tables('plane', 1.0, origin[0], origin[1], dw, dh))
gains = torch.from_numpy(rng.integers(3500, 4700, (n, 3)).astype(np.uint16)).cuda()
feather = 64 * 32
for source, src, size in (('bgr', bgr, None), ('yuv420', planes, (sw, sh))):
    out = torch.zeros((dh, dw, 3), dtype=torch.uint8, device='cuda')
    each = torch.zeros((n, dh, dw, 3), dtype=torch.uint8, device='cuda')
    acc = torch.zeros((dh, dw, 4), dtype=torch.int64, device='cuda')
    wsum = torch.zeros((dh, dw, 3), dtype=torch.int64, device='cuda')

    def each_torch():
        ctx.warp_fixed_plane(src, mats, each, 'each', origin, inverse_map=True, size=size)
        ctx.order_torch_after()
        with torch.cuda.stream(stream):
            wsum.zero_()
            for k in range(n):
                wsum.add_(each[k].to(torch.int64) * int(4096))
        ctx.order_after_torch()

    cases = [('plate_basis', lambda: ctx.plate_fixed_plane(src, mats, out, origin, inverse_map=True, size=size))]
    for mode in ('feather', 'seam'):
        cases.append(('blend_plane_' + mode, lambda mode=mode: ctx.blend_fixed_plane(src, mats, origin, out=out, mode=mode, feather=feather,
                                                                                    gains=gains, acc=acc, inverse_map=True, size=size)))
        cases.append(('blend_ray_' + mode, lambda mode=mode: ctx.blend_ray_surface(src, mats, cols, rows, out=out, mode=mode, feather=feather,
                                                                                  gains=gains, acc=acc, size=size)))
    cases.append(('blend_plane_feather_picture_only', lambda: ctx.blend_fixed_plane(src, mats, origin, out=out, mode='feather', feather=feather,
                                                                                   gains=gains, inverse_map=True, size=size)))
    cases.append(('mosaic', lambda: ctx.warp_fixed_plane(src, mats, out, 'mosaic', origin, inverse_map=True, size=size)))
    cases.append(('each_torch', each_torch))
    kept = {}
    for name, launch in cases:
        out.zero_()
        res['%s_%s' % (source, name)] = timed(launch)
        kept[name] = (out.clone(), acc.clone())
    for mode in ('feather', 'seam'):
        a, b = kept['blend_plane_' + mode], kept['blend_ray_' + mode]
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), 'plane and ray form disagree'
        res['%s_blend_plane_%s_over_plate' % (source, mode)] = round(res['%s_blend_plane_%s' % (source, mode)]['device_us_per_launch'] /
                                                                     res['%s_plate_basis' % source]['device_us_per_launch'], 3)
    res['%s_covered_share' % source] = round(float(kept['blend_plane_seam'][1][..., 3].ne(0).float().mean()), 3)
    del out, each, acc, wsum, kept
del bgr, planes

# ---- exposure ----
for npairs, w, h in ((120, 400, 224), (64, 1280, 720)):
    frames = torch.from_numpy(rng.integers(0, 256, (npairs + 1, h, w, 3), dtype=np.uint8)).cuda()
    M = torch.from_numpy(np.tile(np.array([1, 0, 3.3, 0, 1, -2.2, 0, 0, 1], np.float64), (npairs, 1))).cuda()
    pairs = torch.from_numpy(np.array([(k + 1, k) for k in range(npairs)], np.int32)).cuda()
    key = '%dx%dx%d' % (npairs, w, h)
    res['residual_' + key] = timed(lambda: ctx.pair_residual(frames, M))
    for step in (1, 2):
        res['exposure_step%d_%s' % (step, key)] = timed(lambda: ctx.pair_exposure(frames, pairs, M, step=step, lo=8, hi=247))
    res['exposure_step1_over_residual_' + key] = round(res['exposure_step1_' + key]['device_us_per_launch'] /
                                                       res['residual_' + key]['device_us_per_launch'], 3)
    del frames

# ---- the reference's video ----
if '--no-video' not in sys.argv:
    from evenvizion_amd import blend, capture, stabilization
    from evenvizion_amd.processing.utils import read_homography_dict, superposition_dict
    golden = os.path.join(HERE, 'tests', 'golden')
    hd, info = read_homography_dict(os.path.join(golden, 'ref_dict_with_homography_matrix.json'))
    sup = superposition_dict(hd)
    keys = [k for k in sup if k != 'resize_info']

    def video():
        cap = capture.VideoCapture(os.path.join(golden, 'ref_test_video.mp4'))
        assert cap.isOpened()
        return cap

    pairs, stats = blend.exposure_stats(video(), sup, info)
    g = blend.solve_gains(pairs, stats, len(keys))
    before = [p for _, p in stabilization.stabilized_frames(video(), sup, info, mode='mosaic', placement='warp')][-1]
    plain = blend.blended_mosaic(video(), sup, info, blend='feather', feather_px=32)
    after = blend.blended_mosaic(video(), sup, info, blend='feather', feather_px=32, gains=g)
    seam = blend.blended_mosaic(video(), sup, info, blend='seam', feather_px=32, gains=g)
    # the footprints: a white frame through EVH_WARP_EACH, every eighth frame
    cap = video()
    w0, h0 = int(cap.width), int(cap.height)
    ox, oy, cdw, cdh, matrix_of = stabilization._placement(sup, info, 'warp', 1.0, w0, h0, stabilization.MAX_PIXELS)
    take = [k for k in range(len(keys)) if k % 8 == 0]
    white = torch.full((1, h0, w0), 255, dtype=torch.uint8, device='cuda')
    cover = torch.zeros((len(keys), cdh, cdw), dtype=torch.bool, device='cuda')
    one = torch.zeros((1, cdh, cdw), dtype=torch.uint8, device='cuda')
    for k in range(len(keys)):
        ctx.warp_fixed_plane(white, torch.from_numpy(matrix_of(k + 1).reshape(1, 9)).cuda(), one, 'each', (ox, oy))
        ctx.synchronize()
        cover[k] = one[0] != 0
    union = cover.any(dim=0)

    def gray(p):
        p = torch.from_numpy(p).cuda().to(torch.float64)
        return p[..., 0] * 0.114 + p[..., 1] * 0.587 + p[..., 2] * 0.299

    def edge_step(picture):
        g2, total, count = gray(picture), 0.0, 0
        for k in take:
            for a, b, ua, ub, ga, gb in ((cover[k][:, :-1], cover[k][:, 1:], union[:, :-1], union[:, 1:], g2[:, :-1], g2[:, 1:]),
                                         (cover[k][:-1], cover[k][1:], union[:-1], union[1:], g2[:-1], g2[1:])):
                m = (a != b) & ua & ub
                total += float((ga - gb).abs()[m].sum())
                count += int(m.sum())
        return total / max(count, 1), count

    def all_step(picture):                      # the same difference over every covered pair of neighbours: the picture's own texture
        g2 = gray(picture)
        m = union[:, :-1] & union[:, 1:]
        return float((g2[:, :-1] - g2[:, 1:]).abs()[m].mean())

    res['video'] = dict(frames=len(keys), pairs=len(pairs), pairs_used=int((stats[:, 0] >= 64).sum()),
                        gain_min=[round(float(v), 4) for v in g.min(axis=0)], gain_max=[round(float(v), 4) for v in g.max(axis=0)],
                        canvas=[cdw, cdh], edge_pixels=edge_step(before)[1],
                        edge_step_mosaic=round(edge_step(before)[0], 3), edge_step_feather=round(edge_step(plain)[0], 3),
                        edge_step_feather_exposure=round(edge_step(after)[0], 3), edge_step_seam_exposure=round(edge_step(seam)[0], 3),
                        neighbour_step_mosaic=round(all_step(before), 3), neighbour_step_feather_exposure=round(all_step(after), 3))
ctx.close()
print(json.dumps(res))
