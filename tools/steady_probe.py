"""Stand-alone probe of evh_steady_frames (profiles/steady_frames.txt).
  kernels   32 frames of 1280x720 (BGR, and the same frames as 4:2:0 planes) to 32 output pictures of 1280x720:
              warp_each        evh_warp_fixed_plane, EVH_WARP_EACH, inverse_map, with tap 0's maps: the yardstick -- the same work
                               per pixel as steady ntaps = 1, feather = 0, on the same buffers in the same session;
              steady_tT_fF     evh_steady_frames with T = 1, 5, 9 taps and feather F = 0, 8 pixels, writing pictures and counts.
            Tap 0 is the frame under a shake of a few pixels and a fraction of a degree at zoom 1.04, so that it leaves wedges at
            the borders; taps 1 .. are the frames k-1, k+1, k-2, ... four pixels of pan apart.  The probe asserts that steady_t1_f0
            and warp_each give the same bytes.  Every case is timed `repeats` times; the spread of those is the session's own.
  video     tests/golden/ref_test_video.mp4 with its recorded dictionary through steady.steady_frames at its defaults: the zoom, the
            jitter before and after, the mean shares of the pictures, frames per second of the whole loop.
Device time between two events on the context's stream around a run of launches, after a warm-up, as tools/blend_probe.py does.
usage: python tools/steady_probe.py [seconds per timing, default 0.3] [repeats, default 5] [--no-video]"""
import os, sys, time, json
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, HERE)
import numpy as np, torch
from evenvizion_amd._lib import Context
argv = [a for a in sys.argv[1:] if not a.startswith('--')]
window = float(argv[0]) if argv else 0.3
repeats = int(argv[1]) if len(argv) > 1 else 5
ctx = Context(device=0, max_w=64, max_h=64, max_features=500, max_frames=2)
stream = ctx._torch_stream()
rng = np.random.default_rng(5)
res = {}


def timed(launch):
    def run(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ctx.synchronize()
        e0.record(stream)
        for _ in range(reps):
            launch()
        e1.record(stream)
        ctx.synchronize()
        return e0.elapsed_time(e1) * 1e-3
    run(3)
    reps = max(5, int(window / (run(5) / 5)))
    us = sorted(run(reps) / reps * 1e6 for _ in range(repeats))
    return dict(launches=reps, repeats=repeats, device_us_min=round(us[0], 2), device_us_median=round(us[len(us) // 2], 2),
                device_us_max=round(us[-1], 2))


# ---- kernels ----
n, sw, sh = 32, 1280, 720
bgr = torch.from_numpy(rng.integers(0, 256, (n, sh, sw, 3), dtype=np.uint8)).cuda()
cw, ch = sw // 2, sh // 2
planes = torch.from_numpy(rng.integers(0, 256, (n, sw * sh + 2 * cw * ch), dtype=np.uint8)).cuda()
MAXT = 9
offsets = [0] + [s * d for d in range(1, 5) for s in (-1, 1)]
tap_frame = np.full((n, MAXT), -1, np.int32)
tap_M = np.zeros((n, MAXT, 9))
zoom = np.array([[1 / 1.04, 0, sw / 2 * (1 - 1 / 1.04)], [0, 1 / 1.04, sh / 2 * (1 - 1 / 1.04)], [0, 0, 1]])
for k in range(n):
    th = np.deg2rad(rng.uniform(-0.4, 0.4))
    shake = np.array([[np.cos(th), -np.sin(th), rng.uniform(-24, 24)], [np.sin(th), np.cos(th), rng.uniform(-16, 16)],
                      [rng.uniform(-2e-6, 2e-6), rng.uniform(-2e-6, 2e-6), 1]])
    own = shake @ zoom
    for t, off in enumerate(offsets):
        if 0 <= k + off < n:
            tap_frame[k, t] = k + off
            tap_M[k, t] = (np.array([[1, 0, -4.0 * off], [0, 1, 0], [0, 0, 1]]) @ own).reshape(9)
data_bytes = n * sw * sh * 3
for source, src, size in (('bgr', bgr, None), ('yuv420', planes, (sw, sh))):
    out = torch.zeros((n, sh, sw, 3), dtype=torch.uint8, device='cuda')
    ref = torch.zeros((n, sh, sw, 3), dtype=torch.uint8, device='cuda')
    m0 = torch.from_numpy(np.ascontiguousarray(tap_M[:, 0])).cuda()
    cases = [('warp_each', lambda: ctx.warp_fixed_plane(src, m0, ref, 'each', (0, 0), inverse_map=True, size=size))]
    kept = []
    for ntaps in (1, 5, 9):
        tf = torch.from_numpy(np.ascontiguousarray(tap_frame[:, :ntaps])).cuda()
        tm = torch.from_numpy(np.ascontiguousarray(tap_M[:, :ntaps])).cuda()
        counts = torch.zeros((n, ntaps + 1), dtype=torch.int32, device='cuda')
        kept.append((tf, tm, counts))
        for feather in (0, 8):
            cases.append(('steady_t%d_f%d' % (ntaps, feather),
                          lambda tf=tf, tm=tm, counts=counts, feather=feather: ctx.steady_frames(src, tf, tm, out, feather=feather * 32,
                                                                                                 counts=counts, size=size)))
    for name, launch in cases:
        r = timed(launch)
        r['output_GB_per_s'] = round(data_bytes / (r['device_us_median'] * 1e-6) / 1e9, 1)
        if name == 'steady_t1_f0':
            ctx.synchronize()
            assert torch.equal(out, ref), 'steady ntaps = 1, feather = 0 differs from EVH_WARP_EACH'
        if name.startswith('steady'):
            ctx.synchronize()
            c = kept[(1, 5, 9).index(int(name.split('_')[1][1:]))][2].sum(dim=0).cpu().numpy()
            r['shares'] = [round(float(v) / (n * sw * sh), 5) for v in c]
        res[source + '_' + name] = r
        print(source, name, r, flush=True)
    del out, ref

# ---- video ----
if '--no-video' not in sys.argv:
    from evenvizion_amd import steady
    from evenvizion_amd.component import open_capture
    from evenvizion_amd.processing.utils import read_homography_dict, superposition_dict
    golden = os.path.join(HERE, 'tests', 'golden')
    hd, ri = read_homography_dict(os.path.join(golden, 'ref_dict_with_homography_matrix.json'))
    sup = superposition_dict(hd)
    for fill in (2, 0):
        report = {}
        t = time.perf_counter()
        frames = sum(1 for _ in steady.steady_frames(open_capture(os.path.join(golden, 'ref_test_video.mp4'))[0], sup, ri, fill=fill,
                                                     report=report))
        wall = time.perf_counter() - t
        out = steady.steady_report(report)
        res['video_fill%d' % fill] = dict(frames=frames, frames_per_s=round(frames / wall, 1), zoom=out['zoom'], zoom_capped=out['zoom_capped'],
                                          jitter_before=out['jitter_before'], jitter_after=out['jitter_after'],
                                          mean_shares=out['mean_shares'])
        print('video fill', fill, res['video_fill%d' % fill], flush=True)
print(json.dumps(res, indent=1))
