"""Stand-alone probe of the matching pictures.
1. evh_draw_matches: output bytes per second at 400x224 x 63 pictures (a chunk of the reference video at its working size) and
   at 1280x720 x 16 pictures, with 0, 500 and 4000 rows per pair (key points inside their frames, as a batch delivers them), one
   call = the paste launch and the line launch.  Device time between two events on the context's stream around a run of calls
   long enough for a window of seconds, after a warm-up (as tools/heatmap_probe.py does).  A call reads 3*w*h bytes per frame
   and writes 6*w*h bytes per picture: compare with the copy rate tools/ubench/bw reports on the same machine.
2. get_homography_dict on the reference's video (tests/golden/ref_test_video.mp4, ["ORB"], resize_width 400) without a sink and
   with one that discards the pictures, alternated: pairs per second by a host clock around the whole call (decoding included).
usage: python tools/draw_probe.py [seconds per case, default 2] [repeats of the video runs, default 3]"""
import os, sys, time, json
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
import numpy as np, torch
from evenvizion_amd._lib import Context
window = float(sys.argv[1]) if len(sys.argv) > 1 else 2.0
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 3
ctx = Context(device=0, max_w=64, max_h=64, max_features=500, max_frames=2)
stream = ctx._torch_stream()
rng = np.random.default_rng(6)
res = {}
for npairs, w, h in ((63, 400, 224), (16, 1280, 720)):
    frames = torch.from_numpy(rng.integers(0, 256, (npairs + 1, h, w, 3), dtype=np.uint8)).cuda()
    out = torch.zeros((npairs, h, 2 * w, 3), dtype=torch.uint8, device='cuda')
    cap = 4000
    pts = np.stack([rng.uniform(0, w, (npairs, cap)), rng.uniform(0, h, (npairs, cap)), rng.uniform(0, w, (npairs, cap)),
                    rng.uniform(0, h, (npairs, cap))], axis=2).astype(np.float32)
    rows = torch.from_numpy(pts).cuda()
    for nrows in (0, 500, 4000):
        counts = torch.full((npairs,), nrows, dtype=torch.int32, device='cuda')

        def run(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ctx.synchronize()
            t = time.perf_counter()
            e0.record(stream)
            for _ in range(reps):
                ctx.draw_matches(frames, rows, counts, out)
            e1.record(stream)
            ctx.synchronize()
            return e0.elapsed_time(e1) * 1e-3, time.perf_counter() - t

        run(3)
        per = run(10)[1] / 10
        reps = max(10, int(window / per))
        dev_s, host_s = run(reps)
        green = int((out[-1] == torch.tensor([0, 255, 0], dtype=torch.uint8, device='cuda')).all(dim=2).sum())
        res['%dx%dx%d_rows%d' % (w, h, npairs, nrows)] = dict(
            calls=reps, device_us_per_call=round(dev_s / reps * 1e6, 2), host_us_per_call=round(host_s / reps * 1e6, 2),
            output_bytes_per_call=out.numel(), output_GBps=round(out.numel() * reps / dev_s * 1e-9, 1),
            read_plus_written_GBps=round((out.numel() + 2 * npairs * h * w * 3) * reps / dev_s * 1e-9, 1),
            line_pixels_in_last_picture=green)
ctx.close()

from evenvizion_amd import capture
from evenvizion_amd.processing import get_homography_dict
MP4 = os.path.join(ROOT, 'tests', 'golden', 'ref_test_video.mp4')


def video(sink):
    t = time.perf_counter()
    d = get_homography_dict(capture.VideoCapture(MP4), features_type_list=['ORB'], matching_sink=sink)
    return (len(d) - 1) / (time.perf_counter() - t)


seen = [0]


def discard(frame_no, picture):
    seen[0] += 1


video(None), video(discard)              # warm-up: contexts, staging buffers, code objects
seen[0] = 0
rates = {'no_sink': [], 'discarding_sink': []}
for _ in range(repeats):
    rates['no_sink'].append(round(video(None), 1))
    rates['discarding_sink'].append(round(video(discard), 1))
res['reference_video_orb_pairs_per_s'] = dict(rates, pictures_per_run=seen[0] // repeats)
print(json.dumps(res))
