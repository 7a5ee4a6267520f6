"""Many videos at once against one after another: N copies of tests/golden/ref_test_video.mp4 through
get_homography_dicts (several captures per GPU call, frames read on a pool of host threads) and, the same captures, in a
loop over get_homography_dict.  File in, dictionaries out: demultiplexing, H.264 decoding, staging and upload included.
usage: python tools/multi_video_probe.py [--videos 16] [--features ORB | SURF,SIFT,ORB] [--ingest bgr|auto|yuv420]
                                         [--max-streams 16] [--decode-threads 8] [--chunk-frames 64] [--repeats 3]
                                         [--root DIR] [--out FILE]

Every form is warmed up once (contexts, staging, first import), then the forms alternate `repeats` times; videos/s and pairs/s
of every run are kept so that the spread between repeats can be set against the difference between the forms.  "decode" times
the captures alone: every frame of one video read on one thread, and all N videos on --decode-threads threads -- the frames/s
the host can deliver, which bounds both forms.  "gpu_ms" is the device time of the many-video form per stage
(evh_profile_read over one extra, untimed run).
--root DIR measures the package of ANOTHER checkout (e.g. the parent commit exported with `git archive` and built) with this
probe; a checkout without get_homography_dicts reports the sequential loop only."""
import argparse, json, os, sys, time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--videos", type=int, default=16)
ap.add_argument("--video", default=os.path.join(HERE, "tests", "golden", "ref_test_video.mp4"))
ap.add_argument("--features", default="ORB", help="comma list in FrameProcessing order, e.g. SURF,SIFT,ORB")
ap.add_argument("--ingest", default="bgr", choices=("bgr", "auto", "yuv420"))
ap.add_argument("--max-streams", type=int, default=16)
ap.add_argument("--decode-threads", type=int, default=8)
ap.add_argument("--chunk-frames", type=int, default=64)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--root", default=HERE, help="checkout whose evenvizion_amd package is measured")
ap.add_argument("--out", default="", help="also write the JSON result here")
args = ap.parse_args()

sys.path.insert(0, os.path.abspath(args.root))
from evenvizion_amd import capture, runtime
from evenvizion_amd.processing import video_processing as VP

features = [f for f in args.features.split(",") if f]
many = getattr(VP, "get_homography_dicts", None)


def captures():
    caps = [capture.VideoCapture(args.video) for _ in range(args.videos)]
    assert all(c.isOpened() for c in caps), "cannot open %s" % args.video
    return caps


def sequential():
    caps = captures()
    t = time.perf_counter()
    out = [VP.get_homography_dict(c, features_type_list=features, ingest=args.ingest) for c in caps]
    return out, time.perf_counter() - t


def together():
    caps = captures()
    t = time.perf_counter()
    out = many(caps, features_type_list=features, ingest=args.ingest, max_streams=args.max_streams,
               decode_threads=args.decode_threads, chunk_frames=args.chunk_frames)
    return out, time.perf_counter() - t


def drain(cap):
    n = 0
    if args.ingest == "bgr":
        while cap.read()[0]:
            n += 1
        return n
    cw, ch = (cap.width + 1) // 2, (cap.height + 1) // 2
    y, cb, cr = np.empty((cap.height, cap.width), np.uint8), np.empty((ch, cw), np.uint8), np.empty((ch, cw), np.uint8)
    while cap.read_yuv420_into(y, cb, cr):
        n += 1
    return n


def decode_rates():
    t = time.perf_counter()
    n1 = drain(captures()[0])
    one = n1 / (time.perf_counter() - t)
    caps = captures()
    t = time.perf_counter()
    with ThreadPoolExecutor(max_workers=args.decode_threads) as pool:
        n = sum(pool.map(drain, caps))
    return dict(frames_per_video=n1, one_thread_fps=round(one, 1), pool_fps=round(n / (time.perf_counter() - t), 1),
                pool_threads=args.decode_threads)


forms = [("sequential", sequential)] + ([("together", together)] if many else [])
res = dict(root="this tree" if os.path.abspath(args.root) == HERE else args.root, videos=args.videos, features=features,
           ingest=args.ingest, max_streams=args.max_streams, decode_threads=args.decode_threads, chunk_frames=args.chunk_frames)
first = {}
for name, f in forms:
    first[name], _ = f()                                  # warm-up of this form
pairs = sum(len(d) - 1 for d in first["sequential"])
if many:
    res["equal"] = first["together"] == first["sequential"]
for name, _ in forms:
    res[name] = dict(seconds=[], videos_per_s=[], pairs_per_s=[])
for _ in range(args.repeats):
    for name, f in forms:
        _, dt = f()
        r = res[name]
        r["seconds"].append(round(dt, 3)); r["videos_per_s"].append(round(args.videos / dt, 2)); r["pairs_per_s"].append(round(pairs / dt, 1))
for name, _ in forms:
    v = res[name]["pairs_per_s"]
    res[name].update(median_pairs_per_s=float(np.median(v)), spread_pairs_per_s=round(max(v) - min(v), 1))
if many:
    res["together_over_sequential"] = round(res["together"]["median_pairs_per_s"] / res["sequential"]["median_pairs_per_s"], 3)
    ctx = runtime._ctx                                   # the context the last run used
    if ctx is not None:
        ctx.profile_enable(True)
        ctx.profile_read()
        _, dt = together()
        prof = ctx.profile_read()
        ctx.profile_enable(False)
        res["gpu_ms"] = {k: round(ms, 2) for k, (n, ms) in prof.items() if n}
        res["gpu_ms_total"] = round(sum(ms for n, ms in prof.values()), 1)
        res["profiled_run_seconds"] = round(dt, 3)
res["pairs"] = pairs
res["decode"] = decode_rates()
print(json.dumps(res, indent=1))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
