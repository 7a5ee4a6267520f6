"""The drivers that read a video a second time, end to end over tests/golden/ref_test_video.mp4 (121 frames of 1170x658): file in,
pictures / report / dictionary out on the host -- demultiplexing, decoding, the chunk loop, upload, the device work and the
download.  Timed, each with ingest "bgr" and "auto":
    stabilized_frames(trail=True), comparison_frames, background_plate, heatmap_frames, registration_report,
    refine_homography_dict, get_homography_dict(matching_sink=...)
usage: python tools/second_pass_probe.py [--repeats 3] [--root DIR] [--out FILE]

The dictionary, the superposition and the plate the drivers take come from one first pass that is not timed.  Every driver is
run once as a warm-up (contexts, staging, first import), and a SHA-1 over everything that run returned is kept, so that two
checkouts can be compared for what they computed as well as for how long they took; then the drivers run `repeats` times in
turn.  Every driver hands its results over on the host, so the host clock around a call covers the device work.
--root DIR measures the package of ANOTHER checkout (e.g. the parent commit exported with `git archive` and built) with this
probe.  To set two checkouts against each other, start the probe on them alternately in one job and compare one checkout's
median with the other's range (profiles/second_pass_reader.txt)."""
import argparse, hashlib, json, os, sys, time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--video", default=os.path.join(HERE, "tests", "golden", "ref_test_video.mp4"))
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--root", default=HERE, help="checkout whose evenvizion_amd package is measured")
ap.add_argument("--out", default="", help="also append the JSON result line here")
args = ap.parse_args()

sys.path.insert(0, os.path.abspath(args.root))
from evenvizion_amd import capture, heatmap, moving, registration, stabilization
try:
    from evenvizion_amd import blend
except ImportError:                      # --root names a checkout from before the blended mosaic
    blend = None
from evenvizion_amd.processing.utils import superposition_dict
from evenvizion_amd.processing.video_processing import get_homography_dict


def video():
    cap = capture.VideoCapture(args.video)
    assert cap.isOpened(), "cannot open %s" % args.video
    return cap


first = get_homography_dict(video(), features_type_list=["ORB"])
info = first["resize_info"]
sup = superposition_dict({k: v for k, v in first.items() if k != "resize_info"})
plate = stabilization.background_plate(video(), sup, info)


def sha1(result, h=None):
    """SHA-1 over the bytes, strings and numbers of nested lists and tuples, in order."""
    top = h is None
    h = hashlib.sha1() if top else h
    if isinstance(result, (list, tuple)):
        for item in result:
            sha1(item, h)
    else:
        h.update(result if isinstance(result, bytes) else repr(result).encode())
    return h.hexdigest() if top else None


def pictures(generator):
    """Everything a generator of (frame_no, picture) yields, as bytes in order."""
    return [(no, np.ascontiguousarray(picture).tobytes()) for no, picture in generator]


def matching(ingest):
    got = []
    d = get_homography_dict(video(), features_type_list=["ORB"], ingest=ingest, matching_sink=lambda no, p: got.append((no, p.tobytes())))
    return got, json.dumps(d)


DRIVERS = [
    ("stabilized_frames_trail", lambda ingest: pictures(stabilization.stabilized_frames(video(), sup, info, trail=True, ingest=ingest))),
    ("comparison_frames", lambda ingest: pictures(stabilization.comparison_frames(video(), sup, info, ingest=ingest))),
    ("background_plate", lambda ingest: [a.tobytes() for a in stabilization.background_plate(video(), sup, info, ingest=ingest)[:2]]),
    ("heatmap_frames", lambda ingest: pictures(heatmap.heatmap_frames(video(), sup, info, ingest=ingest))),
    ("registration_report", lambda ingest: json.dumps(registration.registration_report(video(), sup, info, ingest=ingest))),
    ("refine_homography_dict", lambda ingest: json.dumps(moving.refine_homography_dict(video(), first, plate, ingest=ingest))),
    ("get_homography_dict_sink", matching),
]
if blend is not None:
    DRIVERS.append(("blended_mosaic", lambda ingest: blend.blended_mosaic(video(), sup, info, ingest=ingest).tobytes()))
cases = [(name, ingest, run) for name, run in DRIVERS for ingest in ("bgr", "auto")]
res = dict(root="this tree" if os.path.abspath(args.root) == HERE else args.root, video=os.path.basename(args.video),
           frames=len(first), repeats=args.repeats, seconds={}, sha1={})
for name, ingest, run in cases:                               # warm-up, and what was computed
    res["sha1"]["%s/%s" % (name, ingest)] = sha1(run(ingest))
    res["seconds"]["%s/%s" % (name, ingest)] = []
for _ in range(args.repeats):
    for name, ingest, run in cases:
        t = time.perf_counter()
        run(ingest)
        res["seconds"]["%s/%s" % (name, ingest)].append(round(time.perf_counter() - t, 4))
print(json.dumps(res))
if args.out:
    with open(args.out, "a") as fh:
        fh.write(json.dumps(res) + "\n")
