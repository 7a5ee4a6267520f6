"""Stand-alone probe of evh_graph_normal and of the global alignment built on it.
  1. time per launch at 120 edges x 500 rows and at 1 200 edges x 500 rows (6 and 60 frames' worth of a 121-frame video with four
     loop partners per frame), with and without the gate and the Huber weight; beside it the route the entry replaces: the download
     of the rows and the numpy restatement of tests/graph_checks.py (its plain path) on the same rows, for scale.
  2. the reference's video (tests/golden), where present: for each model the edges tried and kept, the cost before and after, the
     ITF and the canvas score of DESIGN section 22 (evh_canvas_refine with iters = 0) of the recorded, the anchored and the aligned
     dictionary.  ORB gives some consecutive pairs of that video fewer than the default 20 inliers (the refusal is recorded), so the
     runs are made with min_inliers = 8.
Device time between two events around a run of calls filling a window of seconds, after a warm-up (as tools/components_probe.py).
usage: python tools/graph_probe.py [seconds per case, default 1] [0 = leave out the video]"""
import os, sys, time, json
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np, torch
import graph_checks as GC
from evenvizion_amd import graph
from evenvizion_amd._lib import Context
window = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
video = len(sys.argv) < 3 or sys.argv[2] != '0'
ctx = Context(device=0, max_w=64, max_h=64, max_features=500, max_frames=2)
stream = ctx._torch_stream()
rng = np.random.default_rng(25)
res = {}
MIN_INLIERS = 8


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


for nedges in (120, 1200):
    nframes, cap = max(6, nedges // 20), 512
    S = np.stack([np.eye(3) + rng.normal(0, [[.01, .01, 30], [.01, .01, 30], [1e-5, 1e-5, 0]]) for _ in range(nframes)])
    i = rng.integers(1, nframes, nedges)
    edges = np.stack([i, (i - 1 - rng.integers(0, 8, nedges)).clip(0)], axis=1).astype(np.int32)
    edges[edges[:, 0] == edges[:, 1], 1] = 0
    a = rng.uniform([0, 0], [400, 224], (nedges, cap, 2))
    rows = np.concatenate([a, a + rng.normal(0, 1.0, a.shape)], axis=2).astype(np.float32)
    H = np.tile(np.eye(3).reshape(1, 9), (nedges, 1))
    counts = np.full(nedges, 500, np.int32)
    d = [torch.from_numpy(x).cuda() for x in (S.reshape(-1), edges, rows, counts, H.reshape(-1))]
    sums = torch.empty((nedges, 154), dtype=torch.float64, device='cuda')
    info = torch.empty((nedges, 4), dtype=torch.int32, device='cuda')
    for name, He, delta in (('plain', None, 0.0), ('gate_huber', d[4], 1.5)):
        reps, dev_us, host_us = timed(lambda: ctx.graph_normal(d[0], d[1], d[2], d[3], None, He, 3.0, delta, sums, info))
        key = 'normal_%d_edges_%s' % (nedges, name)
        res[key] = dict(edges=nedges, rows_per_edge=500, launches=reps, device_us_per_launch=round(dev_us, 1), host_us_per_launch=round(host_us, 1),
                        row_GB_per_s=round(nedges * 500 * 16 / dev_us * 1e-3, 2), used=int(info[:, 0].sum().cpu()))
        print(json.dumps({key: res[key]}), flush=True)
    ctx.synchronize()
    t0 = time.perf_counter()
    h_rows, h_counts = d[2].cpu().numpy(), d[3].cpu().numpy()
    t1 = time.perf_counter()
    GC.normal(S, edges, h_rows, h_counts, exact=False)
    t2 = time.perf_counter()
    key = 'normal_%d_edges_download_and_numpy' % nedges
    res[key] = dict(row_bytes=h_rows.nbytes, download_ms=round((t1 - t0) * 1e3, 2), numpy_ms=round((t2 - t1) * 1e3, 1))
    print(json.dumps({key: res[key]}), flush=True)
ctx.close()

MP4, GOLD = os.path.join(ROOT, 'tests', 'golden', 'ref_test_video.mp4'), os.path.join(ROOT, 'tests', 'golden', 'ref_dict_with_homography_matrix.json')
if video and os.path.exists(MP4) and os.path.exists(GOLD):
    from evenvizion_amd import capture, registration
    from evenvizion_amd.processing.utils import read_homography_dict, superposition_dict
    hd, ri = read_homography_dict(GOLD)
    sup = superposition_dict(hd)
    keys = [k for k in sup if k != 'resize_info']
    cap_of = lambda: capture.VideoCapture(MP4)
    whole = {k: sup[k] for k in keys}
    try:
        graph.align_superposition(cap_of(), whole, ri, iters=0)
    except ValueError as e:
        res['video_min_inliers_20'] = dict(frames=len(keys), refused=str(e))
        print(json.dumps({'video_min_inliers_20': res['video_min_inliers_20']}), flush=True)
    score = lambda d: registration.anchored_homography_dict(cap_of, d, ri, iters=0)
    recorded = score(whole)
    anchored = registration.anchored_homography_dict(cap_of, whole, ri, iters=8)
    anchored_score = score(anchored['superposition'])
    res['video_recorded'] = dict(frames=len(keys), itf=recorded['report_before']['itf'], canvas_score=recorded['canvas_score_before'])
    res['video_anchored'] = dict(frames=len(keys), itf=anchored['report_after']['itf'], canvas_score=anchored_score['canvas_score_before'])
    print(json.dumps({k: res[k] for k in ('video_recorded', 'video_anchored')}), flush=True)
    for model in graph.MODELS:
        got = graph.aligned_homography_dict(cap_of, whole, ri, model=model, min_inliers=MIN_INLIERS)
        rep = got['report']
        res['video_aligned_%s' % model] = dict(frames=len(keys), min_inliers=MIN_INLIERS, edges_tried=len(rep['edges_tried']),
                                               edges_kept=len(rep['edges_kept']), loop_edges_kept=sum(len(v) for v in rep['loop_edges_kept'].values()),
                                               used_min=min(rep['used']), used_max=max(rep['used']), cost_before=rep['cost_before'],
                                               cost_after=rep['cost_after'], accepted=rep['accepted'], itf=rep['report_after']['itf'],
                                               canvas_score=score(got['superposition'])['canvas_score_before'])
        print(json.dumps({'video_aligned_%s' % model: res['video_aligned_%s' % model]}), flush=True)
print(json.dumps(res))
