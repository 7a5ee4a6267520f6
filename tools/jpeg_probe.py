"""Stand-alone probe of evh_jpeg_encode: 120 pictures of 400 x 224 and 64 of 1280 x 720, from evenvizion_amd/synthetic.py's frames
(coloured) and from the frames of tests/golden/ref_test_video.mp4 (resized on the device for the small case, repeated up to the
count), at quality 75 and 90, 4:2:0 and 4:4:4.  Per case: device time per call between two events around a run of calls
(warm-up first; the output buffer holds half the raw size per picture), the call through Context.jpeg_encode with the files
brought to the host (host time, synchronised), bytes out per picture, and the present route on the same buffers: download +
write_ppm, and download + write_png(level=1), host time included, files written to a temporary folder.  Writing the .jpg files is
timed too.  The probe reports; it is not a pass bar.
usage: python tools/jpeg_probe.py [seconds per case, default 1]"""
import json, os, sys, tempfile, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
import ctypes as C
import numpy as np, torch
from evenvizion_amd import capture, synthetic
from evenvizion_amd._lib import Context, JPEG_SUBSAMPLINGS
from evenvizion_amd.matching_pictures import write_png
from evenvizion_amd.pictures import quant_tables, write_jpeg
from evenvizion_amd.stabilization import write_ppm
window = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
ctx = Context(device=0, max_w=64, max_h=64, max_features=500, max_frames=2)
stream = ctx._torch_stream()
res = {}


def video_frames(count):
    cap, out = capture.VideoCapture(os.path.join(ROOT, 'tests', 'golden', 'ref_test_video.mp4')), []
    while len(out) < count:
        ok, f = cap.read()
        if not ok:
            break
        out.append(f)
    return np.stack(out)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ctx.synchronize()
    t = time.perf_counter()
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    ctx.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps, (time.perf_counter() - t) / reps


for w, h, n in ((400, 224, 120), (1280, 720, 64)):
    gray = synthetic.make_stream(5, min(n, 16), w, h)[0]
    synth = np.stack([gray, np.roll(gray, 3, 2), 255 - gray], -1)
    vid = video_frames(min(n, 32))
    sources = {'synthetic': torch.from_numpy(synth[np.arange(n) % len(synth)]).cuda()}
    v = torch.from_numpy(vid).cuda()
    if tuple(vid.shape[1:3]) != (h, w):
        small = torch.zeros((len(vid), h, w, 3), dtype=torch.uint8, device='cuda')
        ctx.resize_area(v, small)
        ctx.synchronize()
        v = small
    sources['video'] = v[torch.arange(n, device='cuda') % len(v)].contiguous()
    cap_bytes = w * h * 3 // 2
    out = torch.zeros((n, cap_bytes), dtype=torch.uint8, device='cuda')
    sizes = torch.zeros(n, dtype=torch.int64, device='cuda')
    folder = tempfile.mkdtemp()
    for name, pics in sources.items():
        key = '%dx%d_x%d_%s' % (w, h, n, name)
        host_route = {}
        for route, write in (('ppm', lambda p, a: write_ppm(p, a)), ('png1', lambda p, a: write_png(p, a, level=1))):
            torch.cuda.synchronize()
            t = time.perf_counter()
            host = pics.cpu().numpy()
            t1 = time.perf_counter()
            for k in range(n):
                write(os.path.join(folder, '%06d.%s' % (k, route)), host[k])
            t2 = time.perf_counter()
            host_route[route] = dict(download_ms=round((t1 - t) * 1e3, 2), write_ms=round((t2 - t1) * 1e3, 2),
                                     bytes_per_picture=int(np.mean([os.path.getsize(os.path.join(folder, '%06d.%s' % (k, route))) for k in range(n)])))
        res[key + '_present_route'] = host_route
        for quality in (75, 90):
            q = np.ascontiguousarray(quant_tables(quality))
            for sub in ('420', '444'):
                def call():
                    ctx.lib.evh_jpeg_encode(ctx.h, pics.data_ptr(), n, w, h, w * 3, w * h * 3, 3, JPEG_SUBSAMPLINGS[sub], q.ctypes.data_as(C.c_void_p),
                                            out.data_ptr(), cap_bytes, cap_bytes, sizes.data_ptr())
                timed(call, 2)
                per = timed(call, 3)[1]
                dev_s, _ = timed(call, max(3, int(window / per)))
                lengths = sizes.cpu().numpy()
                assert lengths.max() <= cap_bytes
                t = time.perf_counter()
                files = ctx.jpeg_encode(pics, q, sub, out=out)
                t1 = time.perf_counter()
                for k, f in enumerate(files):
                    write_jpeg(os.path.join(folder, '%06d.jpg' % k), f)
                t2 = time.perf_counter()
                res['%s_q%d_%s' % (key, quality, sub)] = dict(
                    device_ms_per_call=round(dev_s * 1e3, 3), pictures_per_s=round(n / dev_s), raw_GB_per_s=round(n * w * h * 3 / dev_s * 1e-9, 1),
                    bytes_per_picture=int(lengths.mean()), of_raw=round(float(lengths.mean()) / (w * h * 3), 4),
                    encode_and_download_ms=round((t1 - t) * 1e3, 2), write_ms=round((t2 - t1) * 1e3, 2))
    del sources, out
ctx.close()
print(json.dumps(res, indent=1))
