"""Stream driver -- MI355X counterpart of evenvizion/processing/video_processing.py:27-108.

get_homography_dict keeps the reference signature and result layout
    {frame_no: {"H": 3x3 list}, ..., "resize_info": {"h", "w"}}       (first key is 2)
but instead of one frame pair per Python iteration it reads the capture in chunks (double-buffered: reading and
uploading chunk i+1 overlap the GPU work on chunk i), uploads a chunk once, and runs the whole per-pair body on the GPU (evh_stream_homography_batch_resized: imutils.resize fused into the ingest kernel): ORB on every frame once
(the reference recomputes each frame's features twice), matching / RANSAC #1 / static filter for all
pairs of the chunk in parallel, and the final RANSAC as the sequential scan the running superposition requires
(utils.py:351-358, video_processing.py:102-103).  Consecutive chunks overlap by one frame and carry
{H_sup, H_prev} on the device.

With ingest="auto" / "yuv420" a capture that can hand over the decoder's own 4:2:0 planes (read_yuv420_into) is read that way: 1.5 bytes per pixel are
staged and uploaded instead of 3, and the BGR conversion of capture.read() (video_processing.py:58,70) happens inside the
ingest kernel (evh_stream_homography_batch_yuv420).  The dictionary is the same, bit for bit.
"""
import logging

import numpy as np

from .. import runtime
from .._lib import PAIR_OK, PAIR_CAPACITY, EvhError
from ..frames import DeviceLadder, check_ingest, open_capture, read_frame

CHUNK_FRAMES = 64   # frames uploaded per GPU call (pairs per call = CHUNK_FRAMES - 1)


def resized_shape(frame_shape, resize_width):
    """imutils.resize(width=): r = width / float(w); dim = (width, int(h * r)) (video_processing.py:62)."""
    h0, w0 = frame_shape[:2]
    r = resize_width / float(w0)
    return int(resize_width), int(h0 * r)


def _feature_list(features_type_list):
    """-> the feature list a driver runs with (None: the reference's default); ValueError as the reference raises it."""
    from .frame_processing import DEFAULT_FEATURES
    features = list(features_type_list or DEFAULT_FEATURES)
    for name in features:
        if name not in ("ORB", "SIFT", "SURF"):
            raise ValueError("You need to choose descriptors type")
    return features


def _upload(B, j, spans, cur):
    """Frames of pinned host buffer j to device buffer j on the copy stream, one copy per span (device frame, host frame,
    frames); torch's current stream `cur` (None on the CPU) then waits for them."""
    if cur is None:
        for a, b, n in spans:
            B["dev"][j][a:a + n].copy_(B["host"][j][b:b + n])
        return
    import torch
    with torch.cuda.stream(B["copy_stream"]):
        for a, b, n in spans:
            B["dev"][j][a:a + n].copy_(B["host"][j][b:b + n], non_blocking=True)
        B["up_done"][j].record(B["copy_stream"])
    cur.wait_event(B["up_done"][j])


def _results_to_host(c, B, j, npairs, cur, extra=()):
    """H and status of the first npairs pair slots of buffer j back through pinned memory, behind everything context `c` has
    enqueued; all_done[j] marks their arrival (cur: torch's current stream, None on the CPU).  extra: further (host, device)
    tensors whose first npairs entries come back with them."""
    if cur is not None:
        c.order_torch_after()
    B["H_host"][j][:npairs].copy_(B["H_dev"][j][:npairs], non_blocking=True)
    B["st_host"][j][:npairs].copy_(B["st_dev"][j][:npairs], non_blocking=True)
    for host, device in extra:
        host[:npairs].copy_(device[:npairs], non_blocking=True)
    if cur is not None:
        B["all_done"][j].record(cur)


def _pairs_into(result, frame_no, Hs, sts, none_H_processing, capture_index=None, before_pair=None):
    """Consecutive pairs (Hs f64[k,3,3], sts i32[k]) of one capture into its dictionary: the pair ending at frame f becomes
    result[f] = {"H": ...}.  frame_no: the newest frame already paired; -> the same after these.  capture_index names the
    capture in the log line of the many-captures driver.  before_pair(k, f) is called for pair k of these, ending at frame f,
    before its status is looked at: what the reference does between matching and compute_homography."""
    for k, (Hk, sk) in enumerate(zip(Hs, sts)):
        frame_no += 1
        if before_pair is not None:
            before_pair(k, frame_no)
        if sk != PAIR_OK:
            if capture_index is None:
                logging.info("pair ending at frame %d: no homography (status %d)", frame_no, int(sk))
            else:
                logging.info("capture %d, pair ending at frame %d: no homography (status %d)", capture_index, frame_no, int(sk))
            if not none_H_processing or not np.all(np.isfinite(Hk)):
                # reference behaviour (video_processing.py:94-101): H stays None and None.tolist() raises --
                # always for none_H_processing=False, and for a failing FIRST pair otherwise
                raise AttributeError("'NoneType' object has no attribute 'tolist' (no homography for frame %d, "
                                     "status %d)" % (frame_no, int(sk)))
        result[frame_no] = {"H": Hk.tolist()}
    return frame_no


def rerun_on_larger_slots(ctx, features, nfeatures, dw, dh, max_frames, run, overflowed, what):
    """Some frame delivered more tied key points than a frame slot of `ctx` holds (a pair reported EVH_PAIR_CAPACITY).
    The reference has no such bound (it carries on with every tie, frame_processing.py:59-61), so the work is done again
    -- run(big), which starts from the state the work was entered with; its results are waited for here -- on a context whose
    frame slots are twice as large (same nfeatures, so the same key points for every other frame), doubling again while
    overflowed() still says so, up to the LDS limit of the matching filter.  `what` names the frames in the error."""
    from .._lib import Context, MAX_FEATURES
    # every list grows from what the context that overflowed actually had, each up to its own limit
    feats = max(ctx.max_features, nfeatures)
    sift0 = max(ctx.lib.evh_sift_capacity(ctx.h), runtime.sift_features_for(dw, dh)) if "SIFT" in features else 0
    surf0 = max(ctx.lib.evh_surf_capacity(ctx.h), runtime.surf_features_for(dw, dh)) if "SURF" in features else 0
    grow = 1
    while True:
        at_limit = feats >= MAX_FEATURES and (not sift0 or sift0 * grow >= runtime.TYPE_FEATURES_MAX) and \
            (not surf0 or surf0 * grow >= runtime.TYPE_FEATURES_MAX)
        feats = min(feats * 2, MAX_FEATURES)
        grow *= 2
        try:
            if at_limit:
                raise EvhError("giving up")
            big = Context(device=runtime.device_index(), max_w=max(dw, 64), max_h=max(dh, 64),
                          max_features=feats, max_frames=max_frames)
            if sift0:
                big.sift_enable(min(runtime.TYPE_FEATURES_MAX, sift0 * grow))
            if surf0:
                big.surf_enable(min(runtime.TYPE_FEATURES_MAX, surf0 * grow))
        except EvhError:
            raise EvhError("%s: more key points (ORB ties at the retainBest cut, or SIFT key points) than "
                           "the largest frame slot this device path supports" % what)
        try:
            run(big)
            if runtime.device().type == "cuda":
                import torch
                torch.cuda.synchronize(runtime.device())
            else:                   # (the host-loop unit tests: a scripted context on the CPU)
                big.synchronize()
        finally:
            big.close()
        if not overflowed():
            break


class _MatchingPictures:
    """What get_homography_dict(matching_sink=) adds to a chunk: the resized BGR frames, the rows that entered the final solve
    and the pictures on the device, and the pictures and front statuses back through pinned memory with the chunk's results."""

    def __init__(self, B, chunk_frames, planes, w0, h0, dw, dh, points, dev):
        import torch
        from .._lib import DRAW_POINTS
        if points not in DRAW_POINTS:
            raise ValueError("matching_points must be one of %s" % sorted(DRAW_POINTS))
        self.points, self.dev = points, dev
        npairs = chunk_frames - 1
        self.ladder = DeviceLadder(dev, chunk_frames, planes, (w0, h0), (dw, dh), bgr=True)
        # the picture and front-status buffers live with the staging set B (runtime.staging: pinning is slow, a service
        # processes many videos of one size) and go when it goes
        key = ("pictures", dw, dh)
        if key not in B:
            pin = runtime._pin if dev.type == "cuda" else (lambda t: t)
            B[key] = ([torch.empty((npairs, dh, 2 * dw, 3), dtype=torch.uint8, device=dev) for _ in range(2)],
                      [pin(torch.empty((npairs, dh, 2 * dw, 3), dtype=torch.uint8)) for _ in range(2)],
                      [torch.empty(npairs, dtype=torch.int32, device=dev) for _ in range(2)],
                      [pin(torch.empty(npairs, dtype=torch.int32)) for _ in range(2)])
        self.pic_dev, self.pic_host, self.st1_dev, self.st1_host = B[key]
        self.rows = {}          # row capacity of a context -> (rows, counts): a re-run on larger slots has its own

    def draw(self, c, frames, j):
        """Behind the batch entry `c` has just run on `frames` (the chunk as uploaded): the pictures of its pairs into
        pic_dev[j], their front statuses into st1_dev[j].  -> what _results_to_host brings back besides H and status."""
        import torch
        nb = frames.shape[0]
        _, src, _ = self.ladder(c, frames)
        cap = c.batch_static_info()[1]
        if cap not in self.rows:
            self.rows[cap] = (torch.empty((self.pic_dev[0].shape[0], cap, 4), dtype=torch.float32, device=self.dev),
                              torch.empty(self.pic_dev[0].shape[0], dtype=torch.int32, device=self.dev))
        rows, counts = self.rows[cap]
        c.batch_static_rows(0, nb - 1, rows, counts, self.st1_dev[j])
        c.draw_matches(src, rows, counts, self.pic_dev[j][:nb - 1], status=self.st1_dev[j], frame_step=1, points=self.points)
        return [(self.pic_host[j], self.pic_dev[j]), (self.st1_host[j], self.st1_dev[j])]


def get_homography_dict(capture, resize_width=400, matching_path=None, none_H_processing=True,
                        nfeatures=runtime.NFEATURES, chunk_frames=CHUNK_FRAMES, features_type_list=None, ingest="bgr",
                        matching_sink=None, matching_points="reference"):
    """capture: anything with read() -> (bool, BGR uint8 frame) (cv2.VideoCapture duck type).
    ingest: "bgr" (always read(); the default until the plane path's end-to-end rates have been measured against it, see
    DESIGN.md 3a), "auto" (planes when the capture can deliver them, see frames.first_planes), "yuv420" (planes or ValueError).
    features_type_list: the list the reference hands to FrameProcessing (frame_processing.py:37-40), e.g. ["SIFT", "ORB"];
    None = frame_processing.DEFAULT_FEATURES = the reference's own default ["SURF", "SIFT", "ORB"]; the north-star hot path
    is features_type_list=["ORB"] (one fused ORB pipeline, evh_stream_homography_batch_resized).
    matching_sink: a callable matching_sink(frame_no, picture) that receives the reference's matching picture of every pair
    whose matching succeeded (front status OK: the reference draws before compute_homography, so a pair that then fails still
    has one, a pair without matches has none), in frame order, frame_no being the number of the pair's newer frame (the i of
    matching_vis_{i}.png, first 2) and picture a uint8 array [h, 2w, 3] (BGR, the resized previous frame | the resized current
    frame, one green line per static match; the array is the sink's to keep).  When the call raises for a pair, the pictures
    up to that pair have been delivered.  matching_points: "reference" draws what video_processing.py:69-80 draws -- the newer
    frame's points on the older frame's half and vice versa --, "own_frame" each point on its own frame.  A capture of gray
    frames is refused with a sink (ValueError).  None: nothing of this is computed."""
    import torch
    if matching_path:
        raise NotImplementedError("matching_path (draw_matches + imwrite into a directory) is not taken: pass "
                                  "matching_sink=callable(frame_no, picture) -- matching_pictures.write_png stores a picture; "
                                  "the command line has --matching_pictures")
    check_ingest(ingest)
    first, planes, w0, h0 = open_capture(capture, ingest)
    if matching_sink is not None and not planes and first.ndim != 3:
        raise ValueError("matching_sink takes BGR frames [h,w,3] or decoded planes: the picture is a BGR picture, and the "
                         "reference's capture delivers no gray frames")
    dw, dh = resized_shape((h0, w0), resize_width)
    features = _feature_list(features_type_list)
    # the Context method of a chunk and what it takes besides frames, outputs and state, from planes x multi: the decoder's
    # planes or BGR frames as the source; the fused ORB entry or frame_processing.py:91-104 over the type list
    multi = features != ["ORB"]
    method = "stream_homography_batch" + ("_types" if multi else "") + ("_yuv420" if planes else "")
    size, types = ((w0, h0),) if planes else (), (features,) if multi else ()
    # one staging buffer (pinned host / device) is capped in bytes: 4K BGR frames give 21-frame chunks, not 64
    # (with a sink, a pair's picture of 6*dw*dh bytes is staged too)
    chunk_frames = runtime.chunk_frames_for(max(first.nbytes, 6 * dw * dh if matching_sink is not None else 0),
                                            max(2, int(chunk_frames)))
    # sized for the RESIZED frames: only those go through ORB (evh_resize_area_u8 does not depend on the context's
    # geometry), so a 4K source with resize_width=400 allocates 400-wide buffers
    ctx = runtime.get_context(dw, dh, chunk_frames, nfeatures, sift="SIFT" in features, surf="SURF" in features)
    dev = runtime.device()
    # Double-buffered chunk pipeline: while the GPU works on chunk i the host reads chunk i+1 from the capture into
    # pinned memory and its upload runs on a copy stream; results come back through pinned buffers.  Chunk i is
    # launched BEFORE the results of chunk i-1 are collected, so the device queue never drains.
    B = runtime.staging((chunk_frames,) + first.shape, dev)
    host_np, devbuf, all_done = B["host_np"], B["dev"], B["all_done"]
    H_dev, st_dev, H_host, st_host = B["H_dev"], B["st_dev"], B["H_host"], B["st_host"]
    state = torch.zeros(18, dtype=torch.float64, device=dev)
    # {H_sup, H_prev} as they ENTER each in-flight chunk (and whether there was a state at all): what a chunk is re-run
    # from when one of its frames overflows a frame slot (EVH_PAIR_CAPACITY)
    state_pre = [torch.zeros(18, dtype=torch.float64, device=dev) for _ in range(2)]
    had_state = [False, False]
    cuda = dev.type == "cuda"          # (the host-loop unit test drives this function on the CPU with a scripted context)
    cur = torch.cuda.current_stream(dev) if cuda else None

    pictures = None
    if matching_sink is not None:
        pictures = _MatchingPictures(B, chunk_frames, planes, w0, h0, dw, dh, matching_points, dev)

    homography_dict = {}
    frame_no = [1]          # 1-based index of the newest frame already paired

    def launch(c, jb, nb, with_state):
        getattr(c, method)(devbuf[jb][:nb], *size, H_dev[jb], st_dev[jb], *types, state_in=state if with_state else None,
                           state_out=state, nfeatures=nfeatures, resize_to=(dw, dh))
        # the pictures are drawn here so that a re-run on larger slots draws them again from its own rows
        extra = pictures.draw(c, devbuf[jb][:nb], jb) if pictures is not None else ()
        _results_to_host(c, B, jb, nb - 1, cur, extra)

    def rerun_with_larger_slots(jb, nb, later):
        """A frame of chunk jb delivered more tied key points than a frame slot of `ctx` holds: the chunk is re-run from
        the state it was entered with (rerun_on_larger_slots); the chunk launched after it (computed from a state that is
        now stale) is then re-run as well."""
        if cuda:
            torch.cuda.synchronize(dev)

        def run(big):
            state.copy_(state_pre[jb])
            launch(big, jb, nb, had_state[jb])

        rerun_on_larger_slots(ctx, features, nfeatures, dw, dh, chunk_frames, run,
                              lambda: bool((st_host[jb][:nb - 1].numpy() == PAIR_CAPACITY).any()),
                              "frame %d..%d" % (frame_no[0], frame_no[0] + nb - 1))
        if later is not None:                           # the chunk that was in flight behind it
            lj, ln = later
            state_pre[lj].copy_(state)
            had_state[lj] = True
            launch(ctx, lj, ln, True)

    def collect(jb, nb, later=None):
        if cuda:
            all_done[jb].synchronize()
        if (st_host[jb][:nb - 1].numpy() == PAIR_CAPACITY).any():
            rerun_with_larger_slots(jb, nb, later)
        deliver = None
        if pictures is not None:
            st1, pics = pictures.st1_host[jb].numpy(), pictures.pic_host[jb].numpy()

            def deliver(k, f):
                if st1[k] == PAIR_OK:
                    matching_sink(f, pics[k].copy())
        frame_no[0] = _pairs_into(homography_dict, frame_no[0], H_host[jb][:nb - 1].numpy().reshape(-1, 3, 3),
                                  st_host[jb][:nb - 1].numpy(), none_H_processing, before_pair=deliver)

    j, n = 0, 1
    host_np[0][0] = first
    have_state = False
    exhausted = False
    inflight = None
    try:
        while True:
            while n < chunk_frames and not exhausted:
                if not read_frame(capture, planes, host_np[j][n], w0, h0, frame_no[0] + n):
                    exhausted = True
                    break
                n += 1
            launched = None
            if n >= 2:
                _upload(B, j, [(0, 0, n)], cur)
                # K0 fused into the ingest kernel: level 0 comes straight from the full-size frames (N2); equal sizes
                # are the plain gray conversion
                state_pre[j].copy_(state)               # stream-ordered: after chunk i-1's kernels, before chunk i's
                had_state[j] = have_state
                launch(ctx, j, n, have_state)
                have_state = True
                launched = (j, n)
            if inflight is not None:
                collect(*inflight, later=launched)
            inflight = launched
            if inflight is None:
                break
            host_np[1 - j][0] = host_np[j][n - 1]      # consecutive chunks overlap by one frame
            j, n = 1 - j, 1
    finally:
        if cuda:
            torch.cuda.synchronize(dev)                 # nothing of this call is left in flight on the shared buffers
    homography_dict["resize_info"] = {"h": dh, "w": dw}
    return homography_dict


MAX_STREAMS = 16     # captures of get_homography_dicts live at once (one scan workgroup each)
DECODE_THREADS = 8   # host threads reading frames for get_homography_dicts


class _Stream:
    """One capture inside get_homography_dicts: where it stands and what it has delivered."""

    def __init__(self, index, capture, first, planes, w0, h0):
        self.index, self.capture, self.first, self.planes, self.w0, self.h0 = index, capture, first, planes, w0, h0
        self.frame_no = 1        # 1-based index of the newest frame already paired
        self.read = 1            # frames taken from the capture so far
        self.started = False     # a round has carried its {H_sup, H_prev} out
        self.exhausted = False   # the capture has no further frame
        self.last = None         # index of its newest frame inside its region of the round before (None: not read yet)
        self.done = False        # its entry of the result list is final
        self.result = {}


def _read_frames(st, region):
    """Decode-pool task: the capture's next frames into region[1:], a stream's frames of the pinned staging buffer (frame 0 is
    the carried one).  -> (frames now in the region, error or None); sets st.exhausted when the capture ran dry."""
    n = 1
    try:
        while n < len(region):
            if not read_frame(st.capture, st.planes, region[n], st.w0, st.h0, st.read + 1):
                st.exhausted = True
                break
            st.read += 1
            n += 1
    except Exception as e:          # the capture's own failure: this capture's result, the others go on
        st.exhausted = True
        return n, e
    return n, None


def get_homography_dicts(captures, resize_width=400, none_H_processing=True, nfeatures=runtime.NFEATURES,
                         features_type_list=None, ingest="bgr", chunk_frames=CHUNK_FRAMES, max_streams=MAX_STREAMS,
                         decode_threads=DECODE_THREADS, return_exceptions=False):
    """get_homography_dict for several captures at once -> a list, entry i == get_homography_dict(captures[i], ...) with the
    same options, whatever max_streams, chunk_frames, the captures' lengths and their order.

    One capture alone cannot fill the card: its final RANSAC is a sequential scan (video_processing.py:83-105).  Here up to
    max_streams captures are live; a round hands every live capture up to chunk_frames - 1 new frames behind the frame it
    carries over, all of them go through one evh_streams_homography_batch call (detection and matching over all frames at
    once, one scan per capture side by side), and every capture's {H_sup, H_prev} stay on the device between rounds.  A
    capture that ended gives its place to the next waiting one.  Frames are read by `decode_threads` host threads, one
    capture per task, straight into the pinned staging buffer (libevcap releases the GIL); the reads of round r + 1 overlap
    the GPU work of round r, and one GPU round is in flight.  Captures are grouped by the geometry of their frames and by
    whether they deliver planes (the rule of frames.first_planes, per capture); the groups run one after another.  A capture is
    opened -- its first frame read, which decides its group -- only when a place is free for it, so what is held scales with
    max_streams, not with the list; one that turns out to belong to another group waits, opened, for that group's turn.

    A capture for which get_homography_dict would raise (ValueError: no first frame; AttributeError: a pair without H where
    the reference has none; whatever its read() raises): with return_exceptions=False the call raises that exception for the
    lowest such index once nothing of the call is in flight, with True the exception takes the capture's place in the list.
    A round in which a pair reports EVH_PAIR_CAPACITY is re-run as a whole on larger frame slots (rerun_on_larger_slots)."""
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from types import SimpleNamespace
    check_ingest(ingest)
    features = _feature_list(features_type_list)
    captures = list(captures)
    results = [None] * len(captures)
    max_streams, chunk_frames = max(1, int(max_streams)), max(2, int(chunk_frames))
    stop_after = [len(captures)]          # return_exceptions=False: captures behind the lowest failing index are not run

    def fail(index, exc):
        results[index] = exc
        if not return_exceptions:
            stop_after[0] = min(stop_after[0], index)

    pending = list(enumerate(captures))   # not opened yet
    deferred = {}                         # group key -> captures opened while another group was running, in list order

    def open_next(key):
        """The next capture of group `key` (None: of whatever group comes next), opened; captures of other groups met on the
        way wait in `deferred`."""
        if key is None and deferred:
            key = next(iter(deferred))
        if key in deferred:
            st = deferred[key].pop(0)
            if not deferred[key]:
                del deferred[key]
            return st
        while pending:
            i, capture = pending.pop(0)
            if i > stop_after[0]:
                continue
            try:
                first, planes, w0, h0 = open_capture(capture, ingest)
            except Exception as e:
                fail(i, e)
                continue
            st = _Stream(i, capture, first, planes, w0, h0)
            st.key = (planes, first.shape, w0, h0)
            if key is None or st.key == key:
                return st
            deferred.setdefault(st.key, []).append(st)
        return None

    dev = runtime.device()
    cuda = dev.type == "cuda"          # (the host-loop unit tests drive this function on the CPU with a scripted context)
    pool = ThreadPoolExecutor(max_workers=max(1, int(decode_threads)))
    # what every group runs with: the call's options, and where its captures' results and failures go
    opts = SimpleNamespace(resize_width=resize_width, none_H_processing=none_H_processing, nfeatures=nfeatures, features=features,
                          chunk_frames=chunk_frames, max_streams=max_streams, pool=pool, dev=dev, fail=fail,
                          stop_after=stop_after, results=results)
    try:
        while True:
            head = open_next(None)
            if head is None:
                break
            key = head.key
            more = len(pending) + len(deferred.get(key, ()))          # at most this many further members
            _run_group(opts, head, lambda: open_next(key), 1 + more)
    finally:
        pool.shutdown(wait=True)
        if cuda:
            torch.cuda.synchronize(dev)                 # nothing of this call is left in flight on the shared buffers
    if not return_exceptions and stop_after[0] < len(captures):
        raise results[stop_after[0]]
    return results


def _run_group(opts, head, next_member, at_most):
    """The captures of one geometry (head.key) -- `head`, then whatever next_member() opens, at_most of them -- through rounds
    of evh_streams_homography_batch (see get_homography_dicts).  opts: the call's options and result lists."""
    import torch
    planes, shape, w0, h0 = head.key
    nfeatures, features, chunk_frames, dev, stop_after = opts.nfeatures, opts.features, opts.chunk_frames, opts.dev, opts.stop_after
    cuda = dev.type == "cuda"
    dw, dh = resized_shape((h0, w0), opts.resize_width)
    # the staging buffer is capped in bytes: fewer live captures, then shorter chunks, for large frames
    S = min(opts.max_streams, at_most)
    total = runtime.chunk_frames_for(int(np.prod(shape)), S * chunk_frames)
    S = max(1, min(S, total // 2))
    cf = max(2, min(chunk_frames, total // S))          # frames of one capture in a round, the carried one included
    total = S * cf
    ctx = runtime.get_context(dw, dh, total, nfeatures, sift="SIFT" in features, surf="SURF" in features)
    B = runtime.staging((total,) + tuple(shape), dev)
    host_np, devbuf, all_done = B["host_np"], B["dev"], B["all_done"]
    H_dev, st_dev, H_host, st_host = B["H_dev"], B["st_dev"], B["H_host"], B["st_host"]
    cur = torch.cuda.current_stream(dev) if cuda else None
    state = torch.zeros(S, 18, dtype=torch.float64, device=dev)       # {H_sup, H_prev} of the capture reading in every place
    waiting = [head]                                                  # opened, not placed yet
    drained = [False]                                                 # next_member() has said that no more come
    places = [None] * S                                               # the captures that are still being read

    def finish(st, exc=None):
        if exc is not None:
            opts.fail(st.index, exc)
        else:
            st.result["resize_info"] = {"h": dh, "w": dw}
            opts.results[st.index] = st.result
        st.done = True

    def start_reads(j):
        """A waiting capture into every free place, then every place's next frames into its region of host buffer j, behind
        the frame it carries over (consecutive rounds overlap by one frame)."""
        reads = []
        for k in range(S):
            while places[k] is None and not drained[0]:
                st = waiting.pop(0) if waiting else next_member()
                if st is None:
                    drained[0] = True
                elif st.index < stop_after[0]:
                    places[k] = st
            st = places[k]
            if st is None:
                continue
            region = host_np[j][k * cf:(k + 1) * cf]
            if st.last is None:
                region[0], st.first = st.first, None
            else:
                region[0] = host_np[1 - j][k * cf + st.last]
            reads.append((k, st, opts.pool.submit(_read_frames, st, region)))
        return reads

    def launch(c, j, table, state_in, state_out):
        segs = [(a, n, not st.started) for (_, st, a, n, _) in table]
        nb = segs[-1][0] + segs[-1][1]
        c.streams_homography_batch(devbuf[j][:nb], segs, H_dev[j], st_dev[j], features=features, state_in=state_in,
                                   state_out=state_out, nfeatures=nfeatures, resize_to=(dw, dh),
                                   size=(w0, h0) if planes else None)
        _results_to_host(c, B, j, nb - 1, cur)

    def collect(j, table, idx, state_in, state_out):
        """The results of the round in flight: re-run on larger slots if a frame overflowed, the states back to their places,
        every capture's pairs into its dictionary."""
        if cuda:
            all_done[j].synchronize()
        rows = np.concatenate([np.arange(a, a + n - 1) for (_, _, a, n, _) in table])

        def overflowed():
            return bool((st_host[j].numpy()[rows] == PAIR_CAPACITY).any())

        if overflowed():
            if cuda:
                torch.cuda.synchronize(dev)

            rerun_on_larger_slots(ctx, features, nfeatures, dw, dh, total,
                                  lambda big: launch(big, j, table, state_in, state_out), overflowed,
                                  "captures %s" % [st.index for (_, st, _, _, _) in table])
        state[idx] = state_out
        Hs = H_host[j].numpy().reshape(-1, 3, 3)
        sts = st_host[j].numpy()
        for (k, st, a, n, last_round) in table:
            st.started = True
            try:
                st.frame_no = _pairs_into(st.result, st.frame_no, Hs[a:a + n - 1], sts[a:a + n - 1], opts.none_H_processing, st.index)
            except AttributeError as e:
                finish(st, e)
                if places[k] is st:
                    places[k] = None
                continue
            if last_round:
                finish(st)

    j = 0
    reads = start_reads(j)
    inflight = None
    while reads or inflight is not None:
        counts = []
        for k, st, fut in reads:                        # read while the round before this one runs on the GPU
            n, err = fut.result()
            st.last = n - 1
            counts.append((k, st, n, err))
        if inflight is not None:                        # one GPU round in flight: collected before the next is launched
            collect(*inflight)
            inflight = None
        table, pos = [], 0
        for k, st, n, err in counts:
            if st.exhausted and places[k] is st:
                places[k] = None                        # ran dry: the place goes to the next waiting capture
            if st.done:
                continue                                # failed in the round just collected
            if st.index > stop_after[0]:
                st.done = True                          # behind the lowest failing index nothing more is run
                places[k] = None
            elif err is not None:
                finish(st, err)
            elif n < 2:
                finish(st)                              # nothing new: the capture has ended and leaves the table
            else:
                table.append((k, st, pos, n, st.exhausted))
                pos += n
        if table:
            _upload(B, j, [(a, k * cf, n) for (k, _, a, n, _) in table], cur)     # the segments back to back on the device
            idx = torch.tensor([k for (k, _, _, _, _) in table], dtype=torch.long, device=dev)
            state_in = state[idx]                       # as the round is entered: what a re-run starts from
            state_out = torch.zeros_like(state_in)
            launch(ctx, j, table, state_in, state_out)
            inflight = (j, table, idx, state_in, state_out)
        j = 1 - j
        reads = start_reads(j)                          # the next round's frames, while this one runs
