"""Every batch entry of libevhip once, all outputs (H, status, state out) into one .npz: what two builds are compared by.

    python tools/batch_entries_dump.py OUT.npz              run and save
    python tools/batch_entries_dump.py --compare A.npz B.npz   byte-for-byte comparison, exit status 1 on any difference

Frames: three synthetic streams of 3, 2 and 4 frames at 400x224, nfeatures 500.  Each entry runs adaptive and with
force_max_iters; the fused entries with ORB, the _types entries (and the ragged entries, which take a list too) with ["ORB"],
["SIFT", "ORB"] and the default ["SURF", "SIFT", "ORB"], SIFT and SURF enabled at small capacities; packed BGR and 4:2:0 planes
where an entry has both forms."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

W, H = 400, 224
LENS = (3, 2, 4)
LISTS = (["ORB"], ["SIFT", "ORB"], ["SURF", "SIFT", "ORB"])


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files))
    for k in sorted(set(A.files) & set(B.files)):
        if A[k].dtype != B[k].dtype or A[k].shape != B[k].shape or A[k].tobytes() != B[k].tobytes():
            bad.append(k)
    nbytes = sum(A[k].nbytes for k in A.files)
    print("%s vs %s: %d arrays, %d bytes, %s" % (a, b, len(A.files), nbytes, "all equal byte for byte" if not bad else "DIFFERENT: %s" % bad))
    return 1 if bad else 0


def run(path):
    import torch
    from evenvizion_amd import synthetic as S
    from evenvizion_amd._lib import Context, MODE_INDEPENDENT_PAIRS, MODE_STREAM
    rng = np.random.default_rng(5)
    gray = [S.make_stream(90 + i, n, W, H)[0] for i, n in enumerate(LENS)]
    planes = [[(g,) + S.chroma_for(rng, g) for g in st] for st in gray]
    bgr = [np.stack([S.yuv420_to_bgr_host(*p) for p in st]) for st in planes]        # the frames the planes convert to
    total = sum(LENS)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_bgr = [dev(b) for b in bgr]
    d_all = dev(np.concatenate(bgr))
    d_packed = [dev(np.stack([np.concatenate([a.reshape(-1) for a in p]) for p in st])) for st in planes]
    d_packed_all = torch.cat(d_packed)
    segs, at = [], 0
    for n in LENS:
        segs.append((at, n, 1))
        at += n
    c = Context(device=0, max_w=W, max_h=H, max_features=500, max_frames=total)
    c.sift_enable(4096)
    c.surf_enable(2048)
    out = {}

    def outputs(n, nstate=None):
        st = torch.full((18,) if nstate is None else (nstate, 18), -7.25, dtype=torch.float64, device="cuda")
        return torch.full((n, 9), -7.25, dtype=torch.float64, device="cuda"), torch.full((n,), -9, dtype=torch.int32, device="cuda"), st

    def keep(name, *arrays):
        c.synchronize()
        torch.cuda.synchronize()
        for tag, a in zip(("H", "status", "state"), arrays):
            out["%s.%s" % (name, tag)] = a.cpu().numpy()

    def carried(name, call, frames, **kw):
        """A stream entry on one stream in two chunks with the state carried (the second overlaps the first by one frame)."""
        n = frames.shape[0]
        cut = max(2, n - 1)
        Hk, sk, state = outputs(cut - 1)
        call(frames[:cut], Hk, sk, state_in=None, state_out=state, **kw)
        keep(name + ".chunk0", Hk, sk, state)
        if n - cut + 1 >= 2:
            Hk, sk, _ = outputs(n - cut)
            call(frames[cut - 1:], Hk, sk, state_in=state, state_out=state, **kw)
            keep(name + ".chunk1", Hk, sk, state)

    for force in (False, True):
        f = "forced" if force else "adaptive"
        kw = dict(force_max_iters=force)
        # fused ORB entries
        Hk, sk, _ = outputs(4)
        c.pair_homography_batch(d_all[:8], 4, MODE_INDEPENDENT_PAIRS, Hk, sk, **kw)
        keep("pair.%s.independent" % f, Hk, sk)
        Hk, sk, _ = outputs(total - 1)
        c.pair_homography_batch(d_all, total - 1, MODE_STREAM, Hk, sk, **kw)
        keep("pair.%s.stream" % f, Hk, sk)
        for i in range(len(LENS)):
            carried("stream.%s.%d" % (f, i), c.stream_homography_batch, d_bgr[i], **kw)
            carried("stream_resized.%s.%d" % (f, i), c.stream_homography_batch, d_bgr[i], resize_to=(300, 168), **kw)
            carried("stream_yuv420.%s.%d" % (f, i), lambda fr, *a, **k: c.stream_homography_batch_yuv420(fr, (W, H), *a, **k),
                    d_packed[i], **kw)
        multi = torch.stack([b[:2] for b in d_bgr])
        Hm = torch.full((3, 1, 9), -7.25, dtype=torch.float64, device="cuda")
        sm = torch.full((3, 1), -9, dtype=torch.int32, device="cuda")
        stm = torch.full((3, 18), -7.25, dtype=torch.float64, device="cuda")
        c.multi_stream_homography_batch(multi, Hm, sm, state_out=stm, **kw)
        keep("multi.%s.first" % f, Hm, sm, stm)
        c.multi_stream_homography_batch(multi, Hm, sm, state_in=stm, state_out=stm, **kw)
        keep("multi.%s.carried" % f, Hm, sm, stm)
        rows, counts, st1 = c.stream_static_batch(d_all, **kw)
        c.synchronize()
        live = torch.arange(rows.shape[1], device="cuda")[None, :] < counts[:, None]      # rows past a pair's count are leftovers
        keep("static.%s" % f, rows * live[..., None], counts, st1)
        state = torch.full((18,), -7.25, dtype=torch.float64, device="cuda")
        Hk, sk = c.stream_scan(rows, counts, st1, state_out=state, **kw)
        keep("scan.%s" % f, Hk, sk, state)
        # entries that take a type list
        for feats in LISTS:
            t = "+".join(feats)
            Hk, sk, _ = outputs(4)
            c.pair_homography_batch_types(d_all[:8], 4, MODE_INDEPENDENT_PAIRS, Hk, sk, feats, **kw)
            keep("pair_types.%s.%s.independent" % (f, t), Hk, sk)
            Hk, sk, _ = outputs(total - 1)
            c.pair_homography_batch_types(d_all, total - 1, MODE_STREAM, Hk, sk, feats, resize_to=(300, 168), **kw)
            keep("pair_types.%s.%s.stream_resized" % (f, t), Hk, sk)
            carried("stream_types.%s.%s" % (f, t), lambda fr, *a, **k: c.stream_homography_batch_types(fr, *a, features=feats, **k),
                    d_bgr[2], **kw)
            carried("stream_types_yuv420.%s.%s" % (f, t),
                    lambda fr, *a, **k: c.stream_homography_batch_types_yuv420(fr, (W, H), *a, features=feats, **k), d_packed[2], **kw)
            for form, frames, size in (("bgr", d_all, None), ("yuv420", d_packed_all, (W, H))):
                Hk, sk, state = outputs(total - 1, len(LENS))
                c.streams_homography_batch(frames, segs, Hk, sk, features=feats, state_in=None, state_out=state, size=size, **kw)
                keep("streams.%s.%s.%s.first" % (f, t, form), Hk, sk, state)
                Hk, sk, _ = outputs(total - 1)
                c.streams_homography_batch(frames, [(a, n, 0) for a, n, _ in segs], Hk, sk, features=feats, state_in=state,
                                           state_out=state, size=size, resize_to=(300, 168), **kw)
                keep("streams.%s.%s.%s.carried_resized" % (f, t, form), Hk, sk, state)
    c.close()
    np.savez(path, **out)
    ok = sum(int((a == 0).sum()) for k, a in out.items() if k.endswith(".status") and not k.startswith("static"))
    print("%s: %d arrays, %d pair slots with status 0" % (path, len(out), ok))


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    run(sys.argv[1])
