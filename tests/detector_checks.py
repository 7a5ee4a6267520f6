"""The device side of the SIFT / SURF tests: contexts with the detectors enabled, frames onto the device, and the
bit-for-bit comparison of a downloaded key-point list with the oracle's.  Shared by tests/test_gpu_sift.py and
tests/test_gpu_detector_groups.py."""
import numpy as np
import pytest
import torch


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_ctx(w, h, frames=4, sift=4096, feats=500):
    from evenvizion_amd._lib import Context
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU; there is no CPU fallback")
    c = Context(device=0, max_w=w, max_h=h, max_features=feats, max_frames=frames)
    c.sift_enable(sift)
    return c


def make_surf_ctx(w, h, frames=4, surf=4096, sift=0):
    from evenvizion_amd._lib import Context
    c = Context(device=0, max_w=w, max_h=h, max_features=500, max_frames=frames)
    c.surf_enable(surf)
    if sift:
        c.sift_enable(sift)
    return c


def _same_keypoints(g, o):
    assert len(g["xy"]) == len(o["xy"]), (len(g["xy"]), len(o["xy"]))
    for k in ("xy", "size", "angle", "response"):
        assert np.array_equal(g[k].view(np.uint32), o[k].view(np.uint32)), k
    assert np.array_equal(g["octave"], o["octave"])
    assert np.array_equal(g["desc"], o["desc"])


def _same_surf(g, o):
    assert len(g["xy"]) == len(o["xy"]), (len(g["xy"]), len(o["xy"]))
    for k in ("xy", "size", "angle", "response", "desc"):
        assert np.array_equal(g[k].view(np.uint32), o[k].view(np.uint32)), k
    assert np.array_equal(g["octave"], o["octave"]) and np.array_equal(g["laplacian"], o["laplacian"])
