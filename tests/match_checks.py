"""The oracle's side of the match-stage tests: the filter and the static filter composed from the oracle's parts, and the
bit-for-bit row comparison.  Shared by tests/test_oracle_match_edges.py and tests/test_gpu_match_edges.py
(tests/match_families.py itself does not import the oracle)."""
import numpy as np

import match_families as F
from oracle import oracle as O


def oracle_filter(idx, d, xy_q, xy_t, ratio, min_matches, f32=False):
    """evh_ratio_unique_filter[_f32] composed from the oracle's parts, as evo_match_static composes them"""
    empty = np.zeros((0, 4), np.float32)
    if len(idx) == 0 or len(xy_t) == 0:
        return F.NO_DESCRIPTORS, empty
    oq, ot = (O.ratio_unique_f32 if f32 else O.ratio_unique)(idx, d, ratio)
    if len(oq) < min_matches:
        return F.FEW_MATCHES, empty
    if len(oq) == 0:
        return F.OK, empty
    a, b = O.remove_double(xy_q[oq], xy_t[ot])
    return F.OK, np.ascontiguousarray(np.c_[a, b], dtype=np.float32)


def oracle_static(H, rows):
    if len(rows) == 0:
        return np.zeros((0, 4), np.float32)
    a, b = O.static_filter(H, rows[:, :2], rows[:, 2:])
    return np.ascontiguousarray(np.c_[a, b], dtype=np.float32)


def same_rows(got, want):
    return got.shape == want.shape and np.array_equal(F.bits(got), F.bits(want))
