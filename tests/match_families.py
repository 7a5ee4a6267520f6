"""Seeded adversarial inputs for the stage between detection and the solver -- 2-NN matching (k_knn2, k_knn2_f32), the
Lowe-ratio / one-to-one / duplicate-coordinate filter (k_filter<false>, k_filter<true> + k_filter_dup + k_filter_out),
remove_double_matching over concatenated rows (k_merge_dup + k_merge) and the static-point filter (static_filter_block) --
and plain references that do not go through the oracle.  Shared by tests/test_oracle_match_edges.py (CPU) and
tests/test_gpu_match_edges.py (device).

The sizes come from the kernels' constants: MT_TILE = 512 train rows per LDS tile and 256 queries x 64 chunks per trip of
k_knn2; four waves over ranges of per = (nt + 3) >> 2 train rows and 64 queries per workgroup in k_knn2_f32; 256-wide
compaction chunks, the 8-way unrolled duplicate search, 5 * kcap * 4 bytes of LDS (opt-in above 48 KB: kcap >= 2458;
EVH_FILTER_LDS_MAX = 150 KB: the global-scratch form from kcap = 7681) and the 2048-row tile of k_filter_dup in the
filter; 1024-row tiles and 256-row workgroups in k_merge_dup; HB = 2048 histogram bins, 256 threads and 64-lane ballots in
static_filter_block.  Every generator is seeded and returns named cases; this file imports neither torch nor libevhip.
"""
import numpy as np

from evenvizion_amd.processing import matching, utils

OK, NO_DESCRIPTORS, FEW_MATCHES = 0, 1, 2
FLT_MAX = np.float32(3.4028234663852886e38)
MT_TILE = 512


# ---- plain references -----------------------------------------------------------------------------------------------------
def _sq_dist(q, t):
    """int64 [nq, nt] squared L2 distances of integer-valued rows (every product sum is far below 2^53: exact in float64)"""
    q = np.asarray(q, np.float64); t = np.asarray(t, np.float64)
    out = np.empty((len(q), len(t)), np.int64)
    qn = (q * q).sum(1); tn = (t * t).sum(1)
    for c0 in range(0, len(q), 2048):
        g = q[c0:c0 + 2048] @ t.T
        out[c0:c0 + 2048] = np.rint(qn[c0:c0 + 2048, None] + tn[None, :] - 2.0 * g).astype(np.int64)
    return out


def u8_dist(q, t, hamming=False):
    """int64 [nq, nt]: sum (q - t)^2 over the 32 bytes, or the number of differing bits"""
    q = np.asarray(q, np.uint8).reshape(-1, 32); t = np.asarray(t, np.uint8).reshape(-1, 32)
    if hamming:
        return _sq_dist(np.unpackbits(q, axis=1), np.unpackbits(t, axis=1))
    return _sq_dist(q, t)


def _best_two(key):
    """indices of the two smallest keys of every row, the lowest index first among equals; -1 where there is no such row"""
    nq, nt = key.shape
    idx = np.full((nq, 2), -1, np.int32)
    if nt:
        order = np.argsort(key, axis=1, kind="stable")[:, :2]
        idx[:, :order.shape[1]] = order
    return idx


def ref_knn2_u8(q, t, hamming=False):
    """BruteForce knnMatch(q, t, 2) on 32-byte rows -> (idx i32[nq,2], d u32[nq,2]); a missing neighbour is -1 / 0xFFFFFFFF"""
    D = u8_dist(q, t, hamming)
    idx = _best_two(D)
    d = np.full(idx.shape, 0xFFFFFFFF, np.uint32)
    for k in range(2):
        ok = idx[:, k] >= 0
        d[ok, k] = D[ok, idx[ok, k]].astype(np.uint32)
    return idx, d


def ref_knn2_f32_int(q, t):
    """The same on float32 rows with integer values 0..255 (dim 64 or 128): every partial sum is an integer below 2^24, so
    any float32 summation order is exact; distance = sqrt(float32(D)); neighbours are ordered by that float32 distance
    (two D above 2^22 can round to one distance and tie).  A missing neighbour is -1 / FLT_MAX."""
    D = _sq_dist(q, t)
    assert D.size == 0 or D.max() < (1 << 24)
    dist = np.sqrt(D.astype(np.float32))
    idx = _best_two(dist)
    d = np.full(idx.shape, FLT_MAX, np.float32)
    for k in range(2):
        ok = idx[:, k] >= 0
        d[ok, k] = dist[ok, idx[ok, k]]
    return idx, d, D


class DMatch:
    def __init__(self, q, t, d):
        self.queryIdx, self.trainIdx, self.distance = q, t, d


def ref_ratio_unique(idx, dist, ratio):
    """lowes_ratio_test + filter_corresponding_points on DMatch-like objects; dist: Python-float distances [nq,2]
    -> [(train, query), ...]"""
    raw = [[DMatch(i, int(t), float(d)) for t, d in zip(ti, di) if t >= 0] for i, (ti, di) in enumerate(zip(idx, dist))]
    return matching.lowes_ratio_test(raw, ratio)


def u8_distances(d2):
    """DMatch.distance of the integer form: sqrt(float32(D))"""
    return np.sqrt(np.asarray(d2, np.uint32).astype(np.float32)).astype(np.float64)


def ref_remove_double(rows):
    """utils.remove_double_matching on f32[n,4] rows -> f32[m,4]"""
    rows = np.asarray(rows, np.float32).reshape(-1, 4)
    a, b = utils.remove_double_matching(rows[:, :2], rows[:, 2:])
    if not a:
        return np.zeros((0, 4), np.float32)
    return np.ascontiguousarray(np.c_[np.array(a, np.float32), np.array(b, np.float32)], dtype=np.float32)


def ref_filter(idx, dist, xy_q, xy_t, ratio, min_matches):
    """What evh_ratio_unique_filter[_f32] computes (matching.py:104-119): -> (status, rows f32[m,4])"""
    empty = np.zeros((0, 4), np.float32)
    if len(idx) == 0 or len(xy_t) == 0:
        return NO_DESCRIPTORS, empty
    m = ref_ratio_unique(idx, dist, ratio)
    if len(m) < min_matches:
        return FEW_MATCHES, empty
    rows = np.array([np.r_[xy_q[q], xy_t[t]] for t, q in m], np.float32).reshape(-1, 4)
    return OK, ref_remove_double(rows)


def ref_static(H, rows):
    """find_point_displacement + get_largest_group_points -> (kept rows f32[m,4], groups dict)"""
    rows = np.asarray(rows, np.float32).reshape(-1, 4)
    g = utils.find_point_displacement(np.asarray(H, np.float64), rows[:, :2], rows[:, 2:])
    if len(rows) == 0:
        return rows.copy(), g
    a, b = utils.get_largest_group_points(g, rows[:, :2], rows[:, 2:])
    return np.ascontiguousarray(np.c_[a, b], dtype=np.float32), g


def bits(a):
    """float32 array as uint32: +0.0 and -0.0 differ, as the bit-for-bit comparisons need"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- K1: k_knn2 -----------------------------------------------------------------------------------------------------------
K1_NT = (1, 2, 3, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1537)
K1_NQ = (1, 63, 64, 65, 255, 256, 257, 1000)
# (position, code): the trains at these indices are B + 16 e_code; two positions with one code are exact copies, the second
# one in a later 512-row tile.  First and last rows of tiles, and both orders of every pair of codes.
_K1_SPECIAL = ((0, 0), (511, 1), (512, 2), (1023, 3), (1024, 4), (300, 5), (700, 6), (600, 0), (1100, 1), (1536, 2), (2, 7), (1, 8))


def _k1_low_entropy(rng, nq, nt):
    base = rng.choice(np.array([0, 255], np.uint8), (7, 32))
    t = base[rng.integers(0, 7, nt)]
    q = rng.choice(np.array([0, 255], np.uint8), (nq, 32))
    own = rng.random(nq) < 0.5                         # half the queries are one of the seven rows with a few bytes flipped
    q[own] = base[rng.integers(0, 7, int(own.sum()))]
    flip = (rng.random((nq, 32)) < 0.06) & own[:, None]
    q ^= (flip * 255).astype(np.uint8)
    return q, t


def _k1_planted(rng, nq, nt):
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    B = rng.integers(0, 200, 32, dtype=np.uint8)
    spec = [(p, c) for p, c in _K1_SPECIAL if p < nt]
    if nt - 1 not in [p for p, _ in spec]:
        spec.append((nt - 1, 9))                      # the last train row
    if nt >= 4 and nt - 2 not in [p for p, _ in spec]:
        spec.append((nt - 2, 8))                      # a copy of row 1 near the end, whatever the size
    codes = sorted(set(c for _, c in spec))
    for p, c in spec:
        t[p] = B; t[p, c] += 16
    pairs = [(a, b) for a in codes for b in codes if a != b] or [(codes[0], codes[0])]
    q = np.tile(B, (nq, 1))
    for i in range(nq):                               # best = the trains of code a (distance 64), second = code b (320)
        a, b = pairs[i % len(pairs)]
        q[i, a] += 16
        if b != a:
            q[i, b] += 8
    return q, t


def _k1_make(kind, rng, nq, nt):
    if kind == "a":
        return _k1_low_entropy(rng, nq, nt)
    if kind == "b":
        row = rng.integers(0, 256, 32, dtype=np.uint8)
        return np.tile(row, (nq, 1)), np.tile(row, (nt, 1))
    if kind == "c":
        return np.zeros((nq, 32), np.uint8), np.full((nt, 32), 255, np.uint8)
    return _k1_planted(rng, nq, nt)


def k1_cases():
    """K1 -> [(name, kind, q u8[nq,32], t u8[nt,32])]: every (nt, nq) of K1_NT x K1_NQ once, the kind a/b/c/d chosen so that
    every (nt, kind) and every (nq, kind) occurs; then nq = 16385 and 16384 + 256 + 1 at a small nt: the second trip of the
    query loop (grid.y is capped at 64 chunks of 256 queries)."""
    rng = np.random.default_rng(5101)
    out = []
    for i, nt in enumerate(K1_NT):
        for j, nq in enumerate(K1_NQ):
            kind = "abcd"[(i + j) % 4]
            q, t = _k1_make(kind, rng, nq, nt)
            out.append(("k1_%s_nq%d_nt%d" % (kind, nq, nt), kind, q, t))
    for kind, nq, nt in (("a", 16385, 5), ("d", 16384 + 256 + 1, 9)):
        q, t = _k1_make(kind, rng, nq, nt)
        out.append(("k1_%s_nq%d_nt%d" % (kind, nq, nt), kind, q, t))
    return out


def tie_stats(D, idx, group=None):
    """From a distance matrix and the reference's answer: (queries with a tie for first or second place, queries whose
    best two lie in different groups, queries whose tied candidates lie in different groups); group maps a train index to
    its tile / range."""
    nq, nt = D.shape
    if nt < 2:
        return 0, 0, 0
    s = np.sort(D, axis=1)
    tie1 = s[:, 0] == s[:, 1]
    tie2 = (s[:, 1] == s[:, 2]) if nt > 2 else np.zeros(nq, bool)
    ties = int((tie1 | tie2).sum())
    if group is None:
        return ties, 0, 0
    g = np.asarray(group)
    cross = int((g[idx[:, 0]] != g[idx[:, 1]]).sum())
    d1 = D[np.arange(nq), idx[:, 1]]
    cand = D == d1[:, None]                            # every train as far away as the second neighbour
    other = (cand & (g[None, :] != g[idx[:, 1]][:, None])).any(1)
    tied_cross = int(((tie1 & (g[idx[:, 0]] != g[idx[:, 1]])) | (tie2 & other)).sum())
    return ties, cross, tied_cross


# ---- K2: k_knn2_f32 -------------------------------------------------------------------------------------------------------
K2_NT = (1, 2, 3, 4, 5, 6, 7, 8, 9, 31, 32, 33, 64, 65, 411)
K2_NQ = (1, 63, 64, 65, 130)


def _k2_planted(rng, nq, nt, dim):
    """The same train row in two different waves' ranges (j // per differs), a copy in the last wave's short range
    included; queries one step away from such a row (tie for first place) or equal to a unique row three steps away from
    it (tie for second place)."""
    per = (nt + 3) >> 2
    t = rng.integers(3, 250, (nt, dim)).astype(np.float32)
    cands = [(0, nt - 1), (per - 1, per), (per, nt - 1), (0, per), (2 * per - 1, 2 * per), (1, 3 * per), (per + 1, 2 * per + 1),
             (2 * per, nt - 2)]
    used, groups = set(), []
    for j1, j2 in cands:
        if 0 <= j1 < j2 < nt and j1 // per != j2 // per and j1 not in used and j2 not in used:
            used.update((j1, j2))
            t[j2] = t[j1]
            u = next((k for k in range(nt - 1, -1, -1) if k not in used), None) if len(groups) % 2 else None
            if u is not None:
                used.add(u)
                t[u] = t[j1]; t[u, 1:4] += 1.0          # squared distance 3 to both copies
            groups.append((j1, u))
    q = rng.integers(3, 250, (nq, dim)).astype(np.float32)
    for i in range(nq):
        if not groups:
            break
        j1, u = groups[i % len(groups)]
        if u is not None and (i // len(groups)) % 2:
            q[i] = t[u]
        else:
            q[i] = t[j1]; q[i, 0] += 1.0
    return q, t


def k2_cases():
    """K2 -> [(name, kind, q f32[nq,dim], t f32[nt,dim])]: every (nt, nq) once, dim 64 / 128 and the kind alternating.
    Kinds: 'int' integer values 0..255, 'low' integer values 0..3 (many equal distances), 'tie' planted ties across the
    waves' ranges -- all three against the exact reference -- and 'frac' (rng.random - 0.5, where the summation order
    matters: oracle only)."""
    rng = np.random.default_rng(5202)
    out = []
    kinds = ("int", "tie", "frac", "low")
    for i, nt in enumerate(K2_NT):
        for j, nq in enumerate(K2_NQ):
            dim = (64, 128)[(i + j // 2) % 2]
            kind = kinds[(i + j) % 4]
            if kind == "int":
                q = rng.integers(0, 256, (nq, dim)).astype(np.float32); t = rng.integers(0, 256, (nt, dim)).astype(np.float32)
            elif kind == "low":
                q = rng.integers(0, 4, (nq, dim)).astype(np.float32); t = rng.integers(0, 4, (nt, dim)).astype(np.float32)
            elif kind == "frac":
                q = (rng.random((nq, dim)) - 0.5).astype(np.float32); t = (rng.random((nt, dim)) - 0.5).astype(np.float32)
            else:
                q, t = _k2_planted(rng, nq, nt, dim)
            out.append(("k2_%s_d%d_nq%d_nt%d" % (kind, dim, nq, nt), kind, q, t))
    for dim in (64, 128):                              # every shape of the planted kind at both widths where ranges are uneven
        for nt in (2, 3, 5, 6, 7, 9, 33, 411):
            q, t = _k2_planted(rng, 130, nt, dim)
            out.append(("k2_tie_d%d_nq130_nt%d" % (dim, nt), "tie", q, t))
    return out


# ---- the filter's inputs ---------------------------------------------------------------------------------------------------
def _coords(n, seed):
    """n distinct exactly representable points"""
    i = np.arange(n, dtype=np.float64)
    return np.ascontiguousarray(np.c_[i * 0.5 + seed, (i * 7 % 1013) * 0.25 + (i // 1013) * 300 + seed], dtype=np.float32)


def dup_keys(m, seed=1.0):
    """f32[m,2] keys with planted duplicates: a key of multiplicity 50 spread over the whole range, pairs that are
    adjacent, 256, 1024 and 2000 rows apart, pairs across row 2047 | 2048, a key whose only other occurrence is the very
    last row, +0.0 / -0.0 as one key (rows 0 and m // 2, with the signs swapped), and rows that share x but not y."""
    xy = _coords(m, seed)
    used = set()

    def plant(pos):
        pos = [p for p in pos if 0 <= p < m]
        if len(pos) < 2 or len(set(pos)) != len(pos) or used & set(pos):
            return
        used.update(pos)
        xy[pos[1:]] = xy[pos[0]]

    if m >= 2:
        used.update((0, m // 2))
        xy[0] = (0.0, -0.0); xy[m // 2] = (-0.0, 0.0)
    plant([5, m - 1])
    k = min(50, m // 4)
    plant(sorted(set(np.linspace(3, m - 3, k).astype(int).tolist())) if k >= 2 else [])
    for pos in ([1, 2], [9, 9 + 256], [17, 17 + 1024], [100, 2100], [2047, 2048], [2040, 2055], [255, 256], [1023, 1024],
                [m - 3, m - 2]):
        plant(pos)
    for p in range(20, m - 1, 97):                     # same x, other y: not a duplicate
        if p not in used and p + 1 not in used:
            xy[p + 1, 0] = xy[p, 0]
    return xy


def filter_case(rng, m, nt, doubles=2, big_claim=300, fails=200, dup=False, f32=False):
    """One filter input with exactly m survivors of the ratio test + one-to-one filter: m queries claim a train of their
    own, `doubles` pairs of queries claim one train each twice, big_claim queries one train, `fails` queries fail the ratio
    test while pointing at claimed and unclaimed trains; the roles are shuffled over the query order.  nt - (claimed) trains
    are never claimed.  dup: the a coordinates of the survivors, by rank, are dup_keys(m).
    -> dict(idx, d2 | dist, xy_q, xy_t, m)"""
    nq = m + 2 * doubles + big_claim + fails
    need = m + doubles + (1 if big_claim else 0)
    assert nt >= need + 1
    trains = rng.permutation(nt)[:need + 1]
    role = np.r_[np.zeros(m, int), np.ones(2 * doubles, int), np.full(big_claim, 2), np.full(fails, 3)]
    role = role[rng.permutation(nq)] if nq else role
    idx = np.zeros((nq, 2), np.int32)
    d0 = rng.integers(1, 1000, nq).astype(np.int64)
    d1 = 4 * d0 + 50                                   # passes the ratio 0.5 with a wide margin
    surv = np.flatnonzero(role == 0)
    idx[surv, 0] = trains[:m]
    dbl = np.flatnonzero(role == 1)
    idx[dbl, 0] = np.repeat(trains[m:m + doubles], 2)[rng.permutation(2 * doubles)] if doubles else 0
    idx[role == 2, 0] = trains[m + doubles] if big_claim else 0
    fl = np.flatnonzero(role == 3)
    idx[fl, 0] = rng.integers(0, nt, len(fl))
    d1[fl] = d0[fl] + rng.integers(0, 3, len(fl))
    idx[:, 1] = (idx[:, 0] + 1 + rng.integers(0, max(nt - 1, 1), nq)) % nt if nt > 1 else -1
    xy_q = _coords(nq, 3.0)
    if dup:
        xy_q[surv] = dup_keys(m, 2000.0)
    out = dict(idx=idx, xy_q=xy_q, xy_t=_coords(nt, 7.0) + np.float32(5000), m=m, ratio=0.5)
    d2 = np.ascontiguousarray(np.c_[d0, d1], dtype=np.uint32)
    if f32:
        out["dist"] = np.sqrt(d2.astype(np.float32))
    else:
        out["d2"] = d2
    return out


def f1_cases():
    """F1 ratio boundary, integer form -> [(name, case)]: rows with D1 = 4 D0 and 4 D0 +- 1 (ratio 0.5), D1 = (100 / 49) D0
    +- 1 (0.7), (16 / 9) D0 +- 1 (0.75), D0 = D1 = 0, D0 = 0 < D1, a missing second neighbour and a missing first one; every
    query claims a train of its own, so the ratio test alone decides.  One case per ratio in {0.5, 0.7, 0.75}."""
    rows = []
    for k in list(range(1, 40)) + [100, 255, 721, 1020, 1442]:
        for dd in (-1, 0, 1):
            rows.append((k * k, 4 * k * k + dd))
            rows.append((49 * k * k, 100 * k * k + dd))
            rows.append((9 * k * k, 16 * k * k + dd))
            rows.append((k, 4 * k + dd))
    rows += [(0, 0), (0, 1), (0, 2080800), (2080800, 2080800), (520200, 2080800), (520199, 2080800), (1, 3), (1, 4), (1, 5)]
    n = len(rows) + 6
    d2 = np.zeros((n, 2), np.uint32); d2[:len(rows)] = rows
    d2[len(rows):] = (1, 400)                          # pass on distance; four of them lack a neighbour
    idx = np.c_[np.arange(n), (np.arange(n) + 1) % n].astype(np.int32)
    idx[len(rows), 1] = -1; idx[len(rows) + 1, 0] = -1; idx[len(rows) + 2] = -1; idx[len(rows) + 3, 1] = -1
    out = []
    for ratio in (0.5, 0.7, 0.75):
        out.append(("f1_ratio%g" % ratio, dict(idx=idx, d2=d2, xy_q=_coords(n, 3.0), xy_t=_coords(n, 9000.0), ratio=ratio)))
    return out


def f1_cases_f32():
    """F1, float form: distances 0, denormals, FLT_MAX and its half, x against 2 x / x / 0.7 / x / 0.75 one ulp either
    side; dist1 * ratio is finite in double for all of them."""
    f = np.float32
    one = [f(0), f(1e-45), f(3e-45), f(1e-40), f(1.1754942e-38), f(1.17549435e-38), f(1), f(3), f(1000.5), f(1442.4978),
           f(1e30), FLT_MAX / f(2), FLT_MAX]
    rows = []
    for x in one:
        for y in one:
            rows.append((x, y))
        for r in (0.5, 0.7, 0.75):
            with np.errstate(over="ignore"):
                y = f(np.float64(x) / r)
            if np.isfinite(y):
                for yy in (np.nextafter(y, f(0)), y, np.nextafter(y, FLT_MAX)):
                    rows.append((x, yy))
    n = len(rows) + 3
    dist = np.ones((n, 2), np.float32); dist[:len(rows)] = rows
    dist[len(rows):] = (1, 20)
    idx = np.c_[np.arange(n), (np.arange(n) + 1) % n].astype(np.int32)
    idx[len(rows), 1] = -1; idx[len(rows) + 1, 0] = -1
    out = []
    for ratio in (0.5, 0.7, 0.75):
        out.append(("f1f_ratio%g" % ratio, dict(idx=idx, dist=dist, xy_q=_coords(n, 3.0), xy_t=_coords(n, 9000.0), ratio=ratio)))
    return out


def f2_cases():
    """F2 claims -> [(name, case, min_matches)]: trains claimed 0, 1, 2 and 300 times; exactly m survivors for m in
    {min_matches - 1, min_matches, 255, 256, 257, 511, 513} (the 256-wide compaction chunks of k_filter) with min_matches
    in {4, 1, 0}; each once with nq >> nt and once with nt >> nq (kcap = max(nq, nt))."""
    rng = np.random.default_rng(5303)
    out = []
    for m, mm in ((3, 4), (4, 4), (0, 1), (1, 1), (0, 0), (255, 4), (256, 4), (257, 4), (511, 4), (513, 4)):
        for shape in ("q", "t"):
            if shape == "q":
                c = filter_case(rng, m, nt=m + 12, doubles=2, big_claim=300, fails=4000)
            else:
                c = filter_case(rng, m, nt=6000, doubles=2, big_claim=300, fails=20)
            out.append(("f2_m%d_min%d_n%s" % (m, mm, shape), c, mm))
    return out


def f3_cases():
    """F3 duplicate coordinates among the survivors -> [(name, case)]: m mod 8 in {0, 1, 7} (the 8-way unrolled search and
    its remainder), keys of multiplicity 1, 2 and 50, first and last occurrence in different 256-chunks, a key whose only
    other occurrence is the last survivor, signed zeros; integer and float form."""
    rng = np.random.default_rng(5404)
    out = []
    for m in (600, 601, 607, 9, 15, 16):
        for f32 in (False, True):
            c = filter_case(rng, m, nt=m + 40, doubles=3, big_claim=30, fails=50, dup=True, f32=f32)
            out.append(("f3_m%d_%s" % (m, "f32" if f32 else "u8"), c))
    return out


F4_KCAPS = (2457, 2458, 7680, 7681, 65535)
F4_REFUSED = 65536


def f4_case():
    """F4 form boundaries: ONE logical input -- 2300 survivors (more than the 2048-row tile of k_filter_dup, with duplicate
    keys on both sides of row 2047 | 2048) among 2450 queries, claims on trains below 2457 -- to be presented with nt
    padded by never-claimed train rows to kcap = 2457 (default dynamic LDS), 2458 (the opt-in above 48 KB), 7680 (the last
    LDS size), 7681 (the first global-scratch size) and 65535 (the largest); 65536 must be refused.
    -> (case with nt = 2457, pad(nt) -> xy_t of that size)"""
    rng = np.random.default_rng(5505)
    c = filter_case(rng, 2300, nt=2457, doubles=10, big_claim=60, fails=70, dup=True)

    def pad(nt):
        xy = np.empty((nt, 2), np.float32)
        xy[:2457] = c["xy_t"]
        xy[2457:] = _coords(nt - 2457, 123.0) + np.float32(20000)
        return xy
    return c, pad


def f4_case_three_tiles():
    """F4, a second logical input: 4203 survivors -- three 2048-row tiles of k_filter_dup, the last of 107 rows (13 x 8 + 3:
    the remainder loop) -- among 4353 queries, claims on trains below 4300; two keys of dup_keys(4203) have occurrences in
    all three tiles (rows 3 .. 4200, 50 of them, and rows 5 and 4202), so `first` and `last` are carried across tiles.
    Presented at kcap 7680 (the last LDS size) and 7681 (the first global-scratch size) by the same padding.
    -> (case with nt = 4300, pad(nt) -> xy_t of that size)"""
    c = filter_case(np.random.default_rng(5606), 4203, nt=4300, doubles=10, big_claim=60, fails=70, dup=True)

    def pad(nt):
        xy = np.empty((nt, 2), np.float32)
        xy[:4300] = c["xy_t"]
        xy[4300:] = _coords(nt - 4300, 123.0) + np.float32(20000)
        return xy
    return c, pad


F4_THREE_TILES_KCAPS = (7680, 7681)


# ---- D1: remove_double_matching over concatenated rows -----------------------------------------------------------------
D1_N = (0, 1, 255, 256, 257, 1023, 1024, 1025, 15000)


def d1_cases():
    """D1 -> [(name, rows f32[n,4])]: dup_keys over n rows (first and last occurrence in different 1024-row tiles and
    different 256-row workgroups of k_merge_dup, the last occurrence in the final row, signed zeros), b distinct per row
    so that the row a key's b came from is identified."""
    out = []
    for n in D1_N:
        rows = np.zeros((n, 4), np.float32)
        if n:
            rows[:, :2] = dup_keys(n, 40.0) if n > 1 else _coords(1, 40.0)
            rows[:, 2:] = _coords(n, 11.0) + np.float32(30000)
        out.append(("d1_n%d" % n, rows))
    return out


# ---- S1-S4: the static filter --------------------------------------------------------------------------------------------
EYE = np.eye(3)
S1_N = (1, 7, 63, 64, 65, 255, 256, 257, 1000, 4000)
S4_H = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-1.0 / 200.0, 0.0, 1.0]])


def _rows_with_disp(disp_xy, seed=10.0):
    """rows whose a points are distinct exact points and b = a + displacement (exact in float32 for the values used)"""
    d = np.asarray(disp_xy, np.float64).reshape(-1, 2)
    a = _coords(len(d), seed).astype(np.float64)
    rows = np.ascontiguousarray(np.c_[a, a + d], dtype=np.float32)
    assert np.array_equal(rows[:, 2:].astype(np.float64), a + d)
    return rows


def s1_cases():
    """S1 half-integer displacements: exactly k + 0.5, axis-aligned and as 3-4-5 multiples (1.5 s, 2 s) with s odd; Python's
    round sends half to even (0.5 -> 0, 1.5 -> 2, 2.5 -> 2), so bins pair up differently than under half-up; n across the
    64-lane ballot chunks and the 256-thread strides."""
    out = []
    for n in S1_N:
        i = np.arange(n)
        k = np.array([0, 1, 2, 3, 4, 1, 2, 7, 8, 2])[i % 10]
        d = np.zeros((n, 2))
        ax = (i // 10) % 3
        d[ax == 0, 0] = k[ax == 0] + 0.5
        d[ax == 1, 1] = -(k[ax == 1] + 0.5)
        s = 2 * k[ax == 2] + 1                          # 2.5 s = 5 k + 2.5
        d[ax == 2] = np.c_[1.5 * s, 2.0 * s]
        out.append(("s1_n%d" % n, EYE, _rows_with_disp(d)))
    return out


def _tie_rows(prefix, bins, pop, tail=0):
    """`prefix` rows in bins of one (displacements 100, 101, ...), then `pop` rows of each of `bins` interleaved
    (displacements 3, 5, 7), then `tail` more singletons"""
    d = [100 + i for i in range(prefix)]
    for _ in range(pop):
        d += [3 + 2 * b for b in range(bins)]
    d += [400 + i for i in range(tail)]
    return _rows_with_disp(np.c_[np.array(d, np.float64), np.zeros(len(d))])


def s2_cases():
    """S2 equal populations: two and three bins of the same size, interleaved; the winner is the bin whose first member
    comes first -- at row 0, at row 63 (the last lane of the first ballot chunk) / 64, and at row 200 / 250 (the last
    wave's stride of the 256 threads)."""
    out = []
    for bins in (2, 3):
        for prefix in (0, 63, 64, 200, 250):
            out.append(("s2_b%d_first%d" % (bins, prefix), EYE, _tie_rows(prefix, bins, 40, tail=9)))
    rows = _tie_rows(0, 2, 130)                          # the tie over more than one 256-thread stride
    out.append(("s2_long", EYE, rows))
    return out


def s3_cases():
    """S3 displacements at and beyond HB = 2048 bins (the quadratic path): 2047 stays in the histogram, 2048 leaves it."""
    z = lambda d: np.c_[np.asarray(d, np.float64), np.zeros(len(d))]
    out = []
    out.append(("s3_max2047", EYE, _rows_with_disp(z([2047] * 5 + [3] * 4 + [2046] * 5 + [2047]))))
    out.append(("s3_one2048", EYE, _rows_with_disp(z([3] * 4 + [2048] + [2047] * 6 + [5] * 6))))
    out.append(("s3_2048_wins", EYE, _rows_with_disp(z([2047] * 5 + [2048] * 6 + [2047.5] * 3))))
    out.append(("s3_all_big", EYE, _rows_with_disp(z([3000, 5000, 3000, 5000, 5000, 4000] * 50 + [3000] * 7))))
    out.append(("s3_one_big_among_small", EYE, _rows_with_disp(z([4] * 300 + [5000] + [6] * 299 + [4] * 5))))
    d = [2500 + i for i in range(70)]                  # singletons first, then an equal-population tie inside the big path
    for _ in range(30):
        d += [3000, 7, 5000]
    out.append(("s3_big_tie", EYE, _rows_with_disp(z(d))))
    d = [5000, 3000] * 300 + [2048.5] * 100
    out.append(("s3_big_tie_from_row0", EYE, _rows_with_disp(z(d))))
    return out


def s4_cases():
    """S4 the horizon: H = I with H[2,0] = -1/200 sends x = 200 to infinity; rows at x = 200 +- 2^-k have tw = -+2^-k / 200
    and finite displacements of about 40000 * 2^k * |(x, y)| / 200 -- above 2^31 for k = 16 (float32 resolves 2^-16 next to
    200), each in a bin of its own in the reference.  A bin of two ordinary rows (x = 0: tw = 1) follows them and is the
    reference's largest group; a device that folds the huge displacements into one saturated bin picks that one instead."""
    rows = []
    for k in (16, 15, 14, 12, 10):
        for sgn in (1.0, -1.0):
            for y in (0.0, 50.0, 100.0, 150.0, 225.0):
                rows.append((200.0 + sgn * 2.0 ** -k, y, 7.0, 3.0))
    rows += [(0.0, 10.0, 3.0, 14.0), (0.0, 20.0, 4.0, 23.0)]     # displacement 5, twice
    rows += [(0.0, 30.0, 0.0, 41.0)]
    return [("s4_horizon", S4_H, np.array(rows, np.float32))]


def static_cases():
    return s1_cases() + s2_cases() + s3_cases() + s4_cases()


# ---- the chained stage ------------------------------------------------------------------------------------------------------
CHAIN_H = np.array([[1.0, 0.0, 4990.0], [0.0, 1.0, 5003.5], [0.0, 0.0, 1.0]])


def chain_case():
    """Descriptors whose 2-NN output makes a meaningful filter input: most queries are a train row with a few bytes moved
    (ratio passes), some trains are wanted by two queries, some queries are far from everything; a coordinates repeat."""
    rng = np.random.default_rng(5606)
    nq, nt = 1500, 1400
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    src = rng.integers(0, nt, nq)
    src[:1100] = rng.permutation(nt)[:1100]
    q = t[src].copy()
    noise = rng.integers(0, 6, (nq, 32), dtype=np.uint8)
    q = np.where(q < 250, q + noise, q).astype(np.uint8)
    far = rng.random(nq) < 0.1
    q[far] = rng.integers(0, 256, (int(far.sum()), 32), dtype=np.uint8)
    xy_t = _coords(nt, 7.0) + np.float32(5000)
    # a = its train's b moved back by CHAIN_H's translation, up to 3 px off: the static filter has groups to choose from
    xy_q = (xy_t[src] - CHAIN_H[:2, 2].astype(np.float32) + rng.integers(0, 4, (nq, 2)).astype(np.float32)).astype(np.float32)
    xy_q[::37] = xy_q[5]
    return q, t, xy_q, xy_t
