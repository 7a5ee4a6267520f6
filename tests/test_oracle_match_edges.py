"""The oracle's matchers and match filters on the adversarial families of tests/match_families.py, against plain references
that do not go through the oracle (int64 distances with a stable argsort, the pure-Python lowes_ratio_test /
filter_corresponding_points / remove_double_matching / find_point_displacement / get_largest_group_points), bit for bit.
Runs without a GPU: this is what makes the oracle a legitimate checker for tests/test_gpu_match_edges.py, and the
conditions a family must meet (how many ties, across which tiles) are asserted here on the reference alone."""
import numpy as np
import pytest

import match_families as F
from match_checks import oracle_filter, oracle_static, same_rows
from oracle import oracle as O

K1 = F.k1_cases()
K2 = F.k2_cases()


def check_filter(c, min_matches, tag):
    f32 = "dist" in c
    d = c["dist"] if f32 else c["d2"]
    dist = c["dist"].astype(np.float64) if f32 else F.u8_distances(c["d2"])
    st_r, rows_r = F.ref_filter(c["idx"], dist, c["xy_q"], c["xy_t"], c["ratio"], min_matches)
    st_o, rows_o = oracle_filter(c["idx"], d, c["xy_q"], c["xy_t"], c["ratio"], min_matches, f32)
    assert st_o == st_r and same_rows(rows_o, rows_r), (tag, st_o, st_r, len(rows_o), len(rows_r))
    return st_r, rows_r


# ---- K1 / K2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hamming", [False, True], ids=["l2", "hamming"])
def test_k1_oracle_knn2_against_int64_reference(hamming):
    ties = {}                                          # (kind, second query trip) -> [tied queries, queries]
    cross_d = 0
    for name, kind, q, t in K1:
        idx_r, d_r = F.ref_knn2_u8(q, t, hamming)
        idx_o, d_o = O.knn2(q, t, hamming)
        assert np.array_equal(idx_o, idx_r) and np.array_equal(d_o, d_r), (name, np.flatnonzero((idx_o != idx_r).any(1))[:8])
        if kind == "b" and len(t) > 1:
            assert (idx_r == (0, 1)).all() and (d_r == 0).all(), name
        if kind == "c" and len(t) > 1:
            assert (idx_r == (0, 1)).all() and (d_r == (256 if hamming else 2080800)).all(), name
        if kind in "ad":
            n_tie, cross, _ = F.tie_stats(F.u8_dist(q, t, hamming), idx_r, np.arange(len(t)) // F.MT_TILE)
            acc = ties.setdefault((kind, len(q) > 16384), [0, 0])
            acc[0] += n_tie; acc[1] += len(q)
            if kind == "d":
                cross_d += cross
    print("K1 %s: tied queries (kind, second trip) -> [tied, all] %s; kind d best two in different tiles: %d"
          % ("hamming" if hamming else "l2", ties, cross_d))
    assert len(ties) == 4
    for key, (n_tie, n) in ties.items():              # the family's condition, from the reference alone: it holds for the
        assert 4 * n_tie >= n, (key, n_tie, n)        # swept sizes and for the two 16 k-query cases separately
    assert cross_d >= 32


def test_k1_covers_every_pair_of_sizes_and_the_second_query_trip():
    seen = set((len(q), len(t)) for _, _, q, t in K1)
    assert all((nq, nt) in seen for nq in F.K1_NQ for nt in F.K1_NT)
    assert sum(len(q) > 16384 for _, _, q, _ in K1) >= 2 and (16385, 5) in seen and (16384 + 256 + 1, 9) in seen
    for kind in "abcd":
        assert set(len(t) for _, k, _, t in K1 if k == kind) >= set(F.K1_NT)
        assert set(len(q) for _, k, q, _ in K1 if k == kind) >= set(F.K1_NQ)


def test_k2_oracle_knn2_f32_against_exact_reference():
    tied_cross = tied_last = 0
    for name, kind, q, t in K2:
        idx_o, d_o = O.knn2_f32(q, t)
        assert np.isfinite(q).all() and np.isfinite(t).all()
        if kind == "frac":                            # the summation order matters: the oracle is the only checker
            continue
        idx_r, d_r, D = F.ref_knn2_f32_int(q, t)
        assert np.array_equal(idx_o, idx_r) and np.array_equal(F.bits(d_o), F.bits(d_r)), (name, np.flatnonzero((idx_o != idx_r).any(1))[:8])
        if kind == "tie":
            per = (len(t) + 3) >> 2
            tied_cross += F.tie_stats(D, idx_r, np.arange(len(t)) // per)[2]
            if len(t) > 3 * per and len(t) - 3 * per < per:         # the last wave's range is short
                d1 = D[np.arange(len(q)), idx_r[:, 1]]
                cand = D == d1[:, None]                # every train as far away as the second neighbour
                tied_last += int((cand[:, 3 * per:].any(1) & cand[:, :3 * per].any(1)).sum())
    print("K2: queries whose tied candidates lie in different waves' ranges: %d; one of them in the last wave's short "
          "range: %d" % (tied_cross, tied_last))
    assert tied_cross >= 32 and tied_last >= 32
    seen = set((len(q), len(t)) for _, _, q, t in K2)
    assert all((nq, nt) in seen for nq in F.K2_NQ for nt in F.K2_NT)
    assert set(q.shape[1] for _, _, q, _ in K2) == {64, 128}


# ---- F1 - F4 ---------------------------------------------------------------------------------------------------------------
def test_f1_ratio_boundary_both_forms():
    for name, c in F.f1_cases() + F.f1_cases_f32():
        st, rows = check_filter(c, 4, name)
        assert st == F.OK
        d = c["dist"].astype(np.float64) if "dist" in c else F.u8_distances(c["d2"])
        both = (c["idx"] >= 0).all(1)
        passed = both & (d[:, 0] < d[:, 1] * c["ratio"])
        assert len(rows) == passed.sum() and 0 < passed.sum() < both.sum(), name
        assert np.isfinite(d[:, 1] * c["ratio"]).all()
    c = F.f1_cases()[0][1]
    D0, D1 = c["d2"][:, 0].astype(np.int64), c["d2"][:, 1].astype(np.int64)
    assert (D1 == 4 * D0).sum() > 40 and (D1 == 4 * D0 + 1).sum() > 40 and (D1 == 4 * D0 - 1).sum() > 40
    assert ((D0 == 0) & (D1 == 0)).any() and ((D0 == 0) & (D1 > 0)).any()
    assert (c["idx"][:, 1] < 0).any() and (c["idx"][:, 0] < 0).any()
    dist = F.f1_cases_f32()[0][1]["dist"]
    assert (dist == 0).any() and ((dist > 0) & (dist < 1.1754944e-38)).any() and (dist == F.FLT_MAX).any()


def test_f2_claims_and_exact_survivor_counts():
    seen = set()
    for name, c, mm in F.f2_cases():
        st, rows = check_filter(c, mm, name)
        m = len(F.ref_ratio_unique(c["idx"], F.u8_distances(c["d2"]), 0.5))
        assert m == c["m"], (name, m)
        assert st == (F.FEW_MATCHES if m < mm else F.OK) and len(rows) == (0 if m < mm else m), (name, st, len(rows))
        claims = np.bincount(c["idx"][(F.u8_distances(c["d2"])[:, 0] < F.u8_distances(c["d2"])[:, 1] * 0.5), 0],
                             minlength=len(c["xy_t"]))
        assert {0, 2, 300} <= set(claims.tolist()) and (m == 0 or 1 in claims)
        seen.add((m, mm, len(c["idx"]) > len(c["xy_t"])))
    for m, mm in ((3, 4), (4, 4), (0, 1), (1, 1), (0, 0), (255, 4), (256, 4), (257, 4), (511, 4), (513, 4)):
        assert (m, mm, True) in seen and (m, mm, False) in seen


def test_f3_duplicate_coordinates_among_survivors():
    for name, c in F.f3_cases():
        st, rows = check_filter(c, 4, name)
        assert st == F.OK and len(rows) < c["m"]
        if c["m"] >= 600:
            keys = F.dup_keys(c["m"], 2000.0)
            _, inv, cnt = np.unique(keys + np.float32(0), axis=0, return_inverse=True, return_counts=True)
            assert {1, 2} <= set(cnt.tolist()) and cnt.max() == 50
            inv = np.asarray(inv).reshape(-1)
            last = inv[-1]                             # the key of the very last survivor occurs exactly once before
            assert cnt[last] == 2
            first_of = {}
            far = 0
            for i, k in enumerate(inv):
                first_of.setdefault(k, i)
                far += (i // 256 != first_of[k] // 256)
            assert far >= 10
            assert np.signbit(rows[0, 1]) and not np.signbit(rows[0, 0])      # the first occurrence's bits: (+0.0, -0.0)
    assert set(c["m"] % 8 for _, c in F.f3_cases()) >= {0, 1, 7}


def test_f4_one_logical_input_at_every_form_boundary():
    c, pad = F.f4_case()
    assert len(c["idx"]) <= min(F.F4_KCAPS) and c["idx"].max() < 2457
    want = None
    for kcap in F.F4_KCAPS:
        cc = dict(c, xy_t=pad(kcap))
        st, rows = check_filter(cc, 4, "f4_kcap%d" % kcap)
        assert st == F.OK
        if want is None:
            want = rows
        assert same_rows(rows, want)
    m = c["m"]
    assert m > 2048 and 5 * 2457 * 4 <= 48 * 1024 < 5 * 2458 * 4 and 5 * 7680 * 4 <= 150 * 1024 < 5 * 7681 * 4
    keys = F.dup_keys(m, 2000.0)
    assert np.array_equal(keys[2047], keys[2048]) and np.array_equal(keys[100], keys[2100]) and np.array_equal(keys[2040], keys[2055])
    assert len(want) < m


# ---- D1 ----------------------------------------------------------------------------------------------------------------------
def test_d1_remove_double_over_concatenated_rows():
    for name, rows in F.d1_cases():
        want = F.ref_remove_double(rows)
        if len(rows):
            a, b = O.remove_double(rows[:, :2], rows[:, 2:])
            got = np.ascontiguousarray(np.c_[a, b], dtype=np.float32)
        else:
            got = np.zeros((0, 4), np.float32)
        assert same_rows(got, want), name
        n = len(rows)
        if n >= 255:
            assert len(want) < n
            last = np.flatnonzero((rows[:, :2] == rows[-1, :2]).all(1))
            assert len(last) == 2 and last[0] == 5      # the final row is the last occurrence of row 5's key
            k, = np.flatnonzero((want[:, :2] == rows[5, :2]).all(1))
            assert np.array_equal(want[k, 2:], rows[-1, 2:])
            assert np.signbit(want[0, 1]) and not np.signbit(want[0, 0])
            assert np.array_equal(want[0, 2:], rows[n // 2, 2:])
        if n == 15000:
            _, cnt = np.unique(rows[:, :2] + np.float32(0), axis=0, return_counts=True)
            assert cnt.max() == 50
            assert np.array_equal(rows[17, :2], rows[17 + 1024, :2]) and np.array_equal(rows[9, :2], rows[9 + 256, :2])
    assert [len(r) for _, r in F.d1_cases()] == list(F.D1_N)


# ---- S1 - S4 -----------------------------------------------------------------------------------------------------------------
STATIC = F.static_cases()


@pytest.mark.parametrize("name,H,rows", STATIC, ids=[s[0] for s in STATIC])
def test_static_filter_oracle_against_python_reference(name, H, rows):
    want, groups = F.ref_static(H, rows)
    got = oracle_static(H, rows)
    assert same_rows(got, want), (name, len(got), len(want))
    keys = list(groups)
    if name.startswith("s1"):
        a = rows[:, :2].astype(np.float64); b = rows[:, 2:].astype(np.float64)
        disp = np.sqrt(((a - b) ** 2).sum(1))
        assert (disp % 1.0 == 0.5).all()
        assert all(k % 2 == 0 for k in keys)           # half to even: every bin is even, 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
        assert 0 in keys and (len(rows) < 7 or 2 in keys)
    if name.startswith("s2"):
        pops = sorted((len(v) for v in groups.values()), reverse=True)
        assert pops[0] == pops[1] and len(want) == pops[0]
        first = int(name.split("first")[1]) if "first" in name else 0
        assert np.array_equal(want[0], rows[first])
    if name.startswith("s3"):
        assert (max(keys) >= 2048) == (name != "s3_max2047")
        assert 2047 in keys if name in ("s3_max2047", "s3_one2048", "s3_2048_wins") else True
    if name in ("s3_big_tie", "s3_big_tie_from_row0"):
        pops = sorted((len(v) for v in groups.values()), reverse=True)
        assert pops[0] == pops[1] and max(groups, key=lambda k: len(groups[k])) >= 2048


def test_s4_reference_keeps_the_horizon_rows_apart():
    (name, H, rows), = F.s4_cases()
    x = rows[:, 0].astype(np.float64); y = rows[:, 1].astype(np.float64)
    tw = H[2, 0] * x + H[2, 1] * y + H[2, 2]
    assert (tw != 0).all()
    want, groups = F.ref_static(H, rows)
    huge = [k for k in groups if 2 ** 31 <= k < 2 ** 53]
    assert len(huge) >= 3 and all(len(groups[k]) == 1 for k in huge)
    assert max(len(v) for v in groups.values()) == 2 and len(want) == 2
    assert np.array_equal(want, rows[-3:-1])


def test_static_sizes():
    assert [len(r) for _, _, r in F.s1_cases()] == list(F.S1_N)


# ---- the chained stage -------------------------------------------------------------------------------------------------------
def test_chain_case_is_a_meaningful_filter_input():
    q, t, xy_q, xy_t = F.chain_case()
    idx, d2 = O.knn2(q, t)
    idx_r, d_r = F.ref_knn2_u8(q, t)
    assert np.array_equal(idx, idx_r) and np.array_equal(d2, d_r)
    c = dict(idx=idx, d2=d2, xy_q=xy_q, xy_t=xy_t, ratio=0.5)
    st, rows = check_filter(c, 4, "chain")
    passed = F.u8_distances(d2)[:, 0] < F.u8_distances(d2)[:, 1] * 0.5
    m = len(F.ref_ratio_unique(idx, F.u8_distances(d2), 0.5))
    assert st == F.OK and 600 < len(rows) < m < passed.sum() < len(q)
