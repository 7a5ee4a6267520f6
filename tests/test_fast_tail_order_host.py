"""Host: pass 2 of fast_nms_queue_ordered (evh_detect_fast.h) emulated in numpy -- four waves, 28 lanes each with one dword of the
28-row x 4-dword survivor bitmap, pop-counts, a prefix sum over the lanes, every dword expanded lowest bit first into the wave's
quarter of the list -- against a plain row-major scan of the tile.  The list, the wave totals and the row-count bytes must be what
fast_nms_collect_ordered leaves: the survivors of wave w's rows 7w .. 7w+6 in row-major order from lst[256 w], their number in
wtot[w], the survivors of tile row r in byte r & 3 of rowcnt[r >> 2]."""
import numpy as np
import pytest

FT_W, FT_H = 128, 28
X0, Y0 = 24 + 128, 31 + 28


def cand(s, y, x):
    return (int(s) << 24) | (int(y) << 12) | int(x)


def bitmap_of(mask):
    bm = np.zeros(FT_H * 4, np.uint32)
    for r, cx in zip(*np.nonzero(mask)):
        bm[4 * r + (cx >> 5)] |= np.uint32(1) << np.uint32(cx & 31)
    return bm


def pass2_emulated(bm, score):
    lst = np.full(1024, 0xFFFFFFFF, np.uint64)
    wtot = np.zeros(4, np.int64)
    rowcnt = np.zeros(8, np.uint32)
    for w in range(4):
        words = [int(bm[28 * w + lane]) for lane in range(28)]
        cnt = [bin(m).count("1") for m in words]
        incl = np.cumsum(cnt)
        wtot[w] = incl[27]
        for lane in range(28):
            row, cx0 = 7 * w + (lane >> 2), (lane & 3) * 32
            if lane & 3 == 0:
                rsum = sum(cnt[lane:lane + 4])
                if rsum:
                    rowcnt[row >> 2] |= np.uint32(rsum << (8 * (row & 3)))
            out, m = 256 * w + int(incl[lane]) - cnt[lane], words[lane]
            while m:
                b = (m & -m).bit_length() - 1
                m &= m - 1
                assert out < 256 * (w + 1)
                lst[out] = cand(score[row, cx0 + b], Y0 + row, X0 + cx0 + b)
                out += 1
    return lst, wtot, rowcnt


def row_major(mask, score):
    lst = np.full(1024, 0xFFFFFFFF, np.uint64)
    wtot = np.zeros(4, np.int64)
    rowcnt = np.zeros(8, np.uint32)
    for w in range(4):
        k = 256 * w
        for r in range(7 * w, 7 * w + 7):
            for cx in range(FT_W):
                if mask[r, cx]:
                    lst[k] = cand(score[r, cx], Y0 + r, X0 + cx)
                    k += 1
            n = int(mask[r].sum())
            rowcnt[r >> 2] |= np.uint32(n << (8 * (r & 3)))
        wtot[w] = k - 256 * w
    return lst, wtot, rowcnt


def _masks(density):
    if density == "densest":         # one survivor per 2 x 2 block, on the even or the odd rows and columns: 256 in a wave
        for oy in (0, 1):
            for ox in (0, 1):
                m = np.zeros((FT_H, FT_W), bool)
                m[oy::2, ox::2] = True
                yield m
        return
    rng = np.random.default_rng(int(density * 1000) + 3)
    made = 0
    while made < 6:
        m = rng.random((FT_H, FT_W)) < density
        if all(m[7 * w:7 * w + 7].sum() <= 256 for w in range(4)):     # a wave's quarter of the list holds 256
            made += 1
            yield m


@pytest.mark.parametrize("density", [0.0, 1 / 64, 1 / 4, "densest"])
def test_bitmap_order_equals_row_major_scan(density):
    rng = np.random.default_rng(1)
    n = 0
    for mask in _masks(density if density == "densest" else float(density)):
        score = rng.integers(20, 255, (FT_H, FT_W))
        got, want = pass2_emulated(bitmap_of(mask), score), row_major(mask, score)
        for g, w_ in zip(got, want):
            assert np.array_equal(g, w_)
        n += int(mask.sum())
    assert (n == 0) == (density == 0.0)
    if density == "densest":
        assert n == 2 * (14 * 64) + 2 * (14 * 64)
