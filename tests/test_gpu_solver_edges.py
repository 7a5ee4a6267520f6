"""The device's homography solver (evh_ransac.hip) on the adversarial families of tests/solver_families.py, through every
entry that takes rows: Context.find_homography (plain, force_max_iters at 2000 and at 37), Context.compute_homography
(Hsup None and a strong Hsup) and Context.stream_scan on crafted pairs (k_ransac_final_stream; k_scan_hyp / k_scan_finish
when forced), against the oracle and the float64 reference; then the tolerance mode (SOLVER_FAST) on the same sets.
Bars: masks, info and statuses exactly equal; H bit-equal where the parity suite asserts it for the entry, elsewhere
rtol 1e-9 / atol 1e-12."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import solver_families as F
from oracle import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_parity import BAR_ABS, BAR_AFF, BAR_CORNER, BAR_HERR, corner_err, h_err  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = F.all_sets()
IDS = ["%s-%s" % (fam, name) for fam, name, _ in SETS]
RUNS = ((False, 2000), (True, 2000), (True, 37))
# a strong plane for compute_homography's pre-transform (float64 -> float32 rows on both sides)
HSUP = np.array([[1.03, 0.02, 41.5], [-0.015, 0.97, -23.25], [2.5e-5, -1.5e-5, 1.0]])
CTX_ARGS = dict(device=0, max_w=640, max_h=480, max_features=1200, max_frames=4)


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU; there is no CPU fallback")
    from evenvizion_amd._lib import Context
    c = Context(**CTX_ARGS)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1, 4)).cuda()


def kcap(c):
    return int(c.lib.evh_orb_capacity(c.h))


def _close(Hg, Ho):
    return np.allclose(Hg, Ho, rtol=1e-9, atol=1e-12)


def _scan(c, pairs, st1, state_in=None, state_out=None, force=False):
    """Context.stream_scan on crafted pairs: rows f32[npairs, kcap, 4] (zero beyond each count)"""
    cap = kcap(c)
    rows = np.zeros((len(pairs), cap, 4), np.float32)
    counts = np.zeros(len(pairs), np.int32)
    for p, r in enumerate(pairs):
        assert len(r) <= cap
        rows[p, :len(r)] = r; counts[p] = len(r)
    H, st = c.stream_scan(torch.from_numpy(rows).cuda(), torch.from_numpy(counts).cuda(),
                          torch.from_numpy(np.asarray(st1, np.int32)).cuda(), state_in=state_in, state_out=state_out,
                          force_max_iters=force)
    c.synchronize()
    return H.cpu().numpy().reshape(-1, 3, 3), st.cpu().numpy()


def _exact_runs(c, rows):
    """all three entries on one set -> dict of results (device)"""
    out = {}
    for force, mi in RUNS:
        out[("find", force, mi)] = c.find_homography(dev(rows), max_iters=mi, force_max_iters=force)
    out[("compute", None)] = c.compute_homography(rows)
    out[("compute", "sup")] = c.compute_homography(rows, HSUP)
    return out


@pytest.mark.parametrize("fam,name,rows", SETS, ids=IDS)
def test_exact_mode_against_oracle(ctx, fam, name, rows):
    got = _exact_runs(ctx, rows)
    for force, mi in RUNS:
        Hg, mg, ig = got[("find", force, mi)]
        Ho, mo, io = O.find_homography(rows[:, :2], rows[:, 2:], max_iters=mi, force_max_iters=force)
        tag = (name, force, mi)
        assert (Hg is None) == (Ho is None), tag
        assert np.array_equal(mg, mo), (tag, np.flatnonzero(mg != mo))
        assert np.array_equal(ig, io), (tag, ig, io)
        if Ho is not None:
            if mo.sum() >= 512:                    # test_find_homography_many_inliers: bit for bit
                assert np.array_equal(Hg, Ho), (tag, np.abs(Hg - Ho).max())
            assert _close(Hg, Ho), (tag, np.abs(Hg - Ho).max())
            F.check_solution(Hg, mg, rows, str(tag))
    for key, hs in ((None, None), ("sup", HSUP)):
        sg, Hg = got[("compute", key)]
        so, Ho = O.compute_homography(rows[:, :2], rows[:, 2:], hs)
        assert sg == so, (name, key, sg, so)
        if so == O.OK:
            assert _close(Hg, Ho), (name, key, np.abs(Hg - Ho).max())
    if fam == "F4":                                # the mask is is_inlier's float32 evaluation, err == 9 included
        assert np.array_equal(got[("find", False, 2000)][1].astype(bool), F.boundary_expected(rows, F.F4_H)[1])


def test_largest_row_counts(ctx):
    """F7 content at the largest n each entry accepts: kcap * max_frames rows for find_homography, kcap for
    compute_homography."""
    cap = kcap(ctx)
    big = F.f7_sizes((cap * CTX_ARGS["max_frames"], cap), seed=717)
    for name, rows in big:
        for force, mi in ((False, 2000), (True, 37)):
            Hg, mg, ig = ctx.find_homography(dev(rows), max_iters=mi, force_max_iters=force)
            Ho, mo, io = O.find_homography(rows[:, :2], rows[:, 2:], max_iters=mi, force_max_iters=force)
            assert Ho is not None and Hg is not None and np.array_equal(mg, mo) and np.array_equal(ig, io), (name, ig, io)
            assert np.array_equal(Hg, Ho), (name, np.abs(Hg - Ho).max())
            F.check_solution(Hg, mg, rows, name)
    rows = big[1][1]
    for hs in (None, HSUP):
        sg, Hg = ctx.compute_homography(rows, hs)
        so, Ho = O.compute_homography(rows[:, :2], rows[:, 2:], hs)
        assert sg == so and (so != O.OK or _close(Hg, Ho)), (sg, so)


@pytest.mark.parametrize("force", [False, True])
def test_stream_scan_on_crafted_rows(ctx, force):
    """Context.stream_scan on hand-made pairs with a mixed status1 (failure codes take none_H_processing), an empty pair and
    a pair that fails the 0.7 gate, against the Python mirror of the oracle's scan; split in two with state_in / state_out it
    equals the single call bit for bit; a failing first pair ends the scan with NaN."""
    pairs = F.scan_pairs(kcap(ctx))
    rl = [p[0] for p in pairs]; st1 = np.array([p[1] for p in pairs], np.int32)
    Hm, sm = F.scan_mirror(rl, st1, force=force)
    assert (sm == O.OK).sum() >= 6 and (sm == O.LOW_INLIER_RATIO).any() and (sm == O.NO_FINAL_H).any()
    Hg, sg = _scan(ctx, rl, st1, force=force)
    assert np.array_equal(sg, sm), (sg, sm)
    assert _close(Hg, Hm), np.abs(Hg - Hm).max()
    k = 5
    state = torch.zeros(18, dtype=torch.float64, device="cuda")
    Ha, sa = _scan(ctx, rl[:k], st1[:k], state_out=state, force=force)
    Hb, sb = _scan(ctx, rl[k:], st1[k:], state_in=state, force=force)
    assert np.array_equal(np.r_[Ha, Hb], Hg) and np.array_equal(np.r_[sa, sb], sg)
    st_bad = st1[:4].copy(); st_bad[0] = O.FEW_MATCHES
    Hf, sf = _scan(ctx, rl[:4], st_bad, force=force)
    Hfm, sfm = F.scan_mirror(rl[:4], st_bad, force=force)
    assert np.array_equal(sf, sfm) and np.isnan(Hf).all() and np.isnan(Hfm).all()


# ---- tolerance mode -------------------------------------------------------------------------------------------------------
def _bars(Hf, He, rows):
    lo = rows[:, :2].min(0); hi = rows[:, :2].max(0)
    T = np.array([[1, 0, lo[0]], [0, 1, lo[1]], [0, 0, 1.0]])
    w, h = (hi - lo)
    return {"corner": corner_err(Hf @ T, He @ T, w, h), "abs": float(np.abs(Hf[2, :2] - He[2, :2]).max()),
            "aff_rel": float((np.abs(Hf[:2] - He[:2]) / np.maximum(np.abs(He[:2]), [[1e-3, 1e-3, 1.0]] * 2)).max()),
            "h_err": h_err(Hf, He)}


def _fast_vs_exact(Hf, He, mask, rows, tag):
    """finite; cost no worse than the better of the exact H and the float64 refit; inside the BAR_* of test_fast_solver_mode
    where the float64 spectrum of the normalised J^T J says the set is well conditioned"""
    assert np.isfinite(Hf).all(), tag
    sel = mask.astype(bool)
    a = rows[sel, :2].astype(np.float64); b = rows[sel, 2:].astype(np.float64)
    ce = F.cost(He, a, b)
    Hr = F.dlt64(a, b) if sel.sum() > 4 else He
    cr = F.cost(Hr, a, b) if Hr is not None else np.inf
    cf = F.cost(Hf, a, b)
    assert cf <= max(ce, cr) * (1 + 1e-6) + F.cost_floor(b), (tag, cf, ce, cr)
    if F.normalised_jtj_cond(He, a) <= F.WELL_CONDITIONED:
        m = _bars(Hf, He, rows[sel])
        assert m["corner"] <= BAR_CORNER and m["abs"] <= BAR_ABS and m["aff_rel"] <= BAR_AFF and m["h_err"] <= BAR_HERR, (tag, m)


@pytest.mark.parametrize("fam,name,rows", SETS, ids=IDS)
def test_fast_mode_matches_exact_mode(ctx, fam, name, rows):
    """SOLVER_FAST on every family: masks, RANSAC iterations, inlier counts and statuses as the exact mode's (info[2], LM's
    iteration count, may differ); H finite and no worse than the exact mode's or the float64 refit's."""
    from evenvizion_amd._lib import SOLVER_EXACT, SOLVER_FAST
    ex = _exact_runs(ctx, rows)
    ctx.set_solver_mode(SOLVER_FAST)
    try:
        fa = _exact_runs(ctx, rows)
    finally:
        ctx.set_solver_mode(SOLVER_EXACT)
    for force, mi in RUNS:
        He, me, ie = ex[("find", force, mi)]
        Hf, mf, i_f = fa[("find", force, mi)]
        tag = (name, force, mi)
        assert (Hf is None) == (He is None) and np.array_equal(mf, me) and np.array_equal(i_f[:2], ie[:2]), (tag, i_f, ie)
        if He is not None:
            _fast_vs_exact(Hf, He, me, rows, tag)
    for key, hs in ((None, None), ("sup", HSUP)):
        se, He = ex[("compute", key)]
        sf, Hf = fa[("compute", key)]
        assert sf == se, (name, key, sf, se)
        if se == O.OK and hs is None:
            _fast_vs_exact(Hf, He, ex[("find", False, 2000)][1], rows, (name, key))
        elif se == O.OK:
            assert np.isfinite(Hf).all()


@pytest.mark.parametrize("force", [False, True])
def test_fast_mode_stream_scan(ctx, force):
    from evenvizion_amd._lib import SOLVER_EXACT, SOLVER_FAST
    pairs = F.scan_pairs(kcap(ctx))
    rl = [p[0] for p in pairs]; st1 = np.array([p[1] for p in pairs], np.int32)
    He, se = _scan(ctx, rl, st1, force=force)
    ctx.set_solver_mode(SOLVER_FAST)
    try:
        Hf, sf = _scan(ctx, rl, st1, force=force)
    finally:
        ctx.set_solver_mode(SOLVER_EXACT)
    assert np.array_equal(sf, se) and np.isfinite(Hf).all()


PROF_CHILD = r"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np
import solver_families as F
from evenvizion_amd._lib import Context, SOLVER_FAST
sets = dict((name, rows) for _, name, rows in F.all_sets())
rng = np.random.default_rng(9)
for off, wdt in ((1e4, 2.0), (3e4, 4.0)):          # probes for LM's fall-back: 2-4 px clusters far from the origin, noisy
    a = (np.array([off, 0.7 * off]) + rng.uniform(0, wdt, (60, 2))).astype(np.float32).astype(np.float64)
    H = np.array([[1.01, 0.02, 5], [-0.01, 0.99, -3], [1e-6, -2e-6, 1]])
    sets["probe_cluster_%g" % off] = F._f32(a, F.proj(H, a) + rng.normal(0, 0.3, a.shape))
c = Context(**{ctx!r})
c.set_solver_mode(SOLVER_FAST)
for name in {names!r}:
    st, H = c.compute_homography(sets[name])
    sys.stderr.flush()
    print("CASE %s %d %d" % (name, st, int(np.isfinite(H).all())), file=sys.stderr, flush=True)
c.close()
"""
PROF_NAMES = ["f1_grid", "f6_horizon", "f6_horizon_tilted", "f6_4k_off10000", "f6_perspective", "f6_cluster1", "f6_n5",
              "f1_rare", "f7_n1025", "probe_cluster_10000", "probe_cluster_30000"]


def test_fast_mode_fallbacks_are_reached():
    """EVH_RANSAC_PROF's per-call rotation counts in a fresh process (the variable is read once per process): in the
    tolerance mode Jacobi rotations are counted only when a fall-back ran -- 9x9 when the refit's h33 = 1 LDL^T failed (a
    pivot not positive, or |x| >= 1e12: dlt_rows_fast), 8x8 when LM's LDL^T failed (lm_refine -> fast_solve8).  A generic
    set needs neither; the horizon through the source centroid (h33 = 0 in the normalised frame) must leave the refit's
    LDL^T (f6_horizon went through it before the relative pivot test: a noise pivot, a noise seed); a noisy 2 px cluster
    at a 1e4 px offset must leave LM's (J^T J in raw pixels, once lambda has dropped to 0 after a good first step)."""
    env = dict(os.environ, EVH_RANSAC_PROF="1")
    code = PROF_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), ctx=CTX_ARGS, names=PROF_NAMES)
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    rot = {}
    pend = None
    for line in r.stderr.splitlines():
        m = re.search(r"rotations: 9x9 ([0-9.]+) 8x8 ([0-9.]+)", line)
        if m:
            pend = (float(m.group(1)), float(m.group(2)))
        elif line.startswith("CASE "):
            _, name, st, fin = line.split()
            assert pend is not None, line
            rot[name] = (pend[0], pend[1], int(st), int(fin))
            pend = None
    print("tolerance-mode fall-backs (9x9 refit rotations, 8x8 LM rotations, status, finite):", rot)
    assert set(rot) == set(PROF_NAMES)
    assert rot["f1_grid"][:2] == (0.0, 0.0)
    assert rot["f6_horizon"][0] > 0 and rot["f6_horizon_tilted"][0] > 0
    assert rot["probe_cluster_10000"][1] > 0
    assert all(v[3] == 1 for v in rot.values() if v[2] == 0)
