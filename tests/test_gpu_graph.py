"""evh_graph_normal and the drivers of evenvizion_amd.graph on the device.  The counters must EQUAL the numpy restatement's
(tests/graph_checks.py, itself checked in test_graph_host.py); each of the 154 sums must lie within (used + 8) * 2^-53 * sum |term| of
the restatement's correctly rounded sum -- used - 1 roundings from adding the terms in any order, at most 8 from forming a term out of
the shared, bit-identical U, V, X, Y, w in another association; the gate and the Huber threshold are met exactly on crafted rows; the
solver and the driver are held to the same solve driven by the restatement."""
import json
import os

import numpy as np
import pytest

import graph_checks as GC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MP4 = os.path.join(ROOT, "tests", "golden", "ref_test_video.mp4")
GOLD = os.path.join(ROOT, "tests", "golden", "ref_dict_with_homography_matrix.json")
INLIER_THR, HUBER = 1.0, 0.5


@pytest.fixture(scope="module")
def ctx():
    from evenvizion_amd._lib import Context
    c = Context(device=0, max_w=64, max_h=64, max_features=500, max_frames=2)     # the entry does not depend on these sizes
    yield c
    c.close()


def device_normal(ctx, S, edges, rows, counts, status=None, H_edge=None, inlier_thr=3.0, huber_delta=0.0):
    """Context.graph_normal on host arrays -> (sums f64[ne,154], info i32[ne,4]) on the host"""
    from evenvizion_amd import graph
    sums, info = graph.graph_normal(ctx, S, edges, rows, counts, status, H_edge, inlier_thr, huber_delta)
    ctx.synchronize()
    return sums.cpu().numpy(), info.cpu().numpy()


def within(got, want, info, absolute):
    bound = (info[:, :1].astype(np.float64) + 8) * GC.U53 * absolute
    with np.errstate(invalid="ignore"):
        ok = (np.abs(got - want) <= bound) | (np.isnan(got) & np.isnan(want))
    return ok


@pytest.fixture(scope="module")
def families():
    """the families and the restatement's results for them, computed once"""
    out = {}
    for kind in ("plain", "horizon", "nan"):
        fam = GC.family(kind, 11)
        for gate, delta in ((True, HUBER), (False, 0.0)):
            out[kind, gate, delta] = (fam, GC.normal(fam["S"], fam["edges"], fam["rows"], fam["counts"], None,
                                                     fam["H_edge"] if gate else None, INLIER_THR, delta))
    return out


# ---- counters and sums against the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plain", "horizon", "nan"])
@pytest.mark.parametrize("gate,delta", [(True, HUBER), (False, 0.0)])
def test_counters_equal_and_sums_within_the_rounding_bound(ctx, families, kind, gate, delta):
    fam, (want, winfo, absolute) = families[kind, gate, delta]
    got, info = device_normal(ctx, fam["S"], fam["edges"], fam["rows"], fam["counts"], None, fam["H_edge"] if gate else None, INLIER_THR, delta)
    assert np.array_equal(info, winfo), (info.tolist(), winfo.tolist())
    ok = within(got, want, winfo, absolute)
    worst = np.nanmax(np.where(absolute > 0, np.abs(got - want) / np.where(absolute > 0, absolute, 1) / GC.U53, 0))
    print("%s, gate %s, delta %g: used %s gated %s behind %s; worst |difference| = %.2f x 2^-53 x sum|term| (bound: used + 8)"
          % (kind, gate, delta, info[:, 0].tolist(), info[:, 1].tolist(), info[:, 2].tolist(), worst))
    assert ok.all(), np.argwhere(~ok)[:8].tolist()
    assert (info[:, :3].sum(axis=1) == np.clip(fam["counts"], 0, GC.ROW_CAP)).all() and not info[:, 3].any()
    assert not got[0].any() and not got[11].any() and got[[0, 11]].tobytes() == np.zeros((2, 154)).tobytes()    # counts 0 and -3: +0.0
    if gate:
        assert info[:, 1].sum() > 0 and (kind != "plain" or (info[3:11, 0] > 0).all())
    else:
        assert not info[:, 1].any() and np.array_equal(got[:, 152].tobytes(), got[:, 153].tobytes())
    if kind == "horizon":
        assert info[3, 2] > 0 and info[8, 2] > 0 and info[3, 0] > 0                # frame 1 on either side: some rows behind, some used
    if kind == "nan":
        assert info[4, 2] == 64 and info[7, 2] == 256 and not got[[4, 7]].any()  # frame 2 on either side: every row behind
    assert np.isfinite(got).all()


def test_sums_are_structured(ctx, families):
    fam, _ = families["plain", False, 0.0]
    got, info = device_normal(ctx, fam["S"], fam["edges"], fam["rows"], fam["counts"])
    from evenvizion_amd import graph
    for e in range(3, 11):
        A, g = graph.assemble(got[e:e + 1], [(1, 0)], 2)
        assert np.array_equal(A, A.T) and np.linalg.eigvalsh(A).min() >= -1e-9 * np.abs(A).max()
        Aii = A[8:, 8:]
        assert not Aii[:3, 3:6].any() and Aii[2, 2] == Aii[5, 5] == info[e, 0]      # weights 1: sum w = used


# ---- boundaries, with values chosen exact ------------------------------------------------------------------------------------------------------
def one_row(a, b):
    rows = np.zeros((1, 4, 4), np.float32)
    rows[0, 0] = (a[0], a[1], b[0], b[1])
    return rows


def test_gate_boundary_is_met_exactly(ctx):
    """H_e an integer translation, the row a 3-4-5 triangle away, inlier_thr = 5: used; bx one float32 ulp outward: gated"""
    S = np.stack([np.eye(3), GC.translation(7.0, -2.0)])
    He = GC.translation(10.0, 20.0)[None]
    edges, counts = np.array([[0, 1]], np.int32), np.array([1], np.int32)
    b = (30.0 + 10.0 + 3.0, 40.0 + 20.0 + 4.0)                                   # H_e . a + (3, 4)
    _, info = device_normal(ctx, S, edges, one_row((30.0, 40.0), b), counts, None, He, 5.0)
    assert info.tolist() == [[1, 0, 0, 0]]
    out = (float(np.nextafter(np.float32(b[0]), np.float32(np.inf))), b[1])
    _, info = device_normal(ctx, S, edges, one_row((30.0, 40.0), out), counts, None, He, 5.0)
    assert info.tolist() == [[0, 1, 0, 0]]
    sums, info = device_normal(ctx, S, edges, one_row((30.0, 40.0), out), counts, None, None, 5.0)      # no matrices: no gate
    assert info.tolist() == [[1, 0, 0, 0]] and sums[0, 153] > 0
    for rows in (one_row((30.0, 40.0), b), one_row((30.0, 40.0), out)):
        assert np.array_equal(GC.normal(S, edges, rows, counts, None, He, 5.0)[1], device_normal(ctx, S, edges, rows, counts, None, He, 5.0)[1])
    _, info = device_normal(ctx, S, edges, one_row((30.0, 40.0), (1e4, 1e4)), counts, None, He, float("inf"))
    assert info.tolist() == [[1, 0, 0, 0]]
    _, info = device_normal(ctx, S, edges, one_row((30.0, 40.0), b), counts, None, np.full((1, 3, 3), np.nan), 5.0)
    assert info.tolist() == [[0, 1, 0, 0]]                                      # a NaN compares false


def test_huber_boundary_is_met_exactly(ctx):
    """The same construction on the plane: q == delta^2 keeps w = 1; one ulp outward takes w = delta / sqrt(q) < 1"""
    S = np.stack([np.eye(3), GC.translation(7.0, -2.0)])
    edges, counts = np.array([[0, 1]], np.int32), np.array([1], np.int32)
    a = (30.0, 40.0)
    b = (a[0] - 7.0 - 3.0, a[1] + 2.0 - 4.0)                                     # P_j = P_i - (3, 4)
    sums, info = device_normal(ctx, S, edges, one_row(a, b), counts, huber_delta=5.0)
    assert info.tolist() == [[1, 0, 0, 0]] and sums[0, 152] == sums[0, 153] == 25.0 and sums[0, 15] == 1.0       # [15] is A_ii[2][2] = sum w
    out = (float(np.nextafter(np.float32(b[0]), np.float32(-np.inf))), b[1])
    sums, info = device_normal(ctx, S, edges, one_row(a, out), counts, huber_delta=5.0)
    want = GC.normal(S, edges, one_row(a, out), counts, huber_delta=5.0)
    assert sums[0, 153] > 25.0 and sums[0, 152] < sums[0, 153] and 0.999 < sums[0, 15] < 1.0
    assert sums[0, 152] == want[0][0, 152] and sums[0, 153] == want[0][0, 153] and sums[0, 15] == want[0][0, 15]        # one row: the atoms, bit for bit
    plain, _ = device_normal(ctx, S, edges, one_row(a, out), counts, huber_delta=0.0)
    assert plain[0, 152:153].tobytes() == plain[0, 153:154].tobytes() and plain[0, 15] == 1.0


def test_plane_points_are_those_of_transform_points(ctx, families):
    """g_i[2] of a single row under weights 1 is ru = U - X; with S_j the identity and b = 0 it is U itself"""
    fam, _ = families["plain", False, 0.0]
    pts = fam["rows"][5, :64, :2].astype(np.float64)
    want = ctx.transform_points(fam["S"][3:4], np.zeros(64, np.int32), pts)
    S = np.stack([fam["S"][3], np.eye(3)])
    rows = np.zeros((64, 1, 4), np.float32)
    rows[:, 0, :2] = fam["rows"][5, :64, :2]
    got, info = device_normal(ctx, S, np.tile(np.array([[0, 1]], np.int32), (64, 1)), rows, np.ones(64, np.int32))
    assert (info[:, 0] == 1).all() and got[:, 136 + 2].tobytes() == want[:, 0].copy().tobytes() and got[:, 136 + 5].tobytes() == want[:, 1].copy().tobytes()


# ---- flags ------------------------------------------------------------------------------------------------------------------------------
def test_flagged_edges_get_zeros_and_leave_their_neighbours_alone(ctx, families):
    fam, _ = families["plain", True, HUBER]
    args = (fam["rows"], fam["counts"])
    clean, cinfo = device_normal(ctx, fam["S"], fam["edges"], *args, None, fam["H_edge"], INLIER_THR, HUBER)
    edges = fam["edges"].copy()
    edges[3], edges[5], edges[8] = (2, 2), (-1, 3), (1, GC.NFRAMES)
    status = np.zeros(12, np.int32)
    status[6], status[8] = 4, 2
    got, info = device_normal(ctx, fam["S"], edges, *args, status, fam["H_edge"], INLIER_THR, HUBER)
    want = GC.normal(fam["S"], edges, *args, status, fam["H_edge"], INLIER_THR, HUBER)
    assert np.array_equal(info, want[1])
    assert info[[3, 5, 6, 8]].tolist() == [[0, 0, 0, 1], [0, 0, 0, 1], [0, 0, 0, 2], [0, 0, 0, 3]]
    assert got[[3, 5, 6, 8]].tobytes() == np.zeros((4, 154)).tobytes()
    others = [e for e in range(12) if e not in (3, 5, 6, 8)]
    assert got[others].tobytes() == clean[others].tobytes() and np.array_equal(info[others], cinfo[others])


# ---- purity -----------------------------------------------------------------------------------------------------------------------------
def test_two_calls_and_permuted_lists_return_the_same_bytes(ctx, families):
    fam, _ = families["horizon", True, HUBER]
    call = lambda order: device_normal(ctx, fam["S"], fam["edges"][order], fam["rows"][order], fam["counts"][order], None,
                                       fam["H_edge"][order], INLIER_THR, HUBER)
    same = np.arange(12)
    a, b = call(same), call(same)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    order = np.random.default_rng(2).permutation(12)
    c = call(order)
    assert c[0].tobytes() == a[0][order].tobytes() and c[1].tobytes() == a[1][order].tobytes()


def test_reversing_an_edge_swaps_its_blocks(ctx, families):
    fam, (want, winfo, absolute) = families["plain", False, 0.0]
    fwd, info = device_normal(ctx, fam["S"], fam["edges"], fam["rows"], fam["counts"])
    rows = np.ascontiguousarray(fam["rows"][:, :, [2, 3, 0, 1]])
    rev, rinfo = device_normal(ctx, fam["S"], np.ascontiguousarray(fam["edges"][:, ::-1]), rows, fam["counts"])
    assert np.array_equal(info, rinfo)
    back = rev.copy()
    back[:, 0:36], back[:, 36:72] = rev[:, 36:72], rev[:, 0:36]
    back[:, 72:136] = rev[:, 72:136].reshape(-1, 8, 8).transpose(0, 2, 1).reshape(-1, 64)
    back[:, 136:144], back[:, 144:152] = rev[:, 144:152], rev[:, 136:144]
    # r changes sign with the edge and so does J of either end: A and g = J^T r keep their values, entry by entry
    ok = within(back, want, winfo, absolute)
    assert ok.all(), np.argwhere(~ok)[:8].tolist()               # not the same bytes as fwd: the terms associate differently
    assert within(fwd, want, winfo, absolute).all()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(ctx, families):
    import torch
    from evenvizion_amd import _lib
    fam, _ = families["plain", True, HUBER]
    dev = "cuda:0"
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dt).contiguous()
    S, edges, rows = t(fam["S"].reshape(-1), torch.float64), t(fam["edges"], torch.int32), t(fam["rows"], torch.float32)
    counts, H = t(fam["counts"], torch.int32), t(fam["H_edge"].reshape(-1), torch.float64)
    sums = torch.full((12, 154), 7.25, dtype=torch.float64, device=dev)
    info = torch.full((12, 4), -9, dtype=torch.int32, device=dev)
    good = dict(S=S.data_ptr(), nframes=6, edges=edges.data_ptr(), nedges=12, rows=rows.data_ptr(), row_cap=320, counts=counts.data_ptr(),
                status=None, H=H.data_ptr(), thr=1.0, delta=0.5, sums=sums.data_ptr(), info=info.data_ptr())
    order = ("S", "nframes", "edges", "nedges", "rows", "row_cap", "counts", "status", "H", "thr", "delta", "sums", "info")

    def call(**over):
        a = dict(good)
        a.update(over)
        return ctx.lib.evh_graph_normal(ctx.h, *[a[k] for k in order])
    bad = [dict(S=None), dict(edges=None), dict(rows=None), dict(counts=None), dict(sums=None), dict(info=None), dict(nframes=0),
           dict(nedges=0), dict(nedges=-1), dict(row_cap=0), dict(nedges=(1 << 22) + 1), dict(thr=float("nan")), dict(delta=float("nan")),
           dict(thr=-1.0), dict(rows=rows.data_ptr() + 4), dict(S=S.data_ptr() + 4), dict(sums=sums.data_ptr() + 4)]
    for over in bad:
        assert call(**over) == -1, over
        assert b"evh_graph_normal" in ctx.lib.evh_last_error_string(ctx.h)
    ctx.synchronize()
    assert (sums == 7.25).all() and (info == -9).all()
    assert call(thr=-1.0, H=None) == 0                           # no gate: the threshold is not looked at
    with pytest.raises(ValueError):
        ctx.graph_normal(S, edges[:, :1], rows, counts)
    with pytest.raises(ValueError):
        ctx.graph_normal(S, edges, rows, counts.to(torch.int64))
    with pytest.raises(ValueError):
        ctx.graph_normal(S.cpu(), edges, rows, counts)
    ctx.synchronize()
    assert _lib.GRAPH_NSUMS == 154


# ---- the solver on the device -------------------------------------------------------------------------------------------------------------
def test_solver_on_the_device_closes_the_loop(ctx):
    from evenvizion_amd import graph
    truth, given = GC.loop_path()
    sup, ri = {k + 1: m for k, m in enumerate(given)}, {"w": GC.LOOP_W, "h": GC.LOOP_H}
    edges, _ = graph.loop_candidates(sup, ri, min_gap=2, max_partners=6)
    N, _ = graph.plane_normalisation(sup, ri)
    rows, counts = GC.loop_rows(truth, edges)
    import torch
    d_rows, d_counts, d_edges = (torch.from_numpy(a).cuda() for a in (rows, counts, np.asarray(edges, np.int32)))

    def on_device(S):
        out = graph.graph_normal(ctx, S, d_edges, d_rows, d_counts)
        ctx.order_torch_after()
        return out
    got, rep = graph.solve_graph(given, graph.evaluator(on_device, edges), "homography", 10, 0, N)
    host, hrep = graph.solve_graph(given, graph.evaluator(lambda S: GC.normal(S, edges, rows, counts, exact=False), edges), "homography", 10, 0, N)
    e = GC.loop_errors(got, truth)
    apart = max(GC.corner_error(a, b, GC.LOOP_W, GC.LOOP_H) for a, b in zip(got, host))
    print("device: worst corner %.3g px, cost %.3g -> %.3g, %d accepted; %.3g px from the restatement's solve"
          % (max(e), rep["cost_before"], rep["cost_after"], rep["accepted"], apart))
    assert max(e) <= 1e-6 and apart <= 1e-6


# ---- the driver -----------------------------------------------------------------------------------------------------------------------------
def pan_scene(n=12, w=320, h=240, step=24, err=0.25, seed=5):
    """An out-and-back pan of n textured BGR frames cut from one scene (synthetic.make_canvas) at integer offsets, n/2 out and n/2
    back -> (frames, truth, given): the dictionary is err px per pair off"""
    from evenvizion_amd import synthetic
    rng = np.random.default_rng(seed)
    off = [step * k if k < n // 2 else step * (n - 1 - k) for k in range(n)]
    canvas = synthetic.make_canvas(rng, w + max(off), h)
    frames = [np.ascontiguousarray(np.repeat(canvas[64:64 + h, 64 + o:64 + o + w, None], 3, axis=2)) for o in off]
    return frames, [GC.translation(float(o)) for o in off], [GC.translation(o + err * k) for k, o in enumerate(off)]


@pytest.fixture(scope="module")
def pan():
    return pan_scene()


def test_the_driver_closes_a_pan(pan):
    """12 frames of 320 x 240, 6 out and 6 back at 24 px per frame, the dictionary 0.25 px per pair off (2.75 px at the last frame,
    1.375 px in the mean).  Every returning frame keeps a loop edge; the mean and the last corner error end below the dictionary's;
    the same driver fed by the restatement on the rows it downloaded ends within 1e-6 px."""
    from evenvizion_amd import graph
    from evenvizion_amd.synthetic import SyntheticCapture
    frames, truth, given = pan
    sup, ri = {k + 1: S for k, S in enumerate(given)}, {"w": 320, "h": 240}
    kw = dict(min_gap=2, max_partners=3)
    got, rep = graph.align_superposition(SyntheticCapture(list(frames)), sup, ri, **kw)
    host, hrep = graph.align_superposition(SyntheticCapture(list(frames)), sup, ri, normal=lambda *a: GC.normal(*a[:4], None, *a[4:], exact=False), **kw)
    err = lambda mats: [GC.corner_error(a, b, 320, 240) for a, b in zip(mats, truth)]
    e0, e, eh = err(given), err([got[k + 1] for k in range(12)]), err([host[k + 1] for k in range(12)])
    apart = max(GC.corner_error(got[k], host[k], 320, 240) for k in got)
    print("dictionary mean %.3f last %.3f px; aligned mean %.4f last %.4f px; %d of %d edges kept, used %d..%d rows; cost %.4g -> %.4g in "
          "%d steps; %.3g px from the restatement's" % (np.mean(e0), e0[-1], np.mean(e), e[-1], len(rep["edges_kept"]), len(rep["edges_tried"]),
                                                      min(rep["used"]), max(rep["used"]), rep["cost_before"], rep["cost_after"],
                                                      rep["accepted"], apart))
    assert list(got) == list(sup) and np.abs(got[1] - given[0]).max() <= 1e-12
    assert all(k in rep["loop_edges_kept"] for k in range(7, 13)), rep["loop_edges_kept"]
    assert np.mean(e) < np.mean(e0) and e[-1] < e0[-1] and rep["cost_after"] < rep["cost_before"]
    assert rep["edges_kept"] == hrep["edges_kept"] and rep["used"] == hrep["used"] and min(rep["used"]) >= 20
    assert apart <= 1e-6
    same, rep0 = graph.align_superposition(SyntheticCapture(list(frames)), sup, ri, iters=0, **kw)
    assert all(np.abs(same[k] - sup[k]).max() <= 1e-12 for k in sup) and rep0["edges_kept"] == rep["edges_kept"]
    with pytest.raises(ValueError, match="fewer frames"):
        graph.align_superposition(SyntheticCapture(list(frames[:8])), sup, ri, **kw)
    with pytest.raises(ValueError, match="do not connect"):
        graph.align_superposition(SyntheticCapture(list(frames)), sup, ri, min_inliers=100000, **kw)


def test_stride_spreads_the_nodes_corrections(pan):
    from evenvizion_amd import graph
    from evenvizion_amd.synthetic import SyntheticCapture
    frames, truth, given = pan
    sup, ri = {k + 1: S for k, S in enumerate(given)}, {"w": 320, "h": 240}
    got, rep = graph.align_superposition(SyntheticCapture(list(frames)), sup, ri, stride=2, min_gap=1, max_partners=3)
    assert rep["nodes"] == [1, 3, 5, 7, 9, 11] and list(got) == list(sup)
    for k in range(1, 12, 2):                                   # a frame between two nodes carries the correction of the node before it
        D0 = np.dot(got[k], np.linalg.inv(sup[k]))
        D1 = np.dot(got[k + 1], np.linalg.inv(sup[k + 1]))
        assert np.abs(D0 / D0[2, 2] - D1 / D1[2, 2]).max() <= 1e-9


# ---- the reference's video ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recorded():
    from evenvizion_amd.processing.utils import read_homography_dict, superposition_dict
    hd, ri = read_homography_dict(GOLD)
    sup = superposition_dict(hd)
    return {k: sup[k] for k in sup if k != "resize_info"}, ri


def test_the_reference_video(recorded):
    """The whole video at 400 x 224 with its recorded matrices.  ORB alone gives 17 to 49 static rows per consecutive pair of the first
    40 frames (the same counts as the stream pass gives for those pairs), so the default min_inliers = 20 breaks the chain at the first
    pair with fewer, frames 12 and 13 with 17 -- the driver refuses and names it -- and the run is made with min_inliers = 8.  The cost does
    not rise and every kept edge has its inliers.  Nothing else is claimed for this video; DESIGN section 25 records the figures."""
    from evenvizion_amd import capture, graph
    sup, ri = recorded
    got = graph.aligned_homography_dict(lambda: capture.VideoCapture(MP4), sup, ri, min_inliers=8)
    rep = got["report"]
    print("%d frames: %d of %d edges kept (%d loop edges), used %d..%d, cost %.5g -> %.5g in %d accepted steps, ITF %.3f -> %.3f dB"
          % (len(sup), len(rep["edges_kept"]), len(rep["edges_tried"]), sum(len(v) for v in rep["loop_edges_kept"].values()), min(rep["used"]),
             max(rep["used"]), rep["cost_before"], rep["cost_after"], rep["accepted"], rep["report_before"]["itf"], rep["report_after"]["itf"]))
    assert rep["cost_after"] <= rep["cost_before"] and all(u >= 8 for u in rep["used"])
    assert len(rep["used"]) == len(rep["edges_kept"]) >= len(sup) - 1
    assert list(got["superposition"]) == list(sup) and len(got["homography"]) == len(sup) - 1
    json.dumps({k: v for k, v in rep.items() if not k.startswith("loop_edges")})        # the report is plain data
    first = {k: sup[k] for k in list(sup)[:16]}
    with pytest.raises(ValueError, match=r"do not connect .* min_inliers = 20 dropped \d+ consecutive edges, the first: \(\d+, \d+\): status 0, \d+ inliers"):
        graph.align_superposition(capture.VideoCapture(MP4), first, ri)


def test_component_writes_the_aligned_files_only_on_request(tmp_path, monkeypatch):
    from evenvizion_amd import component
    monkeypatch.chdir(tmp_path)
    base = ["--path_to_video", MP4, "--features", "ORB"]
    plain = component.main(base + ["--experiment_name", "plain"])
    folder = component.main(base + ["--experiment_name", "aligned", "--global_align", "1", "--graph_partners", "1", "--graph_min_inliers", "8"])
    old = sorted(os.listdir(plain))
    assert sorted(os.listdir(folder)) == sorted(old + ["dict_with_homography_matrix_aligned.json", "graph_report.json"])
    for name in old:
        with open(os.path.join(plain, name), "rb") as a, open(os.path.join(folder, name), "rb") as b:
            assert a.read() == b.read(), name
    with open(os.path.join(folder, "dict_with_homography_matrix_aligned.json")) as f:
        aligned = json.load(f)
    with open(os.path.join(folder, "dict_with_homography_matrix.json")) as f:
        first = json.load(f)
    with open(os.path.join(folder, "graph_report.json")) as f:
        report = json.load(f)
    assert list(aligned) == list(first) and aligned["resize_info"] == first["resize_info"] == {"h": 224, "w": 400}
    assert np.asarray(aligned[list(aligned)[0]]["H"]).shape == (3, 3)
    assert report["cost_after"] <= report["cost_before"] and report["model"] == "homography" and all(u >= 8 for u in report["used"])
    assert {"edges_tried", "edges_kept", "loop_edges", "loop_edges_kept", "cost_before", "cost_after", "steps", "accepted", "report_before",
            "report_after"} <= set(report)
