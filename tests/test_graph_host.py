"""The host side of global alignment: the numpy restatement of evh_graph_normal (tests/graph_checks.py) against finite differences
and exact rational arithmetic, the assembly and the motion models on scripted blocks, the solver on the loop of DESIGN section 22
driven by the restatement, the choice of loop edges, the refusals and the header.  No GPU: the device is held to graph_checks in
test_gpu_graph.py."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import graph_checks as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = GC.LOOP_W, GC.LOOP_H


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------
def test_fma_rounds_once():
    rng = np.random.default_rng(5)
    a, b = rng.normal(0, 1, 200), rng.normal(0, 100, 200)
    c = -(a * b) + rng.normal(0, 1e-14, 200)                  # heavy cancellation: a*b + c with two roundings is far off
    got = GC.fma(a, b, c)
    for k in range(200):
        exact = Fraction(a[k]) * Fraction(b[k]) + Fraction(c[k])
        assert got[k] == float(exact), k                      # float(Fraction) rounds to nearest, ties to even
    assert np.isnan(GC.fma(np.nan, 1.0, 1.0)) and GC.fma(np.inf, 1.0, 1.0) == np.inf


def test_jacobian_agrees_with_central_differences():
    """J of pi((I + Delta) . S . p) by d0..d7 at Delta = 0, for S . p = the plane point (U, V)"""
    rng = np.random.default_rng(6)
    for _ in range(5):
        S = np.eye(3) + rng.normal(0, [[.05, .05, 5], [.05, .05, 5], [1e-3, 1e-3, 0]])
        p = np.array([rng.uniform(0, 60), rng.uniform(0, 40), 1.0])
        P = np.dot(S, p)
        U, V = P[0] / P[2], P[1] / P[2]
        Ju, Jv = GC.jacobian(U, V)
        for k in range(8):
            h = 1e-6
            out = []
            for sgn in (1, -1):
                D = np.eye(3)
                D.reshape(-1)[k] += sgn * h
                Q = np.dot(D, P)
                out.append((Q[0] / Q[2], Q[1] / Q[2]))
            assert abs((out[0][0] - out[1][0]) / (2 * h) - Ju[0, k]) <= 1e-6 * max(1, abs(Ju[0, k])), k
            assert abs((out[0][1] - out[1][1]) / (2 * h) - Jv[0, k]) <= 1e-6 * max(1, abs(Jv[0, k])), k


def test_the_two_paths_of_the_restatement_agree():
    fam = GC.family("plain", 3)
    a = GC.normal(fam["S"], fam["edges"], fam["rows"], fam["counts"], None, fam["H_edge"], 1.0, 0.5, exact=True)
    b = GC.normal(fam["S"], fam["edges"], fam["rows"], fam["counts"], None, fam["H_edge"], 1.0, 0.5, exact=False)
    assert np.array_equal(a[1], b[1]) and a[1][:, 1].sum() > 0 and a[1][9].tolist()[:1] != [320]     # the gate drops some rows
    # the plain path does not fuse the plane points' multiply-add: U may differ in its last bit, a residual of 0.4 px at U = 300 by
    # 1e-13 of itself; the sums agree to 1e-10 of their absolute terms, which is all the solver runs need
    assert (np.abs(a[0] - b[0]) <= 1e-10 * a[2]).all()
    assert a[1][0].tolist() == [0, 0, 0, 0] and not a[0][0].any() and not a[0][11].any()                # counts 0 and -3
    assert a[1][10, :3].sum() == 320                                                                    # 400 is taken as the capacity
    sums = a[0][9]
    for base in (0, 36):                                      # structure: the u and the v rows do not meet, [2][2] = [5][5] = sum w
        A = np.zeros((8, 8))
        A[np.triu_indices(8)] = sums[base:base + 36]
        assert not A[:3, 3:6].any() and A[2, 2] == A[5, 5] > 0
    assert sums[152] <= sums[153] and sums[153] > 0          # Huber never exceeds the squares


# ---- assembly and models ---------------------------------------------------------------------------------------------------------------
def test_assemble_on_scripted_blocks():
    from evenvizion_amd import graph
    rng = np.random.default_rng(9)
    sums = rng.normal(0, 1, (4, 154))
    edges = [(1, 0), (2, 1), (2, 0), (0, 2)]
    A, g = graph.assemble(sums, edges, 3)
    A2, g2 = GC.assemble(sums, edges, 3)
    assert np.allclose(A, A2, rtol=0, atol=1e-12) and np.allclose(g, g2, rtol=0, atol=1e-12) and np.array_equal(A, A.T)
    one = np.zeros((1, 154))
    one[0, 72 + 8 * 2 + 5] = 7.0                              # A_ij[2][5] of edge (1, 0)
    one[0, 5] = 3.0                                           # A_ii[0][5]
    one[0, 36 + 35] = 2.0                                     # A_jj[7][7]
    one[0, 136 + 4], one[0, 144 + 6] = 11.0, 13.0
    A, g = graph.assemble(one, [(1, 0)], 2)
    assert A[8 + 2, 5] == A[5, 8 + 2] == 7.0 and A[8, 8 + 5] == A[8 + 5, 8] == 3.0 and A[7, 7] == 2.0
    assert g[8 + 4] == 11.0 and g[6] == 13.0 and np.count_nonzero(A) == 5 and np.count_nonzero(g) == 2
    A, g = graph.assemble(np.ones((3, 154)), [(0, 0), (-1, 1), (1, 2)], 2)       # what the device flags adds nothing
    assert not A.any() and not g.any()


def test_basis_holds_the_four_models():
    from evenvizion_amd.graph import BASIS, MODELS
    assert tuple(BASIS) == MODELS and [BASIS[m].shape for m in MODELS] == [(8, 2), (8, 4), (8, 6), (8, 8)]
    delta = lambda x: np.concatenate([x, [0.0]]).reshape(3, 3)
    assert np.array_equal(delta(np.dot(BASIS["translation"], [3.0, 4.0])), [[0, 0, 3], [0, 0, 4], [0, 0, 0]])
    assert np.array_equal(delta(np.dot(BASIS["similarity"], [.1, .2, 3.0, 4.0])), [[.1, -.2, 3], [.2, .1, 4], [0, 0, 0]])
    assert np.array_equal(delta(np.dot(BASIS["affine"], np.arange(1.0, 7))), [[1, 2, 3], [4, 5, 6], [0, 0, 0]])
    assert np.array_equal(BASIS["homography"], np.eye(8))


# ---- the solver on the loop --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loop():
    from evenvizion_amd import graph
    truth, given = GC.loop_path()
    sup, ri = {k + 1: m for k, m in enumerate(given)}, {"w": W, "h": H}
    edges, loops = graph.loop_candidates(sup, ri, min_gap=2, max_partners=6)
    N, scale = graph.plane_normalisation(sup, ri)
    return truth, given, edges, N


def solve(loop, model, edges, noise=0.0, seed=0, iters=10):
    from evenvizion_amd import graph
    truth, given, _, N = loop
    rows, counts = GC.loop_rows(truth, edges, noise, seed)
    ev = graph.evaluator(lambda S: GC.normal(S, edges, rows, counts, exact=False), edges)
    got, rep = graph.solve_graph(given, ev, model, iters, 0, N)
    return GC.loop_errors(got, truth), rep, got


@pytest.mark.parametrize("model", ["translation", "similarity", "affine", "homography"])
def test_the_loop_closes(loop, model):
    """Integer translations and integer grid points: the rows are exact in float32 and the truth has cost exactly 0.  From the
    dictionary that is 0.25 px per pair off, 10 steps end within 1e-6 px at every corner of every frame: a zero-residual problem
    converges quadratically (measured: 1e-14 px)."""
    truth, given, edges, _ = loop
    e0 = GC.loop_errors(given, truth)
    assert abs(np.mean(e0) - 1.875) <= 1e-12 and abs(e0[-1] - 3.75) <= 1e-12
    e, rep, got = solve(loop, model, edges)
    print("%s: %d edges, worst corner %.3g px, cost %.3g -> %.3g in %d accepted steps" % (model, len(edges), max(e), rep["cost_before"],
                                                                                      rep["cost_after"], rep["accepted"]))
    assert max(e) <= 1e-6 and rep["cost_after"] < rep["cost_before"] and np.abs(got[0] - given[0]).max() <= 1e-12
    assert rep["accepted"] <= rep["steps"] <= 10


@pytest.mark.parametrize("seed", [7, 8])
@pytest.mark.parametrize("model", ["translation", "similarity", "affine", "homography"])
def test_loop_edges_beat_the_chain_under_noise(loop, model, seed):
    """0.05 px of Gaussian noise on both points: the mean corner error with the loop edges lies below that with the consecutive
    edges alone, and below the dictionary's 1.875 px.  Measured (loop / consecutive): homography 0.083 / 0.436 and 0.090 / 0.259 px,
    translation 0.003 / 0.010 and 0.005 / 0.035 px for seeds 7 and 8."""
    truth, given, edges, _ = loop
    chain = [e for e in edges if e[0] - e[1] == 1]
    assert len(chain) == 15 and len(edges) > 40
    with_loops, rep, _ = solve(loop, model, edges, 0.05, seed)
    without, _, _ = solve(loop, model, chain, 0.05, seed)
    print("%s, seed %d: mean corner error %.4f px with %d edges, %.4f px with the 15 consecutive ones" % (model, seed, np.mean(with_loops),
                                                                                                     len(edges), np.mean(without)))
    assert np.mean(with_loops) < np.mean(without) < 1.875 and rep["cost_after"] <= rep["cost_before"]


def test_the_cost_never_rises_and_zero_steps_change_nothing(loop):
    from evenvizion_amd import graph
    truth, given, edges, N = loop
    rows, counts = GC.loop_rows(truth, edges, 0.05, 7)
    costs = []

    def normal(S):
        out = GC.normal(S, edges, rows, counts, huber_delta=0.02, exact=False)
        costs.append(out[0][:, 152].sum())
        return out
    got, rep = graph.solve_graph(given, graph.evaluator(normal, edges), "affine", 6, 0, N)
    assert rep["evaluations"] == len(costs) and rep["cost_after"] == min(costs) < costs[0] == rep["cost_before"]
    same, rep0 = graph.solve_graph(given, graph.evaluator(normal, edges), "affine", 0, 0, N)
    assert np.array_equal(same, np.stack(given)) and rep0["steps"] == 0
    for bad in (dict(model="rigid"), dict(iters=-1), dict(iters=2.5), dict(fixed=16)):
        with pytest.raises(ValueError):
            graph.solve_graph(given, None, **bad)
    other, _ = graph.solve_graph(given, graph.evaluator(normal, edges), "translation", 4, 15, N)   # another gauge: frame 15 is held
    assert np.abs(other[15] - given[15]).max() <= 1e-12 and np.abs(other[0] - given[0]).max() > 1.0


# ---- the choice of edges ---------------------------------------------------------------------------------------------------------------
def test_loop_candidates_on_the_path():
    from evenvizion_amd import graph
    truth, given = GC.loop_path()
    sup, ri = {k + 1: m for k, m in enumerate(truth)}, {"w": W, "h": H}
    off = [m[0, 2] for m in truth]
    overlap = lambda i, j: max(0.0, W - abs(off[i] - off[j])) / W
    assert abs(graph.footprint_overlap(truth[15], truth[2], W, H) - overlap(15, 2)) <= 1e-12
    assert graph.footprint_overlap(truth[0], GC.translation(200.0), W, H) == 0.0
    assert graph.footprint_overlap(truth[0], np.full((3, 3), np.nan), W, H) == 0.0
    edges, loops = graph.loop_candidates(sup, ri)                            # min_gap 8, min_overlap 0.3, max_partners 4
    assert edges[:15] == [(k, k - 1) for k in range(1, 16)]
    for i, js in loops.items():
        assert all(j < i - 8 and overlap(i, j) >= 0.3 for j in js) and len(js) <= 4
        assert all(abs(a - b) >= 8 for a in js for b in js if a != b)
        best = max(range(0, i - 8), key=lambda j: (overlap(i, j), -j))
        assert js[0] == best
    assert loops[15] == [0] and loops[14][0] == 1 and loops[9] == [0] and sorted(loops) == [9, 10, 11, 12, 13, 14, 15]
    assert edges[15:] == [(i, j) for i in sorted(loops) for j in loops[i]]
    edges, loops = graph.loop_candidates(sup, ri, min_gap=2, max_partners=2)
    assert all(len(js) <= 2 for js in loops.values()) and loops[15] == [0, 2] and loops[3] == [0]
    assert graph.loop_candidates(sup, ri, min_gap=2, min_overlap=0.95)[1] == {15: [0], 14: [1], 13: [2], 12: [3], 11: [4], 10: [5], 9: [6]}
    assert graph.loop_candidates(sup, ri, max_partners=0)[1] == {}
    for bad in (dict(min_gap=0), dict(min_gap=1.5), dict(max_partners=-1), dict(min_overlap=0), dict(min_overlap=1.5)):
        with pytest.raises(ValueError):
            graph.loop_candidates(sup, ri, **bad)


def test_disconnected_graphs_and_min_inliers():
    from evenvizion_amd import graph
    graph.check_connected([(1, 0), (2, 1), (3, 0)], 4)
    with pytest.raises(ValueError, match="do not connect 2 of the 5 node frames to frame 0"):
        graph.check_connected([(1, 0), (2, 1), (4, 3)], 5)
    with pytest.raises(ValueError, match="node 0"):
        graph.check_connected([(1, 0), (2, 1)], 4, fixed=3)
    info = np.array([[25, 3, 0, 0], [19, 0, 0, 0], [20, 0, 0, 0], [90, 0, 0, 2], [90, 0, 0, 0], [90, 0, 0, 1]])
    status = np.array([0, 0, 0, 0, 4, 0])
    assert graph.keep_edges(status, info, 20).tolist() == [True, False, True, False, False, False]
    assert graph.keep_edges(status, info, 26).tolist() == [False] * 6


def test_frames_between_nodes_follow_the_node_before_them():
    from evenvizion_amd import graph
    S = np.stack([GC.translation(3.0 * k) for k in range(7)])
    S[4] = np.nan
    nodes = [0, 3, 6]
    moved = [S[0], np.dot(GC.translation(0.5, 1.0), S[3]), np.dot(GC.translation(-2.0), S[6])]
    out = graph.spread_corrections(S, nodes, moved)
    want = [0, 3, 6, 9.5, None, 15.5, 16]
    for k, x in enumerate(want):
        if x is None:
            assert np.isnan(out[k]).all()
        else:
            assert np.abs(out[k] - GC.translation(x, 1.0 if k in (3, 5) else 0.0)).max() <= 1e-12, k


class NeverRead:
    def __getattr__(self, name):
        raise AssertionError("the capture was touched: %s" % name)


@pytest.mark.parametrize("bad", [dict(model="rigid"), dict(iters=-1), dict(stride=0), dict(stride=1.5), dict(min_inliers=0), dict(ingest="rgb"),
                                 dict(inlier_thr=-1.0), dict(huber_delta=float("nan")), dict(fixed=2), dict(min_gap=0),
                                 dict(resize_info={"w": 0, "h": 4}), dict(resize_info={"w": 40000, "h": 30000})])
def test_the_driver_refuses_before_anything_is_opened(bad, monkeypatch):
    from evenvizion_amd import graph, runtime

    def no_context(*a, **k):
        raise AssertionError("a context was opened")

    monkeypatch.setattr(runtime, "get_context", no_context)
    kw = dict(resize_info={"w": 8, "h": 4})
    kw.update(bad)
    ri = kw.pop("resize_info")
    sup = {1: np.eye(3), 2: np.eye(3)}
    with pytest.raises(ValueError, match="stride" if ri["w"] == 40000 else None):
        graph.align_superposition(NeverRead(), sup, ri, **kw)


def test_too_many_nodes_and_a_cost_that_is_not_finite_are_refused():
    from evenvizion_amd import graph
    sup = {k + 1: GC.translation(float(k)) for k in range(2 * graph.MAX_NODES + 1)}
    with pytest.raises(ValueError, match="stride = 2 makes 513 node frames"):
        graph.align_superposition(NeverRead(), sup, {"w": 8, "h": 4}, stride=2)
    truth, given = GC.loop_path()
    edges = [(k, k - 1) for k in range(1, 16)]
    rows, counts = GC.loop_rows(truth, edges)
    bad = np.stack(given)
    bad[5, 2, 2] = 1e-320                                      # tw is finite and positive: the rows are used, and U = x / tw overflows
    with pytest.raises(ValueError, match="not finite"):
        graph.solve_graph(bad, graph.evaluator(lambda S: GC.normal(S, edges, rows, counts, exact=False), edges))


def test_command_line_takes_the_flags():
    from evenvizion_amd import component
    args = component.parser().parse_args([])
    assert args.global_align == 0 and args.graph_model == "homography" and args.graph_partners == 4 and args.graph_gap == 8
    assert args.graph_min_inliers == 20 and component.parser().parse_args(["--graph_min_inliers", "8"]).graph_min_inliers == 8
    args = component.parser().parse_args(["--global_align", "1", "--graph_model", "affine", "--graph_partners", "2", "--graph_gap", "5"])
    assert (args.global_align, args.graph_model, args.graph_partners, args.graph_gap) == (1, "affine", 2, 5)
    with pytest.raises(SystemExit):
        component.parser().parse_args(["--graph_model", "rigid"])
    with pytest.raises(ValueError, match="one video"):
        component.main(["--path_to_videos", "a.npy", "b.npy", "--global_align", "1"])


# ---- the header ------------------------------------------------------------------------------------------------------------------------
def test_header_library_and_signature_table_declare_the_entry():
    from evenvizion_amd import _lib, graph
    text = open(os.path.join(ROOT, "include", "evhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint evh_graph_normal\s*\(", code) and "evh_graph_normal" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["evh_graph_normal"][1]) == 14 and hasattr(_lib.Context, "graph_normal")
    assert re.search(r"EVH_GRAPH_NSUMS = 154\b", code) and re.search(r"EVH_GRAPH_BAD_INDEX = 1, EVH_GRAPH_BAD_STATUS = 2\b", code)
    assert (_lib.GRAPH_NSUMS, _lib.GRAPH_BAD_INDEX, _lib.GRAPH_BAD_STATUS) == (154, 1, 2) == (GC.NSUMS, GC.BAD_INDEX, GC.BAD_STATUS)
    assert graph.NSUMS == 154 and _lib.GRAPH_INFO == ("used", "gated", "behind", "flags")
    _lib.build()
    assert hasattr(_lib.load(), "evh_graph_normal")
