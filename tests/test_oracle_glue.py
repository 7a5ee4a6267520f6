"""Oracle (oracle/) vs the golden vectors captured from the reference's own Python glue
(tests/golden/make_glue_goldens.py) and the reference's known-answer artefact (metrics_file.txt)."""
import json
import os

import numpy as np
import pytest

from oracle import oracle as O

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_lowes_ratio_and_unique_filter(goldens):
    for c in goldens["lowes_ratio_test"]:
        q, t = O.ratio_unique(np.array(c["idx"]), np.array(c["d2"]), c["ratio"])
        got = [[int(a), int(b)] for a, b in zip(t, q)]   # reference tuples are (trainIdx, queryIdx)
        assert got == c["matches"]


def test_ratio_half_equals_integer_test():
    # d0 < 0.5*d1 on f32 square roots  <=>  4*D0 < D1 in integers
    rng = np.random.default_rng(1)
    D0 = rng.integers(0, 520200, 20000); D1 = np.maximum(D0, rng.integers(0, 2080800, 20000))
    D1[:5000] = 4 * D0[:5000] + rng.integers(-1, 2, 5000)
    D1 = np.clip(D1, D0, 2080800)
    idx = np.tile(np.array([[0, 1]]), (len(D0), 1)); idx[:, 0] = np.arange(len(D0))  # all trains distinct
    q, _ = O.ratio_unique(idx, np.stack([D0, D1], 1), 0.5)
    want = np.nonzero(4 * D0 < D1)[0]
    assert np.array_equal(q, want)


def test_remove_double_matching(goldens):
    for c in goldens["remove_double_matching"]:
        a, b = O.remove_double(c["a"], c["b"])
        assert np.array_equal(a, np.float32(c["out_a"]).reshape(-1, 2))
        assert np.array_equal(b, np.float32(c["out_b"]).reshape(-1, 2))


def test_static_filter(goldens):
    for c in goldens["static_filter"]:
        a, b = O.static_filter(c["H"], c["a"], c["b"])
        assert np.array_equal(a, np.float32(c["out_a"]).reshape(-1, 2))
        assert np.array_equal(b, np.float32(c["out_b"]).reshape(-1, 2))


def test_matrix_superposition(goldens):
    for c in goldens["matrix_superposition"]:
        assert np.array_equal(O.matrix_superposition(c["H"], c["S"], False), np.array(c["sup_false"]))
        assert np.array_equal(O.matrix_superposition(c["H"], c["S"], True), np.array(c["sup_true"]))


def test_kat_f12_metrics_file(goldens):
    """The reference's only numeric artefact: metrics_file.txt == max fixed-plane coordinate over the example
    video, recomputed here from the committed golden H JSON through the oracle's matrix_superposition."""
    want = float(open(os.path.join(GOLD, "ref_metrics_file.txt")).read().split(":")[1])
    assert want == 863.0428982580879
    d = json.load(open(os.path.join(GOLD, "ref_dict_with_homography_matrix.json")))
    ri = d.pop("resize_info")
    assert ri == {"h": 224, "w": 400} and len(d) == 120
    ys, xs = np.mgrid[0:ri["h"], 0:ri["w"]].astype(np.float64)
    sup, first, maxima = None, True, [float(max(xs.max(), ys.max()))]   # frame 1: identity
    for k in sorted(d, key=int):
        sup = O.matrix_superposition(np.array(d[k]["H"]), sup, first)
        first = False
        den = sup[2, 0] * xs + sup[2, 1] * ys + sup[2, 2]
        u = (sup[0, 0] * xs + sup[0, 1] * ys + sup[0, 2]) / den
        v = (sup[1, 0] * xs + sup[1, 1] * ys + sup[1, 2]) / den
        maxima.append(float(max(u.max(), v.max())))
    assert np.array_equal(sup, np.array(goldens["kat_f12"]["sup_last"]))
    # the reference skips the append for the last frame (processing_visualization.py:414-418)
    assert max(maxima[:-1]) == want
    assert max(maxima) == goldens["kat_f12"]["max_including_last"]


def test_compute_homography_pretransform_and_gate(goldens, monkeypatch):
    for c in goldens["compute_homography"]:
        a = np.float32(c["a"]); b = np.float32(c["b"])
        if c["Hsup"] is not None:
            Hs = np.array(c["Hsup"])
            # the oracle pre-transforms in f64 and hands f32 to findHomography (cv2 converts to CV_32F)
            pa = np.float32(c["passed_a"]); pb = np.float32(c["passed_b"])
            st, H = O.compute_homography(a, b, Hs)
            st2, H2 = O.compute_homography(pa, pb, None)
            assert st == st2 and np.array_equal(H, H2)
        else:
            assert np.array_equal(np.float32(c["passed_a"]), a)
        assert c["thr"] == 3.0 and c["method"] == 8


# ---- heat-map field, superposition chain, point transforms: plane_goldens.json (tests/golden/make_plane_goldens.py) ----

def _plane_goldens():
    with open(os.path.join(GOLD, "plane_goldens.json")) as f:
        return json.load(f)


def _chain_inputs():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_plane_goldens", os.path.join(GOLD, "make_plane_goldens.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.chain_inputs


def _sha(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a, np.float64).tobytes()).hexdigest()


def same_bits(got, want):
    """Bit equality of f64 arrays, except that any NaN equals any NaN (the sign and payload of 0/0 are not pinned)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got[~gn].view(np.int64), want[~wn].view(np.int64)))


def test_plane_field_reference_video():
    """Every superposed matrix of the reference video: the oracle's field hashes and maxima equal those of the
    reference's np.apply_along_axis(homography_transformation) + np.max, and heatmap_video_processing's returned
    value is the maximum over all frames but the last."""
    g = _plane_goldens()["video"]
    fr = g["frames"]
    assert len(fr) == 121 and [f["frame"] for f in fr] == list(range(1, 122))
    Hs = np.array([f["H"] for f in fr]).reshape(-1, 3, 3)
    field, mx = O.fixed_plane_field(Hs, 400, 224)
    assert [i for i in range(len(fr)) if mx[i] != fr[i]["max"]] == []
    assert [i for i in range(len(fr)) if _sha(field[i]) != fr[i]["field_sha256"]] == []
    assert g["heatmap_video_processing"] == g["max_excluding_last"] == float(np.max(mx[:-1])) == 863.0428982580879
    _, mx2 = O.fixed_plane_field(Hs, 400, 224, want_field=False, threads=1)
    assert np.array_equal(mx, mx2)


def test_plane_field_edges():
    """Small grids, whole fields: horizons crossing the grid, d = 0 (+/-inf, 0/0 = NaN), overflow, negative maxima,
    an all -inf field (np.max = -inf) and a field with one NaN (np.max = NaN)."""
    grids = _plane_goldens()["grids"]
    names = {c["name"] for c in grids}
    assert {"nan", "all_neg_inf", "pm_inf", "horizon", "huge", "negative"} <= names
    seen = set()
    for c in grids:
        field, mx = O.fixed_plane_field(np.array(c["H"]), c["w"], c["h"])
        assert same_bits(field[0], np.array(c["field"]).reshape(c["h"], c["w"], 2)), (c["name"], c["w"], c["h"])
        assert same_bits(mx[0], c["max"]), (c["name"], c["w"], c["h"], mx[0], c["max"])
        seen.add("nan" if np.isnan(c["max"]) else "-inf" if c["max"] == -np.inf else "inf" if c["max"] == np.inf
                 else "neg" if c["max"] < 0 else "pos")
    assert seen == {"nan", "-inf", "inf", "neg", "pos"}


def test_superposition_chain_reference():
    s = _plane_goldens()["superposition"]
    c = s["chain"]
    Hs = _chain_inputs()(c["n"], c["seed"])
    assert _sha(Hs) == c["inputs_sha256"]                  # the regenerated inputs are the ones the reference saw
    sup = O.superposition_chain(list(Hs))
    for i, want in zip(c["samples"], c["sup"]):
        assert np.array_equal(sup[i].ravel(), np.array(want)), i
    assert np.array_equal(sup[-1].ravel(), np.array(c["last"]))
    for nc in s["none_chains"]:
        got = O.superposition_chain([None if p < 0 else Hs[p] for p in nc["pattern"]])
        want = nc["sup"]
        assert list(want) == [str(k) for k in range(1, len(got) + 2)]
        assert want["1"] == np.eye(3).ravel().tolist()
        for k, m in enumerate(got):
            assert np.array_equal(m.ravel(), np.array(want[str(k + 2)])), (nc["pattern"], k)
    assert s["first_none_exception"] == "TypeError"
    with pytest.raises(TypeError):
        O.superposition_chain([None, Hs[0]])


def test_transform_points_around_reference():
    """np.around(homography_transformation(...), decimals): half-way values at every decimals, w = 0, the
    1170 <-> 400 coefficients and inverse matrices."""
    cases = _plane_goldens()["around"]
    assert {c["decimals"] for c in cases} == {0, 1, 2, 8, 15} and any(c["inverse"] for c in cases)
    for c in cases:
        pts = np.array(c["pts"]).reshape(-1, 2)
        got = O.transform_points(np.array(c["M"]), np.zeros(len(pts), np.int32), pts, c["kx"], c["ky"], c["decimals"])
        assert same_bits(got, np.array(c["out"]).reshape(-1, 2)), c


def test_fixed_coordinates_reference():
    """from_original_to_fix / from_fix_to_original on whole coordinate dicts (both fixtures): H, or inv(H) for the
    way back, per frame, rounded to 2 decimals."""
    hd = json.load(open(os.path.join(GOLD, "ref_dict_with_homography_matrix.json")))
    hd.pop("resize_info")
    sup = O.superposition_chain([np.array(hd[k]["H"]) for k in sorted(hd, key=int)])
    sup = {1: np.eye(3), **{int(k): m for k, m in zip(sorted(hd, key=int), sup)}}
    pg = _plane_goldens()["fixed_coordinates"]
    gg = json.load(open(os.path.join(GOLD, "glue_goldens.json")))["fixed_coordinates"]
    as_xy = lambda rows: np.array([[r["x1"], r["y1"]] if isinstance(r, dict) else r for r in rows], np.float64)
    for g in (pg, gg):
        (oh, ow), (rh, rw) = g["original_shape"], g["resize_shape"]
        for k in g["original"]:
            M = sup[int(k)]
            orig, fixed, back = as_xy(g["original"][k]), as_xy(g["fixed"][k]), as_xy(g["back"][k])
            idx = np.zeros(len(orig), np.int32)
            assert np.array_equal(O.transform_points(M, idx, orig, rw / ow, rh / oh, 2), fixed), k
            assert np.array_equal(O.transform_points(np.linalg.inv(M), idx, fixed, ow / rw, oh / rh, 2), back), k


def test_hv_through_transform_points(goldens):
    """glue_goldens "hv": homography_transformation of a float32 point, unrounded."""
    for c in goldens["matrix_superposition"]:
        got = O.transform_points(np.array(c["H"]), [0], np.float32(c["v"]).astype(np.float64)[None], decimals=-1)
        assert got[0].tolist() == c["hv"]


def test_kat_f12_through_the_field_oracle(goldens):
    """metrics_file.txt from the committed H JSON through the oracle's chain and field, in the reference's order."""
    d = json.load(open(os.path.join(GOLD, "ref_dict_with_homography_matrix.json")))
    d.pop("resize_info")
    sup = [np.eye(3)] + O.superposition_chain([np.array(d[k]["H"]) for k in sorted(d, key=int)])
    assert np.array_equal(sup[-1], np.array(goldens["kat_f12"]["sup_last"]))
    _, mx = O.fixed_plane_field(np.array(sup), 400, 224, want_field=False)
    assert float(np.max(mx[:-1])) == goldens["kat_f12"]["max_excluding_last"] == 863.0428982580879
    assert float(np.max(mx)) == goldens["kat_f12"]["max_including_last"]
