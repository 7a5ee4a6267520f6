"""GPU: the three f64 glue kernels behind the example script's outputs, bit for bit against the reference's own
arithmetic (tests/golden/plane_goldens.json, captured by tests/golden/make_plane_goldens.py) and the CPU oracle:
    evh_fixed_plane_field   heat-map field + np.max   (metrics_file.txt, heatmap.max_movement)
    evh_superposition_scan  utils.superposition_dict
    evh_transform_points    np.around(homography_transformation(...))   (fixed_coordinates.json)
Run with: python -m pytest tests -m gpu   (on the MI355X box)."""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import oracle as O  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIELD_BUDGET = 1 << 30          # bytes of device field a case may request (n * h * w * 2 * 8)
ORACLE_BUDGET = 2_000_000_000   # pixel evaluations the oracle does per case; above it, a sample of frames is checked


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU; there is no CPU fallback")
    from evenvizion_amd._lib import Context
    c = Context(device=0, max_w=64, max_h=64, max_features=500, max_frames=2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def plane():
    with open(os.path.join(GOLD, "plane_goldens.json")) as f:
        return json.load(f)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float64).tobytes()).hexdigest()


def same_bits(got, want):
    """Bit equality of f64 arrays, except that any NaN equals any NaN (the sign and payload of 0/0 are not pinned)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got[~gn].view(np.int64), want[~wn].view(np.int64)))


def device_field(ctx, Hs, w, h, with_field=True):
    """(field f64[n,h,w,2] on the host or None, maxima f64[n]) from evh_fixed_plane_field."""
    Hs = np.ascontiguousarray(Hs, np.float64).reshape(-1, 3, 3)
    if not with_field:
        return None, ctx.fixed_plane_max(Hs, w, h)
    f = torch.empty(len(Hs), h, w, 2, dtype=torch.float64, device="cuda")
    m = ctx.fixed_plane_max(Hs, w, h, field=f)
    return f.cpu().numpy(), m


# ---- heat-map field -------------------------------------------------------------------------------------------------

def test_reference_video_every_frame(ctx, plane):
    """All 121 superposed matrices of the reference video: per-frame np.max and sha256 of the whole 224 x 400 x 2
    field equal the reference's np.apply_along_axis(homography_transformation), frame by frame."""
    fr = plane["video"]["frames"]
    Hs = np.array([f["H"] for f in fr]).reshape(-1, 3, 3)
    field, m = device_field(ctx, Hs, 400, 224)
    bad_max = [f["frame"] for i, f in enumerate(fr) if m[i] != f["max"]]
    bad_field = [f["frame"] for i, f in enumerate(fr) if _sha(field[i]) != f["field_sha256"]]
    assert bad_max == [] and bad_field == [], "frames whose max / field differ from the reference: %s / %s" % (bad_max, bad_field)
    assert np.array_equal(device_field(ctx, Hs, 400, 224, with_field=False)[1], m)


def test_max_movement_is_the_reference_return_value(plane):
    """heatmap.max_movement on the reference's superposed dict == heatmap_video_processing's recorded return."""
    from evenvizion_amd import heatmap, runtime
    fr = plane["video"]["frames"]
    sup = {f["frame"]: np.array(f["H"]).reshape(3, 3) for f in fr}
    runtime.reset()
    try:
        keys, m = heatmap.frame_maxima(sup, plane["video"]["resize_info"])
        assert keys == [f["frame"] for f in fr] and m.tolist() == [f["max"] for f in fr]
        assert heatmap.max_movement(sup, plane["video"]["resize_info"]) == plane["video"]["heatmap_video_processing"] \
            == 863.0428982580879
    finally:
        runtime.reset()


def test_synthetic_grids_whole_field(ctx, plane):
    """1x1 .. 65x5 grids: horizons crossing the grid, d = 0 (+/-inf and 0/0), overflow, negative maxima, an all -inf
    field (np.max = -inf) and fields with a NaN (np.max = NaN); field and max bit for bit, with and without the field."""
    by_grid = {}
    for c in plane["grids"]:
        by_grid.setdefault((c["w"], c["h"]), []).append(c)
    bad = []
    for (w, h), cases in by_grid.items():
        Hs = np.array([c["H"] for c in cases])
        field, m = device_field(ctx, Hs, w, h)
        _, m2 = device_field(ctx, Hs, w, h, with_field=False)
        for i, c in enumerate(cases):
            if not same_bits(field[i], np.array(c["field"]).reshape(h, w, 2)):
                bad.append(("field", w, h, c["name"]))
            if not (same_bits(m[i], c["max"]) and same_bits(m2[i], c["max"])):
                bad.append(("max", w, h, c["name"], float(m[i]), float(m2[i]), c["max"]))
    assert bad == []


def _matrices(n, rng):
    """n superposed-looking matrices (a random near-identity chain) with the edge matrices spliced in."""
    steps = np.eye(3) + rng.normal(0, 1, (n, 3, 3)) * np.array([[3e-3, 3e-3, 2.0], [3e-3, 3e-3, 2.0], [3e-6, 3e-6, 0]])
    Hs = np.array(O.superposition_chain(list(steps)))
    at = np.zeros(0, np.int64)
    if n >= 7:
        special = [[[1, 0, 0], [0, 1, 0], [0, 0, 0]],          # NaN at (0, 0), +inf elsewhere
                   [[0, 0, -1], [0, 0, -1], [0, 0, 0]],        # all -inf
                   [[1, 0, 1], [0, -1, -1], [0, 0, 0]],        # +/-inf
                   [[-1, 0, -10], [0, -1, -20], [0, 0, 1]],    # negative maximum
                   [[1, 0, 0], [0, 1, 0], [-1e-3, 5e-4, 1]]]   # horizon inside the larger grids
        at = rng.choice(n, len(special), replace=False)
        Hs[at] = np.array(special, np.float64)
    return Hs, at


@pytest.mark.parametrize("w,h", [(1, 1), (255, 1), (257, 3), (400, 224), (1280, 720), (3840, 2160)])
@pytest.mark.parametrize("n", [1, 7, 121, 2000])
def test_field_sizes_vs_oracle(ctx, w, h, n):
    """Grid sizes from one pixel to 4K (more than 1024 blocks x 256 threads: the grid-stride loop runs) and up to
    2000 matrices per call; the field where it fits in FIELD_BUDGET, maxima otherwise, against the oracle."""
    rng = np.random.default_rng(w * 7919 + h * 31 + n)
    Hs, special = _matrices(n, rng)
    with_field = n * h * w * 16 <= FIELD_BUDGET
    field, m = device_field(ctx, Hs, w, h, with_field)
    if n * w * h <= ORACLE_BUDGET:
        check = np.arange(n)
    else:
        check = np.unique(np.concatenate([[0, n - 1], special, rng.choice(n, 12, replace=False)]))
    if with_field:
        for i in check:
            want_field, want_max = O.fixed_plane_field(Hs[i], w, h)
            assert same_bits(m[i], want_max[0]), (i, m[i], want_max[0])
            assert same_bits(field[i], want_field[0]), i
    else:
        _, want_max = O.fixed_plane_field(Hs[check], w, h, want_field=False)
        assert same_bits(m[check], want_max), check[~np.array([same_bits(a, b) for a, b in zip(m[check], want_max)])]
    if with_field:
        assert np.array_equal(device_field(ctx, Hs, w, h, with_field=False)[1].view(np.int64), m.view(np.int64))
    if n >= 7:
        assert np.isnan(m).sum() >= 1 and (m == -np.inf).sum() >= 1


def test_field_capacity_is_refused(ctx):
    """w * h above INT_MAX is refused before anything is launched; the field tensor must match n * h * w * 2."""
    from evenvizion_amd._lib import EvhError
    with pytest.raises(EvhError, match="INT_MAX"):
        ctx.fixed_plane_max(np.eye(3)[None], 65536, 32768)
    with pytest.raises(ValueError):
        ctx.fixed_plane_max(np.eye(3)[None], 8, 8, field=torch.empty(1, 8, 7, 2, dtype=torch.float64, device="cuda"))
    assert ctx.fixed_plane_max(np.eye(3)[None], 46340, 1).tolist() == [46339.0]   # the context is still usable


# ---- superposition scan --------------------------------------------------------------------------------------------

def test_superposition_chain_reference(ctx, plane):
    """The 2000-step chain the reference superposed: sampled steps and the last one, bit for bit."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_plane_goldens", os.path.join(GOLD, "make_plane_goldens.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    c = plane["superposition"]["chain"]
    Hs = mod.chain_inputs(c["n"], c["seed"])
    assert _sha(Hs) == c["inputs_sha256"]
    got = ctx.superposition_scan(Hs)
    for i, want in zip(c["samples"], c["sup"]):
        assert np.array_equal(got[i].ravel(), np.array(want)), i
    assert np.array_equal(got[-1].ravel(), np.array(c["last"]))


def test_superposition_dict_with_none(plane):
    """utils.superposition_dict (the mirror) with None H in the middle and at the end, as the reference records them."""
    import importlib.util
    from evenvizion_amd import runtime
    from evenvizion_amd.processing import utils
    spec = importlib.util.spec_from_file_location("make_plane_goldens", os.path.join(GOLD, "make_plane_goldens.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    Hs = mod.chain_inputs()
    try:
        for nc in plane["superposition"]["none_chains"]:
            d = {k + 2: {"H": None if p < 0 else Hs[p]} for k, p in enumerate(nc["pattern"])}
            got = utils.superposition_dict(d)
            assert [str(k) for k in got] == list(nc["sup"])
            for k, v in got.items():
                assert np.array_equal(np.asarray(v, np.float64).ravel(), np.array(nc["sup"][str(k)])), (nc["pattern"], k)
    finally:
        runtime.reset()


@pytest.mark.parametrize("n", [1, 2, 3, 65, 2000, 20000])
def test_superposition_scan_vs_oracle(ctx, n):
    rng = np.random.default_rng(n)
    Hs = np.eye(3) + rng.normal(0, 1, (n, 3, 3)) * np.array([[3e-3, 3e-3, 2.0], [3e-3, 3e-3, 2.0], [3e-6, 3e-6, 3e-3]])
    got = ctx.superposition_scan(Hs)
    want = np.array(O.superposition_chain(list(Hs)))
    bad = np.nonzero(~np.all(got.reshape(n, 9).view(np.int64) == want.reshape(n, 9).view(np.int64), axis=1))[0]
    assert bad.size == 0, "first differing step %d of %d" % (bad[0], n)


# ---- point transforms ----------------------------------------------------------------------------------------------

def test_transform_points_around_reference(ctx, plane):
    """np.around(homography_transformation(...), decimals) as the reference computes it: half-way values at decimals
    0, 1, 2, 8, 15, w = 0, the 1170 <-> 400 coefficients and inverse matrices -- one call for every case of a
    (kx, ky, decimals), each point on its own matrix."""
    groups = {}
    for c in plane["around"]:
        groups.setdefault((c["kx"], c["ky"], c["decimals"]), []).append(c)
    for (kx, ky, dec), cases in groups.items():
        mats, idx, pts, want = [], [], [], []
        for j, c in enumerate(cases):
            p = np.array(c["pts"]).reshape(-1, 2)
            mats.append(np.array(c["M"]).reshape(3, 3)); pts.append(p); idx += [j] * len(p)
            want.append(np.array(c["out"]).reshape(-1, 2))
        got = ctx.transform_points(np.array(mats), np.array(idx, np.int32), np.concatenate(pts), kx, ky, dec)
        assert same_bits(got, np.concatenate(want)), (kx, ky, dec)


def test_fixed_coordinates_reference(plane):
    """fixed_coordinate_system (the mirror) on the recorded coordinate dict: to the fixed plane and back."""
    from evenvizion_amd import runtime
    from evenvizion_amd.processing import fixed_coordinate_system as fcs, utils
    g = plane["fixed_coordinates"]
    hd, _ = utils.read_homography_dict(os.path.join(GOLD, "ref_dict_with_homography_matrix.json"))
    try:
        sup = utils.superposition_dict(hd)
        orig = {int(k): [{"x1": x, "y1": y} for x, y in v] for k, v in g["original"].items()}
        fx = fcs.from_original_to_fix(orig, sup, g["original_shape"], g["resize_shape"])
        back = fcs.from_fix_to_original(fx, sup, g["original_shape"], g["resize_shape"])
        for k in orig:
            assert [[float(r["x1"]), float(r["y1"])] for r in fx[k]] == g["fixed"][str(k)], k
            assert [[float(r["x1"]), float(r["y1"])] for r in back[k]] == g["back"][str(k)], k
    finally:
        runtime.reset()


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 100000])
def test_transform_points_vs_oracle(ctx, n):
    """Many points over up to 4096 matrices picked at random, every decimals form, w = 0 rows included."""
    rng = np.random.default_rng(1000 + n)
    nmat = int(min(4096, max(1, n)))
    mats = np.eye(3) + rng.normal(0, 1, (nmat, 3, 3)) * np.array([[3e-2, 3e-2, 20.], [3e-2, 3e-2, 20.], [3e-5, 3e-5, 0]])
    mats[: nmat // 8] = np.linalg.inv(mats[: nmat // 8])
    if nmat >= 2:
        mats[1] = [[1.0, 0.0, -5.0], [0.0, 1.0, 0.0], [1.0, 0.0, -5.0]]           # w = 0 on the line x = 5
    idx = rng.integers(0, nmat, n).astype(np.int32)
    pts = rng.uniform(0, 1170, (n, 2))
    half = rng.random(n) < 0.25                       # exact binary halves: the rounding ties of np.around
    pts[half] = rng.integers(-4000, 4000, (int(half.sum()), 2)) / 8.0
    if n >= 2:
        idx[: n // 16 + 1] = 1; pts[: n // 16 + 1, 0] = 5.0
    for kx, ky in ((1.0, 1.0), (400 / 1170, 224 / 658), (1170 / 400, 658 / 224)):
        for dec in (-1, 0, 1, 2, 8, 15):
            got = ctx.transform_points(mats, idx, pts, kx, ky, dec)
            want = O.transform_points(mats, idx, pts, kx, ky, dec)
            assert got.shape == (n, 2) and same_bits(got, want), (kx, ky, dec)
