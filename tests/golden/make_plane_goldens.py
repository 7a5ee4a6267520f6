#!/usr/bin/env python3
"""Capture golden vectors for the reference's heat-map field and point transforms by running the reference itself.

Runs ONLY where the reference checkout exists (see make_glue_goldens.REF); writes tests/golden/plane_goldens.json,
which travels with the repo.  Imports the reference with make_glue_goldens' inert cv2 / imutils stubs, so only its
numpy arithmetic executes:
    np.max(np.apply_along_axis(homography_transformation, 2, make_template(shape), H))
                                            (processing_visualization.py:347-365, 401-419; utils.py:71-92)
    heatmap_video_processing's returned value (the skip-last-frame rule; rendering patched out)
    utils.superposition_dict                (utils.py:118-145, 184-211)
    np.around(homography_transformation / inverse_homography_transformation, decimals)
    fixed_coordinate_system.from_original_to_fix / from_fix_to_original   (fixed_coordinate_system.py:56-69, 109-122)
Fixtures are data (inputs + expected outputs); no reference source text is stored.  Large inputs are not stored
either: they are regenerated from chain_inputs() (numpy's legacy RandomState, whose streams are frozen) and pinned
by a sha256 of their bytes.
"""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

SHAPE = (224, 400)                         # resize_info of the reference's example video (h, w)
GRIDS = [(1, 1), (1, 37), (37, 1), (17, 9), (65, 5)]  # (w, h) of the synthetic fields
# matrices whose fields hit the edges of np.max and of the arithmetic order (row-major 3x3)
SYNTH = {
    "perspective": [[1.01, 0.02, 3.5], [-0.01, 0.99, -2.25], [1e-4, -2e-4, 1.0]],
    "dense": [[0.9123456789, -0.3141592653, 17.123456789], [0.2718281828, 1.1414213562, -9.87654321],
              [3.3e-4, -1.7e-4, 0.9987654321]],
    "horizon": [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-0.1, 0.05, 1.0]],        # d = 0 at (10, 0), sign change
    "horizon_y": [[0.5, -0.25, 3.0], [0.125, 2.0, -1.0], [0.03, -0.4, 1.2]],  # d crosses zero between rows
    "huge": [[1e200, -3e199, 7.0], [2.0, 1e250, 0.0], [1e-100, 0.0, 1.0]],
    "negative": [[-1.0, 0.0, -10.0], [0.0, -1.0, -20.0], [0.0, 0.0, 1.0]],
    "nan": [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]],                # 0/0 at (0, 0), +inf elsewhere
    "all_neg_inf": [[0.0, 0.0, -1.0], [0.0, 0.0, -1.0], [0.0, 0.0, 0.0]],
    "pm_inf": [[1.0, 0.0, 1.0], [0.0, -1.0, -1.0], [0.0, 0.0, 0.0]],          # d = 0, numerators +/- non-zero
}
CHAIN_SEED, CHAIN_N = 20261016, 2000
CHAIN_SAMPLES = [0, 1, 2, 3, 7, 64, 65, 127, 255, 256, 511, 999, 1000, 1023, 1024, 1500, 1997, 1998, 1999]


def chain_inputs(n=CHAIN_N, seed=CHAIN_SEED):
    """The per-frame H of the random near-identity chain (f64[n,3,3]); shared with the tests."""
    rs = np.random.RandomState(seed)
    return np.eye(3) + rs.normal(0, 1, (n, 3, 3)) * np.array([[2e-3, 2e-3, 1.5], [2e-3, 2e-3, 1.5], [2e-6, 2e-6, 0]])


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float64).tobytes()).hexdigest()


def fl(a):
    return [float(v) for v in np.asarray(a, np.float64).ravel()]


def main():
    from make_glue_goldens import import_reference
    _, utils, _, _ = import_reference()
    import evenvizion.processing.fixed_coordinate_system as fcs
    import evenvizion.visualization.processing_visualization as pv
    np.seterr(all="ignore")
    out = {}

    def field(H, w, h):
        return np.apply_along_axis(utils.homography_transformation, 2, pv.make_template((h, w, 3)), H)

    # ---- the reference video: every superposed matrix of its committed H JSON ----------------------------------------
    hd, ri = utils.read_homography_dict(os.path.join(HERE, "ref_dict_with_homography_matrix.json"))
    assert (ri["h"], ri["w"]) == SHAPE
    sup = utils.superposition_dict(hd)
    keys = list(sup.keys())
    frames = []
    for k in keys:
        F = field(sup[k], ri["w"], ri["h"])
        assert F.shape == SHAPE + (2,) and F.dtype == np.float64
        frames.append(dict(frame=int(k), H=fl(sup[k]), max=float(np.max(F)), field_sha256=sha(F)))

    # heatmap_video_processing itself, on a stub capture with as many frames as the dict: rendering patched out
    class Cap:
        def __init__(self, n):
            self.n = n

        def read(self):
            if self.n == 0:
                return False, None
            self.n -= 1
            return True, np.zeros(SHAPE + (3,), np.uint8)

    class Imutils:
        @staticmethod
        def resize(img, width):
            assert width == SHAPE[1]
            return img

    pv.imutils = Imutils
    pv.heatmap_frame_processing = lambda *a, **k: None
    with tempfile.TemporaryDirectory() as tmp:
        returned = pv.heatmap_video_processing(sup, Cap(len(sup)), os.path.join(tmp, "heatmap"), SHAPE[1])
    out["video"] = dict(resize_info=ri, frames=frames, heatmap_video_processing=float(returned),
                        max_excluding_last=float(np.max([f["max"] for f in frames[:-1]])))

    # ---- synthetic grids: whole fields ----------------------------------------------------------------------------------
    grids = []
    for w, h in GRIDS:
        for name, H in SYNTH.items():
            F = field(np.array(H, np.float64), w, h)
            grids.append(dict(w=w, h=h, name=name, H=fl(H), max=float(np.max(F)), field=fl(F)))
    out["grids"] = grids

    # ---- superposition_dict ---------------------------------------------------------------------------------------------
    Hs = chain_inputs()
    d = utils.superposition_dict({k + 2: {"H": Hs[k]} for k in range(CHAIN_N)})
    assert list(d.keys()) == [1] + list(range(2, CHAIN_N + 2))
    chain = dict(seed=CHAIN_SEED, n=CHAIN_N, inputs_sha256=sha(Hs), samples=CHAIN_SAMPLES,
                 sup=[fl(d[k + 2]) for k in CHAIN_SAMPLES], last=fl(d[CHAIN_N + 1]))
    none_chains = []
    for pattern in ([0, 1, None, 2, 3], [0, None, None, 1], [0, 1, 2, None], [0, None], [0, 1, None, None, 2, None]):
        frames_h = {k + 2: {"H": None if p is None else Hs[100 + p]} for k, p in enumerate(pattern)}
        r = utils.superposition_dict(frames_h)
        none_chains.append(dict(pattern=[-1 if p is None else 100 + p for p in pattern],
                                sup={str(k): fl(v) for k, v in r.items()}))
    try:
        utils.superposition_dict({2: {"H": None}, 3: {"H": Hs[0]}})
        first_none = None
    except Exception as e:  # noqa
        first_none = type(e).__name__
    out["superposition"] = dict(chain=chain, none_chains=none_chains, first_none_exception=first_none)

    # ---- np.around(homography_transformation(...)) -----------------------------------------------------------------------
    rng = np.random.default_rng(20261017)
    cases = []

    def around_case(H, pts, kx, ky, decimals, inverse):
        tf = utils.inverse_homography_transformation if inverse else utils.homography_transformation
        res = [np.around(tf([kx * x, ky * y], H), decimals=decimals) for x, y in pts]
        M = np.linalg.inv(np.asarray(H, np.float64)) if inverse else np.asarray(H, np.float64)
        cases.append(dict(H=fl(H), M=fl(M), inverse=inverse, pts=[fl(p) for p in pts], kx=kx, ky=ky,
                          decimals=decimals, out=[fl(r) for r in res]))

    eye = np.eye(3)
    halves = [(0.125, -0.125), (-0.375, 0.375), (2.5, -2.5), (0.25, -0.75), (1.5, 0.5), (0.0, -0.0), (1e-16, 5e-16)]
    for dec in (0, 1, 2, 8, 15):
        around_case(eye, halves, 1.0, 1.0, dec, False)
    Hv = np.array(sup[keys[60]], np.float64)
    pts = [tuple(p) for p in rng.uniform(0, 1170, (24, 2))] + [(0.0, 0.0), (1169.0, 657.0), (585.5, 329.25)]
    for dec in (0, 1, 2, 8, 15):
        around_case(Hv, pts, 400 / 1170, 224 / 658, dec, False)
        around_case(Hv, pts, 1170 / 400, 658 / 224, dec, True)
    # w = 0: +/- inf and 0/0
    Hw = np.array([[1.0, 0.0, -5.0], [0.0, 1.0, 0.0], [1.0, 0.0, -5.0]])
    for dec in (0, 2, 15):
        around_case(Hw, [(5.0, 3.0), (5.0, -3.0), (5.0, 0.0), (4.0, 1.0), (6.0, 1.0)], 1.0, 1.0, dec, False)
    out["around"] = cases

    # ---- fixed_coordinate_system on a whole coordinate dict ----------------------------------------------------------------
    oc = {k: [{"x1": float(x), "y1": float(y)} for x, y in rng.uniform(0, [1170, 658], (3, 2))] for k in (2, 30, 61, 121)}
    oc[45] = [{"x1": 0.0, "y1": 0.0}, {"x1": 1170.0, "y1": 658.0}, {"x1": 585.0, "y1": 329.0}]
    fx = fcs.from_original_to_fix(oc, sup, [658, 1170], [224, 400])
    back = fcs.from_fix_to_original(fx, sup, [658, 1170], [224, 400])
    tofloat = lambda dd: {str(k): [[float(r["x1"]), float(r["y1"])] for r in v] for k, v in dd.items()}
    out["fixed_coordinates"] = dict(original=tofloat(oc), fixed=tofloat(fx), back=tofloat(back),
                                    original_shape=[658, 1170], resize_shape=[224, 400])

    path = os.path.join(HERE, "plane_goldens.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes; heatmap_video_processing =", out["video"]["heatmap_video_processing"])


if __name__ == "__main__":
    main()
