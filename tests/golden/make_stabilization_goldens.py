#!/usr/bin/env python3
"""Capture golden vectors for the canvas geometry of the reference's stabilised view by running the reference itself.

Runs ONLY where the reference checkout exists (see make_glue_goldens.REF); writes tests/golden/stabilization_goldens.json,
which travels with the repo.  Imports the reference with make_glue_goldens' inert cv2 / imutils stubs, so only its numpy
arithmetic executes:
    stabilization.get_reference_system        (visualization/stabilization.py:100-126)
    stabilization.initialize_background       (visualization/stabilization.py:220-249; its canvas shape is :241-244)
on the superposition (utils.superposition_dict) of ref_dict_with_homography_matrix.json, on runs of its frames, and on the
same matrices with the middle of their corner range subtracted from [0][2] and [1][2] (so that min_x / min_y are negative:
the reference's canvas takes their absolute value).
imutils.resize is replaced by zeros of the shape imutils would return.  Fixtures are data (inputs + expected outputs); no
reference source text is stored.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

ORIGINAL_SHAPE = (658, 1170)           # frames of the reference's example video (h, w)
CASES = [("all", 1, 121, False), ("head", 1, 12, False), ("middle", 30, 90, False), ("single", 61, 61, False),
         ("all_centred", 1, 121, True), ("tail_centred", 100, 121, True)]
WIDTHS = [400, 320, 1170]


def main():
    from make_glue_goldens import import_reference
    _, utils, _, _ = import_reference()
    import evenvizion.visualization.stabilization as st

    class Imutils:
        @staticmethod
        def resize(img, width):
            h, w = img.shape[:2]
            return np.zeros((int(h * (width / float(w))), width, 3), np.uint8)

    st.imutils = Imutils
    hd, ri = utils.read_homography_dict(os.path.join(HERE, "ref_dict_with_homography_matrix.json"))
    sup = utils.superposition_dict(hd)
    frame = np.zeros(ORIGINAL_SHAPE + (3,), np.uint8)
    cases = []
    for name, a, b, centre in CASES:
        d = {k: np.array(sup[k], np.float64) for k in range(a, b + 1)}
        shift = [0.0, 0.0]
        if centre:
            c0 = st.get_reference_system(d)
            shift = [(c0["max_x"] + c0["min_x"]) / 2.0, (c0["max_y"] + c0["min_y"]) / 2.0]
            for m in d.values():
                m[0][2] -= shift[0] * m[2][2]
                m[1][2] -= shift[1] * m[2][2]
        corner = st.get_reference_system(d)
        shapes = []
        for width in WIDTHS:
            background = st.initialize_background(frame, width, corner)
            resized = Imutils.resize(frame, width).shape
            shapes.append(dict(width=width, frame_shape=[int(resized[0]), int(resized[1])],
                               panorama_shape=[int(background.shape[0]), int(background.shape[1])]))
        cases.append(dict(name=name, first=a, last=b, shift=shift, corner_dict={k: int(v) for k, v in corner.items()},
                          shapes=shapes))
    out = dict(original_shape=list(ORIGINAL_SHAPE), resize_info=ri,
               sup={str(k): [float(v) for v in np.asarray(sup[k], np.float64).ravel()] for k in sup}, cases=cases)
    path = os.path.join(HERE, "stabilization_goldens.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes;", [(c["name"], c["corner_dict"]) for c in cases])


if __name__ == "__main__":
    main()
