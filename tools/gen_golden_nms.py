#!/usr/bin/env python3
"""Golden vectors for the DIoU-NMS keypoint thinning BY RUNNING THE REFERENCE ITSELF.

Build container only (needs /root/reference).  ``diou_nms`` and ``process_diou_nms`` are compiled out of the reference's utils/common.py
by name -- the file as a whole imports cv2 and torchvision, the two functions are pure NumPy -- and run unmodified on the seeded recipes
of tests/nms_ref.py, given as objects with cv2.KeyPoint's ``pt``, ``size`` and ``response``.  Each ``tests/golden/nms_*.npz`` holds the
recipe, the rows the function returned in its order, and the NumPy version; the detector recipes also hold their keypoints (this
project's own restatement of the detector made them), so no test has to detect again.  Nothing from the reference's source is written.

    python tools/gen_golden_nms.py
"""
import ast
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tests import nms_ref  # noqa: E402

REFERENCE_FILE = "/root/reference/utils/common.py"
OUT = os.path.join(ROOT, "tests", "golden")


def _reference_functions(path, names):
    """The requested top-level functions of the reference's file: its own code, executed, not copied."""
    tree = ast.parse(open(path).read())
    ns = {"np": np}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in names]


class KeyPoint:
    __slots__ = ("pt", "size", "response", "row")

    def __init__(self, row, x, y, size, response):
        self.row, self.pt, self.size, self.response = row, (float(x), float(y)), float(size), float(response)


def main():
    _, process_diou_nms = _reference_functions(REFERENCE_FILE, ["diou_nms", "process_diou_nms"])
    for name, recipe, want in nms_ref.FIXTURES:
        kp, scores = nms_ref.build_fixture(recipe)
        objs = [KeyPoint(r, *kp[r], scores[r]) for r in range(len(kp))]
        out = process_diou_nms(objs, recipe["radius"] or None, recipe["thr"])
        rows = np.array([k.row for k in out], np.int32)
        assert want is None or len(rows) == want, (name, len(rows), want)
        assert len(set(rows.tolist())) == len(rows)
        arrays = {"recipe/" + k: np.array(v) for k, v in recipe.items()}
        arrays["rows"], arrays["n"], arrays["numpy_version"] = rows, np.array(len(kp)), np.array(np.__version__)
        if recipe["kind"] == "detector":
            arrays["kp"], arrays["scores"] = kp, scores
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **arrays)
        print(f"{name}: {len(kp)} keypoints -> {len(rows)} kept")


if __name__ == "__main__":
    main()
