#!/usr/bin/env python3
"""Golden vectors for the descriptor baselines BY RUNNING THE REFERENCE ITSELF.

Build container only (needs /root/reference).  ``calculate_nndr`` and ``calculate_mnn`` are compiled out of the reference's
eval_matches.py by name -- the file as a whole imports cv2 and the CAR-HyNet package, the two functions are pure torch -- and run
unmodified (CPU, float32) on the portable fixtures of tests/nn_ref.py.  Each ``tests/golden/nn_*.npz`` holds the fixture's recipe (sizes,
seed, descriptor noise, threshold, twin count) and the three arrays each function returned, with their shapes (0-dim where the
reference's ``.squeeze()`` made them so).  Nothing from the reference's source is written.

    python tools/gen_golden_nn.py
"""
import ast
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import nn_ref  # noqa: E402

REFERENCE_FILE = "/root/reference/eval_matches.py"
OUT = os.path.join(ROOT, "tests", "golden")


def _reference_functions(path, names):
    """The requested top-level functions of the reference's file: its own code, executed, not copied."""
    tree = ast.parse(open(path).read())
    ns = {"np": np, "torch": torch}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in names]


def main():
    calculate_nndr, calculate_mnn = _reference_functions(REFERENCE_FILE, ["calculate_nndr", "calculate_mnn"])
    for name, recipe in nn_ref.FIXTURES:
        a, b = nn_ref.build_fixture(recipe)
        arrays = nn_ref.recipe_arrays(recipe)
        counts = []
        for tag, fn in (("nndr", calculate_nndr), ("mnn", calculate_mnn)):
            idx, good, ratios = fn(torch.from_numpy(a), torch.from_numpy(b), recipe["threshold"])
            arrays[f"{tag}/match_indices"], arrays[f"{tag}/good_matches"], arrays[f"{tag}/ratios"] = idx.numpy(), good.numpy(), ratios.numpy()
            counts.append(int(ratios.numel()))
        want = nn_ref.EXPECTED_MATCHES[name]
        assert counts[0] == want[0] and (want[1] is None or counts[1] == want[1]), (name, counts, want)
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **arrays)
        print(f"{name}: A {a.shape}, B {b.shape}: {counts[0]} NNDR / {counts[1]} MNN matches, index shape {arrays['nndr/match_indices'].shape}")


if __name__ == "__main__":
    main()
