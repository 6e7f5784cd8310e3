#!/usr/bin/env python3
"""Golden vectors of a PARAMETER SWEEP, made by running the reference itself: one image pair matched under every
(radius, percentile, min_size) of a grid, as the reference's tools/parameter_search.py does (its model settings:
sinkhorn_iterations=20, match_threshold=0.02; weights synth.make_state_dict(123)).

Runs only where the reference is available (tools/gen_golden.py puts it and the stubs of tools/_ref_stubs on sys.path; the reference
is imported unmodified).  One ``.npz`` per pair and radius under ``tests/golden/``:

    meta                [n, seed, canvas w, canvas h (0: synth's default), radius, sinkhorn iterations]
    match_threshold     0.02
    settings            [k][3] the stored (radius, percentile, min_size), in grid order
    ties                [j][3] settings of the grid that are NOT stored: the reference's OT matrix has an exact tie there (a top-1 /
                        top-2 gap of exactly 0.0 in some row or column), so its own argmax decides a match by evaluation order
    r{r}t{t}m{m}/out/*  what the e2e_* fixtures store and tests/helpers.compare_with_golden reads (kept0/1, matches0/1,
                        matching_scores0/1, gap0/1; indices as int16), or
    r{r}t{t}m{m}/error_type, error_text   where the reference raised

Only recorded inputs and outputs are written.

    python tools/gen_golden_sweep.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as GG  # noqa: E402  (puts the reference and the stubs on sys.path)
from gims_amd import synth  # noqa: E402

RADII, PERCENTILES = (10, 15, 22, 30), (0, 2, 5, 10)
ITERS, THRESHOLD = 20, 0.02
# (name, n, seed, canvas, min_size values).  min_size = 1 behaves as 0 on both pairs (same kept counts, matches and gaps) and is not stored;
# the sparse pair is stored where the component removal acts (with nothing removed most of its settings have an exact tie).
PAIRS = (("n1024sparse", 1024, 2001, (800, 600), (7, 10)),
         ("n512", 512, 7001, None, (0, 7, 10)))
NARROW = {"kept0": np.int16, "kept1": np.int16, "matches0": np.int16, "matches1": np.int16,
          "matching_scores0": np.float32, "matching_scores1": np.float32, "gap0": np.float32, "gap1": np.float32}


def main():
    model = GG.ref_model(synth.make_state_dict(123), {"sinkhorn_iterations": ITERS, "match_threshold": THRESHOLD})
    for name, n, seed, canvas, min_sizes in PAIRS:
        pair = synth.make_pair(n, seed, canvas=canvas)
        n_stored = 0
        for r in RADII:
            arrs, settings, ties = {}, [], []
            for t in PERCENTILES:
                for m in min_sizes:
                    key = f"r{r}t{t}m{m}"
                    try:
                        res = GG.run_reference(model, pair, r, t, m)
                    except Exception as e:      # noqa: BLE001  (recorded as the reference's answer for this setting)
                        arrs[key + "/error_type"], arrs[key + "/error_text"] = np.asarray(type(e).__name__), np.asarray(str(e))
                        settings.append((r, t, m))
                        continue
                    if min(float(res["gap0"].min()), float(res["gap1"].min())) == 0.0:
                        ties.append((r, t, m))
                        continue
                    for k, dt in NARROW.items():
                        assert np.array_equal(res[k].astype(dt), res[k]), (key, k)        # narrowing loses nothing
                        arrs[f"{key}/out/{k}"] = res[k].astype(dt)
                    settings.append((r, t, m))
            cw, ch = canvas if canvas else (0, 0)
            GG.save(f"sweep_{name}_s{seed}_i{ITERS}_r{r}", meta=np.asarray([n, seed, cw, ch, r, ITERS], dtype=np.int64),
                    match_threshold=np.float64(THRESHOLD), settings=np.asarray(settings, dtype=np.int64).reshape(-1, 3),
                    ties=np.asarray(ties, dtype=np.int64).reshape(-1, 3), **arrs)
            n_stored += len(settings)
            if ties:
                print(f"  exact ties, not stored: {ties}")
        print(f"{name}: {n_stored} settings stored")


if __name__ == "__main__":
    main()
