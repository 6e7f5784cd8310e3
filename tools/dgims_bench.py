#!/usr/bin/env python3
"""Timing of the D-GIMS graph build (gims_delaunay_build) next to the adaptive build (gims_agc_build) on the same inputs, and of
match_pairs with delaunay=True next to the default GIMS path.  bench.py is the project's yardstick and is not touched by this.

    python tools/dgims_bench.py [--reps 20]

Prints ONE JSON line.  Build times are HIP-event times of one call on the current stream (median of --reps, the two builds alternated
call by call after a warm-up of each); pairs/s is 8 pairs of 2 x 4096 keypoints per match_pairs call, the two modes alternated, each call
timed with events and synchronised.  The exact-fallback counts (info[5]) of every image are reported as well.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def images_of(kps, descs):
    dev = torch.device("cuda")
    info = torch.zeros((len(kps), 8), dtype=torch.int32, device=dev)
    items = []
    for i, (kp, de) in enumerate(zip(kps, descs)):
        n = len(kp)
        items.append(dict(kpts=torch.from_numpy(np.ascontiguousarray(kp)).to(dev), desc=torch.from_numpy(np.ascontiguousarray(de)).to(dev),
                          kept=torch.empty(n, dtype=torch.int32, device=dev), indptr=torch.empty(n + 1, dtype=torch.int32, device=dev),
                          indices=torch.empty(64 * n, dtype=torch.int32, device=dev), info=info[i]))
    return items, info


def time_builds(kps, descs, reps):
    """Median event times (ms) of the Delaunay and the adaptive build of one batch, alternated; and the fallback counts."""
    from gims_amd import hip
    items, info = images_of(kps, descs)
    arr = hip.make_agc_images(items)
    w_dt = torch.empty(hip.delaunay_workspace_bytes(arr), dtype=torch.uint8, device="cuda")
    w_agc = torch.empty(hip.agc_workspace_bytes(arr, 0), dtype=torch.uint8, device="cuda")
    runs = {"delaunay": lambda: hip.delaunay_build(arr, w_dt),
            "adaptive": lambda: hip.agc_build(arr, 15, 2, 7, w_agc, flags=0)}
    fallbacks = None
    for name, fn in runs.items():       # warm-up (code objects, allocator)
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        if name == "delaunay":
            inf = info.cpu().numpy()
            assert (inf[:, 7] == 0).all(), inf[:, 7]
            fallbacks = inf[:, 5].tolist()
    t = {k: [] for k in runs}
    for _ in range(reps):
        for name, fn in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            t[name].append(a.elapsed_time(b))
    return {k: float(np.median(v)) for k, v in t.items()}, {k: [float(np.min(v)), float(np.max(v))] for k, v in t.items()}, fallbacks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    from gims_amd import GMatcher, synth
    from tests.helpers import pair_to_data
    torch.set_grad_enabled(False)
    res = {"metric": "dgims_build_ms", "unit": "ms"}

    def desc_pm(p, s):          # (1, D, N) channel-major -> (N, D) point-major
        return np.ascontiguousarray(p["descriptors" + s][0].T)
    pairs16 = [synth.make_pair(4096, 6000 + i) for i in range(8)]
    kps = [p["keypoints" + s][0] for p in pairs16 for s in ("0", "1")]
    des = [desc_pm(p, s) for p in pairs16 for s in ("0", "1")]
    geoms = {"16x4096": (kps, des)}
    rp = synth.make_pair_unbalanced(15382, 14870, 12000, 4003)
    geoms["readme_15382_14870"] = ([rp["keypoints0"][0], rp["keypoints1"][0]], [desc_pm(rp, "0"), desc_pm(rp, "1")])
    big = [synth.make_pair(32768, 6100 + i) for i in range(2)]
    geoms["4x32768"] = ([p["keypoints" + s][0] for p in big for s in ("0", "1")], [desc_pm(p, s) for p in big for s in ("0", "1")])
    for name, (k, d) in geoms.items():
        med, rng, fb = time_builds(k, d, a.reps)
        res[name] = {"delaunay_ms": round(med["delaunay"], 4), "adaptive_ms": round(med["adaptive"], 4),
                     "delaunay_range_ms": [round(x, 4) for x in rng["delaunay"]], "adaptive_range_ms": [round(x, 4) for x in rng["adaptive"]],
                     "exact_fallbacks": fb}
        torch.cuda.empty_cache()

    # match_pairs at the headline geometry: 8 pairs x 2 x 4096, D-GIMS next to GIMS
    m = GMatcher({}).eval()
    m.load_state_dict(synth.make_state_dict(123))

    def datas(dl):
        out = []
        for p in pairs16:
            d = pair_to_data(p, 15, 2, 7, device="cuda")
            if dl:
                d["delaunay"] = True
            out.append(d)
        return out
    t = {False: [], True: []}
    for rep in range(a.reps + 3):
        for dl in (False, True):
            ds = datas(dl)
            torch.cuda.synchronize()
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            m.match_pairs(ds)
            ev1.record()
            ev1.synchronize()
            if rep >= 3:
                t[dl].append(ev0.elapsed_time(ev1))
    res["match_pairs_8x2x4096"] = {"gims_pairs_per_s": round(8e3 / float(np.median(t[False])), 2),
                                   "dgims_pairs_per_s": round(8e3 / float(np.median(t[True])), 2),
                                   "gims_ms": round(float(np.median(t[False])), 3), "dgims_ms": round(float(np.median(t[True])), 3)}
    res["value"] = res["16x4096"]["delaunay_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
