"""Image-set matching against match_pairs: the same index pairs through ``GMatcher.match_pairs`` (every pair ingests,
builds and encodes both of its images) and through ``encode_images`` once + ``match_features``, for
  (a) one anchor against 8 partners at 4096 keypoints, adaptive graph (the benchmark's 15 / 2 / 7);
  (b) the same with delaunay=True;
  (c) all 15 pairs of 6 images at 4096;
  (d) one pair at 1024 and at 4096, next to ``forward`` (which ends in a host synchronisation of its own),
and the row-assembly kernel alone (hip.assemble_rows' launch for case (a)'s batch) against its HBM byte count 12 * n_rows * k.

Method: both sides alternate inside one process and one loop; every shape is warmed up first; a run is timed on the host clock between two
device synchronisations (so each figure includes the host's enqueue time, like a caller sees it); --iters runs per side, reported as median,
minimum, maximum and the half-width of the middle 50 % (``spread_ms``); the encode call is timed separately and is NOT part of the
match_features figure.  Stage times (``stage_times_ms``) come from one extra run of each side.  Prints one JSON line, milliseconds.

Usage: python tools/set_bench.py [--iters 12] [--warmup 3] [--kpts 4096] [--cases abcd]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from gims_amd import GMatcher, hip, synth  # noqa: E402

DEV = "cuda"
GRAPH = dict(radius=15, percentile=2, min_size=7)


def image_pool(kpts, count):
    """`count` images of `kpts` keypoints (the two images of consecutive synthetic pairs) as encode_images takes them."""
    pool = []
    for pid in range((count + 1) // 2):
        pair = synth.make_pair(kpts, 1000 + pid)
        for s in "01":
            pool.append({"keypoints": torch.from_numpy(pair["keypoints" + s]).to(DEV), "descriptors": torch.from_numpy(pair["descriptors" + s]).to(DEV),
                         "scores": torch.from_numpy(pair["scores" + s]).to(DEV), "image": pair["image" + s]})
    return pool[:count]


def pair_dicts(pool, pairs, delaunay):
    """Fresh single-pair dicts for match_pairs (it replaces their entries with the kept ones)."""
    out = []
    for i, j in pairs:
        d = dict(device=torch.device(DEV), delaunay=delaunay, **GRAPH)
        for s, im in (("0", pool[i]), ("1", pool[j])):
            d.update({"keypoints" + s: im["keypoints"], "descriptors" + s: im["descriptors"], "scores" + s: im["scores"], "image" + s: im["image"]})
        out.append(d)
    return out


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def summary(ms):
    q1, med, q3 = np.percentile(ms, [25, 50, 75])
    return {"median_ms": round(float(med), 3), "min_ms": round(float(np.min(ms)), 3), "max_ms": round(float(np.max(ms)), 3),
            "spread_ms": round(float(q3 - q1) / 2, 3), "runs": len(ms)}


def stages(model, fn):
    model.enable_timing(True)
    try:
        fn()
        torch.cuda.synchronize()
        return {k: round(float(np.sum(v)), 3) for k, v in sorted(model.stage_times_ms().items())}
    finally:
        model.enable_timing(False)


def compare(model, pool, pairs, delaunay, iters, warmup, with_forward=False):
    sides = {"match_pairs": lambda: model.match_pairs(pair_dicts(pool, pairs, delaunay)),
             "match_features": lambda: model.match_features(feats, pairs)}
    if with_forward:
        sides["forward"] = lambda: model(pair_dicts(pool, pairs, delaunay)[0])
    used = sorted({k for pr in pairs for k in pr})
    index = {k: n for n, k in enumerate(used)}
    encode = lambda: model.encode_images([pool[k] for k in used], delaunay=delaunay, **GRAPH)      # noqa: E731
    feats_used = encode()
    feats = [feats_used[index[k]] if k in index else None for k in range(len(pool))]
    for _ in range(warmup):
        for fn in sides.values():
            fn()
        encode()
    torch.cuda.synchronize()
    ms = {name: [] for name in sides}
    enc = []
    for _ in range(iters):
        for name, fn in sides.items():          # the sides alternate: drift of the clocks or of the box lands on both
            ms[name].append(timed(fn))
        enc.append(timed(encode))
    a, b = model.match_pairs(pair_dicts(pool, pairs, delaunay)), model.match_features(feats, pairs)
    torch.cuda.synchronize()
    equal = all(torch.equal(x["matches0"], y["matches0"]) and torch.equal(x["matching_scores0"], y["matching_scores0"]) for x, y in zip(a, b))
    res = {name: summary(v) for name, v in ms.items()}
    res["encode_images"] = summary(enc)
    res.update(pairs=len(pairs), images=len(used), rows=int(sum(feats[i].n + feats[j].n for i, j in pairs)), results_equal=equal,
               features_minus_pairs_ms=round(res["match_features"]["median_ms"] - res["match_pairs"]["median_ms"], 3),
               not_slower_within_spread=bool(res["match_features"]["median_ms"] <= res["match_pairs"]["median_ms"] + res["match_pairs"]["spread_ms"]),
               stages_match_pairs=stages(model, sides["match_pairs"]), stages_match_features=stages(model, sides["match_features"]))
    return res


def kernel_alone(model, pool, pairs, iters, warmup):
    """The one launch of match_features' `assemble` stage for this batch, timed by HIP events (gims_run_ops_timed)."""
    used = sorted({k for pr in pairs for k in pr})
    feats = dict(zip(used, model.encode_images([pool[k] for k in used], **GRAPH)))
    segs, o = [], 0
    for i, j in pairs:
        segs += [(feats[i].encoded, o), (feats[j].encoded, o + feats[i].n)]
        o += feats[i].n + feats[j].n
    out = torch.empty((o, 256), dtype=torch.float32, device=DEV)
    spl = torch.empty((o, 512), dtype=torch.bfloat16, device=DEV)
    tab = hip.upload(hip.assemble_table(segs, o, 256, DEV), DEV)
    ops = hip.make_ops([hip.op_assemble_rows(tab, len(segs), o, 256, out, spl)])
    pool_ev = hip.EventPool(2)
    ms = []
    for it in range(warmup + iters):
        hip.run_ops_timed(ops, pool_ev)
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append(pool_ev.elapsed_ms()[0])
    nbytes = 12 * o * 256
    med = float(np.median(ms))
    return {"rows": o, "segments": len(segs), "bytes": nbytes, "median_ms": round(med, 4), "min_ms": round(float(np.min(ms)), 4),
            "gb_per_s": round(nbytes / med / 1e6, 1), "share_of_8_tb_per_s": round(nbytes / med / 1e6 / 8000.0, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kpts", type=int, default=4096)
    ap.add_argument("--cases", default="abcdk", help="which of a, b, c, d and k (the kernel alone) to run")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    model = GMatcher({}).eval()
    model.load_state_dict(synth.make_state_dict(123))
    pool = image_pool(a.kpts, 9)
    star = [(0, j) for j in range(1, 9)]
    out = {"kpts": a.kpts, "iters": a.iters, "graph": GRAPH}
    if "a" in a.cases:
        out["a_one_to_8"] = compare(model, pool, star, False, a.iters, a.warmup)
    if "b" in a.cases:
        out["b_one_to_8_delaunay"] = compare(model, pool, star, True, max(a.iters // 2, 2), max(a.warmup // 2, 1))
    if "c" in a.cases:
        out["c_all_pairs_of_6"] = compare(model, pool, [(i, j) for i in range(6) for j in range(i + 1, 6)], False, a.iters, a.warmup)
    if "d" in a.cases:
        for n in (1024, a.kpts):
            out[f"d_one_pair_{n}"] = compare(model, pool if n == a.kpts else image_pool(n, 2), [(0, 1)], False, a.iters, a.warmup, with_forward=True)
    if "k" in a.cases:
        out["assemble_kernel"] = kernel_alone(model, pool, star, 20, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
