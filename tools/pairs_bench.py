"""Pair selection on the device against the torch route, on the ring scene of tests/pairs_ref.py at workload size: D = 256,
512 rows per image, neighbours 200 world rows apart (312 shared rows at ring distance 1, 112 at distance 2, none beyond), N images.

  --route op      GIMS_AUX_SELECT_PAIRS alone by device events around the op (gims_run_ops_timed), median of --iters runs; the pair list and
                  the vote histogram of the scene; the multiply-adds of the vote kernel (padded rows included, self blocks excluded)
  --route torch   the same votes with torch on the same GPU: per image a float32 torch.cdist against the pooled matrix, topk(2,
                  largest=False) per block, the same ratio test on the squared distances; device events, median of --iters runs
  --route match   the time GMatcher.match_features takes for --pairs pairs (a pool of encoded synthetic images, as tools/track_bench.py)
  --all           every N of --ns through `op` and `torch` in ALTERNATING fresh processes (--rounds each), then `match` for all pairs of the
                  smallest N and for the pairs the op selected there; one JSON line per child and a summary line
The vote kernel alone is read from a kernel trace of the `op` route (rocprofv3 --kernel-trace --stats -- python tools/pairs_bench.py --route
op --n N): its share of the i8 MFMA peak is mult_adds / time / (256 CUs * 4 SIMDs * 1024 multiply-adds per clock * 2.4 GHz).

Usage: python tools/pairs_bench.py --all [--ns 64,256,1024] [--iters 10] [--rounds 2] [--no-match]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

DEV = "cuda"
D, PER, STEP, K, RATIO, MIN_VOTES = 256, 512, 200, 20, 0.8, 1
I8_PEAK_MAC = 256 * 4 * 1024 * 2.4e9
GRAPH = dict(radius=15, percentile=2, min_size=7)


def ring(n):
    from tests import pairs_ref as R
    return R.ring_scene(n=n, d=D, n_world=STEP * n, per=PER, step=STEP, noise=0.03, seed=7)


def _median(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4), "runs": len(ms)}


def route_op(n, iters, warmup):
    import torch
    from gims_amd import hip
    descs = [torch.from_numpy(x).to(DEV) for x in ring(n)]
    images = [(t, D, PER, None, PER) for t in descs]
    work = torch.empty(hip.pairs_work_bytes([PER] * n, D), dtype=torch.uint8, device=DEV)
    tab = hip.pairs_table(images, hip.pairs_rq(RATIO), work.numel())
    votes = torch.empty((n, n), dtype=torch.int32, device=DEV)
    out = torch.zeros(hip.pairs_out_layout(n, K)[2], dtype=torch.int32, device=DEV)
    counters = torch.empty(8, dtype=torch.int32, device=DEV)
    ops = hip.make_ops([hip.op_select_pairs(tab, votes, out, counters, work, n, D, PER, K, MIN_VOTES)])
    ev = hip.EventPool(2)
    ms = []
    for it in range(warmup + iters):
        hip.run_ops_timed(ops, ev)
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append(ev.elapsed_ms()[0])
    s = (votes + votes.T).cpu().numpy()
    upper = s[np.triu_indices(n, 1)]
    values, counts = np.unique(upper, return_counts=True)
    n_pairs = int(counters[0])
    res = _median(ms)
    mac = (n * PER) ** 2 * D - n * PER * PER * D
    res.update(route="op", n=n, work_mib=round(work.numel() / 2 ** 20, 1), n_pairs=n_pairs, all_pairs=n * (n - 1) // 2,
               vote_histogram={int(v): int(c) for v, c in zip(values, counts)}, vote_mult_adds=mac,
               op_rate_of_i8_peak=round(mac / (res["median_ms"] * 1e-3) / I8_PEAK_MAC, 4),
               pairs_head=out[:2 * min(n_pairs, 4)].view(-1, 2).tolist())
    return res


def route_torch(n, iters, warmup):
    import torch
    descs = [torch.from_numpy(x).to(DEV) for x in ring(n)]
    pooled = torch.cat(descs)
    r2 = float(np.float32(RATIO)) ** 2
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for it in range(warmup + iters):
        start.record()
        votes = torch.zeros((n, n), dtype=torch.int32, device=DEV)
        for i, x in enumerate(descs):
            two = torch.cdist(x, pooled).view(PER, n, PER).topk(2, dim=2, largest=False)[0] ** 2
            votes[i] = (two[:, :, 0] < r2 * two[:, :, 1]).sum(0)
            votes[i, i] = 0
        stop.record()
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append(start.elapsed_time(stop))
    s = votes + votes.T
    res = _median(ms)
    res.update(route="torch", n=n, pairs_with_votes=int((s.cpu().numpy()[np.triu_indices(n, 1)] >= MIN_VOTES).sum()))
    return res


def route_match(n_pairs, kpts, batch):
    import torch
    from gims_amd import GMatcher, synth
    model = GMatcher({}).eval()
    model.load_state_dict(synth.make_state_dict(123))
    pool = []
    for pid in range(8):
        pair = synth.make_pair(kpts, 1000 + pid)
        for s in "01":
            pool.append({"keypoints": torch.from_numpy(pair["keypoints" + s]).to(DEV), "descriptors": torch.from_numpy(pair["descriptors" + s]).to(DEV),
                         "scores": torch.from_numpy(pair["scores" + s]).to(DEV), "image": pair["image" + s]})
    feats = model.encode_images(pool, **GRAPH)
    every = [(a, b) for a in range(len(pool)) for b in range(a + 1, len(pool))]
    todo = [every[k % len(every)] for k in range(n_pairs)]
    for _ in range(3):
        model.match_features(feats, todo[:batch])
    torch.cuda.synchronize()
    t = time.perf_counter()
    for o in range(0, n_pairs, batch):
        model.match_features(feats, todo[o:o + batch])
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t) * 1e3
    return {"route": "match", "pairs": n_pairs, "total_ms": round(ms, 1), "ms_per_pair": round(ms / n_pairs, 4), "kpts": kpts, "batch": batch}


def child(*args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), *[str(a) for a in args]], stdout=subprocess.PIPE, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"pairs_bench: {' '.join(str(a) for a in args)} ended with {r.returncode}")
    line = r.stdout.strip().splitlines()[-1]
    print(line, flush=True)
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=("op", "torch", "match"))
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--ns", default="64,256,1024")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=2016)
    ap.add_argument("--kpts", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--no-match", action="store_true")
    a = ap.parse_args()
    if a.all:
        summary = {}
        ns = [int(v) for v in a.ns.split(",")]
        for n in ns:
            runs = {"op": [], "torch": []}
            for _ in range(a.rounds):
                for route in ("op", "torch"):                      # alternating fresh processes
                    runs[route].append(child("--route", route, "--n", n, "--iters", a.iters, "--warmup", a.warmup))
            op, th = (float(np.median([r["median_ms"] for r in runs[k]])) for k in ("op", "torch"))
            summary[n] = {"op_ms": op, "torch_ms": th, "torch_over_op": round(th / op, 2), "n_pairs": runs["op"][0]["n_pairs"],
                          "all_pairs": runs["op"][0]["all_pairs"], "op_faster": bool(op < th)}
        if a.no_match:
            print(json.dumps({"summary": summary}))
            return
        n0 = ns[0]
        every = child("--route", "match", "--pairs", n0 * (n0 - 1) // 2, "--kpts", a.kpts, "--batch", a.batch)
        chosen = child("--route", "match", "--pairs", summary[n0]["n_pairs"], "--kpts", a.kpts, "--batch", a.batch)
        summary["match_features"] = {"n": n0, "all_pairs_ms": every["total_ms"], "selected_pairs_ms": chosen["total_ms"],
                                     "selected_plus_op_ms": round(chosen["total_ms"] + summary[n0]["op_ms"], 1)}
        print(json.dumps({"summary": summary}))
        return
    import torch
    torch.set_grad_enabled(False)
    if a.route == "op":
        print(json.dumps(route_op(a.n, a.iters, a.warmup)))
    elif a.route == "torch":
        print(json.dumps(route_torch(a.n, a.iters, a.warmup)))
    else:
        print(json.dumps(route_match(a.pairs, a.kpts, a.batch)))


if __name__ == "__main__":
    main()
