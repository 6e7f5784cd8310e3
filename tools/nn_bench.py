#!/usr/bin/env python3
"""Time the descriptor baselines (gims_amd.baselines.nn_match_pairs) against what a caller can do without them, in plain torch on the same GPU:

  cdist_sort   torch.cdist + torch.sort of every row, as the reference's calculate_nndr / calculate_mnn do (eval_matches.py:13-67);
  cdist_topk   the kinder torch.cdist + torch.topk(2, largest=False);
  ours         one nn_match_pairs call for the whole batch.

Sizes: 16 pairs of 2 x 1024, 8 pairs of 2 x 4096, one pair of 2 x 8192, one pair of 15 382 / 14 870 (synthetic descriptors, gims_amd.synth).
Every figure is the time between two device events around the call(s) of one batch, after warm-up.  Method of measurement: the driver (no
--side) starts one fresh process per side and round, sides alternating, at least three rounds, all on one device, and prints every raw value:
per process the median and the extremes over its timed iterations, and the peak device memory (torch.cuda.max_memory_allocated: inputs,
outputs and -- for `ours` -- the workspace, whose size is also given on its own).  It stops at the first process that fails.

    python tools/nn_bench.py --rounds 3 --out nn_bench.json
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

SIDES = ("cdist_sort", "cdist_topk", "ours")
SIZES = {"16x1024": ("pair", 1024, 16), "8x4096": ("pair", 4096, 8), "1x8192": ("pair", 8192, 1), "1x15382_14870": ("unbalanced", 15382, 1)}


def make_batch(size):
    import torch
    from gims_amd import synth
    kind, n, count = SIZES[size]
    datas = []
    for i in range(count):
        pair = synth.make_pair(n, 1000 + i, desc_noise=0.12) if kind == "pair" else synth.make_pair_unbalanced(15382, 14870, 12000, 4003, desc_noise=0.12)
        datas.append({k: torch.from_numpy(pair[k]).cuda() for k in ("descriptors0", "descriptors1")})
    return datas


def torch_baseline(datas, method, threshold, use_sort):
    """The reference's computation per pair, without its host read (nonzero): mask and nearest index stay on the device."""
    import torch
    outs = []
    for d in datas:
        a, b = d["descriptors0"][0].t(), d["descriptors1"][0].t()
        dist = torch.cdist(a, b)
        two, idx = (torch.sort(dist, dim=1) if use_sort else torch.topk(dist, 2, dim=1, largest=False))
        ratio = two[:, 0] / two[:, 1]
        match = ratio < threshold
        if method == "mnn":
            back = torch.cdist(b, a)
            bidx = (torch.sort(back, dim=1) if use_sort else torch.topk(back, 2, dim=1, largest=False))[1]
            match = match & (bidx[:, 0][idx[:, 0]] == torch.arange(a.shape[0], device=a.device))
        outs.append((match, idx[:, 0], ratio))
    return outs


def run_side(side, sizes, methods, warmup, iters):
    import torch
    from gims_amd import baselines
    results = []
    for size in sizes:
        datas = make_batch(size)
        for method in methods:
            if side == "ours":
                call = lambda: baselines.nn_match_pairs(datas, method, 0.8)                           # noqa: E731
            else:
                call = lambda: torch_baseline(datas, method, 0.8, side == "cdist_sort")                # noqa: E731
            for _ in range(warmup):
                out = call()
            torch.cuda.synchronize()
            del out
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            ms = []
            for _ in range(iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = call()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
                del out
            rec = dict(side=side, size=size, method=method, ms_median=sorted(ms)[len(ms) // 2], ms_min=min(ms), ms_max=max(ms),
                       peak_bytes=int(torch.cuda.max_memory_allocated()), input_bytes=int(base))
            if side == "ours":
                out = call()
                rec["workspace_bytes"] = int(out[0]["_keep"][0].numel())
                rec["fallback_rows"] = [int(v) for o in out for v in o["fallback_rows"].tolist()]
                del out
            results.append(rec)
            print(json.dumps(rec), flush=True)
        del datas
        torch.cuda.empty_cache()
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", choices=SIDES)
    ap.add_argument("--sizes", default=",".join(SIZES))
    ap.add_argument("--methods", default="nndr,mnn")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    a = ap.parse_args()
    sizes, methods = a.sizes.split(","), a.methods.split(",")
    if a.side:
        run_side(a.side, sizes, methods, a.warmup, a.iters)
        return 0
    raw = []
    for r in range(a.rounds):
        for side in SIDES:
            cmd = [sys.executable, os.path.abspath(__file__), "--side", side, "--sizes", a.sizes, "--methods", a.methods, "--warmup", str(a.warmup),
                   "--iters", str(a.iters)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            if p.returncode != 0:
                print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
                print(f"round {r} side {side} failed with {p.returncode}: stopping", file=sys.stderr)
                return 1
            for line in p.stdout.splitlines():
                if line.startswith("{"):
                    raw.append(dict(json.loads(line), round=r))
    summary = {}
    for rec in raw:
        summary.setdefault(f"{rec['size']} {rec['method']}", {}).setdefault(rec["side"], []).append(round(rec["ms_median"], 4))
    slowest, fastest = {}, {}
    for rec in raw:                                      # the claim is about single runs, not medians: slowest of ours against fastest of cdist_topk
        k = f"{rec['size']} {rec['method']}"
        if rec["side"] == "ours":
            slowest[k] = max(slowest.get(k, 0.0), rec["ms_max"])
        elif rec["side"] == "cdist_topk":
            fastest[k] = min(fastest.get(k, float("inf")), rec["ms_min"])
    verdict = {k: dict(slowest_ours_ms=round(slowest[k], 4), fastest_topk_ms=round(fastest[k], 4), holds=slowest[k] < fastest[k]) for k in slowest}
    result = dict(raw=raw, medians_ms_per_process=summary, slowest_ours_below_fastest_topk=verdict)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(dict(medians_ms_per_process=summary, slowest_ours_below_fastest_topk=verdict), indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
