#!/usr/bin/env python3
"""Time guided matching (gims_amd.guided_match_pairs) against the plain matcher and against what a caller can do without it,
in plain torch on the same GPU:

  plain_mnn    nn_match_pairs(..., 'mnn') on the same descriptors: the same passes without a gate, so the difference is what the gate costs;
  torch_gate   torch.cdist, the gate as a float64 mask (x1^T F x0 for every pair of keypoints, the two point-to-line tests), masked_fill,
               topk(2, largest=False) per row and the column argmin for the mutual test;
  ours         one guided_match_pairs call for the whole batch (no prior: every row searches).

Sizes: 8 pairs of 2 x 4096 and one pair of 15 382 / 14 870, d = 256, a 3 px band under a planted F (the two-view scene of
tests/fundamental_ref.py on its 800 x 600 canvas: a row of the small size has about 40 admissible columns, of the large one about 150).
Every figure is the time between two device events around the call(s) of one batch, after warm-up.  The driver (no --side) starts one fresh
process per side and round, sides alternating, all on one device, and prints every raw value: per process the median and the extremes over
its timed iterations, the peak device memory and, for `ours`, the workspace, the rows that went to the exhaustive fallback, the rows matched
and how many of them are true pairs.  It stops at the first process that fails.  Whether `ours` is slower than `torch_gate` anywhere is
printed as it is.

    python tools/guided_bench.py --rounds 3 --out guided_bench.json
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

SIDES = ("plain_mnn", "torch_gate", "ours")
SIZES = {"8x4096": (4096, 4096, 8), "1x15382_14870": (15382, 14870, 1)}
D, THRESH, RATIO = 256, 3.0, 0.8


def make_batch(size):
    """-> (datas on the device, F float32 [P, 3, 3] on the device, true partner of every row int64 [n0] per pair)."""
    import numpy as np
    import torch
    from tests import fundamental_ref as FR
    from tests import guided_ref as R
    n0, n1, count = SIZES[size]
    F = FR.planted_F("general")
    F = (F / np.linalg.norm(F)).astype(np.float32)
    datas, truth = [], []
    for p in range(count):
        rng = np.random.default_rng(500 + p)
        k = min(n0, n1) * 2 // 3                                   # two thirds of the smaller image have a partner
        a, b = FR.project_pair("general", max(n0, n1), rng)
        b = b + 0.5 * rng.standard_normal(b.shape)
        perm = rng.permutation(n1)
        kp1 = (rng.random((n1, 2)) * FR.CANVAS).astype(np.float32)
        kp1[perm[:k]] = b[:k].astype(np.float32)
        A, B = R.unit_rows(rng, n0, D), R.unit_rows(rng, n1, D)
        B[perm[:k]] = R.noisy(rng, A[:k], 0.03)
        B[perm[k:k + k // 2]] = R.noisy(rng, A[:k // 2], 0.03)       # every second true pair has a twin elsewhere in image 1
        gt = -np.ones(n0, np.int64)
        gt[:k] = perm[:k]
        cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()     # noqa: E731
        datas.append(dict(descriptors0=cu(A.T)[None], descriptors1=cu(B.T)[None], keypoints0=cu(a[:n0].astype(np.float32))[None], keypoints1=cu(kp1)[None]))
        truth.append(gt)
    return datas, torch.from_numpy(np.stack([F] * count)).cuda(), truth


def torch_gate(datas, Fs):
    import torch
    outs = []
    t2 = THRESH * THRESH
    for d, F in zip(datas, Fs):
        a, b = d["descriptors0"][0].t(), d["descriptors1"][0].t()
        x0 = torch.cat([d["keypoints0"][0], torch.ones_like(d["keypoints0"][0][:, :1])], 1).double()
        x1 = torch.cat([d["keypoints1"][0], torch.ones_like(d["keypoints1"][0][:, :1])], 1).double()
        l0, l1 = x0 @ F.double().t(), x1 @ F.double()               # the line of every keypoint in the other image
        n = l0 @ x1.t()
        n2 = n * n
        ok = (n2 <= t2 * (l0[:, :2] ** 2).sum(1)[:, None]) & (n2 <= t2 * (l1[:, :2] ** 2).sum(1)[None, :])
        dist = torch.cdist(a, b).masked_fill_(~ok, float("inf"))
        two, idx = torch.topk(dist, 2, dim=1, largest=False)
        ratio = two[:, 0] / two[:, 1]
        back = dist.argmin(0)
        match = (ratio < RATIO) & (back[idx[:, 0]] == torch.arange(a.shape[0], device=a.device))
        outs.append((match, idx[:, 0], ratio))
    return outs


def run_side(side, sizes, warmup, iters):
    import torch
    import gims_amd
    results = []
    for size in sizes:
        datas, Fs, truth = make_batch(size)
        records = torch.ones(len(datas), 8, device="cuda")
        verified = dict(models=Fs, records=records, inlier=[None] * len(datas))
        if side == "ours":
            call = lambda: gims_amd.guided_match_pairs(datas, None, verified, model="fundamental", thresh=THRESH, ratio=RATIO)      # noqa: E731
        elif side == "plain_mnn":
            call = lambda: gims_amd.nn_match_pairs(datas, "mnn", RATIO)                                                               # noqa: E731
        else:
            call = lambda: torch_gate(datas, Fs)                                                                                      # noqa: E731
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
        rec = dict(side=side, size=size, ms_median=sorted(ms)[len(ms) // 2], ms_min=min(ms), ms_max=max(ms), peak_bytes=int(torch.cuda.max_memory_allocated()),
                   input_bytes=int(base))
        out = call()
        torch.cuda.synchronize()
        if side == "torch_gate":
            m0 = [torch.where(m, i, torch.full_like(i, -1)).cpu().numpy() for m, i, _ in out]
        else:
            m0 = [o["matches0"][0].cpu().numpy() for o in out]
        rec["matched"] = [int((m >= 0).sum()) for m in m0]
        rec["matched_true"] = [int(((m == t) & (t >= 0)).sum()) for m, t in zip(m0, truth)]
        rec["true_pairs"] = [int((t >= 0).sum()) for t in truth]
        if side == "ours":
            rec["workspace_bytes"] = int(out[0]["_keep"][0][0].numel())
            rec["fallback_rows"] = [[int(v) for v in o["info"][:2].tolist()] for o in out]
            rec["mean_admissible"] = [round(float(o["n_admissible0"].float().mean()), 1) for o in out]
        elif side == "plain_mnn":
            rec["workspace_bytes"] = int(out[0]["_keep"][0].numel())
            rec["fallback_rows"] = [[int(v) for v in o["fallback_rows"].tolist()] for o in out]
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    a = ap.parse_args()
    sizes = a.sizes.split(",")
    if a.side:
        run_side(a.side, sizes, a.warmup, a.iters)
        return 0
    raw = []
    for r in range(a.rounds):
        for side in SIDES:
            cmd = [sys.executable, os.path.abspath(__file__), "--side", side, "--sizes", a.sizes, "--warmup", str(a.warmup), "--iters", str(a.iters)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            if p.returncode != 0:
                print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
                print(f"round {r} side {side} failed with {p.returncode}: stopping", file=sys.stderr)
                return 1
            for line in p.stdout.splitlines():
                if line.startswith("{"):
                    raw.append(dict(json.loads(line), round=r))
    summary, slowest, fastest = {}, {}, {}
    for rec in raw:
        summary.setdefault(rec["size"], {}).setdefault(rec["side"], []).append(round(rec["ms_median"], 4))
        if rec["side"] == "ours":
            slowest[rec["size"]] = max(slowest.get(rec["size"], 0.0), rec["ms_max"])
        elif rec["side"] == "torch_gate":
            fastest[rec["size"]] = min(fastest.get(rec["size"], float("inf")), rec["ms_min"])
    verdict = {k: dict(slowest_ours_ms=round(slowest[k], 4), fastest_torch_gate_ms=round(fastest[k], 4), ours_slower=slowest[k] >= fastest[k]) for k in slowest}
    result = dict(raw=raw, medians_ms_per_process=summary, ours_against_torch_gate=verdict)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    last = {f"{r['size']} {r['side']}": {k: r[k] for k in r if k not in ("side", "size", "round", "ms_median", "ms_min", "ms_max")} for r in raw}
    print(json.dumps(dict(medians_ms_per_process=summary, ours_against_torch_gate=verdict, last_round=last), indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
