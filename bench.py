#!/usr/bin/env python3
"""Benchmark of the GIMS matcher hot path on MI355X:  image-pairs/sec at 2 x N keypoints.

    python bench.py --gpus N --steps K --warmup W [--kpts 4096 --pairs 8] [--sinkhorn-iters 100] [--dump-outputs DIR] [--full]

A "step" is one pass of the whole hot path (adaptive graph build -> GraphSAGE -> keypoint encoder ->
18-layer self/cross attention -> Sinkhorn -> mutual matching) over one ragged batch of synthetic image pairs
per GPU, through the production path (`GMatcher.match_pairs`: the 18 layers run from the replayed launch
table; with --full the library records a HIP event after each of its launches, on the launch stream).  Inputs are
resident in HBM before the timed region.

A plain run (no --full) does only what the headline figure needs: it sets up, warms up, times the K steps of ONE
workload (2x4096 keypoints, 8 pairs per step per GPU, or --kpts/--pairs), writes the outputs of the last timed step
if --dump-outputs is given, and prints the line: metric, value, unit, higher_is_better, dtype, ms_per_step, config.
No HIP events inside the timed steps, no checks, no extra blocks, no bench_extra.json.

--dump-outputs DIR writes what the timed path handed its caller in its last timed step as DIR/<name>.npy (`dump_outputs`;
float32 / float64, at most 64 MB).  The inputs are seeded: the same arguments give the same inputs in every run, so two
builds can be compared output for output.

--full adds everything else the benchmark measures and checks, as described below.  With no workload flags
the line of a --full run carries BOTH workloads BASELINE.json's metric is quoted on:
  * headline (`value`, `ms_per_step`, `roofline`, `cpu_baseline`): 2x4096 keypoints, 8 pairs per step per GPU
    (BASELINE configs[2], the north-star target >= 200 pairs/s);
  * `"also"`: the same block for 2x1024 keypoints, 32 pairs per step (BASELINE configs[1]), timed the same way
    right after the headline run.
`--kpts/--pairs` select a single workload instead.

Pairs are independent units: with N > 1 every rank (one per GPU, RCCL) matches its own pairs and the per-pair
match statistics are all-gathered over xGMI each step -- the only collective of the path (weak scaling).
`python bench.py --gpus N` without a launcher starts the N ranks itself (child processes, created before this
process touches the GPU; same shape as the reference's mp.spawn launch, train.py:189-197, 231); under
`torch.distributed.run` it reads RANK / LOCAL_RANK / WORLD_SIZE from the environment.

Rank 0 prints ONE compact JSON line (< 4 KB: `compact_line`) as the LAST line of stdout; with --full the full record (every
kernel's roofline, notes, per-layer arrays, the CPU thread sweep, eval, ranks, the extra blocks in full) is written to
`bench_extra.json` next to this file or, if that directory is not writable, to `bench_extra.json` in an output folder below it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2500.0   # dense bf16 MFMA peak, /opt/skills/guides/MI355X_MICROARCH.md
PEAK_F32_VALU_TFLOPS = 157.3  # fp32 vector peak (256 CU x 4 SIMD x 64 lanes... x 2 flop x 2.4 GHz), same guide
PEAK_HBM_GBS = 8000.0       # HBM3E spec

HEADLINE = (4096, 8)
SECOND = (1024, 32)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def _r(x, sig=5):
    """floats to `sig` significant digits (the line is for reading and for the driver's parser, not for archiving)"""
    if isinstance(x, float):
        return float(f"{x:.{sig}g}")
    if isinstance(x, str) and len(x) > 260:          # prose belongs in bench_extra.json
        return x[:257] + "..."
    if isinstance(x, dict):
        return {k: _r(v, sig) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_r(v, sig) for v in x]
    return x


def _pick(d, keys):
    return {k: d[k] for k in keys if d is not None and k in d}


LINE_LIMIT = 4096          # bytes; the driver keeps the last 8000 characters of stdout and parses the last line


def compact_line(res, extra="bench_extra.json"):
    """The one JSON line the driver parses, from the record of `main`: the contract's keys and, for a --full record, the dominant
    kernel's roofline, the cross-attention fraction north_star names, the CPU baseline, per-stage GPU milliseconds, and the extra
    blocks reduced to scalars.  Everything else lives in `extra` (bench_extra.json; None: not written)."""
    cfg = res.get("config", {})
    line = _pick(res, ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                       "vs_baseline", "data"))
    line["dtype"] = res.get("dtype_short", "bf16")
    line["config"] = _pick(cfg, ("workload", "pairs_per_step_per_gpu", "keypoints", "sinkhorn_iterations", "path", "parallelism"))
    if "roofline" in res:
        line["roofline"] = _pick(res["roofline"], ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_source",
                                                   "traffic_profile_head", "avg_launch_ms", "launches_per_step", "algorithmic_work_per_launch"))
    if "cross_attention" in res:
        line["cross_attention"] = _pick(res["cross_attention"], ("kernel", "frac", "achieved", "unit", "avg_launch_ms", "operands"))
    if "cpu_baseline" in res:
        line["cpu_baseline"] = _pick(res["cpu_baseline"], ("value", "unit", "cores", "host_cores", "kind", "sample"))
    if "stage_ms_per_step" in res:
        line["stage_ms_per_step"] = _r(res["stage_ms_per_step"], 4)
    if "host_step_ms" in res:
        line["host_step_ms"] = res["host_step_ms"]
    if "attention" in res:
        line["attention_layers"] = _pick(res["attention"], ("precision", "layers_bf16", "layers_f16", "layers_bf16x3"))
    line["world_size_seen"] = res.get("world_size_seen", 1)
    line.update(_pick(res, ("stats_rows_gathered", "matches_pair0", "sinkhorn_rescues", "host_threads_per_rank", "attention_launches_per_step")))
    par = lambda blk: [_pick(p, ("golden", "rows_equal", "rows", "max_score_err")) for p in (blk.get("parity_vs_reference") or [])]    # noqa: E731
    if par(res):               # the timed batch against the reference's own output for its pair 0 (tests/golden, bench.golden_parity)
        line["parity_pair0"] = par(res)[0]
    if res.get("ranks"):               # proof of the N > 1 launch: [rank, device index, collective backend, pid] of every rank
        line["ranks"] = [[r["rank"], r["device"], r["backend"], r["pid"]] for r in res["ranks"]]
    also = {}
    for name, blk in (res.get("also") or {}).items():
        if "error" in blk:
            also[name] = {"error": str(blk["error"])[:80]}
            continue
        a = _pick(blk, ("value", "ms_per_step", "ms_per_pair"))
        if "cross_attention" in blk:
            a["cross_attention_frac"] = blk["cross_attention"]["frac"]
        if "roofline" in blk:
            a["roofline_kernel"], a["frac"] = blk["roofline"]["kernel"], blk["roofline"]["frac"]
        if "carhynet" in blk:
            a["carhynet_frac"], a["carhynet_patches_per_s"] = blk["carhynet"]["frac"], blk["carhynet"]["patches_per_s"]
        if "from_images" in blk and "value" in blk["from_images"]:
            a["from_images_value"] = blk["from_images"]["value"]
        if "agc_ms_per_image" in blk:
            a["agc_ms_per_image"] = blk["agc_ms_per_image"]
        if "stage_ms_per_step" in blk and name.startswith("readme"):
            a["stage_ms_per_step"] = _r(blk["stage_ms_per_step"], 3)
        if "cpu_baseline" in blk:
            a["cpu_value"] = blk["cpu_baseline"]["value"]
        if par(blk):
            a["parity"] = {"rows_equal": all(p["rows_equal"] for p in par(blk)), "max_score_err": max(p["max_score_err"] for p in par(blk))}
        also[name] = a
    if also:
        line["also"] = also
    if "latency_ms_b1" in res:
        line["latency_ms_b1"] = res["latency_ms_b1"]
    if "train_step" in res:
        t = res["train_step"]
        line["train_step"] = {"error": str(t["error"])[:80]} if "error" in t else _pick(t, ("value", "unit", "ms_per_step"))
    if extra:
        line["extra"] = extra
    line = _r(line)
    out = json.dumps(line, separators=(",", ":"))
    if len(out) >= LINE_LIMIT:            # never lose the line to its own size: shed the optional parts, largest first
        for k in ("also", "stage_ms_per_step", "attention_layers", "attention_launches_per_step", "ranks", "host_step_ms", "matches_pair0", "parity_pair0"):
            line.pop(k, None)
            out = json.dumps(line, separators=(",", ":"))
            if len(out) < LINE_LIMIT:
                break
    return out


def write_extra(res):
    """the full record, for people: next to bench.py, else under gpurun_out/; never fatal"""
    for d in (ROOT, os.path.join(ROOT, "gpurun_out")):
        try:
            os.makedirs(d, exist_ok=True)
            with open(os.path.join(d, "bench_extra.json"), "w") as f:
                json.dump(res, f, indent=1)
            return os.path.join(d, "bench_extra.json")
        except OSError:
            continue
    return None


def make_inputs(pair_ids, kpts, device, maker=None):
    import torch
    from gims_amd import synth
    datas = []
    for pid in pair_ids:
        pair = maker(pid) if maker is not None else synth.make_pair(kpts, 1000 + pid)
        d = {k: torch.from_numpy(v).to(device) for k, v in pair.items() if k not in ("gt_perm", "image0", "image1")}
        d["image0"], d["image1"] = pair["image0"], pair["image1"]
        d.update(device=torch.device(device), radius=15, percentile=2, min_size=7)
        datas.append((d, pair["gt_perm"]))
    return datas


DUMP_LIMIT = 64 << 20      # bytes: what --dump-outputs may write in all (split evenly between the ranks)
DUMP_ROWS = 512            # rows of each 256-d descriptor block that go into the dump (a fixed, seeded sample)


def dump_outputs(out_dir, pair_ids, outs, datas, stats=None, world=1, limit=DUMP_LIMIT):
    """--dump-outputs: what `match_pairs` handed its caller in the LAST timed step, as `out_dir/<name>.npy` (float32; integer arrays as
    float64).  Per pair, `pair<id>_<key>`: the kept keypoint ids and positions, matches and matching scores of both images in full, and of the
    two 256-d descriptor blocks (the kept input descriptors, the matching descriptors after the GNN) the rows `sample_rows<side>`, a fixed
    sample of DUMP_ROWS drawn with the pair id as seed.  `stats`: the all-gathered per-pair statistics (shard.STAT_FIELDS).  Pairs go in
    in the order given while the total stays within `limit` / `world` bytes.  Returns the names written."""
    import torch
    os.makedirs(out_dir, exist_ok=True)
    budget = limit // max(1, world)
    arrays = {}
    if stats is not None:
        arrays["stats"] = stats.float().cpu().numpy()
    used = sum(a.nbytes for a in arrays.values())
    for pid, o, d in zip(pair_ids, outs, datas):
        blk = {}
        for s in "01":
            mdesc = o[f"mdesc{s}"]
            rows = np.sort(np.random.default_rng(2 * int(pid) + int(s)).permutation(mdesc.shape[0])[:DUMP_ROWS])
            rows_t = torch.from_numpy(rows).to(mdesc.device)
            blk[f"kept{s}"] = d[f"kept_kpts{s}_indices"][0]
            blk[f"keypoints{s}"] = o[f"keypoints{s}"][0]
            blk[f"matches{s}"] = o[f"matches{s}"][0]
            blk[f"matching_scores{s}"] = o[f"matching_scores{s}"][0]
            blk[f"sample_rows{s}"] = rows_t
            blk[f"descriptors{s}_sample"] = o[f"descriptors{s}"][0].index_select(1, rows_t).t()
            blk[f"mdesc{s}_sample"] = mdesc.index_select(0, rows_t)
        blk = {k: (v.float() if v.is_floating_point() else v.double()).cpu().numpy() for k, v in blk.items()}
        size = sum(a.nbytes for a in blk.values())
        if used + size > budget:
            break
        used += size
        arrays.update({f"pair{int(pid):04d}_{k}": v for k, v in blk.items()})
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return list(arrays)


def cpu_baseline(kpts, iters, budget_s=60.0, thr=0.2):
    """The oracle (CPU restatement of the reference, oracle/gims_oracle.py) on this host's cores, SURVEY 8(d)'s protocol: ONE untimed
    warm-up pair, then one timed pair at each of 16 / 32 / 64 intra-op threads (capped by the host's core count; the small per-op tensors of
    this path stop scaling well before a 256-core host is full; the sweep stops early when the budget would not leave room for the timed
    pairs), then timed pairs at the BEST thread count until at least three are in (more while the budget lasts, at most 32): the baseline is
    1 / median(seconds per pair) there.  Every timing is listed.  A bounded sample: `budget_s` seconds of CPU work, outside the timed region."""
    import torch
    from gims_amd import synth
    from oracle import gims_oracle as O
    sd = synth.make_state_dict(123)
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    tried = sorted({min(cores, t) for t in (16, 32, 64)})
    t_begin = time.perf_counter()

    def one(nt, pid):
        torch.set_num_threads(nt)
        pair = synth.make_pair(kpts, 1000 + pid)
        d = {k: torch.from_numpy(v) for k, v in pair.items() if k not in ("gt_perm", "image0", "image1")}
        d["image0"], d["image1"] = pair["image0"], pair["image1"]
        d.update(device=torch.device("cpu"), radius=15, percentile=2, min_size=7)
        t0 = time.perf_counter()
        with torch.no_grad():
            O.gmatcher_forward(sd, d, {"sinkhorn_iterations": iters, "match_threshold": thr})
        return time.perf_counter() - t0

    warm = one(tried[0], 0)                     # untimed: first-touch of the weights, thread pool start-up, allocator growth
    per = {}
    for nt in tried:
        per[nt] = [one(nt, 0)]
        used = time.perf_counter() - t_begin
        if used + 3.0 * min(min(v) for v in per.values()) > budget_s:        # keep room for the timed pairs at the best count
            break
    best = min(per, key=lambda nt: per[nt][0])
    pid = 1
    while len(per[best]) < 3 or (time.perf_counter() - t_begin + float(np.median(per[best])) < budget_s and len(per[best]) < 32):
        per[best].append(one(best, pid))
        pid += 1
    med = float(np.median(per[best]))
    runs = [{"threads": nt, "pairs": len(v), "seconds_per_pair": [round(x, 3) for x in v], "pairs_per_s": 1.0 / float(np.median(v))} for nt, v in per.items()]
    return {"value": 1.0 / med, "unit": "pairs/s", "cores": best, "threads": best, "host_cores": cores, "kind": "port", "thread_sweep": runs,
            "warmup_seconds": round(warm, 2), "timed_pairs": len(per[best]), "median_seconds_per_pair": med,
            "sample": f"median of {len(per[best])} pairs of 2x{kpts} keypoints ({iters} Sinkhorn iterations) after 1 warm-up pair, oracle/gims_oracle.py "
                      f"on torch CPU at {best} threads ({med:.2f} s per pair; one pair each at {list(per)} threads chose the count)"}


def golden_parity(kpts, iters, thr, pair_ids, outs, datas):
    """Parity of what was TIMED against the reference itself: every pair of this rank's last timed batch that has a reference golden
    (tests/golden/e2e_n{kpts}_s{1000 + pair}_r15p2m7_i{iters}.npz: the outputs of the unmodified reference on the same synthetic pair,
    tools/gen_golden.py) is compared row by row -- kept ids, both match vectors, scores.  A fixture is data, not the oracle; absent
    fixture -> None (the planted-correspondence guard alone stands)."""
    recs = []
    for slot, pid in enumerate(pair_ids):
        name = f"e2e_n{kpts}_s{1000 + pid}_r15p2m7_i{iters}"
        path = os.path.join(ROOT, "tests", "golden", name + ".npz")
        if not os.path.exists(path):
            continue
        g = np.load(path)
        if abs(float(g["match_threshold"]) - float(thr)) > 1e-9:
            continue
        o, d = outs[slot], datas[slot]
        k0, k1 = (d[f"kept_kpts{s}_indices"][0].cpu().numpy() for s in "01")
        m0, m1 = o["matches0"][0].cpu().numpy(), o["matches1"][0].cpu().numpy()
        s0, s1 = o["matching_scores0"][0].cpu().numpy(), o["matching_scores1"][0].cpu().numpy()
        kept_equal = bool(np.array_equal(k0, g["out/kept0"]) and np.array_equal(k1, g["out/kept1"]))
        differing = (int((m0 != g["out/matches0"]).sum() + (m1 != g["out/matches1"]).sum()) if kept_equal else -1)
        err = float(max(np.abs(s0 - g["out/matching_scores0"]).max(), np.abs(s1 - g["out/matching_scores1"]).max())) if kept_equal else float("inf")
        recs.append({"golden": name, "pair": int(pid), "kept_equal": kept_equal, "rows_equal": kept_equal and differing == 0,
                     "rows_differing": differing, "rows": int(len(m0) + len(m1)), "max_score_err": err})
    return recs or None


def rank_affinity(cores, local_rank, local_world):
    """The slice of the inherited CPU set that rank `local_rank` of `local_world` ranks on this node keeps to: contiguous, equal shares, disjoint
    between the ranks; None (leave the affinity alone) when a share would be a single core."""
    cores = sorted(cores)
    share = len(cores) // max(1, local_world)
    if share < 2:
        return None
    r = local_rank % max(1, local_world)
    return cores[r * share:(r + 1) * share]


# ------------------------------------------------------------------------------------------------ self-launch
def spawn_ranks(n: int) -> int:
    """`python bench.py --gpus N` without a launcher: start the N ranks as child processes (one per GPU) and wait.
    This process has not touched the GPU (no HIP call, no torch.cuda call) and never does; rank 0's stdout (the JSON line)
    is passed through, every rank's stderr goes to ours."""
    import socket
    import subprocess
    from gims_amd.build import build_lib
    build_lib(force=False)                  # compile once here (hipcc only: no GPU), the ranks find the library fresh
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *sys.argv[1:]], env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    # a rank that dies (e.g. the backend refuses the device layout) must not leave its peers waiting in a collective for ever: once one
    # rank has failed, the others get 30 s to finish on their own and are then terminated -- the launcher always returns
    rc, failed_at = 0, None
    while any(p.poll() is None for p in procs):
        time.sleep(0.2)
        codes = [p.poll() for p in procs]
        if failed_at is None and any(c not in (None, 0) for c in codes):
            failed_at = time.monotonic()
            log(f"bench.py launcher: a rank exited with {[c for c in codes if c not in (None, 0)]}; waiting 30 s for the others")
        if failed_at is not None and time.monotonic() - failed_at > 30.0:
            for p in procs:
                if p.poll() is None:
                    p.kill()
    for p in procs:
        rc = max(rc, abs(p.wait()))
    return rc


# ------------------------------------------------------------------------------------------------ one workload
def event_steps(steps, every):
    """Which of the K timed steps carry the stage / per-launch HIP events: every `every`-th, mid-stride (K = 20, every = 5 -> 2, 7, 12, 17)."""
    every = max(1, min(int(every), int(steps)))
    return every, list(range(every // 2, int(steps), every))


def headline_record(model, kpts, pairs, args, world, elapsed, outs, modes, ev_steps, every):
    """The fields of a workload's record that a plain run prints: what was timed, how fast, at which precision."""
    iters = int(model.config["sinkhorn_iterations"])
    flats = outs.flat if isinstance(outs.flat, (list, tuple)) else [outs.flat]
    problems = [(a, b) for f in flats for a, b in zip(f["n0"], f["n1"])]
    nl = getattr(model, "n_lanes_last", 1)          # stream lanes: each stage is launched once per lane
    tier = max(("bf16", "f16", "bf16x3"), key=modes.count)
    events = (f", HIP events around every attention / GEMM launch on the launch stream on {ev_steps} of the {args.steps} timed steps: every {every}th"
              if ev_steps else ", no HIP events inside the timed steps")
    return {
        "metric": f"image-pairs/sec at 2x{kpts} keypoints", "value": world * pairs * args.steps / elapsed, "unit": "pairs/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": ({"bf16": "bf16 MFMA attention and Q/K/V projection", "f16": "f16 MFMA attention (3-pass Q/K/V projection rounded to half)",
                   "bf16x3": "split-bf16x3 MFMA attention"}[tier]
                  + " + split-bf16x3 (f32-class) MFMA linears + bf16x6 (f32-class) similarity and score GEMMs + f32 Sinkhorn") if args.linear_precision == "bf16x3"
                 else "bf16 MFMA attention + f32 MFMA linears + f32 Sinkhorn",
        "dtype_short": ({"bf16": "bf16", "f16": "f16", "bf16x3": "bf16x3"}[tier] + " MFMA attention + "
                        + ("bf16x3" if args.linear_precision == "bf16x3" else "f32") + " MFMA linears + f32 Sinkhorn"),
        "data": "synthetic",
        "config": {"workload": f"{pairs} pairs/step/GPU of 2x{kpts} synthetic keypoints (kept {problems[0][0]}/{problems[0][1]} after AGC r=15 p=2 m=7), "
                               f"256-d descriptors, 18 attentional layers (9 self + 9 cross), {iters} Sinkhorn iterations, match_threshold {model.config['match_threshold']}",
                   "pairs_per_step_per_gpu": pairs, "keypoints": kpts, "sinkhorn_iterations": iters,
                   "path": "GMatcher.match_pairs, production path ("
                           + ("encoder + layer launches replayed from the cached gims_run_ops tables" if model._replays("layers", 2 * kpts * pairs)
                              else "launch by launch: config launch_replay_rows / GIMS_NO_REPLAY")
                           + events + "); "
                           "Python's cyclic GC is frozen + disabled inside the K timed steps" + (" (host_step_ms.max reports the slowest step)" if ev_steps else ""),
                   "parallelism": f"pairs sharded over {world} GPU(s), all-gather of match statistics; {nl} stream lane(s) per GPU"},
    }


def run_workload(model, kpts, pairs, args, world, rank, dev, with_cpu_baseline, guard=True, maker=None, golden=True, full=True, dump=None):
    """Sets up one workload, warms up, times `args.steps` steps, writes the last step's outputs to `dump` (a directory) if given.  A plain run
    (full=False) returns the headline record; full=True adds the stage events of the timed steps, the roofline, the checks and the evaluation of
    what was timed and, with `with_cpu_baseline`, the CPU oracle's throughput.  Ranks other than 0 return None."""
    import torch
    import torch.distributed as dist
    from gims_amd import shard
    my_pairs = shard.shard_indices(world * pairs, rank, world)     # pair i -> rank i mod world
    rank_counts = [len(shard.shard_indices(world * pairs, r, world)) for r in range(world)]
    inputs = make_inputs(my_pairs, kpts, dev, maker)
    torch.cuda.synchronize()

    host_t = {"match_pairs": [], "stats": []}

    def step():
        datas = [dict(d) for d, _ in inputs]              # shallow copies: forward mutates the dict, tensors stay resident
        t0 = time.perf_counter()
        outs = model.match_pairs(datas)
        host_t["datas"] = datas
        t1 = time.perf_counter()
        # per-pair match statistics, all-gathered over RCCL/xGMI: the path's only collective
        stats = shard.gather_stats(shard.pair_stats(my_pairs, outs, dev), counts=rank_counts, presorted=my_pairs == sorted(my_pairs))
        host_t["match_pairs"].append(1e3 * (t1 - t0))
        host_t["stats"].append(1e3 * (time.perf_counter() - t1))
        return outs, stats

    model.enable_timing(False)
    # attention_precision='auto': the first batch after the weights are loaded measures the softmax peakedness of every layer
    # at bf16x3 and decides the kernel per layer; that call is never a timed one (nor a counted warm-up step)
    rep0 = model.attention_report()
    if model.config["attention_precision"] == "auto" and (rep0 is None or not rep0["calibrated"]):
        step()
        torch.cuda.synchronize()
        model.attention_report()
    for _ in range(args.warmup):
        step()
    # long-lived objects (weights, inputs, packed planes) are moved out of the cyclic GC's working set: a full
    # collection over them costs tens of milliseconds and would land inside a timed step
    import gc
    gc.collect()
    gc.freeze()
    gc.disable()           # and no collection at all inside the K timed steps (re-enabled right after them)
    model.enable_timing(full and os.environ.get("GIMS_BENCH_NO_STAGE_TIMERS") is None)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    from gims_amd import hip as _hip
    if full:
        _hip.attention_launch_counts(reset=True)          # which attention kernel serves the TIMED steps (host-side counters of the library)
    # HIP events cost time too (measured: 2.1 % of a 4096 x 8 step when every launch of every timed step is bracketed): the stage / per-launch
    # events are recorded on every `--event-every`-th timed step (default 5: steps 2, 7, 12, 17 of K = 20 -- mid-stride, so that the sample weighs
    # the first step after the synchronisation, which runs 10 % slower on a clock that has just idled, like the K steps do: not at all
    # rather than at 1 in 4), the other steps run bare
    timers = model._timers
    every, ev_idx = event_steps(args.steps, args.event_every)
    ev_steps = len(ev_idx) if timers is not None else 0
    t0 = time.perf_counter()
    for i in range(args.steps):
        if timers is not None:
            model._timers = timers if i in ev_idx else None
        outs, stats = step()
    model._timers = timers
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    attn_counts = {k: v / args.steps for k, v in _hip.attention_launch_counts().items() if v} if full else None
    gc.enable()
    et = torch.tensor([elapsed], device=dev, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(et, op=dist.ReduceOp.MAX)
    elapsed = float(et.item())
    if dump:
        names = dump_outputs(dump, my_pairs, outs, host_t["datas"], stats if rank == 0 else None, world)
        log(f"outputs of the last timed step: {len(names)} arrays in {dump}")
    if not full:
        arep = model.attention_report()          # (folds the last batch's measurement into the per-layer verdict, as the full record does)
        fixed = model.config["attention_precision"]
        modes = list(arep["modes"]) if arep else [fixed if fixed in ("bf16x3", "f16") else "bf16"] * len(model.config["transformer_layers"])
        if rank != 0:
            return None
        res = headline_record(model, kpts, pairs, args, world, elapsed, outs, modes, 0, 0)
        res["stats_rows_gathered"] = int(stats.shape[0])
        res["world_size_seen"] = dist.get_world_size() if world > 1 else 1
        return res
    if model._timers is None:          # diagnostic mode: no stage timers -> no roofline section
        log("host ms/step  match_pairs: " + " ".join(f"{x:6.2f}" for x in host_t["match_pairs"][-args.steps:]))
        return {"value": world * pairs * args.steps / elapsed, "ms_per_step": 1e3 * elapsed / args.steps, "diagnostic": True}
    stage = model.stage_times_ms()
    log(f"---- 2x{kpts} x {pairs} pairs/step")
    log("host ms/step  match_pairs: " + " ".join(f"{x:6.2f}" for x in host_t["match_pairs"][-args.steps:]))
    log("host ms/step  stats      : " + " ".join(f"{x:6.2f}" for x in host_t["stats"][-args.steps:]))
    model.enable_timing(False)

    # ---- correctness guard of what was timed: planted correspondences must be recovered
    assert stats.shape[0] == world * pairs, "the all-gather must return one record per pair of the whole job"
    o, (d, gt) = outs[0], inputs[0]
    m0 = o["matches0"][0].cpu().numpy()
    st = stats.cpu().numpy()

    # ---- evaluation of what was timed (outside the timed region): the synthetic pairs are a permutation + jitter of one
    # point set, i.e. their ground-truth homography is the identity; GT matching, precision / recall, 4-point and RANSAC
    # homographies and the corner-error AUC run on the device (gims_eval_pairs) and the per-pair records are all-gathered
    # exactly like the reference's eval loop would (eval_homography.py:186-259)
    eval_rec = shard.gather_stats(shard.eval_stats(my_pairs, host_t["datas"], outs, [np.eye(3, dtype=np.float32)] * len(my_pairs), dev,
                                                   ransac_iters=3000, seed=1), counts=rank_counts)
    eval_summary = shard.eval_summary(eval_rec)
    ranks_seen = None
    if world > 1:          # proof that the collective backend saw `world` ranks: every rank's (rank, device index, device name, backend)
        ranks_seen = [None] * world
        dist.all_gather_object(ranks_seen, (rank, torch.cuda.current_device(), torch.cuda.get_device_name(), dist.get_backend(), os.getpid()))
    if rank != 0:
        return None

    iters = int(model.config["sinkhorn_iterations"])
    flats = outs.flat if isinstance(outs.flat, (list, tuple)) else [outs.flat]
    problems = [(a, b) for f in flats for a, b in zip(f["n0"], f["n1"])]
    nl = getattr(model, "n_lanes_last", 1)          # stream lanes: each stage is launched once per lane
    stage_ms = {k: float(np.sum(v)) / ev_steps for k, v in stage.items()}
    for k, v in stage.items():
        per = np.asarray(v).reshape(ev_steps, -1).sum(1)
        log(f"stage {k:14s} gpu ms/step: " + " ".join(f"{x:7.2f}" for x in per))
    # algorithmic work per step on this rank (SURVEY 8d formulas, on the kept counts)
    attn_flops_layer = sum(1024.0 * (a * a + b * b) for a, b in problems)          # self layer (both images)
    cross_flops_layer = sum(1024.0 * (2 * a * b) for a, b in problems)
    n_rows = sum(a + b for a, b in problems)
    fused = bool(model.config["fuse_merge"])
    lpl = int(getattr(model, "linear_launches_per_layer", 3 if fused else 4))      # linear launches per layer
    # executed linear flops per layer (with the merge conv folded into MLP0 the 256x256 merge GEMM disappears)
    lin_flops_layer = 2.0 * n_rows * (3 * 256 * 256 + (0 if fused else 256 * 256) + 512 * 512 + 512 * 256)
    ot_bytes = sum(2.0 * iters * (a + 1) * (b + 1) * 4 for a, b in problems)
    ot_fma_flops = sum(4.0 * iters * a * b for a, b in problems)   # resident kernel: one fma per entry per row sweep + one per column sweep
    n_self = sum(1 for t in model.config["transformer_layers"] if t == "self")
    n_cross = len(model.config["transformer_layers"]) - n_self
    L = n_self + n_cross
    per_step = lambda name: float(np.sum(stage.get(name, [0.0]))) / ev_steps          # noqa: E731
    # kernel -> (bound, algorithmic work per launch, avg launch ms (HIP events on the launch stream), peak, unit, launches/step)
    # The "qkv" and "mlp" intervals contain ONLY launches of the split-bf16 GEMM kernel.
    lin_name = "linear_x3p_kernel"
    # which attention kernel every layer ran in the timed steps (attention_precision='auto' decides per layer; the stage
    # labels of the bf16x3 layers carry an _x3 suffix)
    arep = model.attention_report()
    fixed = model.config["attention_precision"]
    modes = list(arep["modes"]) if arep else [fixed if fixed in ("bf16x3", "f16") else "bf16"] * L
    kinds = list(model.config["transformer_layers"])
    cnt = lambda kind, mode: sum(1 for k, m in zip(kinds, modes) if k == kind and m == mode)          # noqa: E731
    cand = {
        lin_name: ("mfma", lin_flops_layer / (lpl * nl), (per_step("qkv") + per_step("qkv_f16") + per_step("qkv_x3") + per_step("mlp")) / (lpl * L * nl),
                   PEAK_BF16_TFLOPS, "TFLOP/s", lpl * L * nl),
    }
    # which split-bf16 attention kernel a launch of this workload takes (the rule of gims_attention: the wide kernel when two 256-query
    # workgroups per CU still fill the chip)
    heads = 4
    groups = 2 * pairs * heads // max(1, nl)
    x3_name = "attention_x3w_kernel" if 8 * -(-groups // 8) * -(-kpts // 256) >= 512 else "attention_x3_kernel"
    f16_name = "attention8_bf16_kernel<F16>"
    for kname, mode, sfx in (("attention8_bf16_kernel", "bf16", ""), (f16_name, "f16", "_f16"), (x3_name, "bf16x3", "_x3")):
        nl_k = cnt("self", mode) + cnt("cross", mode)
        if nl_k:
            cand[kname] = ("mfma", (cnt("self", mode) * attn_flops_layer + cnt("cross", mode) * cross_flops_layer) / (nl_k * nl),
                           (per_step("attn_self" + sfx) + per_step("attn_cross" + sfx)) / (nl_k * nl), PEAK_BF16_TFLOPS, "TFLOP/s", nl_k * nl)
    # Sinkhorn.  Streamed path: one ot_iter_kernel launch per iteration, HBM-bound, priced with SURVEY 8(d)'s algorithmic
    # bytes.  Resident path: `ot_plan` launches per step run ALL iterations with the matrix held in registers + LDS -- no HBM
    # traffic inside the loop, so HBM is not its roof: it is priced on the fp32 vector-ALU roof (2 fma per entry per
    # iteration); SURVEY's byte figure is reported as `hbm_equivalent` for orientation only.
    ot_plan = int(getattr(model, "sinkhorn_plan_last", 0))
    if ot_plan > 0:
        ot_name = "ot_res2_kernel"
        cand[ot_name] = ("valu", ot_fma_flops / ot_plan, per_step("sinkhorn") / ot_plan, PEAK_F32_VALU_TFLOPS, "TFLOP/s", ot_plan)
    else:
        ot_name = "ot_iter_kernel"
        cand[ot_name] = ("hbm", ot_bytes / max(1, iters), per_step("sinkhorn") / max(1, iters), PEAK_HBM_GBS, "GB/s", iters)
    if args.linear_precision != "bf16x3":
        cand["linear_f32_kernel"] = cand.pop(lin_name)[:3] + (157.3, "TFLOP/s", lpl * L)
    totals = {k: v[2] * v[5] for k, v in cand.items()}
    dom = max(totals, key=totals.get)
    rate = lambda v: v[1] / (v[2] * 1e-3) / (1e12 if v[4] == "TFLOP/s" else 1e9)     # noqa: E731
    bound, work, ms, peak, unit, n_launch = cand[dom]
    traffic_tab, traffic_head = {}, None
    tf = os.path.join(ROOT, "profiles", "pmc_traffic.json")       # HBM bytes per launch from rocprofv3 --pmc runs of this command
    if os.path.exists(tf):
        tall = json.load(open(tf))
        traffic_tab = tall.get(f"{kpts}x{pairs}", {})
        traffic_head = (tall.get("_meta") or {}).get("head")

    def traffic_of(name):
        t = traffic_tab.get(name)
        return t.get("hbm_bytes_per_launch") if t else None

    notes = {
        "ot_iter_kernel": "`achieved` uses SURVEY 8(d)'s algorithmic bytes (TWO sweeps of the (N+1)x(M+1) matrix per iteration); the streamed "
                          "kernel reads the matrix ONCE per iteration, so frac can approach 2 x (real HBM rate / peak); real HBM bytes are in `traffic`",
        "ot_resident_kernel": "on-chip Sinkhorn: exp(Z+u+v) stays in registers + LDS for all iterations (no HBM traffic in the loop; real HBM bytes per "
                              "launch in `traffic`), so it is priced on the fp32 vector roof: 2 fma per matrix entry per iteration / 157.3 TFLOP/s; the "
                              "iteration is dominated by the cross-workgroup exchange of column sums (DESIGN.md 4.1), not by the ALU",
        "ot_res2_kernel": "on-chip Sinkhorn, 2-D decomposition (row groups per XCD x 128-column blocks per CU): exp(Z+u+v) stays in registers + LDS for all "
                          "iterations, the wide exchanges stay inside one XCD's L2 and one 0.5-KB edge crosses XCDs (DESIGN.md 4.1); priced on the fp32 "
                          "vector roof: 2 fma per matrix entry per iteration / 157.3 TFLOP/s; `avg_launch_ms` is the stage time (init + solve + selection) "
                          "per on-chip launch",
        x3_name: "the same flash attention on split-bf16 operand pairs (Q, K, V from the 3-pass projection, P split in registers): THREE "
                               "bf16 MFMAs per algorithmic product (hi*hi + hi*lo + lo*hi); `achieved` counts ALGORITHMIC flops, `mfma_issue_frac` is 3x that",
        f16_name: "the bf16 flash kernel instantiated on IEEE-half operands (v_mfma_f32_32x32x16_f16, same rate): Q, K, V from the 3-pass projection "
                  "rounded to half, P rounded to half against a lazily raised row reference (one subtraction per score more than the reference-free "
                  "bf16 pass); holds the 1e-4 score bar on peaked softmaxes where bf16 operands do not",
        "attention8_bf16_kernel": "flash-style attention, head dim 64: per 64-key tile a wave issues 16 MFMAs against ~2 VALU/transcendental issues per "
                                  "score for the softmax, and MFMA and VALU of one SIMD do not overlap (DESIGN.md 4.2); `achieved` counts 4*N*M*64 flops per head",
        lin_name: "split-bf16 GEMMs of a layer: 3 bf16 MFMA passes per algorithmic product (hi*hi+hi*lo+lo*hi, f32-class accuracy) in the MLP and 1 pass "
                  "(plain bf16) in the Q/K/V projection; `achieved` counts ALGORITHMIC flops 2MNK averaged over the launches of a layer, so its ceiling "
                  "against the 2.5 PF/s bf16 peak is about 0.4",
    }
    allk = {k: {"bound": v[0], "avg_launch_ms": float(v[2]), "launches_per_step": v[5], "achieved": rate(v), "unit": v[4],
                "peak": v[3], "frac": rate(v) / v[3], "traffic": traffic_of(k)} for k, v in cand.items()}
    if x3_name in allk:
        allk[x3_name]["mfma_passes"] = 3
        allk[x3_name]["mfma_issue_frac"] = 3.0 * allk[x3_name]["frac"]
    if ot_plan > 0:
        hb = ot_bytes / ot_plan / (cand[ot_name][2] * 1e-3) / 1e9
        allk[ot_name]["hbm_equivalent"] = {"achieved": hb, "unit": "GB/s", "note": "SURVEY 8(d) bytes / time: what a streamed implementation would "
                                           "have to move; NOT a roofline fraction of this kernel (the matrix never leaves the chip)"}
    # second view of the GEMM launches: short-K products (K = 256 / 512) over 4-byte-per-element operands and results
    lin_bytes_launch = n_rows * (256 * 2 + 768 * 2 + 512 * 4 + 512 * 4 + 512 * 4 + 3 * 256 * 4) / (lpl * nl) if fused else None
    if lin_bytes_launch and lin_name in cand:
        lms = cand[lin_name][2]
        allk[lin_name]["hbm_view"] = {"algorithmic_bytes_per_launch": lin_bytes_launch, "achieved": lin_bytes_launch / (lms * 1e-3) / 1e9,
                                      "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": lin_bytes_launch / (lms * 1e-3) / 1e9 / PEAK_HBM_GBS}
    roofline = {"kernel": dom, "bound": bound, "achieved": rate(cand[dom]), "peak": peak, "unit": unit,
                "frac": rate(cand[dom]) / peak, "traffic": traffic_of(dom),
                "traffic_source": "profiles/pmc_traffic.json (static: rocprofv3 --pmc passes of this command, not measured in this run)",
                "traffic_profile_head": traffic_head,
                "avg_launch_ms": float(ms), "launches_per_step": n_launch, "algorithmic_work_per_launch": work,
                "note": notes.get(dom, ""), "all": allk}
    # the fraction north_star names: cross-attention against the bf16 MFMA roof (the kernel family most cross layers ran)
    xmode = max(("bf16", "f16", "bf16x3"), key=lambda md: cnt("cross", md))
    n_x = cnt("cross", xmode)
    xms = per_step("attn_cross" + {"bf16": "", "f16": "_f16", "bf16x3": "_x3"}[xmode]) / max(1, n_x * nl)
    cross = {"kernel": {"bf16": "attention8_bf16_kernel", "f16": f16_name, "bf16x3": x3_name}[xmode], "bound": "mfma", "avg_launch_ms": xms,
             "launches_per_step": n_x * nl, "achieved": cross_flops_layer / nl / (xms * 1e-3) / 1e12 if xms > 0 else 0.0,
             "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "mfma_passes": 3 if xmode == "bf16x3" else 1, "operands": xmode}
    cross["frac"] = cross["achieved"] / PEAK_BF16_TFLOPS
    cross["mfma_issue_frac"] = cross["mfma_passes"] * cross["frac"]
    k0 = host_t["datas"][0]["kept_kpts0_indices"][0].cpu().numpy()
    k1 = host_t["datas"][0]["kept_kpts1_indices"][0].cpu().numpy()
    v = m0 >= 0
    correct = int((k1[m0[v]] == gt[k0[v]]).sum())
    if guard:
        assert v.sum() > 0.5 * kpts and correct > 0.9 * v.sum(), ("benchmark output is not a valid matching", int(v.sum()), correct)
    # ... and, where the reference's own output for a pair of the batch is on file, that is the guard: every row, scores within 1e-4
    parity = None
    if maker is None and golden:          # (golden=False: other weights than the fixtures')
        parity = golden_parity(kpts, iters, float(model.config["match_threshold"]), my_pairs, outs, host_t["datas"])
        if parity and guard:
            bad = [p for p in parity if not p["rows_equal"] or not p["max_score_err"] < 1e-4]
            assert not bad, ("the timed batch differs from the reference golden", bad)
    steps_ms = np.asarray(host_t["match_pairs"][-args.steps:]) + np.asarray(host_t["stats"][-args.steps:])
    res = headline_record(model, kpts, pairs, args, world, elapsed, outs, modes, ev_steps, every)
    res.update({
        "roofline": roofline,
        "cross_attention": cross,
        "attention": {"precision": fixed, "layers_bf16": modes.count("bf16"), "layers_f16": modes.count("f16"), "layers_bf16x3": modes.count("bf16x3"),
                      "threshold": arep["threshold"] if arep else None, "tail_threshold": arep["tail_threshold"] if arep else None,
                      "peak_per_layer": [round(float(x), 4) for x in arep["peak"].max(1)] if arep else None,
                      "tail_per_layer": [round(float(x), 4) for x in arep["tail"].max(1)] if arep else None,
                      "operand_range_per_layer": [round(float(x), 2) for x in arep["range"].max(1)] if arep else None,
                      "note": "peak = mean over the queries of the largest softmax probability, tail = fraction of queries whose largest probability "
                              "exceeds 1/2 (worst head per layer), range = max |Q|, |K|, |V| as stored -- all reported by the attention kernels; 'auto' runs "
                              "a layer on IEEE-half operands (same MFMA rate, 3-pass projection) when peak or tail exceed their thresholds, on "
                              "split-bf16 pairs (3 MFMA passes) only when the operands leave half's range"},
        "stage_ms_per_step": stage_ms,
        "host_step_ms": {"median": float(np.median(steps_ms)), "max": float(steps_ms.max())},
        "matches_pair0": {"matched": int(v.sum()), "correct_vs_planted": correct},
        "parity_vs_reference": parity,
        "attention_launches_per_step": attn_counts,        # e.g. {"wave8": 18, "x3_guarded": 18}: the 8-wave bf16 kernel + the guarded redo launches
        "sinkhorn_rescues": int(__import__("gims_amd.hip", fromlist=["hip"]).sinkhorn_rescues()),       # on-chip solves of this process that gave up and were re-solved (0 on a quiet GPU)
        "stats_rows_gathered": int(st.shape[0]), "stat_fields": list(shard.STAT_FIELDS),
        "world_size_seen": dist.get_world_size() if world > 1 else 1,
        "ranks": [{"rank": r[0], "device": r[1], "device_name": r[2], "backend": r[3], "pid": r[4]} for r in ranks_seen] if ranks_seen else None,
        "eval": {"note": "quality of the timed outputs against the planted correspondences (identity homography): GT matching, "
                         "precision / recall, corner-error AUC of the 4-point and RANSAC homographies (gims_eval_pairs + all-gather).  "
                         "The RANSAC here is this library's own sampler and 4-point solver: its inlier sets are NOT those of "
                         "cv2.findHomography(..., RANSAC) (eval_homography.py:191, 216-227; OpenCV is absent from this image, so that parity is "
                         "unpinned) -- the AUC values are on synthetic pairs and are not COCO numbers",
                 **{k: (round(v, 3) if isinstance(v, float) else [round(x, 3) for x in v] if isinstance(v, list) else v)
                    for k, v in eval_summary.items()}},
    })
    if with_cpu_baseline:
        res["cpu_baseline"] = cpu_baseline(kpts, iters, budget_s=args.cpu_budget if (kpts, pairs) == HEADLINE or args.kpts is not None else args.cpu_budget / 3.0,
                                           thr=float(model.config["match_threshold"]))
    return res


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kpts", type=int, default=None, help="keypoints per image (default: the 4096 headline; with --full + the 1024 block)")
    ap.add_argument("--pairs", type=int, default=None, help="image pairs per step per GPU (default 8 at 4096, 32 otherwise)")
    ap.add_argument("--sinkhorn-iters", type=int, default=100)
    ap.add_argument("--linear-precision", default="bf16x3", choices=["bf16x3", "f32"])
    ap.add_argument("--attention-precision", default="auto", choices=["auto", "bf16", "f16", "bf16x3"],
                    help="'auto' (default): per-layer tiers decided from measured softmax statistics, with the device-side redo; the others fix one tier")
    ap.add_argument("--streams", type=int, default=1, help="independent sub-batches per step on separate HIP streams (1 = single stream)")
    ap.add_argument("--event-every", type=int, default=5, help="record the stage / per-launch HIP events on every n-th timed step (1 = every step: costs 2 %% of the headline step)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-budget", type=float, default=60.0, help="seconds of CPU-oracle work for the headline workload (a third of it for the second block)")
    ap.add_argument("--latency", action="store_true", help="also time ONE pair through the reference-shaped forward() (latency_ms_b1)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed step as DIR/<name>.npy (float32 / float64, at most 64 MB; see dump_outputs)")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline figure: stage events, roofline, checks and evaluation of the timed batch, CPU baseline, "
                         "the other workloads and precisions, latency, pipeline and training step, bench_extra.json")
    return ap


def main():
    args = parser().parse_args()

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(spawn_ranks(args.gpus))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # N > 1: every rank keeps to its own slice of the host's cores (the step is host-bound within ~1 % of the GPU time: N interpreters, their
    # launch threads and torch's intra-op pools must not fight over the same cores).  Done BEFORE anything touches the GPU or starts a thread
    # pool.  GIMS_BENCH_NO_PIN=1 leaves the affinity alone.
    full_affinity = sorted(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None
    host_threads = None
    if world > 1 and full_affinity and os.environ.get("GIMS_BENCH_NO_PIN") is None:
        mine = rank_affinity(full_affinity, local_rank, int(os.environ.get("LOCAL_WORLD_SIZE", str(world))))
        if mine:
            os.sched_setaffinity(0, mine)
            host_threads = min(len(mine), 16)
            os.environ.setdefault("OMP_NUM_THREADS", str(host_threads))
    import torch
    if host_threads:
        torch.set_num_threads(host_threads)
    elif world == 1:
        # the timed loop has no CPU-parallel work; an intra-op pool as wide as a 256-core host only adds spinning threads next to the launch thread
        host_threads = min(16, len(full_affinity) if full_affinity else (os.cpu_count() or 1))
        torch.set_num_threads(host_threads)
    if world != args.gpus:
        log(f"note: --gpus {args.gpus} but WORLD_SIZE={world}; using WORLD_SIZE")
    import torch.distributed as dist
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        # GIMS_BENCH_BACKEND=gloo + fewer GPUs than ranks is a DRY RUN of the multi-rank code path on one GPU (ranks share
        # the device; combine with GIMS_OT_RESIDENT=0: the on-chip Sinkhorn kernel needs the whole GPU to itself)
        backend = os.environ.get("GIMS_BENCH_BACKEND", "nccl")
        local_dev = local_rank % max(1, torch.cuda.device_count())
        torch.cuda.set_device(local_dev)
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_dev))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    else:
        torch.cuda.set_device(0)
    dev = f"cuda:{torch.cuda.current_device()}"
    torch.set_grad_enabled(False)

    import __graft_entry__
    if world > 1:            # one rank per node (re)builds a stale library, the others wait: no concurrent hipcc runs on one tree
        if local_rank == 0:
            __graft_entry__.build()
        dist.barrier()
    __graft_entry__.build()
    from gims_amd import GMatcher, synth

    model = GMatcher({"sinkhorn_iterations": args.sinkhorn_iters, "linear_precision": args.linear_precision,
                      "streams": args.streams, "attention_precision": args.attention_precision}).eval()
    model.load_state_dict(synth.make_state_dict(123))

    if args.kpts is not None:
        loads = [(args.kpts, args.pairs if args.pairs is not None else (8 if args.kpts >= 4096 else 32))]
    else:
        loads = [HEADLINE, SECOND] if args.full else [HEADLINE]
    blocks = args.full and args.kpts is None          # the extra blocks below: --full with no workload flags
    base = args.full and world == 1 and not args.no_cpu_baseline
    results = [run_workload(model, k, p, args, world, rank, dev, base, full=args.full, dump=args.dump_outputs if i == 0 else None)
               for i, (k, p) in enumerate(loads)]
    if rank == 0 and results[0] is not None:
        results[0]["host_threads_per_rank"] = host_threads if host_threads else torch.get_num_threads()
    peaked = None
    if blocks:
        # the same headline workload with PEAKED attention (query / key projections of every layer scaled up like the
        # `peakede2e_*` reference goldens: mean softmax row maximum ~0.8): 'auto' routes those layers to the IEEE-half kernels --
        # the throughput of the mode that keeps the 1e-4 score bar there
        model_p = GMatcher({"sinkhorn_iterations": args.sinkhorn_iters, "linear_precision": args.linear_precision, "streams": args.streams}).eval()
        model_p.load_state_dict(synth.make_state_dict(123, gains={"attn.proj.0": 2.0, "attn.proj.1": 2.0}))
        peaked = run_workload(model_p, HEADLINE[0], HEADLINE[1], args, world, rank, dev, False, guard=False, golden=False)
        del model_p
    evalset = None
    if blocks:
        # the reference's eval scripts run sinkhorn_iterations=20, match_threshold=0.02 (eval_homography.py:117-119, eval_matches.py:135):
        # the headline workload at that setting (parity: the e2e_*_i20 goldens)
        model_e = GMatcher({"sinkhorn_iterations": 20, "match_threshold": 0.02, "linear_precision": args.linear_precision, "streams": args.streams}).eval()
        model_e.load_state_dict(synth.make_state_dict(123))
        evalset = run_workload(model_e, HEADLINE[0], HEADLINE[1], args, world, rank, dev, False, guard=False)
        del model_e
    readme = None
    if blocks and world == 1:
        # the reference's one PUBLISHED hot-path configuration (README.md:143-163: 15 382 / 14 870 keypoints, N != M; eval setting: 20 iterations,
        # threshold 0.02; graph build 5.72 + 6.19 s and matching 3.48 s on an RTX 3090 there), on the density-matched synthetic pair the
        # `ube2e_n15382_*` reference golden pins; 2 pairs per step
        try:
            import copy
            from gims_amd import synth
            model_r = GMatcher({"sinkhorn_iterations": 20, "match_threshold": 0.02, "linear_precision": args.linear_precision}).eval()
            model_r.load_state_dict(synth.make_state_dict(123))
            a5 = copy.copy(args)
            a5.steps, a5.warmup = min(args.steps, 5), min(args.warmup, 2)
            readme = run_workload(model_r, 15382, 2, a5, world, rank, dev, False, guard=False,
                                  maker=lambda pid: synth.make_pair_unbalanced(15382, 14870, 12000, 3003 + pid))
            readme["agc_ms_per_image"] = readme["stage_ms_per_step"].get("agc", 0.0) / 4.0
            readme["config"]["setting"] = ("README.md:143-163 shape: 15382 / 14870 keypoints per pair (12000 in common), sinkhorn_iterations=20, "
                                           "match_threshold=0.02; the reference reports 5.72 + 6.19 s graph build and 3.48 s matching per pair on an RTX 3090")
            del model_r
        except Exception as e:   # noqa: BLE001  (an extra block: it must never cost the headline line)
            readme = {"error": f"{type(e).__name__}: {e}"}
    if rank == 0:
        res = results[0]
        if readme is not None:
            res.setdefault("also", {})["readme_boat_15k"] = readme
        if evalset is not None:
            evalset["config"]["setting"] = "the reference's eval scripts: sinkhorn_iterations=20, match_threshold=0.02 (eval_homography.py:117-119)"
            res.setdefault("also", {})[f"2x{HEADLINE[0]}_eval_setting"] = evalset
        if len(results) > 1:
            res.setdefault("also", {}).update({f"2x{k}": r for (k, _), r in zip(loads[1:], results[1:])})
        if peaked is not None:
            peaked["config"]["weights"] = "synthetic, query/key projection gain 2.0 (the `peakede2e_*` goldens' weights): peaked softmax rows"
            res.setdefault("also", {})[f"2x{HEADLINE[0]}_peaked_attention"] = peaked
        if world == 1 and blocks:
            # BASELINE config 5: CAR-HyNet descriptors for both images + 2x8192-keypoint matching, 2 pairs per step
            try:
                from tools.pipeline_bench import measure as pipeline_measure, measure_from_images
                res.setdefault("also", {})["pipeline_2x8192"] = pipeline_measure(8192, 2, 3)
                # the same chain with SURVEY row f4 (patch extraction from a resident image + keypoints) inside the timed region
                res["also"]["pipeline_2x8192"]["from_images"] = measure_from_images(8192, 2, 3)
            except Exception as e:   # noqa: BLE001
                res.setdefault("also", {})["pipeline_2x8192"] = {"error": f"{type(e).__name__}: {e}"}
        if world == 1 and (args.latency or blocks):
            res["latency_ms_b1"] = latency_b1(model, [k for k, _ in loads], dev)
        if world == 1 and blocks:
            # one training step (train() mode forward, backward, Adam) per pair of 2x2048 keypoints, the
            # reference's training configuration; its CPU leg (one oracle step, ~5 s) only next to the main CPU baseline
            try:                     # an extra block: it must never cost the headline line
                from tools.train_bench import measure as train_measure
                res["train_step"] = train_measure(2048, 6, 2, "bf16x6", with_cpu=base)
            except Exception as e:   # noqa: BLE001
                res["train_step"] = {"error": f"{type(e).__name__}: {e}"}
    if world > 1:
        dist.destroy_process_group()
    if rank == 0:
        if world > 1 and args.full and not args.no_cpu_baseline:
            # N > 1: the CPU baseline of rank 0 AFTER the job (the other ranks are gone, the collective backend is shut down), on the
            # host's full core set again -- a SCALE record then carries its own baseline
            if full_affinity:
                os.sched_setaffinity(0, full_affinity)
            try:
                res["cpu_baseline"] = cpu_baseline(loads[0][0], args.sinkhorn_iters, budget_s=args.cpu_budget)
            except Exception as e:   # noqa: BLE001  (never lose the line of a multi-GPU run to its baseline)
                res["cpu_baseline"] = {"error": f"{type(e).__name__}: {e}"}
        if args.full:
            log(f"full record: {write_extra(res)}")
        sys.stderr.flush()
        print(compact_line(res, extra="bench_extra.json" if args.full else None), flush=True)


def latency_b1(model, sizes, dev):
    """ONE pair through the reference-shaped GMatcher.forward (B = 1, what eval_homography.py does per pair): median wall
    time of a call including its device synchronisation, steady state."""
    import torch
    out = {}
    for kpts in sizes:
        (d, _), = make_inputs([0], kpts, dev)
        ts = []
        for i in range(12):
            dd = dict(d)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model(dd)
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        out[f"2x{kpts}"] = float(np.median(ts[4:]))
    return out


if __name__ == "__main__":
    main()
