#!/usr/bin/env python3
"""Every output of ``hip.verify_pairs`` on a fixed list of sets, written to one ``.npz`` -- to compare two commits byte for byte
(a change of the kernels of csrc/verify.hip that is meant to change no output).

    python tools/verify_dump.py -o this.npz             # in a checkout of this commit, and
    python tools/verify_dump.py -o parent.npz           # the same file in a checkout of the other one, in a process of its own
    python tools/verify_dump.py --compare parent.npz this.npz

The scenes are those of tests/verify_ref.py, tests/fundamental_ref.py and tests/pose_ref.py and nothing else of the repository is read, so
the file runs unchanged in a checkout that has these three and ``gims_amd.hip.verify_pairs``.

Sets: 5 homography sets (K = 3 .. 2049), 10 fundamental sets (K = 7 .. 2049 on both scenes), 20 pose sets (K = 4 .. 2049 on the four
scenes).  Every set runs at iters in {17, 500, 3000} x lo_iters in {0, 8}, once in one call per model (at the threshold of its restatement)
and once in one call of all 35 (3 px).  Arrays per set run: the mask, the record, the model / pose floats.

``--compare`` prints the number of arrays compared and of set runs with a model, names the first array that differs, and exits 1 if there
is one."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ITERS = (17, 500, 3000)
LO_ITERS = (0, 8)
SEED = 1
MIXED_THRESH = 3.0


def make_sets():
    """[(name, model, thresh of a single-model call, kp0, kp1, matches0, intrinsics or None)]"""
    from tests import fundamental_ref as RF, pose_ref as RP, verify_ref as RH
    sets = []
    for K in (3, 5, 64, 257, 2049):
        kp0, kp1, m0 = RH.planted_spec(K)[:3]
        sets.append((f"K{K}", "homography", RH.THRESH, kp0, kp1, m0, None))
    for config in RF.CONFIGS:
        for K in (7, 9, 65, 1025, 2049):
            kp0, kp1, m0 = RF.planted_spec(K, config)[:3]
            sets.append((f"{config}_K{K}", "fundamental", RF.THRESH, kp0, kp1, m0, None))
    for config in RP.CONFIGS:
        for K in (4, 6, 65, 257, 2049):
            kp0, kp1, m0 = RP.planted_spec(K, config)[:3]
            sets.append((f"{config}_K{K}", "pose", RP.THRESH, kp0, kp1, m0, RP.cameras(config)[:2]))
    return sets


def run(sets, thresh, iters, lo_iters, out, prefix):
    import torch
    from gims_amd import hip
    dev = torch.device("cuda", torch.cuda.current_device())
    items = []
    for name, model, _, kp0, kp1, m0, cams in sets:
        it = dict(kpts0=torch.from_numpy(kp0).to(dev), kpts1=torch.from_numpy(kp1).to(dev), matches0=torch.from_numpy(m0).to(dev),
                  inlier=torch.full((len(kp0),), 255, dtype=torch.uint8, device=dev), record=torch.full((8,), -7.0, device=dev),
                  homography=torch.full((hip.VERIFY_POSE_FLOATS if model == "pose" else 9,), -7.0, device=dev), model=model)
        if cams is not None:
            it["intrinsics"] = cams
        items.append(it)
    work = hip.verify_pairs(items, thresh, iters, lo_iters, SEED)
    torch.cuda.synchronize()
    del work
    for (name, model, *_), it in zip(sets, items):
        key = f"{prefix}/{model}/{name}/iters{iters}/lo{lo_iters}"
        out[key + "/mask"] = it["inlier"].cpu().numpy()
        out[key + "/record"] = it["record"].cpu().numpy()
        out[key + "/model"] = it["homography"].cpu().numpy()


def dump(path):
    sets = make_sets()
    out = {}
    for iters in ITERS:
        for lo_iters in LO_ITERS:
            for model in ("homography", "fundamental", "pose"):
                own = [s for s in sets if s[1] == model]
                run(own, own[0][2], iters, lo_iters, out, "single")
            run(sets, MIXED_THRESH, iters, lo_iters, out, "mixed")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **out)
    with_model = sum(1 for k, v in out.items() if k.endswith("/record") and v[1] == 1.0)
    print(f"verify_dump: {len(out)} arrays of {len(out) // 3} set runs, {with_model} with a model -> {path}")


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    if sorted(a.files) != sorted(b.files):
        print(f"verify_dump: the two files hold different arrays ({len(a.files)} and {len(b.files)})")
        return 1
    with_model = 0
    for k in sorted(a.files):
        x, y = a[k], b[k]
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            print(f"verify_dump: {k} differs\n  {path_a}: {x.ravel()[:24]}\n  {path_b}: {y.ravel()[:24]}")
            return 1
        with_model += int(k.endswith("/record") and x[1] == 1.0)
    print(f"verify_dump: {len(a.files)} arrays of {len(a.files) // 3} set runs are byte for byte equal, {with_model} set runs with a model")
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-o", "--output", default="verify_dump.npz")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), help="compare two dumps instead of running")
    args = ap.parse_args(argv)
    if args.compare:
        return compare(*args.compare)
    dump(args.output)
    return 0


if __name__ == "__main__":
    sys.exit(main())
