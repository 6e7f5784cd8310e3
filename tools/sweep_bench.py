#!/usr/bin/env python3
"""Settings per second of a parameter sweep over ONE pair: ``GMatcher.sweep`` (--mode sweep) against one ``forward()`` call per setting
(--mode forward: what a caller of the reference's tools/parameter_search.py does, and all a tree without ``sweep`` can do).  bench.py is
the project's yardstick and is not touched by this.

    python tools/sweep_bench.py --mode sweep   [--tree DIR] [--repeat 8] [--passes 2]
    python tools/sweep_bench.py --mode forward --tree PARENT_CHECKOUT

``--tree`` names the source tree whose ``gims_amd`` is imported (default: this one), so that one copy of this script times two commits in
alternating processes of one GPU command.  The grid is r {10, 15, 22, 30} x t {0, 2, 5, 10} x m {0, 1, 7, 10} (64 settings) repeated
``--repeat`` times, on synth.make_pair(4096, 1000) and on the sparse synth.make_pair(1024, 2001, canvas=(800, 600)); model settings
sinkhorn_iterations=20, match_threshold=0.02 as in parameter_search.py.  Per pair: one untimed pass over every setting (every shape warm),
then ``--passes`` timed passes, each a host clock around the whole pass that ends in a device synchronisation.  A setting under which an
image keeps nothing is caught (forward) or recorded (sweep) and counts as a setting, as parameter_search.py's loop does.  Prints ONE JSON line.
"""
import argparse
import json
import os
import sys
import time

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["sweep", "forward"], required=True)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--repeat", type=int, default=8)
    ap.add_argument("--passes", type=int, default=2)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from gims_amd import GMatcher, synth
    torch.set_grad_enabled(False)
    grid = [(r, t, m) for r in (10, 15, 22, 30) for t in (0, 2, 5, 10) for m in (0, 1, 7, 10)] * a.repeat
    model = GMatcher({"sinkhorn_iterations": 20, "match_threshold": 0.02}).eval()
    model.load_state_dict(synth.make_state_dict(123))
    res = {"mode": a.mode, "tree": os.path.abspath(a.tree), "settings": len(grid)}
    for name, pair in (("n4096_s1000", synth.make_pair(4096, 1000)), ("n1024sparse_s2001", synth.make_pair(1024, 2001, canvas=(800, 600)))):
        base = {k: torch.from_numpy(v).cuda() for k, v in pair.items() if k not in ("gt_perm", "image0", "image1")}
        base.update(image0=pair["image0"], image1=pair["image1"], device=torch.device("cuda"))

        def one_pass():
            empty = 0
            if a.mode == "sweep":
                recs = model.sweep(base, grid)
                empty = sum(r["error"] is not None for r in recs)
            else:
                for r, t, m in grid:
                    try:
                        model(dict(base, radius=r, percentile=t, min_size=m))
                    except ValueError:
                        empty += 1
            torch.cuda.synchronize()
            return empty
        empty = one_pass()                      # warm-up: every shape of the timed passes
        rates = []
        for _ in range(a.passes):
            t0 = time.perf_counter()
            one_pass()
            rates.append(len(grid) / (time.perf_counter() - t0))
        res[name] = {"settings_per_s": [round(x, 2) for x in rates], "settings_that_kept_nothing": empty}
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
