#!/usr/bin/env python3
"""Golden vectors at dustbin logits (bin_score, alpha) that matter, BY RUNNING THE REFERENCE ITSELF (build container only).

Every other fixture was made at synth's bin_score = 1.  On this project's synthetic weights the row maxima of the score matrix
run from ~45 to ~95, so alpha = 1 (and anything up to ~20) leaves the dustbin a far-away constant: the start potentials, the
re-derivation bounds of the on-chip Sinkhorn kernel and the dustbin terms of the reverse pass never see a competitive dustbin.
Here alpha is chosen PER PAIR from the reference's own score matrix (tapped with the log_optimal_transport spy of
tools/gen_golden.py): -2, about the 10th / 50th / 90th percentile of the row maxima, and one value above the largest row max
(nothing is matched).  Each alpha is rounded to float32 and stored with the weight seed; the tests read both from the fixture.

  bine2e_*   end-to-end outputs (kept ids, matches, scores, OT gaps) at five alphas for four pairs
  seede2e_*  end-to-end outputs at alpha = 1 with two more weight seeds (BN folding, merge-into-MLP0 fold, head permutation)
  binloss_*  forward_train's loss and d loss / d scores, d loss / d bin_score at the p50 / p90 alphas (layout of trainloss_*)
  binstep_*  one trainstep_*-style fixture (every parameter gradient) at the p50 alpha

Only seeds and outputs are stored.  Prints, and asserts, the matched fraction of every fixture.

    python tools/gen_golden_alpha.py [--only bin|seed|loss]
"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402  (imports the reference)
import gen_golden_grads as GG  # noqa: E402
import gen_golden_train as GT  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gims_amd import synth  # noqa: E402

WSEED = 123
# (tag, pair spec, iterations, match threshold); pair spec = [kind (0 make_pair, 1 make_pair_unbalanced), n0, n1, n_common, seed,
# canvas w, canvas h (0: synth's default)] -- tests/helpers.py:alpha_pair regenerates the pair from it
BIN_PAIRS = [("n256_s1002_i100", [0, 256, 256, 0, 1002, 0, 0], 100, 0.2),
             ("n1024_s1001_i20", [0, 1024, 1024, 0, 1001, 0, 0], 20, 0.02),
             ("n1500_900_c700_s3001_i100", [1, 1500, 900, 700, 3001, 0, 0], 100, 0.2),
             ("n1024sparse_s2001_i20", [0, 1024, 1024, 0, 2001, 800, 600], 20, 0.02)]
SEED_PAIRS = [("n1024_s1000_i100", [0, 1024, 1024, 0, 1000, 0, 0], 100, 0.2),
              ("n4096_s1001_i20", [0, 4096, 4096, 0, 1001, 0, 0], 20, 0.02),
              ("n1500_900_c700_s3001_i100", [1, 1500, 900, 700, 3001, 0, 0], 100, 0.2)]
EXTRA_WSEEDS = (7, 2024)
RAD, PCT, MS = 15, 2, 7


def make(spec):
    kind, n0, n1, nc, seed, cw, ch = spec
    canvas = (cw, ch) if cw else None
    if kind == 0:
        return synth.make_pair(n0, seed, canvas=canvas)
    return synth.make_pair_unbalanced(n0, n1, nc, seed, canvas=canvas)


def score_matrix(pair, iters):
    """The reference's score matrix (the input of log_optimal_transport) of one pair, at the default weights."""
    model = G.ref_model(synth.make_state_dict(WSEED), {"sinkhorn_iterations": iters})
    return G.run_reference(model, pair, RAD, PCT, MS, capture=True)["scores"].astype(np.float64)


def alphas_of(scores):
    """-2, p10 / p50 / p90 of the row maxima, and one alpha above the largest score: float32 values, with their tags."""
    rmax = scores.max(1)
    return [("m2", np.float32(-2.0)),
            ("p10", np.float32(np.percentile(rmax, 10))),
            ("p50", np.float32(np.percentile(rmax, 50))),
            ("p90", np.float32(np.percentile(rmax, 90))),
            ("top", np.float32(np.ceil(scores.max()) + 10.0))]


def e2e(name, spec, iters, thr, wseed, alpha, expect_none=False):
    t0 = time.time()
    pair = make(spec)
    model = G.ref_model(synth.make_state_dict(wseed, bin_score=float(alpha)), {"sinkhorn_iterations": iters, "match_threshold": thr})
    r = G.run_reference(model, pair, RAD, PCT, MS)
    frac = float((r["matches0"] >= 0).mean())
    arrs = {"out/" + k: v for k, v in r.items()}
    arrs.update(pair=np.asarray(spec, dtype=np.int64), meta=np.asarray([RAD, PCT, MS, iters], dtype=np.int64),
                match_threshold=np.float64(thr), bin_score=np.float32(alpha), weight_seed=np.int64(wseed), matched_frac=np.float64(frac))
    G.save(name, **arrs)
    print(f"  alpha {float(alpha):9.4f}  matched {frac:6.1%} of {len(r['matches0'])} kept rows  ({time.time() - t0:.1f} s)", flush=True)
    if expect_none:
        assert frac == 0.0, (name, frac)
    else:
        assert frac > 0.0, (name, frac)
    return frac


def main():
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
    alphas = {}
    for tag, spec, iters, thr in BIN_PAIRS:
        sc = score_matrix(make(spec), iters)
        alphas[tag] = alphas_of(sc)
        rm = sc.max(1)
        print(f"{tag}: {sc.shape[0]} x {sc.shape[1]} scores, row max {rm.min():.2f} .. {rm.max():.2f} (median {np.median(rm):.2f})", flush=True)
    if only in (None, "bin"):
        for tag, spec, iters, thr in BIN_PAIRS:
            for atag, a in alphas[tag]:
                e2e(f"bine2e_{tag}_a{atag}", spec, iters, thr, WSEED, a, expect_none=atag == "top")
    if only in (None, "seed"):
        for ws in EXTRA_WSEEDS:
            for tag, spec, iters, thr in SEED_PAIRS:
                e2e(f"seede2e_{tag}_w{ws}", spec, iters, thr, ws, np.float32(1.0))
    if only in (None, "loss"):
        w = dict(GT.WEIGHTS)
        for tag, spec, iters, ltag in (("n256_s1002_i100", BIN_PAIRS[0][1], 100, "n256_s1002_i100"),
                                       ("n1024sparse_s2001_i20", BIN_PAIRS[3][1], 20, "n1024sparse_s2001_i20")):
            for atag, a in alphas[tag]:
                if atag not in ("p50", "p90"):
                    continue
                model = G.ref_model(synth.make_state_dict(WSEED, bin_score=float(a)), {**w, "sinkhorn_iterations": iters})
                ex = dict(pair=np.asarray(spec, dtype=np.int64), bin_score=np.float32(a), weight_seed=np.int64(WSEED))
                print(f"binloss_{ltag}_a{atag}: alpha {float(a):.4f}", flush=True)
                GT.one(f"binloss_{ltag}_a{atag}", model, [make(spec)], RAD, PCT, MS, iters, extra=ex)
        a = dict(alphas["n256_s1002_i100"])["p50"]
        ex = dict(pair=np.asarray(BIN_PAIRS[0][1], dtype=np.int64), bin_score=np.float32(a), weight_seed=np.int64(WSEED))
        GG.one("binstep_n256_s1002_i100_ap50", synth.make_state_dict(WSEED, bin_score=float(a)), {**w}, [make(BIN_PAIRS[0][1])], RAD, PCT, MS,
               extra=ex)


if __name__ == "__main__":
    torch.set_grad_enabled(False)
    main()
