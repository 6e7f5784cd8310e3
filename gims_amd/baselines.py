"""Classical descriptor baselines on the device: the nearest-neighbour distance ratio test (NNDR) and its mutual-nearest variant (MNN).

The reference compares its learned matcher against ``calculate_nndr`` / ``calculate_mnn`` (eval_matches.py:13-67): ``torch.cdist`` of the two
descriptor sets, a full ``torch.sort`` of every row, the ratio of the two smallest distances against a threshold and, for MNN, the mutual
nearest test.  Here both are ONE batched call into the kernel library (``gims_nn_match``, csrc/nn.hip; semantics in include/gims_hip.h):
nothing of size n0 x n1 is stored, every decision is taken on exact float64 distances, exact ties go to the lowest index.

``nndr`` / ``mnn`` keep the reference's signature and return shapes; ``nn_match_pairs`` is the batched, asynchronous form whose results go
straight into ``gims_amd.evalh.evaluate_pairs`` next to the learned matcher's."""
from __future__ import annotations

from typing import List, Sequence

import numpy as np
import torch

from . import hip

METHODS = ("nndr", "mnn")


def _check_counts(n0: int, n1: int, method: str):
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")
    if n0 < 1 or n1 < 2:
        raise ValueError(f"{method}: the ratio test needs a second-nearest neighbour, i.e. at least 2 descriptors in the second set (got {n0} and {n1})")
    if method == "mnn" and n0 < 2:
        raise ValueError(f"mnn: the mutual test sorts the first set for every descriptor of the second and reads its second neighbour, "
                         f"so the first set needs at least 2 descriptors (got {n0})")


def _point_major(desc, device) -> torch.Tensor:
    """(D, N) or (1, D, N), tensor or array -> float32 [N, D] on the device (the kernels are point-major)."""
    t = torch.as_tensor(desc) if isinstance(desc, np.ndarray) else desc
    if t.dim() == 3:
        t = t[0]
    if t.dim() != 2:
        raise ValueError(f"descriptors must have shape (D, N) or (1, D, N), got {tuple(t.shape)}")
    return t.to(device=device, dtype=torch.float32).t().contiguous()


def nn_match_pairs(datas: Sequence[dict], method: str = "nndr", threshold: float = 0.8, *, exhaustive: bool = False, debug: bool = False) -> List[dict]:
    """Batched, asynchronous.  datas: dicts with ``descriptors0`` / ``descriptors1`` of shape (1, D, N) (what ``Matching`` and the front
    end produce; ``keypoints*`` / ``image*`` may be present and are not read).  One dict per pair comes back, all device tensors:

    ``matches0`` [1, n0] int64 (-1: no match), ``matching_scores0`` [1, n0] float32 (1 - ratio on matches, 0 elsewhere: a confidence
    order for the evaluation's four-point homography), ``ratios0`` [1, n0] float32, ``nn0`` / ``nn0_second`` [1, n0] int32 (the two exact
    nearest rows of the second set), ``dist0`` / ``dist0_second`` [1, n0] float32, ``match0`` [1, n0] uint8, ``fallback_rows`` int32 [2]
    (rows re-solved exhaustively: first against second set, second against first); for ``mnn`` also ``matches1`` [1, n1] int64 and
    ``nn1`` [1, n1] int32.  ``exhaustive=True`` sends every row through the exhaustive float64 path (same results, bit for bit);
    ``debug=True`` adds ``debug`` [n0, 4] (include/gims_hip.h).  No host synchronisation."""
    if len(datas) == 0:
        return []
    for d in datas:
        _check_counts(int(d["descriptors0"].shape[-1]), int(d["descriptors1"].shape[-1]), method)
    first = datas[0]["descriptors0"]
    dev = first.device if isinstance(first, torch.Tensor) and first.is_cuda else torch.device("cuda", torch.cuda.current_device())
    mutual = method == "mnn"
    ab = [(_point_major(d["descriptors0"], dev), _point_major(d["descriptors1"], dev)) for d in datas]
    s0, s1 = sum(a.shape[0] for a, _ in ab), sum(b.shape[0] for _, b in ab)
    pools = {name: torch.empty(s0, dtype=dt, device=dev) for name, dt in hip.NN_OUTPUTS}
    info = torch.empty((len(ab), 4), dtype=torch.int32, device=dev)
    m1 = torch.empty(s1, dtype=torch.int64, device=dev) if mutual else None
    c1 = torch.empty(s1, dtype=torch.int32, device=dev) if mutual else None
    dbg = torch.empty((s0, 4), dtype=torch.float32, device=dev) if debug else None
    items, outs, o0, o1 = [], [], 0, 0
    for p, (a, b) in enumerate(ab):
        n0, n1 = a.shape[0], b.shape[0]
        it = dict(a=a, b=b, mutual=mutual, threshold=threshold, info=info[p], **{k: v[o0:o0 + n0] for k, v in pools.items()})
        out = dict(matches0=it["matches0"][None], matching_scores0=it["scores0"][None], ratios0=it["ratio"][None], nn0=it["nn1"][None],
                   nn0_second=it["nn2"][None], dist0=it["d1"][None], dist0_second=it["d2"][None], match0=it["match"][None],
                   fallback_rows=info[p, :2])
        if mutual:
            it.update(matches1=m1[o1:o1 + n1], cnn1=c1[o1:o1 + n1])
            out.update(matches1=it["matches1"][None], nn1=it["cnn1"][None])
        if debug:
            it["debug"] = dbg[o0:o0 + n0]
            out["debug"] = it["debug"]
        items.append(it)
        outs.append(out)
        o0, o1 = o0 + n0, o1 + n1
    work = hip.nn_match(items, hip.NN_EXHAUSTIVE if exhaustive else 0)
    outs[0]["_keep"] = (work, items)          # inputs and workspace stay alive as long as the results do
    return outs


def _reference_shaped(desc_a, desc_b, threshold, method):
    da = torch.as_tensor(desc_a) if isinstance(desc_a, np.ndarray) else desc_a
    db = torch.as_tensor(desc_b) if isinstance(desc_b, np.ndarray) else desc_b
    if da.dim() != 2 or db.dim() != 2:
        raise ValueError(f"descriptors must have shape (D, N), got {tuple(da.shape)} and {tuple(db.shape)}")
    _check_counts(int(da.shape[1]), int(db.shape[1]), method)
    out = nn_match_pairs([dict(descriptors0=da[None], descriptors1=db[None])], method, threshold)[0]
    matches = out["match0"][0].bool()
    match_indices = matches.nonzero().squeeze()            # the one host read (the count), as in the reference
    good_matches = out["nn0"][0].long()[match_indices]
    return match_indices, good_matches, out["ratios0"][0][matches]


def nndr(desc_a, desc_b, threshold: float = 0.8):
    """``calculate_nndr(descriptor_a, descriptor_b, threshold)`` (eval_matches.py:13-35): (D, N) descriptors (device tensors, or NumPy
    arrays that are moved to the current device) -> (match_indices int64, good_matches int64, ratios float32) on the device, with the
    reference's ``.squeeze()`` shapes: no match -> index tensors of shape (0,); exactly one -> 0-dim indices and ratios of shape (1,)."""
    return _reference_shaped(desc_a, desc_b, threshold, "nndr")


def mnn(desc_a, desc_b, threshold: float = 0.8):
    """``calculate_mnn`` (eval_matches.py:37-67): ``nndr`` plus the mutual-nearest test.  Raises ValueError when the first set has fewer than
    2 descriptors (the reference indexes a second neighbour there and raises an IndexError)."""
    return _reference_shaped(desc_a, desc_b, threshold, "mnn")
