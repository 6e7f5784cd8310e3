"""Guided matching: refill a verified pair's matches under its model, on the device (kernels: gims_amd/csrc/nn.hip,
GIMS_AUX_GUIDED_MATCH).

``verify_pairs`` fits H, F or E to a pair and uses the model only to drop rows of ``matches0``.  The keypoints the matcher left unmatched
are never looked at again, although the model now says where each one's partner must lie: a band of a few pixels instead of the whole
second image.  ``guided_match_pairs`` runs the descriptor match of ``nn_match_pairs`` again between the two keypoint sets, counting only
partners that agree with the pair's model -- both keypoints within ``thresh`` pixels of the other's epipolar line, or of the other's image
under H and its inverse --, and adds what it finds to the matches that are kept.  The gate removes the twin that spoils a ratio test and the
match that contradicts the model.  The specification is this library's own (include/gims_hip.h has it in full; tests/guided_ref.py is its
NumPy restatement).  The model is not refitted: run ``verify_pairs`` on the result for that."""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from . import hip
from .baselines import _point_major
from .verify import RECORD_FIELDS, _is_camera_pair

KEEP = ("inliers", "all", "none")
_MODELS = ("homography", "fundamental", "pose")


def _pose_fundamental(E: torch.Tensor, cams, dev) -> torch.Tensor:
    """F = K1^-T E K0^-1 on the device in float64, rounded to float32 [9]: the inverses of the (host) intrinsics ride up in a table."""
    k0, k1 = (np.asarray(k.cpu() if isinstance(k, torch.Tensor) else k, dtype=np.float64).reshape(3, 3) for k in cams)
    both = hip.upload(np.stack([np.linalg.inv(k1).T, np.linalg.inv(k0)]).view(np.int64), dev).view(torch.float64)      # the bits, as they are
    return (both[0] @ E.reshape(3, 3).double() @ both[1]).float().reshape(9).contiguous()


def _checked(n_pairs, outs, verified, model, intrinsics, keep):
    """Everything that is refused before the device is touched -> (model names per pair, camera pairs per pair)."""
    if keep not in KEEP:
        raise ValueError(f"guided_match: keep must be one of {KEEP}, got {keep!r}")
    if n_pairs == 0 or (outs is not None and len(outs) != n_pairs):
        raise ValueError(f"guided_match: datas ({n_pairs}) and outs ({'none' if outs is None else len(outs)}) must be non-empty lists of one length")
    if len(verified["models"]) != n_pairs or len(verified["records"]) != n_pairs or len(verified["inlier"]) != n_pairs:
        raise ValueError(f"guided_match: verified holds {len(verified['models'])} models, {len(verified['records'])} records and "
                         f"{len(verified['inlier'])} inlier masks for {n_pairs} pairs: lists of unequal length")
    models = list(model) if isinstance(model, (list, tuple)) else [model] * n_pairs
    if len(models) != n_pairs or any(m not in _MODELS for m in models):
        raise ValueError(f"guided_match: model must be one of {_MODELS} or a list of one per pair, got {model!r}")
    cams = [None] * n_pairs
    if "pose" in models:
        if intrinsics is None:
            raise ValueError("guided_match: model='pose' needs intrinsics=(K0, K1)")
        cams = list(intrinsics) if len(intrinsics) == n_pairs and not _is_camera_pair(intrinsics) else [intrinsics] * n_pairs
        if len(cams) != n_pairs or any(m == "pose" and (c is None or not _is_camera_pair(c)) for m, c in zip(models, cams)):
            raise ValueError("guided_match: intrinsics must be one (K0, K1) pair of 3x3 matrices or a list of one per pair")
    return models, cams


def _run(sets, outs, verified, models, cams, thresh, ratio, max_distance, mutual, keep, exhaustive) -> List[dict]:
    """sets: (a [n0, d], b [n1, d], kpts0 [n0, 2], kpts1 [n1, 2]) per pair, device tensors."""
    dev = sets[0][0].device
    P = len(sets)
    s0, s1 = sum(s[0].shape[0] for s in sets), sum(s[1].shape[0] for s in sets)
    pools = {name: torch.empty(s0, dtype=dt, device=dev) for name, dt in hip.GUIDED_OUTPUTS}
    info = torch.empty((P, 8), dtype=torch.int32, device=dev)
    m1 = torch.empty(s1, dtype=torch.int64, device=dev) if mutual else None
    c1 = torch.empty(s1, dtype=torch.int32, device=dev) if mutual else None
    ok_col = RECORD_FIELDS.index("ok")
    items, results, o0, o1 = [], [], 0, 0
    for p, (a, b, k0, k1) in enumerate(sets):
        n0, n1 = a.shape[0], b.shape[0]
        fitted = verified["models"][p].reshape(9).float().contiguous()
        if models[p] == "pose":
            fitted = _pose_fundamental(fitted, cams[p], dev)
        it = dict(a=a, b=b, kpts0=k0, kpts1=k1, model=fitted, kind="homography" if models[p] == "homography" else "fundamental",
                  ok=verified["records"][p, ok_col:ok_col + 1], mutual=mutual, thresh=thresh, threshold=ratio, max_distance=max_distance,
                  info=info[p], **{k: v[o0:o0 + n0] for k, v in pools.items()})
        if keep != "none" and outs is not None:
            it["prior"] = outs[p]["matches0"].reshape(-1).contiguous()
            if "matching_scores0" in outs[p]:
                it["prior_scores"] = outs[p]["matching_scores0"].reshape(-1).float().contiguous()
            if keep == "inliers":
                it["prior_mask"] = verified["inlier"][p].reshape(-1).contiguous()
        res = dict(matches0=it["matches0"][None], matching_scores0=it["scores0"][None], added0=it["added0"][None], nn0=it["nn1"][None],
                   nn0_second=it["nn2"][None], dist0=it["d1"][None], dist0_second=it["d2"][None], ratios0=it["ratio"][None],
                   n_admissible0=it["n_admissible"][None], info=info[p], model=fitted)
        if mutual:
            it.update(matches1=m1[o1:o1 + n1], cnn1=c1[o1:o1 + n1])
            res.update(matches1=it["matches1"][None], nn1=it["cnn1"][None])
        items.append(it)
        results.append(res)
        o0, o1 = o0 + n0, o1 + n1
    keepalive = hip.guided_match(items, hip.NN_EXHAUSTIVE if exhaustive else 0)
    results[0]["_keep"] = (keepalive, items)          # inputs and workspace stay alive as long as the results do
    return results


def guided_match_pairs(datas: Sequence[dict], outs: Optional[Sequence[dict]], verified: dict, *, model="fundamental", intrinsics=None,
                       thresh: float = 3.0, ratio: float = 0.8, max_distance: Optional[float] = None, mutual: bool = True, keep: str = "inliers",
                       exhaustive: bool = False) -> List[dict]:
    """Batched, asynchronous.  ``datas``: the dicts of ``nn_match_pairs`` / ``verify_pairs`` (``descriptors0`` / ``descriptors1`` of shape
    (1, D, N), ``keypoints0`` / ``keypoints1`` of shape (1, N, 2)); ``outs``: the matcher's per-pair results (``matches0`` [1, n0] int64 and,
    if present, ``matching_scores0``), or None for no prior; ``verified``: the dict ``verify_pairs`` returned for them -- its ``models``, the
    ``ok`` column of its ``records`` and its ``inlier`` masks are read where they lie on the device.

    ``keep``: ``'inliers'`` keeps the matches ``verify_pairs`` accepted (the prior masked by ``verified['inlier']``), ``'all'`` every match
    of ``outs``, ``'none'`` starts from nothing.  A kept match is FIXED: its row does not search and its column is taken.  Every other row
    searches the columns that are ADMISSIBLE under the model within ``thresh`` pixels and matches its nearest one iff the ratio to the
    second nearest admissible one is below ``ratio``, the distance is at most ``max_distance`` (None: no limit) and, with ``mutual``, the
    column's nearest admissible row is this one.  A pair without a model (``ok`` = 0, or a non-finite entry) keeps its fixed rows only.

    ``model``: ``'homography'``, ``'fundamental'`` or ``'pose'`` -- what ``verify_pairs`` was called with --, or a list of one per pair.
    ``'pose'`` needs the same ``intrinsics``; F = K1^-T E K0^-1 is formed on the device in float64 and rounded to float32.

    One dict per pair comes back, all device tensors, accepted unchanged by ``build_tracks``, ``verify_pairs`` and
    ``evalh.evaluate_pairs``: ``matches0`` [1, n0] int64, ``matching_scores0`` [1, n0] (a fixed row keeps its score, or 1; an added one has
    1 - ratio), ``added0`` [1, n0] uint8 (1 on rows this call matched), ``matches1`` [1, n1] (with ``mutual``), ``nn0`` / ``nn0_second`` /
    ``dist0`` / ``dist0_second`` / ``ratios0`` (the two nearest admissible columns), ``n_admissible0`` [1, n0] int32, ``info`` int32 [8]
    (hip.GUIDED_INFO) and ``model`` float32 [9], the matrix the gate used.  ``exhaustive=True`` sends every row through the exhaustive
    float64 path (same results, bit for bit).  ValueError before the device is touched: lists of unequal length, an unknown ``keep`` or
    model, ``'pose'`` without intrinsics, descriptor and keypoint counts that differ.  No host synchronisation."""
    models, cams = _checked(len(datas), outs, verified, model, intrinsics, keep)
    for p, d in enumerate(datas):
        for side in "01":
            nd, nk = int(d["descriptors" + side].shape[-1]), int(d["keypoints" + side].shape[-2])
            if nd != nk:
                raise ValueError(f"guided_match_pairs: pair {p}: {nd} descriptors and {nk} keypoints in image {side}: the counts differ")
    first = datas[0]["descriptors0"]
    dev = first.device if isinstance(first, torch.Tensor) and first.is_cuda else torch.device("cuda", torch.cuda.current_device())
    kp = lambda t: torch.as_tensor(t).to(device=dev, dtype=torch.float32).reshape(-1, 2).contiguous()      # noqa: E731
    sets = [(_point_major(d["descriptors0"], dev), _point_major(d["descriptors1"], dev), kp(d["keypoints0"]), kp(d["keypoints1"])) for d in datas]
    return _run(sets, outs, verified, models, cams, thresh, ratio, max_distance, mutual, keep, exhaustive)


def guided_match_features(feats, pairs, outs: Optional[Sequence[dict]], verified: dict, *, model="fundamental", intrinsics=None,
                          thresh: float = 3.0, ratio: float = 0.8, max_distance: Optional[float] = None, mutual: bool = True,
                          keep: str = "inliers", exhaustive: bool = False) -> List[dict]:
    """``guided_match_pairs`` over an image set: ``feats`` are ``ImageFeatures`` (``descriptors`` [n, D] point-major, ``keypoints`` [n, 2]),
    ``pairs`` the index pairs given to ``match_features``, ``outs`` its results (or None) and ``verified`` what ``verify_pairs`` returned for
    them.  Nothing is copied: the rows of the features are read where they lie."""
    pairs = [(int(a), int(b)) for a, b in pairs]
    models, cams = _checked(len(pairs), outs, verified, model, intrinsics, keep)
    for k, f in enumerate(feats):
        if int(f.descriptors.shape[0]) != int(f.keypoints.shape[0]):
            raise ValueError(f"guided_match_features: image {k}: {int(f.descriptors.shape[0])} descriptors and {int(f.keypoints.shape[0])} keypoints: "
                             "the counts differ")
    for p, (a, b) in enumerate(pairs):
        if not (0 <= a < len(feats) and 0 <= b < len(feats)):
            raise ValueError(f"guided_match_features: pair {p}: the image index of ({a}, {b}) is out of range (0 .. {len(feats) - 1})")
    rows = lambda f: (f.descriptors if f.descriptors.stride(-1) == 1 else f.descriptors.contiguous()).float()      # noqa: E731
    sets = [(rows(feats[a]), rows(feats[b]), feats[a].keypoints.float().contiguous(), feats[b].keypoints.float().contiguous()) for a, b in pairs]
    return _run(sets, outs, verified, models, cams, thresh, ratio, max_distance, mutual, keep, exhaustive)
