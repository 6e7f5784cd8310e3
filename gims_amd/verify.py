"""Geometric verification without a ground truth: the RANSAC homography over a set of correspondences and its inlier mask.

The reference's drivers end in ``H, mask = cv2.findHomography(points0, points1, cv2.RANSAC | cv2.USAC_DEFAULT)`` and report the count of the
mask as ``correct_matches`` (eval_homography.py:191, eval_matches.py:71,164, tools/parameter_search.py:161).  Here that step is ONE batched
call into the kernel library (``gims_verify_pairs``, csrc/verify.hip): best 4-point hypothesis, then a guarded local optimisation
(least-squares refits on normalised inliers, accepted only while the inlier count does not fall).  The estimator is this library's own and
fully specified in include/gims_hip.h; parity with OpenCV's USAC is not claimed (its sampler cannot be reproduced from outside), so inlier
counts compare among runs of this library, not with the reference's.

``find_homography`` has the shape of the OpenCV call; ``verify_pairs`` is the batched, asynchronous form that takes what ``match_pairs``,
``forward``, ``sweep`` records and ``nn_match_pairs`` return.

A homography counts the right matches only on planar scenes and pure rotations.  For a camera that moved through a 3-D scene the same
call fits a FUNDAMENTAL matrix instead (``model='fundamental'``, ``find_fundamental``): 8-point hypotheses scored by Sampson distance,
then the same guarded local optimisation with a rank-2 model.  That estimator, too, is this library's own (include/gims_hip.h); it is not
OpenCV's ``findFundamentalMat``, and no essential matrix or pose is derived from it."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import hip

RECORD_FIELDS = hip.VERIFY_FIELDS        # columns of the per-set record (float32): see include/gims_hip.h GIMS_VERIFY_*


def _image_size(d: dict):
    """(height, width) of image 0 as evalh.evaluate_pairs reads them (a 1xHxWx3 tensor or the HxWx3 array the reference loads)."""
    shape0 = d["image0"].shape
    return (int(shape0[1]), int(shape0[2])) if len(shape0) == 4 else (int(shape0[0]), int(shape0[1]))


def _points(d: dict, o: dict, side: str) -> torch.Tensor:
    k = o["keypoints" + side] if "keypoints" + side in o else d["keypoints" + side]
    return k[0].contiguous().float()


def verify_pairs(datas: Sequence[dict], outs: Sequence[dict], thresh: float = 3.0, iters: int = 3000, lo_iters: int = 8, seed: int = 0,
                 h_refs: Optional[Sequence[np.ndarray]] = None, model="homography") -> dict:
    """datas: the dicts ``match_pairs`` / ``forward`` mutated (kept keypoints; image shapes are read only with ``h_refs``); outs: the
    per-pair results (``matches0`` [1, n0] int64; a result that carries its own ``keypoints0`` / ``keypoints1``, like a sweep record's
    ``result``, is read from there).  ``h_refs``: optional 3x3 homographies mapping image 0 to image 1 for the ``err_corner`` column.

    Returns device tensors: ``records`` [P, 8] float32 (RECORD_FIELDS in the first columns; ``n_inliers`` is the reference's
    ``correct_matches``), ``homographies`` [P, 3, 3] float32, ``inlier`` (list of per-pair uint8 [n0] masks, 0 on unmatched keypoints).
    ``lo_iters=0`` is the estimator of ``evalh.evaluate_pairs``.  One batched call, asynchronous on the current stream.

    ``model``: ``'homography'`` (the default) or ``'fundamental'``, or a list of one per pair.  ``models`` [P, 3, 3] is the fitted model of
    every pair -- H, or F with ``x1^T F x0 = 0``, unit Frobenius norm, rank 2 -- and ``homographies`` is the same tensor under its old name.
    ``'fundamental'`` needs eight correspondences, has no ``err_corner`` (-1) and cannot be combined with ``h_refs``."""
    P = len(outs)
    if P == 0 or len(datas) != P or (h_refs is not None and len(h_refs) != P):
        raise ValueError("verify_pairs: datas, outs (and h_refs) must be non-empty lists of one length")
    models = list(model) if isinstance(model, (list, tuple)) else [model] * P
    if len(models) != P:
        raise ValueError("verify_pairs: model must be 'homography', 'fundamental' or a list of one per pair")
    models = [hip.verify_model(m) for m in models]
    if h_refs is not None and any(m == hip.VERIFY_MODELS["fundamental"] for m in models):
        raise ValueError("verify_pairs: h_refs cannot be combined with model='fundamental' (there is no error column for F)")
    dev = outs[0]["matches0"].device
    records = torch.zeros((P, 8), dtype=torch.float32, device=dev)
    homs = torch.zeros((P, 9), dtype=torch.float32, device=dev)
    n0s = [int(o["matches0"].shape[-1]) for o in outs]
    in_all = torch.empty(sum(n0s), dtype=torch.uint8, device=dev)
    items, inl, c = [], [], 0
    for p, (d, o) in enumerate(zip(datas, outs)):
        m = in_all[c:c + n0s[p]]
        c += n0s[p]
        it = dict(kpts0=_points(d, o, "0"), kpts1=_points(d, o, "1"), matches0=o["matches0"].reshape(-1).contiguous(), inlier=m,
                  record=records[p], homography=homs[p], model=models[p])
        if h_refs is not None:
            it["height"], it["width"] = _image_size(d)
            it["h_ref"] = h_refs[p]
        items.append(it)
        inl.append(m)
    keep = hip.verify_pairs(items, thresh, iters, lo_iters, seed)
    fitted = homs.view(P, 3, 3)
    return dict(records=records, homographies=fitted, models=fitted, inlier=inl, _keep=(keep, items))


def _find(name, model, least, points0, points1, thresh, iters, lo_iters, seed):
    dev = points0.device if isinstance(points0, torch.Tensor) and points0.is_cuda else torch.device("cuda", torch.cuda.current_device())
    p0 = torch.as_tensor(points0).to(device=dev, dtype=torch.float32).reshape(-1, 2).contiguous()
    p1 = torch.as_tensor(points1).to(device=dev, dtype=torch.float32).reshape(-1, 2).contiguous()
    if p0.shape != p1.shape:
        raise ValueError(f"{name}: {tuple(p0.shape)} and {tuple(p1.shape)} points do not correspond row by row")
    k = int(p0.shape[0])
    if k < least:
        return None, None
    record = torch.zeros(8, dtype=torch.float32, device=dev)
    hom = torch.zeros(9, dtype=torch.float32, device=dev)
    mask = torch.empty(k, dtype=torch.uint8, device=dev)
    work = hip.verify_pairs([dict(kpts0=p0, kpts1=p1, matches0=None, inlier=mask, record=record, homography=hom, model=model)], thresh, iters,
                            lo_iters, seed)
    ok = bool(record[RECORD_FIELDS.index("ok")].item())              # the host read: the stream has passed the call, `work` may go
    del work
    return (hom.view(3, 3), mask.view(k, 1)) if ok else (None, None)


def find_homography(points0, points1, thresh: float = 3.0, iters: int = 3000, lo_iters: int = 8, seed: int = 0):
    """``cv2.findHomography(points0, points1, cv2.RANSAC, thresh, maxIters=iters)`` in shape: ``points0`` / ``points1`` are [K, 2] (or
    [K, 1, 2]) tensors or arrays of corresponding points, row i with row i.  Returns ``(H [3, 3] float32, mask [K, 1] uint8)`` as device
    tensors, or ``(None, None)`` when there is no model (fewer than four points, or no sample with a model), like OpenCV.

    This call SYNCHRONISES with the device (it reads whether a model was found); the batched ``verify_pairs`` does not."""
    return _find("find_homography", "homography", 4, points0, points1, thresh, iters, lo_iters, seed)


def find_fundamental(points0, points1, thresh: float = 3.0, iters: int = 3000, lo_iters: int = 8, seed: int = 0):
    """``cv2.findFundamentalMat(points0, points1, cv2.FM_RANSAC, thresh, maxIters=iters)`` in shape: ``points0`` / ``points1`` are [K, 2]
    (or [K, 1, 2]) tensors or arrays of corresponding points, row i with row i.  Returns ``(F [3, 3] float32, mask [K, 1] uint8)`` as device
    tensors -- ``x1^T F x0 = 0`` for ``x0 = (x, y, 1)`` of ``points0``, F of rank 2 with unit Frobenius norm, ``thresh`` a Sampson distance
    in pixels -- or ``(None, None)`` when there is no model (fewer than eight points, or no sample with a model).  The estimator is this
    library's own (include/gims_hip.h), not OpenCV's.

    This call SYNCHRONISES with the device (it reads whether a model was found); the batched ``verify_pairs(model='fundamental')`` does not."""
    return _find("find_fundamental", "fundamental", 8, points0, points1, thresh, iters, lo_iters, seed)
