"""Geometric verification without a ground truth: the RANSAC homography over a set of correspondences and its inlier mask.

The reference's drivers end in ``H, mask = cv2.findHomography(points0, points1, cv2.RANSAC | cv2.USAC_DEFAULT)`` and report the count of the
mask as ``correct_matches`` (eval_homography.py:191, eval_matches.py:71,164, tools/parameter_search.py:161).  Here that step is ONE batched
call into the kernel library (``gims_verify_pairs``, csrc/verify.hip): best 4-point hypothesis, then a guarded local optimisation
(least-squares refits on normalised inliers, accepted only while the inlier count does not fall).  The estimator is this library's own and
fully specified in include/gims_hip.h; parity with OpenCV's USAC is not claimed (its sampler cannot be reproduced from outside), so inlier
counts compare among runs of this library, not with the reference's.

``find_homography`` has the shape of the OpenCV call; ``verify_pairs`` is the batched, asynchronous form that takes what ``match_pairs``,
``forward``, ``sweep`` records and ``nn_match_pairs`` return."""
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
                 h_refs: Optional[Sequence[np.ndarray]] = None) -> dict:
    """datas: the dicts ``match_pairs`` / ``forward`` mutated (kept keypoints; image shapes are read only with ``h_refs``); outs: the
    per-pair results (``matches0`` [1, n0] int64; a result that carries its own ``keypoints0`` / ``keypoints1``, like a sweep record's
    ``result``, is read from there).  ``h_refs``: optional 3x3 homographies mapping image 0 to image 1 for the ``err_corner`` column.

    Returns device tensors: ``records`` [P, 8] float32 (RECORD_FIELDS in the first columns; ``n_inliers`` is the reference's
    ``correct_matches``), ``homographies`` [P, 3, 3] float32, ``inlier`` (list of per-pair uint8 [n0] masks, 0 on unmatched keypoints).
    ``lo_iters=0`` is the estimator of ``evalh.evaluate_pairs``.  One batched call, asynchronous on the current stream."""
    P = len(outs)
    if P == 0 or len(datas) != P or (h_refs is not None and len(h_refs) != P):
        raise ValueError("verify_pairs: datas, outs (and h_refs) must be non-empty lists of one length")
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
                  record=records[p], homography=homs[p])
        if h_refs is not None:
            it["height"], it["width"] = _image_size(d)
            it["h_ref"] = h_refs[p]
        items.append(it)
        inl.append(m)
    keep = hip.verify_pairs(items, thresh, iters, lo_iters, seed)
    return dict(records=records, homographies=homs.view(P, 3, 3), inlier=inl, _keep=(keep, items))


def find_homography(points0, points1, thresh: float = 3.0, iters: int = 3000, lo_iters: int = 8, seed: int = 0):
    """``cv2.findHomography(points0, points1, cv2.RANSAC, thresh, maxIters=iters)`` in shape: ``points0`` / ``points1`` are [K, 2] (or
    [K, 1, 2]) tensors or arrays of corresponding points, row i with row i.  Returns ``(H [3, 3] float32, mask [K, 1] uint8)`` as device
    tensors, or ``(None, None)`` when there is no model (fewer than four points, or no sample with a model), like OpenCV.

    This call SYNCHRONISES with the device (it reads whether a model was found); the batched ``verify_pairs`` does not."""
    dev = points0.device if isinstance(points0, torch.Tensor) and points0.is_cuda else torch.device("cuda", torch.cuda.current_device())
    p0 = torch.as_tensor(points0).to(device=dev, dtype=torch.float32).reshape(-1, 2).contiguous()
    p1 = torch.as_tensor(points1).to(device=dev, dtype=torch.float32).reshape(-1, 2).contiguous()
    if p0.shape != p1.shape:
        raise ValueError(f"find_homography: {tuple(p0.shape)} and {tuple(p1.shape)} points do not correspond row by row")
    k = int(p0.shape[0])
    if k < 4:
        return None, None
    record = torch.zeros(8, dtype=torch.float32, device=dev)
    hom = torch.zeros(9, dtype=torch.float32, device=dev)
    mask = torch.empty(k, dtype=torch.uint8, device=dev)
    work = hip.verify_pairs([dict(kpts0=p0, kpts1=p1, matches0=None, inlier=mask, record=record, homography=hom)], thresh, iters, lo_iters, seed)
    ok = bool(record[RECORD_FIELDS.index("ok")].item())              # the host read: the stream has passed the call, `work` may go
    del work
    return (hom.view(3, 3), mask.view(k, 1)) if ok else (None, None)
