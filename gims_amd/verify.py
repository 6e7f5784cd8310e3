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
OpenCV's ``findFundamentalMat``.

With calibrated cameras the step after that is the relative POSE (``model='pose'`` with ``intrinsics``, ``estimate_pose``): five-point
hypotheses on camera coordinates -- which, unlike the 8-point system, stay determined on a planar or plane-dominated scene --, the same
guarded local optimisation followed by a projection onto the essential manifold, then the one of the four decompositions (R, t) of E
that puts the most inliers in front of both cameras.  It stands where the reference has ``estimate_pose`` (utils/common.py:392-416,
``cv2.findEssentialMat`` + ``cv2.recoverPose``); ``pose_error``, ``epipolar_error`` and ``pose_summary`` are its ``compute_pose_error``,
``compute_epipolar_error`` and the AUC it reports them with.  The estimator is this library's own (include/gims_hip.h)."""
from __future__ import annotations

import math
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
                 h_refs: Optional[Sequence[np.ndarray]] = None, model="homography", intrinsics=None) -> dict:
    """datas: the dicts ``match_pairs`` / ``forward`` mutated (kept keypoints; image shapes are read only with ``h_refs``); outs: the
    per-pair results (``matches0`` [1, n0] int64; a result that carries its own ``keypoints0`` / ``keypoints1``, like a sweep record's
    ``result``, is read from there).  ``h_refs``: optional 3x3 homographies mapping image 0 to image 1 for the ``err_corner`` column.

    Returns device tensors: ``records`` [P, 8] float32 (RECORD_FIELDS in the first columns; ``n_inliers`` is the reference's
    ``correct_matches``), ``homographies`` [P, 3, 3] float32, ``inlier`` (list of per-pair uint8 [n0] masks, 0 on unmatched keypoints).
    ``lo_iters=0`` is the estimator of ``evalh.evaluate_pairs``.  One batched call, asynchronous on the current stream.

    ``model``: ``'homography'`` (the default) or ``'fundamental'``, or a list of one per pair.  ``models`` [P, 3, 3] is the fitted model of
    every pair -- H, or F with ``x1^T F x0 = 0``, unit Frobenius norm, rank 2 -- and ``homographies`` is the same tensor under its old name.
    ``'fundamental'`` needs eight correspondences, has no ``err_corner`` (-1) and cannot be combined with ``h_refs``.

    ``'pose'`` needs ``intrinsics``: one ``(K0, K1)`` pair of 3x3 array-likes for all pairs, or a list of one per pair (None where the
    pair has another model); ``thresh`` stays in pixels.  ``models`` then holds E (``x1^T E x0 = 0`` in camera coordinates, unit norm),
    and the result also has ``R`` [P, 3, 3], ``t`` [P, 3] (unit norm; ``x1 ~ R x0 + t``) and ``n_front`` [P] (the inliers in front of both
    cameras), zero for the pairs of another model.  Five correspondences suffice.  A call without a pose pair allocates and returns
    exactly what it did before this model existed."""
    P = len(outs)
    if P == 0 or len(datas) != P or (h_refs is not None and len(h_refs) != P):
        raise ValueError("verify_pairs: datas, outs (and h_refs) must be non-empty lists of one length")
    models = list(model) if isinstance(model, (list, tuple)) else [model] * P
    if len(models) != P:
        raise ValueError("verify_pairs: model must be 'homography', 'fundamental' or a list of one per pair")
    models = [hip.verify_model(m) for m in models]
    if h_refs is not None and any(m != hip.VERIFY_MODELS["homography"] for m in models):
        raise ValueError("verify_pairs: h_refs cannot be combined with model='fundamental' or 'pose' (there is no error column for F or E)")
    pose = [m == hip.VERIFY_MODELS["pose"] for m in models]
    cams = [None] * P
    if any(pose):
        if intrinsics is None:
            raise ValueError("verify_pairs: model='pose' needs intrinsics=(K0, K1)")
        cams = list(intrinsics) if len(intrinsics) == P and not _is_camera_pair(intrinsics) else [intrinsics] * P
        if len(cams) != P or any(is_pose and (c is None or not _is_camera_pair(c)) for is_pose, c in zip(pose, cams)):
            raise ValueError("verify_pairs: intrinsics must be one (K0, K1) pair of 3x3 matrices or a list of one per pair")
    elif intrinsics is not None:
        raise ValueError("verify_pairs: intrinsics are read with model='pose' only")
    dev = outs[0]["matches0"].device
    records = torch.zeros((P, 8), dtype=torch.float32, device=dev)
    width = hip.VERIFY_POSE_FLOATS if any(pose) else 9
    homs = torch.zeros((P, width), dtype=torch.float32, device=dev)
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
        if pose[p]:
            it["intrinsics"] = cams[p]
        items.append(it)
        inl.append(m)
    keep = hip.verify_pairs(items, thresh, iters, lo_iters, seed)
    fitted = homs[:, :9].view(P, 3, 3) if any(pose) else homs.view(P, 3, 3)
    out = dict(records=records, homographies=fitted, models=fitted, inlier=inl, _keep=(keep, items))
    if any(pose):
        out.update(R=homs[:, 9:18].unflatten(1, (3, 3)), t=homs[:, 18:21], n_front=homs[:, 21])      # zero where the pair has another model
    return out


def _is_camera_pair(c) -> bool:
    try:
        return len(c) == 2 and all(np.asarray(k.cpu() if isinstance(k, torch.Tensor) else k).shape == (3, 3) for k in c)
    except (TypeError, ValueError):
        return False


def _one_set(name, model, least, width, points0, points1, thresh, iters, lo_iters, seed, **item):
    """One set of row-by-row correspondences through ``gims_verify_pairs``: ``(model floats [width], mask [K] uint8)`` as device tensors,
    or None below ``least`` points or without a model.  ``item``: further fields of the set (``intrinsics``).  One host read."""
    dev = points0.device if isinstance(points0, torch.Tensor) and points0.is_cuda else torch.device("cuda", torch.cuda.current_device())
    p0 = torch.as_tensor(points0).to(device=dev, dtype=torch.float32).reshape(-1, 2).contiguous()
    p1 = torch.as_tensor(points1).to(device=dev, dtype=torch.float32).reshape(-1, 2).contiguous()
    if p0.shape != p1.shape:
        raise ValueError(f"{name}: {tuple(p0.shape)} and {tuple(p1.shape)} points do not correspond row by row")
    k = int(p0.shape[0])
    if k < least:
        return None
    record = torch.zeros(8, dtype=torch.float32, device=dev)
    out = torch.zeros(width, dtype=torch.float32, device=dev)
    mask = torch.empty(k, dtype=torch.uint8, device=dev)
    work = hip.verify_pairs([dict(kpts0=p0, kpts1=p1, matches0=None, inlier=mask, record=record, homography=out, model=model, **item)],
                            thresh, iters, lo_iters, seed)
    ok = bool(record[RECORD_FIELDS.index("ok")].item())              # the host read: the stream has passed the call, `work` may go
    del work
    return (out, mask) if ok else None


def _find(name, model, least, points0, points1, thresh, iters, lo_iters, seed):
    r = _one_set(name, model, least, 9, points0, points1, thresh, iters, lo_iters, seed)
    return (r[0].view(3, 3), r[1].view(-1, 1)) if r is not None else (None, None)


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


def estimate_pose(kpts0, kpts1, K0, K1, thresh: float = 1.0, iters: int = 3000, lo_iters: int = 8, seed: int = 0):
    """The reference's ``estimate_pose(kpts0, kpts1, K0, K1, thresh)`` (utils/common.py:392-416) in shape: ``kpts0`` / ``kpts1`` are [K, 2]
    tensors or arrays of corresponding pixel coordinates, ``K0`` / ``K1`` the 3x3 intrinsics, ``thresh`` a Sampson distance in pixels
    (divided by the reference's own mean focal length inside).  Returns ``(R [3, 3], t [3], mask [K] bool)`` as device tensors with
    ``x1 ~ R x0 + t`` and ``|t| = 1``, or ``None`` below five points or without a model.  The estimator is this library's own
    (include/gims_hip.h), not OpenCV's.

    This call SYNCHRONISES with the device (it reads whether a model was found); the batched ``verify_pairs(model='pose')`` does not."""
    cams = tuple(np.asarray(c.cpu() if isinstance(c, torch.Tensor) else c, dtype=np.float64) for c in (K0, K1))
    r = _one_set("estimate_pose", "pose", 5, hip.VERIFY_POSE_FLOATS, kpts0, kpts1, thresh, iters, lo_iters, seed, intrinsics=cams)
    return (r[0][9:18].view(3, 3), r[0][18:21], r[1].bool()) if r is not None else None


def _f64(a, dev=None) -> torch.Tensor:
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))
    return t.to(device=dev if dev is not None else t.device, dtype=torch.float64)


def pose_error(T_0to1, R, t):
    """The reference's ``compute_pose_error`` (utils/common.py:492-498), batched: ``T_0to1`` [..., 4, 4] (or [..., 3, 4]), ``R`` [..., 3, 3],
    ``t`` [..., 3] -> ``(error_t, error_R)`` in degrees, float64 tensors of the leading shape.  The translation error is the angle between
    the directions, taken up to sign; both angles come from ``atan2(|sin|, cos)`` in float64 -- the reference's ``arccos`` loses half the
    digits near 0 degrees.  A zero ``t`` (a pair without a pose) gives 90 degrees."""
    R = _f64(R)
    T, t = _f64(T_0to1, R.device), _f64(t, R.device)
    Rg, tg = T[..., :3, :3], T[..., :3, 3]
    D = R.transpose(-1, -2) @ Rg
    axis = torch.stack([D[..., 2, 1] - D[..., 1, 2], D[..., 0, 2] - D[..., 2, 0], D[..., 1, 0] - D[..., 0, 1]], -1)
    err_r = torch.rad2deg(torch.atan2(axis.norm(dim=-1), D.diagonal(dim1=-2, dim2=-1).sum(-1) - 1.0))
    err_t = torch.rad2deg(torch.atan2(torch.linalg.cross(t, tg, dim=-1).norm(dim=-1), (t * tg).sum(-1).abs()))
    err_t = torch.where((t.norm(dim=-1) == 0) | (tg.norm(dim=-1) == 0), torch.full_like(err_t, 90.0), err_t)
    return err_t, err_r


def epipolar_error(kpts0, kpts1, T_0to1, K0, K1):
    """The reference's ``compute_epipolar_error`` (utils/common.py:456-475): the symmetric squared epipolar distance of every
    correspondence ``kpts0[i] <-> kpts1[i]`` ([..., N, 2] pixels) under the ground-truth pose, in camera coordinates; float64 [..., N]."""
    k0 = _f64(kpts0)
    dev = k0.device
    k1, T, K0, K1 = _f64(kpts1, dev), _f64(T_0to1, dev), _f64(K0, dev), _f64(K1, dev)
    one = torch.ones_like(k0[..., :1])
    x0 = torch.cat([(k0[..., 0:1] - K0[..., None, 0, 2:3]) / K0[..., None, 0, 0:1], (k0[..., 1:2] - K0[..., None, 1, 2:3]) / K0[..., None, 1, 1:2], one], -1)
    x1 = torch.cat([(k1[..., 0:1] - K1[..., None, 0, 2:3]) / K1[..., None, 0, 0:1], (k1[..., 1:2] - K1[..., None, 1, 2:3]) / K1[..., None, 1, 1:2], one], -1)
    tv = T[..., :3, 3]
    z = torch.zeros_like(tv[..., 0])
    skew = torch.stack([torch.stack([z, -tv[..., 2], tv[..., 1]], -1), torch.stack([tv[..., 2], z, -tv[..., 0]], -1),
                        torch.stack([-tv[..., 1], tv[..., 0], z], -1)], -2)
    E = skew @ T[..., :3, :3]
    Ep0 = x0 @ E.transpose(-1, -2)
    Etp1 = x1 @ E
    p1Ep0 = (x1 * Ep0).sum(-1)
    return p1Ep0 ** 2 * (1.0 / (Ep0[..., 0] ** 2 + Ep0[..., 1] ** 2) + 1.0 / (Etp1[..., 0] ** 2 + Etp1[..., 1] ** 2))


def pose_summary(errors, thresholds=(5, 10, 20)) -> dict:
    """The pose AUC the reference's family of matchers is reported with: ``errors`` holds, per pair, ``max(error_t, error_R)`` in
    degrees or an ``(error_t, error_R)`` couple; a pair without a pose (None, NaN or infinite) counts as an infinite error.  Returns
    ``auc`` (percent, one per threshold, over ``evalh.pose_auc``), ``n_pairs`` and ``n_posed``."""
    from .evalh import pose_auc
    worst = []
    for e in errors:
        if e is None:
            worst.append(math.inf)
            continue
        v = [float(x) for x in (e if isinstance(e, (tuple, list)) else [e])]
        worst.append(math.inf if any(math.isnan(x) for x in v) else max(v))
    return dict(auc=[100.0 * a for a in pose_auc(worst, thresholds)], n_pairs=len(worst), n_posed=sum(1 for e in worst if math.isfinite(e)),
                thresholds=tuple(thresholds))
