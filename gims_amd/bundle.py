"""Bundle adjustment: joint refinement of cameras and points, on the device (kernels: gims_amd/csrc/ba.hip,
GIMS_AUX_BUNDLE_ADJUST).

``resect_images`` gives every image a pose from its own correspondences and ``triangulate_tracks`` gives every track a point from cameras
taken as known, so the errors of the incremental loop only accumulate.  ``bundle_adjust`` is the step that joins what the loop has
estimated: it moves the free cameras and the points together so that the reprojection cost over all the inlier observations goes down,
in one asynchronous op and without reading tracks, keypoints, points or poses back::

    estimate_pose(0, 1) -> triangulate_tracks -> resect_images(the rest) -> triangulate_tracks(all) -> bundle_adjust -> ...

The specification (include/gims_hip.h has it in full; tests/ba_ref.py is its NumPy restatement).  World to camera is ``x_c = R X + t``.
``iters`` Levenberg-Marquardt rounds; a round eliminates the points (Schur complement), factors the dense reduced camera system (6 x 6
blocks, at most 128 free cameras) by Cholesky -- or, with ``solver='pcg'``, solves it by preconditioned conjugate gradients without
forming it (GIMS_AUX_BUNDLE_ADJUST_PCG; at most 65536 free cameras) --, substitutes back, and is taken iff the cost goes
down and every observation stays in front of its camera; after five rounds in a row that were not taken the rest do nothing.  The
inlier set is an input and is not decided again.  All arithmetic is float64; the output bytes are identical across runs.

The gauge.  A reconstruction is defined up to a similarity: seven numbers that no observation fixes.  ``fixed`` names the cameras that do
not move; the default is the first two posed images in index order, which fixes position, orientation and -- through the distance between
the two -- the scale.  With fewer than two fixed cameras the damping alone keeps the rounds regular and the result drifts.

Focal lengths.  ``refine_focal`` (with ``solver='pcg'``; DESIGN.md 4.22, GIMS_AUX_BUNDLE_ADJUST_FOCAL) makes the focal lengths unknowns: every
posed image belongs to at most one focal group, and a group has one unknown, a relative scale of ``fx`` and ``fy`` of all its images (the
aspect ratio and the principal point stay).  A group collects the observations of all its images, those of fixed cameras included: fixing
a pose fixes the gauge, not the lens."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import hip
from .resect import _nonempty
from .triangulate import _host


class Adjusted:
    """The result of ``bundle_adjust``.  Device tensors: ``xyz`` float64 [T, 3] (points that were not active are copied through), ``records``
    float64 [n, 18] -- the camera records of the op, the format ``triangulate_tracks`` takes as ``cameras`` -- and its views ``R`` [n, 3, 3] and
    ``t`` [n, 3] (absent, fixed and held cameras are copied through), ``obs_error`` float32 [n_obs] (pixels, under the final state; -1 for an
    observation that was not active), ``cam_obs`` int32 [n] (active observations per image), ``history`` float64 [iters + 1, 2] ({cost,
    lambda} at the start and after every round), ``taken`` uint8 [iters].  With ``solver='pcg'`` also ``cg_used`` int32 [iters] (the
    conjugate-gradient iterations of every round) and ``cg_res`` float64 [iters] (sqrt(rho_stop / rho_0), the preconditioned residual the
    round's iteration stopped at, relative to its start); both are ``None`` for the dense solver.  ``mode``: the host list of the cameras'
    modes (0 absent, 1 fixed, 2 free).  ``K`` float64 [n, 4]: the view fx, fy, cx, cy of ``records``.  With ``refine_focal`` also
    ``focal_scale`` float64 [n_groups] (refined focal / starting focal of every group; 1 for a held group), ``group_obs`` int32 [n_groups]
    (the active observations of the group's images) and ``group``, the host list of the images' dense group ids (-1: fixed intrinsics);
    the three are ``None`` without it.

    ``stats`` (n_free, n_fixed, n_held, n_points, n_active_obs, n_bad_obs, rounds_taken, status) reads the op's counters back on first
    access, and ``cameras()`` reads the records: these two synchronise with the device; everything else is handed over asynchronously."""

    def __init__(self, views: dict, mode, K, keep, group=None):
        self.xyz, self.records = views["xyz"], views["cams"]
        self.R, self.t = self.records[:, 4:13].unflatten(1, (3, 3)), self.records[:, 13:16]
        self.obs_error, self.cam_obs, self.history, self.taken = views["obs_error"], views["cam_obs"], views["history"], views["taken"]
        self.cg_used, self.cg_res = views.get("cg_used"), views.get("cg_res")
        self.mode = [int(m) for m in mode]
        self.K = self.records[:, 0:4]
        self.focal_scale, self.group_obs = views.get("focal_scale"), views.get("group_obs")
        self.group = None if group is None else [int(g) for g in group]
        self._K, self._counters, self._keep, self._stats = K, views["counters"], keep, None

    @property
    def stats(self) -> dict:
        if self._stats is None:
            with torch.cuda.device(self._counters.device):
                pin = torch.empty(8, dtype=torch.int32, pin_memory=True)
                pin.copy_(self._counters, non_blocking=True)
                done = torch.cuda.Event()
                done.record()
                done.synchronize()      # the host synchronisation of .stats
            self._stats = dict(zip(hip.BA_COUNTERS, (int(v) for v in pin.tolist())))
        return self._stats

    def cameras(self):
        """The host ``(K, R, t)`` triple for the next ``triangulate_tracks`` / ``resect_images`` / ``bundle_adjust`` call; the absent
        cameras hold NaN poses, as they did on the way in.  With ``refine_focal`` K holds the refined fx and fy of the records.

        This call SYNCHRONISES with the device: it reads the records back."""
        rec = self.records.cpu().numpy()
        R, t = rec[:, 4:13].reshape(-1, 3, 3).copy(), rec[:, 13:16].copy()
        absent = np.array(self.mode, dtype=np.int64) == hip.BA_ABSENT
        R[absent], t[absent] = np.nan, np.nan
        K = self._K.copy()
        if self.group is not None:
            K[:, 0, 0], K[:, 1, 1] = rec[:, 0], rec[:, 1]
        return K, R, t

    def __len__(self):
        return int(self.xyz.shape[0])

    def __repr__(self):
        return f"Adjusted(n_points={len(self)}, n_images={len(self.mode)}, n_free={sum(m == hip.BA_FREE for m in self.mode)})"


def _focal_groups(name, refine_focal, solver, posed, K):
    """The dense host group ids int32 [n_images] (-1: fixed intrinsics) of ``refine_focal``, or None."""
    if refine_focal is None:
        return None
    if solver != "pcg":
        raise ValueError(f"{name}: refine_focal needs the matrix-free solver: pass solver='pcg' (the dense reduced system has no focal block)")
    n_images = len(posed)
    group = np.full(n_images, -1, np.int32)
    if isinstance(refine_focal, str):
        if refine_focal not in ("shared", "per_image"):
            raise ValueError(f"{name}: refine_focal must be None, 'shared', 'per_image' or {n_images} integers, got {refine_focal!r}")
        group[posed] = 0 if refine_focal == "shared" else np.arange(int(posed.sum()), dtype=np.int32)
    else:
        try:
            ids = list(refine_focal)
        except TypeError:
            raise ValueError(f"{name}: refine_focal must be None, 'shared', 'per_image' or {n_images} integers, got {refine_focal!r}") from None
        if len(ids) != n_images:
            raise ValueError(f"{name}: refine_focal holds {len(ids)} group ids for {n_images} images")
        for k, g in enumerate(ids):
            if isinstance(g, bool) or not isinstance(g, (int, np.integer)):
                raise ValueError(f"{name}: refine_focal[{k}] = {g!r}: a group id must be an integer (-1: the intrinsics stay fixed)")
            if g < -1:
                raise ValueError(f"{name}: refine_focal[{k}] = {g}: a group id must be >= -1 (-1: the intrinsics stay fixed)")
        dense = {}
        for k, g in enumerate(ids):                                # dense ids in the order of first appearance among the posed images
            if posed[k] and g >= 0:
                group[k] = dense.setdefault(int(g), len(dense))
    for g in range(int(group.max()) + 1 if n_images else 0):
        mine = np.flatnonzero(group == g)
        ratio = K[mine, 0, 0] / K[mine, 1, 1]
        if (np.abs(ratio - ratio[0]) > 1e-12 * np.abs(ratio[0])).any():
            raise ValueError(f"{name}: the images {mine.tolist()} of one focal group have different fx / fy ratios: one scale cannot serve them "
                             "(give them groups of their own)")
    return group


def _check(points, tracks, images, cameras, fixed, use_obs, use_points, iters, huber, lambda0, solver="dense", cg_iters=64, cg_tol=1e-6, refine_focal=None):
    """Everything bundle_adjust checks before the device is touched -> (keypoint tensors, host records, host K, modes, obs mask, point mask,
    focal groups or None)."""
    name = "bundle_adjust"
    if solver not in ("dense", "pcg"):
        raise ValueError(f"{name}: solver must be 'dense' or 'pcg', got {solver!r}")
    if isinstance(cg_iters, bool) or not isinstance(cg_iters, (int, np.integer)) or not 1 <= cg_iters <= hip.BA_PCG_MAX_CG_ITERS:
        raise ValueError(f"{name}: cg_iters must be an integer in 1 .. {hip.BA_PCG_MAX_CG_ITERS}, got {cg_iters!r}")
    if isinstance(cg_tol, bool) or not (isinstance(cg_tol, (int, float)) and math.isfinite(cg_tol) and 0 <= cg_tol < 1):
        raise ValueError(f"{name}: cg_tol must be finite with 0 <= cg_tol < 1, got {cg_tol!r}")
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or not 0 <= iters <= 255:
        raise ValueError(f"{name}: iters must be an integer in 0 .. 255, got {iters!r}")
    if isinstance(huber, bool) or not (isinstance(huber, (int, float)) and math.isfinite(huber) and huber >= 0):
        raise ValueError(f"{name}: huber must be finite and >= 0 (pixels; 0: the squared loss), got {huber!r}")
    if isinstance(lambda0, bool) or not (isinstance(lambda0, (int, float)) and math.isfinite(lambda0) and lambda0 > 0 and float(np.float32(lambda0)) > 0
                                         and math.isfinite(float(np.float32(lambda0)))):
        raise ValueError(f"{name}: lambda0 must be finite and > 0 (as a float32), got {lambda0!r}")
    for attr in ("indptr", "obs_image", "obs_keypoint", "image_start"):
        if not hasattr(tracks, attr):
            raise ValueError(f"{name}: tracks must be the Tracks of build_tracks (it has no {attr})")
    for attr in ("xyz", "obs_inlier", "valid"):
        if not hasattr(points, attr):
            raise ValueError(f"{name}: points must be the Points3D of triangulate_tracks (it has no {attr})")
    start = list(tracks.image_start)
    n_images = len(start) - 1
    if len(images) != n_images:
        raise ValueError(f"{name}: {len(images)} images are given, the tracks were built over {n_images}")
    kpts = []
    for k, im in enumerate(images):
        t = im.keypoints if hasattr(im, "keypoints") else im
        if not isinstance(t, torch.Tensor) or not t.dtype.is_floating_point:
            raise ValueError(f"{name}: image {k}: the keypoints must be a floating-point tensor, got {getattr(t, 'dtype', type(t).__name__)}")
        if t.numel() != 2 * (start[k + 1] - start[k]) or (t.dim() >= 1 and t.numel() and t.shape[-1] != 2):
            raise ValueError(f"{name}: image {k}: keypoints of shape {tuple(t.shape)}, the tracks were built over {start[k + 1] - start[k]} keypoints ([n_k, 2])")
        kpts.append(t)
    if not isinstance(cameras, (tuple, list)) or len(cameras) != 3:
        raise ValueError(f"{name}: cameras must be (K [n, 3, 3], R [n, 3, 3], t [n, 3])")
    try:
        K, R, t = _host(cameras[0], "K", (None, 3, 3)), _host(cameras[1], "R", (None, 3, 3)), _host(cameras[2], "t", (None, 3))
    except ValueError as e:
        raise ValueError(str(e).replace("triangulate_tracks", name)) from None
    if not len(K) == len(R) == len(t) == n_images:
        raise ValueError(f"{name}: {len(K)} / {len(R)} / {len(t)} cameras (K / R / t) for {n_images} images")
    posed = np.isfinite(R).all(axis=(1, 2)) & np.isfinite(t).all(axis=1) if n_images else np.zeros(0, bool)
    Kp = K[posed]
    if len(Kp) and ((Kp[:, 0, 1] != 0).any() or (Kp[:, 1, 0] != 0).any() or (Kp[:, 2] != np.array([0.0, 0.0, 1.0])).any()):
        raise ValueError(f"{name}: K must be [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]: skew or another last row is not supported")
    if len(Kp) and not (np.isfinite(Kp).all() and (Kp[:, 0, 0] > 0).all() and (Kp[:, 1, 1] > 0).all()):
        raise ValueError(f"{name}: the K of a posed camera must be finite with fx > 0 and fy > 0")
    if fixed is None:
        fixed = [int(k) for k in np.flatnonzero(posed)[:2]]
    fixed = list(fixed)
    for k in fixed:
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= k < n_images:
            raise ValueError(f"{name}: fixed holds {k!r}: an image index must be an integer in 0 .. {n_images - 1}")
        if not posed[k]:
            raise ValueError(f"{name}: fixed holds {k}: that image has no pose (its R or t is not finite)")
    mode = np.where(posed, hip.BA_FREE, hip.BA_ABSENT).astype(np.int32)
    mode[fixed] = hip.BA_FIXED
    group = _focal_groups(name, refine_focal, solver, posed, K)
    n_free = int((mode == hip.BA_FREE).sum())
    if solver == "dense" and n_free > hip.BA_MAX_FREE_CAMERAS:
        raise ValueError(f"{name}: {n_free} free cameras, at most {hip.BA_MAX_FREE_CAMERAS} (fix more of them, adjust a part of the set, or use solver='pcg')")
    if n_free > hip.BA_PCG_MAX_FREE_CAMERAS:
        raise ValueError(f"{name}: {n_free} free cameras, at most {hip.BA_PCG_MAX_FREE_CAMERAS} with solver='pcg'")
    device = tracks.indptr.device
    for attr in ("indptr", "obs_image", "obs_keypoint"):
        x = getattr(tracks, attr)
        if not isinstance(x, torch.Tensor) or x.dtype != torch.int32 or x.device != device:
            raise ValueError(f"{name}: tracks.{attr} must be an int32 tensor on {device}, got {getattr(x, 'dtype', None)} on {getattr(x, 'device', None)}")
    T, n_obs = tracks.indptr.numel() - 1, tracks.obs_image.numel()
    xyz = points.xyz
    if not isinstance(xyz, torch.Tensor) or xyz.dtype != torch.float64 or tuple(xyz.shape) != (T, 3) or xyz.device != device:
        raise ValueError(f"{name}: points.xyz must be a float64 tensor [{T}, 3] on {device}, got {getattr(xyz, 'dtype', None)} "
                         f"{tuple(getattr(xyz, 'shape', ()))} on {getattr(xyz, 'device', None)}")
    obs = points.obs_inlier if use_obs is None else use_obs
    if not isinstance(obs, torch.Tensor) or obs.dtype not in (torch.bool, torch.uint8) or tuple(obs.shape) != (n_obs,) or obs.device != device:
        raise ValueError(f"{name}: use_obs must be a bool or uint8 tensor [{n_obs}] on {device} (points.obs_inlier)")
    pts = points.valid if use_points is None else use_points
    if not isinstance(pts, torch.Tensor) or pts.dtype not in (torch.bool, torch.uint8) or tuple(pts.shape) != (T,) or pts.device != device:
        raise ValueError(f"{name}: use_points must be a bool or uint8 tensor [{T}] on {device} (points.valid or points.filter(...))")
    for k, x in enumerate(kpts):
        if x.device != device:
            raise ValueError(f"{name}: image {k}: the keypoints are on {x.device}, the tracks on {device}")
    if device.type != "cuda":
        raise ValueError(f"{name}: the tracks are on {device}: cameras and points are adjusted on the GPU, from device tensors")
    counts = [start[k + 1] - start[k] for k in range(n_images)]
    return kpts, hip.triangulate_cameras(K, R, t, counts), K, mode, obs, pts, group


def bundle_adjust(points, tracks, images, cameras, *, fixed=None, use_obs=None, use_points=None, iters: int = 20, huber: float = 0.0,
                  lambda0: float = 1e-4, solver: str = "dense", cg_iters: int = 64, cg_tol: float = 1e-6, refine_focal=None) -> Adjusted:
    """Refine the posed cameras and the points jointly, on the device.

    ``points``: the ``Points3D`` of ``triangulate_tracks`` (the starting points); ``tracks``: the ``Tracks`` they belong to; ``images``: the
    list the tracks were built over -- ``ImageFeatures`` or [n_k, 2] tensors of pixel coordinates.  ``cameras``: the host triple ``(K [n, 3,
    3], R [n, 3, 3], t [n, 3])`` of ``triangulate_tracks`` and ``Poses.cameras`` (the starting cameras); an image whose R or t is not
    finite is ABSENT: its observations are ignored.  ``fixed``: the image indices that do not move (default: the first two posed images in
    index order -- this fixes the gauge, scale included; see the module text); every other posed camera is free, at most 128 of them.
    ``use_obs``: bool / uint8 [n_obs], the observations that enter the cost (default ``points.obs_inlier``); the set is NOT decided again
    inside the op.  ``use_points``: bool / uint8 [T] (default ``points.valid``).  A point needs two such observations in posed cameras to
    move; a free camera with fewer than four is held.  ``iters``: Levenberg-Marquardt rounds (0 .. 255); ``huber``: the Huber bound in
    pixels, 0 for the squared loss; ``lambda0``: the starting damping.

    ``solver``: ``'dense'`` factors the reduced camera system by Cholesky (at most 128 free cameras); ``'pcg'`` solves it by preconditioned
    conjugate gradients without forming it (at most 65536 free cameras): at most ``cg_iters`` (1 .. 256) iterations per
    round, stopped early once the preconditioned residual has fallen to ``cg_tol`` (0 <= cg_tol < 1) of its start.  The two arguments are
    checked and then ignored by ``'dense'``.

    ``refine_focal`` (``solver='pcg'`` only): ``None`` keeps every K as given; ``'shared'`` refines one relative scale of
    the focal lengths of all posed images; ``'per_image'`` one per posed image; a sequence of ``n_images`` integers gives every image its
    focal group (-1: its intrinsics stay fixed).  ``Adjusted.focal_scale`` has the refined / starting focal of every group, ``Adjusted.K``
    and ``Adjusted.cameras()`` the refined intrinsics.  A group with fewer than four active observations is held.

    ValueError, before the device is touched: a count that disagrees with ``tracks.image_start``, cameras of another shape or count, a K
    of a posed camera with skew, another last row or a focal length that is not positive, an index of ``fixed`` out of range or without a
    pose, more than 128 free cameras (65536 with ``solver='pcg'``), tensors of a wrong dtype, shape or device, a parameter out of range,
    ``refine_focal`` with ``solver='dense'``, of a wrong length, with an id that is no integer or is below -1, or with a group whose
    images differ in fx / fy.

    Host synchronisation: NONE.  ``Adjusted.stats`` and ``Adjusted.cameras()`` read back."""
    kpts, rec, K, mode, obs, pts, group = _check(points, tracks, images, cameras, fixed, use_obs, use_points, iters, huber, lambda0, solver, cg_iters, cg_tol,
                                                 refine_focal)
    device = tracks.indptr.device
    with torch.cuda.device(device):
        allk = torch.cat([k.reshape(-1, 2).float() for k in kpts]).contiguous() if kpts else torch.zeros((0, 2), device=device)
        T, n_obs, n = tracks.indptr.numel() - 1, tracks.obs_image.numel(), allk.shape[0]
        dev_cams = (hip.upload_large(rec.view(np.uint8).reshape(-1), device).view(torch.float64).view(-1, hip.TRI_CAMERA_WORDS) if rec.size
                    else torch.zeros((1, hip.TRI_CAMERA_WORDS), dtype=torch.float64, device=device))
        views, keep = hip.bundle_adjust(tracks.indptr.contiguous(), _nonempty(tracks.obs_image.contiguous(), (1,), torch.int32),
                                        _nonempty(tracks.obs_keypoint.contiguous(), (1,), torch.int32), _nonempty(obs.contiguous().view(torch.uint8), (1,), torch.uint8),
                                        _nonempty(pts.contiguous().view(torch.uint8), (1,), torch.uint8), _nonempty(allk, (1, 2), torch.float32),
                                        _nonempty(points.xyz.contiguous(), (1, 3), torch.float64), dev_cams, mode, iters=int(iters), huber=float(huber),
                                        lambda0=float(lambda0), T=T, n_obs=n_obs, n=n, solver=solver, cg_iters=int(cg_iters), cg_tol=float(cg_tol), group=group)
    return Adjusted(views, mode, K, keep, group)
