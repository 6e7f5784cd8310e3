"""Robust multi-view triangulation of tracks from known cameras, on the device (kernels: gims_amd/csrc/triangulate.hip,
GIMS_AUX_TRIANGULATE_TRACKS).

``build_tracks`` ends with "keypoint 17 of image 0 = keypoint 230 of image 3 = keypoint 5 of image 7"; what every consumer of tracks with
posed images does next is turn each of them into a 3-D point and find out which of its observations are wrong.  ``triangulate_tracks`` does
that for all tracks in one asynchronous op, without reading the tracks or the keypoints back.

The specification (include/gims_hip.h has it in full; tests/triangulate_ref.py is its NumPy restatement).  World to camera is
``x_c = R X + t``.  Per track: up to ``max_hyp`` two-view midpoints, spread evenly over the pairs of its observations, are scored by their
reprojection inliers (depth > 0, error <= ``thresh`` pixels); the inlier set of the best one gives the midpoint of all its rays, which at
most ``refine_iters`` guarded Gauss-Newton rounds on the reprojection cost refine; every observation is then classified once.  A track needs
two inliers from two images (else NO_MODEL) and a largest angle between inlier rays of ``min_angle`` degrees (else LOW_ANGLE: the point is
still given).  All arithmetic is float64; the outputs of a track are bit-identical alone or in any batch."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import hip

TOO_SHORT, NO_MODEL, LOW_ANGLE, TOO_LONG = hip.TRI_TOO_SHORT, hip.TRI_NO_MODEL, hip.TRI_LOW_ANGLE, hip.TRI_TOO_LONG


class Points3D:
    """The result of ``triangulate_tracks``.  Device tensors, one entry per track: ``xyz`` float64 [T, 3] (zeros without a model), ``status``
    uint8 [T] (bits TOO_SHORT = 1, NO_MODEL = 2, LOW_ANGLE = 4, TOO_LONG = 8), ``valid`` bool [T] (``status == 0``), ``n_inliers`` int32 [T],
    ``max_angle`` float32 [T] (degrees, the largest angle at the point between two inlier rays), ``rms_error`` float32 [T] (pixels, over the
    inliers); one entry per observation of the ``Tracks``: ``obs_inlier`` uint8 [n_obs], ``obs_error`` float32 [n_obs] (pixels; -1 for an
    observation that is bad, behind its camera, or of a track without a model).

    ``stats`` (n_ok, n_low_angle, n_no_model, n_too_short, n_too_long, n_bad_obs, n_inlier_obs) reads the op's counters back on first
    access: it is the ONE member that synchronises with the device; everything else is handed over asynchronously."""

    def __init__(self, views: dict, keep):
        self.xyz, self.status, self.n_inliers = views["xyz"], views["status"], views["n_inliers"]
        self.max_angle, self.rms_error = views["max_angle"], views["rms_error"]
        self.obs_inlier, self.obs_error = views["obs_inlier"], views["obs_error"]
        self.valid = self.status == 0
        self._counters, self._keep, self._stats = views["counters"], keep, None

    @property
    def stats(self) -> dict:
        if self._stats is None:
            with torch.cuda.device(self._counters.device):
                pin = torch.empty(8, dtype=torch.int32, pin_memory=True)
                pin.copy_(self._counters, non_blocking=True)
                done = torch.cuda.Event()
                done.record()
                done.synchronize()      # the one host synchronisation of a Points3D
            self._stats = dict(zip(hip.TRI_COUNTERS, (int(v) for v in pin.tolist())))
        return self._stats

    def filter(self, min_views: int = 2, max_rms: float | None = None) -> torch.Tensor:
        """bool [T]: the valid tracks with at least ``min_views`` inlier observations and, when given, an rms error of at most ``max_rms``."""
        mask = self.valid & (self.n_inliers >= int(min_views))
        return mask if max_rms is None else mask & (self.rms_error <= float(max_rms))

    def __len__(self):
        return int(self.status.shape[0])

    def __repr__(self):
        return f"Points3D(n_tracks={len(self)}, n_obs={int(self.obs_inlier.shape[0])})"


def _host(x, name, shape):
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    if a.dtype.kind not in "fiu" or a.ndim != len(shape) or any(s is not None and s != d for s, d in zip(shape, a.shape)):
        want = "[" + ", ".join("n" if s is None else str(s) for s in shape) + "]"
        raise ValueError(f"triangulate_tracks: {name} must be a real array of shape {want}, got {a.dtype} {tuple(a.shape)}")
    return a.astype(np.float64)


def _check(tracks, images, cameras, thresh, min_angle, max_hyp, refine_iters):
    """Everything triangulate_tracks checks before the device is touched -> (keypoint tensors, host camera records)."""
    for name, v, lo, hi in (("max_hyp", max_hyp, 0, 65535), ("refine_iters", refine_iters, 0, 255)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError(f"triangulate_tracks: {name} must be an integer in {lo} .. {hi}, got {v!r}")
    if not (isinstance(thresh, (int, float)) and math.isfinite(thresh) and thresh > 0):
        raise ValueError(f"triangulate_tracks: thresh must be finite and > 0, got {thresh!r}")
    if not (isinstance(min_angle, (int, float)) and math.isfinite(min_angle) and 0 <= min_angle < 180):
        raise ValueError(f"triangulate_tracks: min_angle must be in [0, 180) degrees, got {min_angle!r}")
    for name in ("indptr", "obs_image", "obs_keypoint", "image_start"):
        if not hasattr(tracks, name):
            raise ValueError(f"triangulate_tracks: tracks must be the Tracks of build_tracks (it has no {name})")
    start = list(tracks.image_start)
    n_images = len(start) - 1
    if len(images) != n_images:
        raise ValueError(f"triangulate_tracks: {len(images)} images are given, the tracks were built over {n_images}")
    kpts = []
    for k, im in enumerate(images):
        t = im.keypoints if hasattr(im, "keypoints") else im
        if not isinstance(t, torch.Tensor) or not t.dtype.is_floating_point:
            raise ValueError(f"triangulate_tracks: image {k}: the keypoints must be a floating-point tensor, got {getattr(t, 'dtype', type(t).__name__)}")
        if t.numel() != 2 * (start[k + 1] - start[k]) or (t.dim() >= 1 and t.numel() and t.shape[-1] != 2):
            raise ValueError(f"triangulate_tracks: image {k}: keypoints of shape {tuple(t.shape)}, the tracks were built over {start[k + 1] - start[k]} "
                             "keypoints ([n_k, 2])")
        kpts.append(t)
    device = tracks.indptr.device
    if isinstance(cameras, torch.Tensor):                        # the op's records on the device: Adjusted.records of bundle_adjust
        if cameras.dtype != torch.float64 or tuple(cameras.shape) != (n_images, hip.TRI_CAMERA_WORDS) or cameras.device != device or device.type != "cuda":
            raise ValueError(f"triangulate_tracks: device camera records must be a float64 tensor [{n_images}, {hip.TRI_CAMERA_WORDS}] on the tracks' "
                             f"GPU, got {cameras.dtype} {tuple(cameras.shape)} on {cameras.device}")
        for name in ("indptr", "obs_image", "obs_keypoint"):
            x = getattr(tracks, name)
            if x.dtype != torch.int32 or x.device != device:
                raise ValueError(f"triangulate_tracks: tracks.{name} must be an int32 tensor on {device}, got {x.dtype} on {x.device}")
        for k, x in enumerate(kpts):
            if x.device != device:
                raise ValueError(f"triangulate_tracks: image {k}: the keypoints are on {x.device}, the tracks on {device}")
        return kpts, cameras.contiguous()
    if not isinstance(cameras, (tuple, list)) or len(cameras) != 3:
        raise ValueError("triangulate_tracks: cameras must be (K [n, 3, 3], R [n, 3, 3], t [n, 3])")
    K, R, t = _host(cameras[0], "K", (None, 3, 3)), _host(cameras[1], "R", (None, 3, 3)), _host(cameras[2], "t", (None, 3))
    if not len(K) == len(R) == len(t) == n_images:
        raise ValueError(f"triangulate_tracks: {len(K)} / {len(R)} / {len(t)} cameras (K / R / t) for {n_images} images")
    if n_images and ((K[:, 0, 1] != 0).any() or (K[:, 1, 0] != 0).any() or (K[:, 2] != np.array([0.0, 0.0, 1.0])).any()):
        raise ValueError("triangulate_tracks: K must be [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]: skew or another last row is not supported")
    counts = [start[k + 1] - start[k] for k in range(n_images)]
    for name in ("indptr", "obs_image", "obs_keypoint"):
        x = getattr(tracks, name)
        if x.dtype != torch.int32 or x.device != device:
            raise ValueError(f"triangulate_tracks: tracks.{name} must be an int32 tensor on {device}, got {x.dtype} on {x.device}")
    for k, x in enumerate(kpts):
        if x.device != device:
            raise ValueError(f"triangulate_tracks: image {k}: the keypoints are on {x.device}, the tracks on {device}")
    if device.type != "cuda":
        raise ValueError(f"triangulate_tracks: the tracks are on {device}: they are triangulated on the GPU, from device tensors")
    return kpts, hip.triangulate_cameras(K, R, t, counts)


def triangulate_tracks(tracks, images, cameras, *, thresh: float = 4.0, min_angle: float = 1.5, max_hyp: int = 64, refine_iters: int = 10) -> Points3D:
    """Triangulate every track of ``tracks`` (the ``Tracks`` of ``build_tracks``) on the device.

    ``images``: the list the tracks were built over -- ``ImageFeatures`` (``.keypoints`` is read) or [n_k, 2] tensors of pixel coordinates;
    they are concatenated as ``Tracks.points`` does.  ``cameras``: ``(K [n, 3, 3], R [n, 3, 3], t [n, 3])`` as arrays or tensors, world to
    camera ``x_c = R X + t``; they are turned into the op's float64 records on the host (give them as host values: a device tensor is copied
    back first, which waits for the device); or the op's own records as a device tensor float64 [n, 18] (``Adjusted.records`` of
    ``bundle_adjust``), which are used where they lie, with no host step.  ``thresh``: the inlier bound in pixels; ``min_angle``: degrees;
    ``max_hyp``: the number of two-view hypotheses per track (0: none, every observation enters the solve); ``refine_iters``: Gauss-Newton
    rounds.

    ValueError, before the device is touched: a count that disagrees with ``tracks.image_start``, cameras of another shape or count, a K
    with skew or a last row other than (0, 0, 1), tensors of a wrong dtype or on different devices, a parameter out of range.

    Host synchronisation: NONE -- the host already knows the number of tracks and observations.  ``Points3D.stats`` reads the counters."""
    kpts, rec = _check(tracks, images, cameras, thresh, min_angle, max_hyp, refine_iters)
    device = tracks.indptr.device
    with torch.cuda.device(device):
        allk = torch.cat([k.reshape(-1, 2).float() for k in kpts]).contiguous() if kpts else torch.zeros((0, 2), device=device)
        if allk.numel() == 0:
            allk = torch.zeros((1, 2), device=device)[:0]
        views, keep = hip.triangulate_tracks(tracks.indptr.contiguous(), tracks.obs_image.contiguous(), tracks.obs_keypoint.contiguous(), allk, rec,
                                             thresh=float(thresh), min_angle=float(min_angle), max_hyp=int(max_hyp), refine_iters=int(refine_iters))
    return Points3D(views, keep)


def cameras_from_pose(K0, K1, R, t):
    """The two-camera ``cameras`` of one ``estimate_pose`` / ``verify_pairs(model='pose')`` result: camera 0 is the world, camera 1 is
    ``x1 ~ R x0 + t``.  The points come out in the pair's own scale (|t| = 1 for an estimated pose)."""
    host = lambda x: np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float64)      # noqa: E731
    K0, K1, R, t = host(K0).reshape(3, 3), host(K1).reshape(3, 3), host(R).reshape(3, 3), host(t).reshape(3)
    return np.stack([K0, K1]), np.stack([np.eye(3), R]), np.stack([np.zeros(3), t])
