"""Absolute camera poses from 2-D to 3-D matches (resection), on the device (kernels: gims_amd/csrc/resect.hip,
GIMS_AUX_RESECT_IMAGES).

``triangulate_tracks`` gives the tracks of posed images their 3-D points; an image that has no pose yet observes keypoints whose tracks
already have one.  ``resect_images`` turns those 2-D to 3-D correspondences into the image's pose, for many images in one asynchronous op
and without reading ``track_of``, the points or the keypoints back -- which closes the incremental loop on the device::

    estimate_pose(0, 1) -> triangulate_tracks -> resect_images(the rest) -> triangulate_tracks(all) -> ...

The specification (include/gims_hip.h has it in full; tests/resect_ref.py is its NumPy restatement).  World to camera is ``x_c = R X + t``.
Per image: ``iters`` P3P hypotheses from three sampled correspondences each, scored by their reprojection inliers (depth > 0, error <=
``thresh`` pixels); the best one is refined by at most ``lo_iters`` guarded Gauss-Newton rounds over its inliers; every correspondence is
then classified once.  A pose needs ``max(min_inliers, 4)`` inliers.  All arithmetic is float64; the outputs of an image are bit-identical
alone or in any batch."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import hip
from .triangulate import _host


class Poses:
    """The result of ``resect_images``.  ``image``: the host list of the resected image indices (the entries, in the caller's order).
    Device tensors, one row per entry: ``R`` float64 [m, 3, 3] and ``t`` float64 [m, 3] (world to camera ``x_c = R X + t``; zeros without
    a pose), ``ok`` bool [m], ``n_corr`` int32 [m] (the 2-D to 3-D correspondences the image had), ``n_inliers`` int32 [m], ``rms_error``
    float32 [m] (pixels, over the inliers), ``best_hyp`` / ``best_hyp_inliers`` / ``lo_rounds`` int32 [m]; one slot per keypoint of every
    entry, the entries back to back: ``kp_inlier`` uint8 and ``kp_error`` float32 (pixels; -1 for a keypoint that is no correspondence,
    lies behind the camera, or belongs to an entry without a pose).  ``of_entry(e)`` cuts the slots of one entry.

    ``stats`` (n_ok, n_failed, n_corr_total, n_inlier_total) reads the op's counters back on first access, and ``cameras`` reads the poses:
    these two synchronise with the device; everything else is handed over asynchronously."""

    def __init__(self, views: dict, image, keep):
        self.image = [int(k) for k in image]
        m = len(self.image)
        self.R, self.t = views["pose"][:, :9].reshape(m, 3, 3), views["pose"][:, 9:]
        self.ok = views["ok"] != 0
        self.n_corr, self.n_inliers, self.rms_error = views["n_corr"], views["n_inliers"], views["rms_error"]
        self.best_hyp, self.best_hyp_inliers, self.lo_rounds = views["best_hyp"], views["best_hyp_inliers"], views["lo_rounds"]
        self.kp_inlier, self.kp_error, self.slots = views["kp_inlier"], views["kp_error"], list(views["slots"])
        self._counters, self._keep, self._stats = views["counters"], keep, None

    def of_entry(self, e: int):
        """(kp_inlier, kp_error) of entry e: views of its n_k slots."""
        if not 0 <= e < len(self.image):
            raise ValueError(f"Poses.of_entry: entry {e} is out of range (0 .. {len(self.image) - 1})")
        return self.kp_inlier[self.slots[e]:self.slots[e + 1]], self.kp_error[self.slots[e]:self.slots[e + 1]]

    @property
    def stats(self) -> dict:
        if self._stats is None:
            with torch.cuda.device(self._counters.device):
                pin = torch.empty(8, dtype=torch.int32, pin_memory=True)
                pin.copy_(self._counters, non_blocking=True)
                done = torch.cuda.Event()
                done.record()
                done.synchronize()      # the host synchronisation of .stats
            self._stats = dict(zip(hip.RESECT_COUNTERS, (int(v) for v in pin.tolist())))
        return self._stats

    def cameras(self, K, R, t):
        """The host ``(K, R, t)`` triple for the next ``triangulate_tracks`` call: copies of ``R`` [n, 3, 3] and ``t`` [n, 3] (unposed images
        typically hold NaN, which ``triangulate_tracks`` ignores) with the poses of the ``ok`` entries filled in at their images; an image
        listed twice takes its last ``ok`` entry.  ``K`` [n, 3, 3] (or one 3 x 3 for all) is passed through.

        This call SYNCHRONISES with the device: it reads ``ok`` and the poses back."""
        R, t = _host(R, "R", (None, 3, 3)).copy(), _host(t, "t", (None, 3)).copy()
        K = np.asarray(K.detach().cpu().numpy() if isinstance(K, torch.Tensor) else K, dtype=np.float64)
        if K.shape == (3, 3):
            K = np.tile(K, (len(R), 1, 1))
        if len(self.image) and max(self.image) >= len(R):
            raise ValueError(f"Poses.cameras: image {max(self.image)} was resected, R holds {len(R)} cameras")
        ok, Rd, td = self.ok.cpu().numpy(), self.R.cpu().numpy(), self.t.cpu().numpy()
        for e, k in enumerate(self.image):
            if ok[e]:
                R[k], t[k] = Rd[e], td[e]
        return K, R, t

    def __len__(self):
        return len(self.image)

    def __repr__(self):
        return f"Poses(n_entries={len(self)}, n_keypoints={self.slots[-1]})"


def _params(name, thresh, iters, lo_iters, min_inliers, seed):
    for what, v, lo, hi in (("iters", iters, 0, 65535), ("lo_iters", lo_iters, 0, 255), ("min_inliers", min_inliers, 0, 2 ** 30), ("seed", seed, 0, 2 ** 64 - 1)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError(f"{name}: {what} must be an integer in {lo} .. {hi}, got {v!r}")
    if not (isinstance(thresh, (int, float)) and math.isfinite(thresh) and thresh > 0):
        raise ValueError(f"{name}: thresh must be finite and > 0, got {thresh!r}")


def _intrinsics(name, K, n_images):
    a = K.detach().cpu().numpy() if isinstance(K, torch.Tensor) else np.asarray(K)
    if a.dtype.kind not in "fiu" or a.shape not in ((3, 3), (n_images, 3, 3)):
        raise ValueError(f"{name}: intrinsics must be a real array of shape [3, 3] or [{n_images}, 3, 3], got {a.dtype} {tuple(a.shape)}")
    a = np.tile(a.astype(np.float64), (n_images, 1, 1)) if a.ndim == 2 else a.astype(np.float64)
    if n_images and ((a[:, 0, 1] != 0).any() or (a[:, 1, 0] != 0).any() or (a[:, 2] != np.array([0.0, 0.0, 1.0])).any()):
        raise ValueError(f"{name}: K must be [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]: skew or another last row is not supported")
    return a


def _check(points, tracks, images, intrinsics, which, use, thresh, iters, lo_iters, min_inliers, seed):
    """Everything resect_images checks before the device is touched -> (keypoint tensors, host entry records, image list, use mask)."""
    name = "resect_images"
    _params(name, thresh, iters, lo_iters, min_inliers, seed)
    for attr in ("track_of", "image_start"):
        if not hasattr(tracks, attr):
            raise ValueError(f"{name}: tracks must be the Tracks of build_tracks (it has no {attr})")
    for attr in ("xyz", "valid"):
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
    K = _intrinsics(name, intrinsics, n_images)
    if which is None:
        which = list(range(n_images))
    which = list(which)
    for k in which:
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= k < n_images:
            raise ValueError(f"{name}: which holds {k!r}: an image index must be an integer in 0 .. {n_images - 1}")
    device = tracks.track_of.device
    xyz = points.xyz
    if tracks.track_of.dtype != torch.int32 or tracks.track_of.numel() != start[-1]:
        raise ValueError(f"{name}: tracks.track_of must be an int32 tensor of {start[-1]} entries, got {tracks.track_of.dtype} {tuple(tracks.track_of.shape)}")
    if xyz.dtype != torch.float64 or xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.device != device:
        raise ValueError(f"{name}: points.xyz must be a float64 tensor [T, 3] on {device}, got {xyz.dtype} {tuple(xyz.shape)} on {xyz.device}")
    mask = points.valid if use is None else use
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8) or mask.shape != (xyz.shape[0],) or mask.device != device:
        raise ValueError(f"{name}: use must be a bool or uint8 tensor [{xyz.shape[0]}] on {device} (points.valid or points.filter(...))")
    for k, x in enumerate(kpts):
        if x.device != device:
            raise ValueError(f"{name}: image {k}: the keypoints are on {x.device}, the tracks on {device}")
    if device.type != "cuda":
        raise ValueError(f"{name}: the tracks are on {device}: images are resected on the GPU, from device tensors")
    counts = [start[k + 1] - start[k] for k in range(n_images)]
    return kpts, hip.resect_cameras(K, counts, which), which, mask


def _nonempty(t: torch.Tensor, shape, dtype):
    """An empty tensor has no address; the op wants one (it reads nothing through it)."""
    return t if t.numel() else torch.zeros(shape, dtype=dtype, device=t.device)


def resect_images(points, tracks, images, intrinsics, which=None, *, use=None, thresh: float = 4.0, iters: int = 1024, lo_iters: int = 8,
                  min_inliers: int = 12, seed: int = 0) -> Poses:
    """The absolute pose of every image of ``which`` from the keypoints whose track has a 3-D point, on the device.

    ``points``: the ``Points3D`` of ``triangulate_tracks``; ``use``: bool / uint8 [T], the points that may serve (default ``points.valid``;
    ``points.filter(...)`` is stricter).  ``tracks``: the ``Tracks`` the points belong to.  ``images``: the list the tracks were built over
    -- ``ImageFeatures`` or [n_k, 2] tensors of pixel coordinates.  ``intrinsics``: K [n, 3, 3] for all images, or one 3 x 3 for all, as host
    values.  ``which``: the image indices to resect, in the order of the result (default: all; an image may be listed twice).  ``thresh``:
    the inlier bound in pixels; ``iters``: P3P hypotheses per image; ``lo_iters``: Gauss-Newton rounds; ``min_inliers``: what a pose needs
    (at least 4); ``seed``: of the sampler.

    ValueError, before the device is touched: a count that disagrees with ``tracks.image_start``, intrinsics of another shape, with skew or a
    last row other than (0, 0, 1), an index of ``which`` out of range, tensors of a wrong dtype or on different devices, a parameter out of
    range.

    Host synchronisation: NONE.  ``Poses.stats`` and ``Poses.cameras`` read back."""
    kpts, rec, which, mask = _check(points, tracks, images, intrinsics, which, use, thresh, iters, lo_iters, min_inliers, seed)
    device = tracks.track_of.device
    with torch.cuda.device(device):
        allk = torch.cat([k.reshape(-1, 2).float() for k in kpts]).contiguous() if kpts else torch.zeros((0, 2), device=device)
        n, T = allk.shape[0], points.xyz.shape[0]
        views, keep = hip.resect_images(_nonempty(tracks.track_of.contiguous(), (1,), torch.int32), _nonempty(points.xyz.contiguous(), (1, 3), torch.float64),
                                              _nonempty(mask.contiguous().view(torch.uint8), (1,), torch.uint8), _nonempty(allk, (1, 2), torch.float32), rec, n=n, T=T,
                                              thresh=float(thresh), iters=int(iters), lo_iters=int(lo_iters), min_inliers=int(min_inliers), seed=int(seed))
    return Poses(views, which, keep)


def absolute_pose(points3d, points2d, K, thresh: float = 4.0, iters: int = 1024, lo_iters: int = 8, seed: int = 0):
    """The single-set form, in the shape of ``cv2.solvePnPRansac``: ``points3d`` [n, 3] and ``points2d`` [n, 2] are corresponding world
    points and pixels (tensors or arrays), ``K`` the 3 x 3 intrinsics.  Returns ``(R [3, 3], t [3], mask [n] bool)`` as device tensors with
    ``x_c = R X + t``, or ``None`` below three points or without a pose of at least four inliers.  It runs through the op of
    ``resect_images`` with every point a track of its own.

    This call SYNCHRONISES with the device (it reads whether a pose was found); ``resect_images`` does not."""
    name = "absolute_pose"
    _params(name, thresh, iters, lo_iters, 0, seed)
    Kh = _intrinsics(name, K, 1)
    X = points3d if isinstance(points3d, torch.Tensor) else torch.as_tensor(np.asarray(points3d))
    uv = points2d if isinstance(points2d, torch.Tensor) else torch.as_tensor(np.asarray(points2d))
    if X.dim() != 2 or X.shape[1] != 3 or tuple(uv.shape) != (X.shape[0], 2):
        raise ValueError(f"{name}: points3d must be [n, 3] and points2d [n, 2], got {tuple(X.shape)} and {tuple(uv.shape)}")
    n = X.shape[0]
    if n < 3:
        return None
    dev = X.device if X.is_cuda else torch.device("cuda", torch.cuda.current_device())
    X, uv = X.to(device=dev, dtype=torch.float64), uv.to(device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        rec = hip.resect_cameras(Kh, [n])
        views, keep = hip.resect_images(torch.arange(n, dtype=torch.int32, device=dev), X.contiguous(), torch.ones(n, dtype=torch.uint8, device=dev),
                                              uv.contiguous(), rec, thresh=float(thresh), iters=int(iters), lo_iters=int(lo_iters), min_inliers=0,
                                              seed=int(seed))
        if not bool(views["ok"][0].item()):      # the host synchronisation of absolute_pose
            return None
    return views["pose"][0, :9].view(3, 3), views["pose"][0, 9:], views["kp_inlier"].bool()
