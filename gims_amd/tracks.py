"""Multi-view tracks from image-set matches, on the device (kernels: gims_amd/csrc/tracks.hip, GIMS_AUX_BUILD_TRACKS).

``match_features`` gives the matches of any list of index pairs over N images and ``verify_pairs`` filters each pair; what every consumer
of such a list -- pose graphs, structure from motion -- does next is merge the pairwise matches into tracks ("keypoint 17 of image 0 =
keypoint 230 of image 3 = keypoint 5 of image 7") and throw away the tracks that contradict themselves.  ``build_tracks`` does that without
reading a single ``matches0`` back.

The specification (include/gims_hip.h has it in full; tests/tracks_ref.py is its NumPy restatement).  Keypoint i of image k is node
``image_start[k] + i``.  Row i of pair (a, b) with j = matches0[i] is an edge iff 0 <= j < n_b, its score (when ``min_score`` is given) is
>= min_score and its inlier flag (when given) is non-zero.  Tracks are the connected components with at least ``min_length`` nodes; a
component that holds two keypoints of one image *conflicts* and is dropped whole (``conflicts='drop'``) or kept and flagged (``'keep'``).
Tracks are numbered by their smallest node and list their observations by image, then keypoint, so the result depends on the edge set
alone -- not on the order of the pairs, nor on the run."""
from __future__ import annotations

from typing import Sequence

import torch

from . import hip
from ._abi import GimsHipError

POLICIES = ("drop", "keep")


class Tracks:
    """The result of ``build_tracks``.  Device tensors: ``track_of`` int32 [N] (the track of every keypoint of every image, or -1),
    ``indptr`` int32 [n_tracks + 1], ``obs_image`` and ``obs_keypoint`` int32 [n_obs] (track t holds observations indptr[t] ..
    indptr[t + 1] - 1), ``conflict`` uint8 [n_tracks] (all zero under ``conflicts='drop'``).  Host values: ``n_tracks``, ``n_obs``,
    ``stats`` (the op's counters: n_tracks, n_obs, n_conflicting -- conflicting components whatever the policy --, n_edges -- accepted
    rows --, n_bad -- matches0 entries outside their image, ignored --, status) and ``image_start`` (the first node of every image, then N)."""

    def __init__(self, track_of, indptr, obs_image, obs_keypoint, conflict, stats, image_start):
        self.track_of, self.indptr, self.obs_image, self.obs_keypoint, self.conflict = track_of, indptr, obs_image, obs_keypoint, conflict
        self.stats, self.image_start = dict(stats), list(image_start)
        self.n_tracks, self.n_obs = int(stats["n_tracks"]), int(stats["n_obs"])

    def of_image(self, k: int) -> torch.Tensor:
        """The view of ``track_of`` for image k: int32 [n_k]."""
        if not 0 <= k < len(self.image_start) - 1:
            raise ValueError(f"Tracks.of_image: image {k} is out of range (0 .. {len(self.image_start) - 2})")
        return self.track_of[self.image_start[k]:self.image_start[k + 1]]

    def lengths(self) -> torch.Tensor:
        """Observations per track: int32 [n_tracks]."""
        return self.indptr[1:] - self.indptr[:-1]

    def points(self, images) -> torch.Tensor:
        """float32 [n_obs, 2]: the keypoint coordinates of the observations, gathered from the ``ImageFeatures`` (or [n_k, 2] tensors)."""
        if len(images) != len(self.image_start) - 1:
            raise ValueError("Tracks.points: one entry per image of the set is needed")
        kpts = [(im.keypoints if hasattr(im, "keypoints") else im).reshape(-1, 2).float() for im in images]
        allk = torch.cat(kpts) if kpts else torch.zeros((0, 2), device=self.track_of.device)
        start = torch.tensor(self.image_start[:-1], dtype=torch.int64, device=self.obs_image.device)
        return allk[start[self.obs_image.long()] + self.obs_keypoint.long()]

    def to_host(self) -> list:
        """One list of (image, keypoint) per track."""
        ptr, im, kp = self.indptr.tolist(), self.obs_image.tolist(), self.obs_keypoint.tolist()
        return [list(zip(im[ptr[t]:ptr[t + 1]], kp[ptr[t]:ptr[t + 1]])) for t in range(self.n_tracks)]

    def __len__(self):
        return self.n_tracks

    def __repr__(self):
        return f"Tracks(n_tracks={self.n_tracks}, n_obs={self.n_obs}, stats={self.stats})"


def _entries(images, pairs, outs, inlier, min_score, min_length, conflicts):
    """Everything build_tracks checks before the device is touched -> (counts, entries as hip.tracks_table takes them, device)."""
    if conflicts not in POLICIES:
        raise ValueError(f"build_tracks: conflicts must be one of {POLICIES}, got {conflicts!r}")
    if isinstance(min_length, bool) or int(min_length) != min_length or min_length < 2:
        raise ValueError(f"build_tracks: min_length must be an integer >= 2, got {min_length!r}")
    if min_score is not None and min_score != min_score:
        raise ValueError("build_tracks: min_score is NaN")
    counts = [int(im.n) if hasattr(im, "n") else int(im) for im in images]
    if not counts or any(c < 0 for c in counts):
        raise ValueError("build_tracks: images must be a non-empty list of ImageFeatures or of keypoint counts >= 0")
    if isinstance(inlier, dict):
        inlier = inlier["inlier"]
    pairs, outs = list(pairs), list(outs)
    if len(pairs) != len(outs) or (inlier is not None and len(inlier) != len(pairs)):
        raise ValueError(f"build_tracks: pairs ({len(pairs)}), outs ({len(outs)})" + (f" and inlier ({len(inlier)})" if inlier is not None else "")
                         + " must be lists of one length")
    entries, device = [], None
    for p, ((a, b), o) in enumerate(zip(pairs, outs)):
        a, b = int(a), int(b)
        if not (0 <= a < len(counts) and 0 <= b < len(counts)):
            raise ValueError(f"build_tracks: pair {p}: the image index of ({a}, {b}) is out of range (0 .. {len(counts) - 1})")
        m0 = o["matches0"]
        sc = None
        if min_score is not None:
            if "matching_scores0" not in o:
                raise ValueError(f"build_tracks: pair {p}: min_score is given and the result has no matching_scores0")
            sc = o["matching_scores0"]
        mask = None if inlier is None else inlier[p]
        row = []
        for name, t, dt in (("matches0", m0, torch.int64), ("matching_scores0", sc, torch.float32), ("inlier", mask, torch.uint8)):
            if t is None:
                row.append(None)
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != dt:
                raise ValueError(f"build_tracks: pair {p}: {name} must be a {dt} tensor, got {getattr(t, 'dtype', type(t).__name__)}")
            if not (t.dim() == 1 or (t.dim() == 2 and t.shape[0] == 1)) or t.shape[-1] != counts[a]:
                raise ValueError(f"build_tracks: pair {p}: {name} has shape {tuple(t.shape)}, image {a} has {counts[a]} keypoints ([1, n] or [n])")
            device = t.device if device is None else device
            if t.device != device:
                raise ValueError(f"build_tracks: pair {p}: {name} is on {t.device}, the tensors before it on {device}")
            row.append(t)
        entries.append((a, b, row))
    return counts, entries, device


def build_tracks(images, pairs: Sequence, outs: Sequence[dict], *, inlier=None, min_score=None, min_length: int = 2, conflicts: str = "drop") -> Tracks:
    """Merge the pairwise matches of an image set into multi-view tracks on the device.

    ``images``: the list of ``ImageFeatures`` (``.n`` is read) or of plain keypoint counts; a count of 0 is allowed.  ``pairs``: the index
    pairs given to ``match_features``; ``outs``: its ``PairResults``, or any list of per-pair dicts with ``matches0`` ([1, n] or [n], int64,
    on the device) and, when ``min_score`` is given, ``matching_scores0`` (float32) -- the results of ``match_pairs`` serve the same way
    when the caller supplies the image indices.  ``inlier``: None, a list of per-pair uint8 masks, or the dict ``verify_pairs`` returns
    (its ``'inlier'`` is used).  ``min_score=None``: scores are not read.  ``conflicts``: ``'drop'`` (a component with two keypoints of one
    image is excluded whole) or ``'keep'`` (it stays and ``conflict`` flags it).

    ValueError, before the device is touched: lists of unequal length, an image index out of range, a ``matches0`` (scores, mask) whose
    length is not the first image's count, tensors on different devices, a wrong dtype, ``min_length < 2``, an unknown policy.

    Host synchronisation: ONE, on the event behind the read-back of the op's six counters, which size the views handed back; none per
    pair -- no ``matches0`` is read on the host.  ``GimsHipError`` if the op reports a non-zero status."""
    counts, entries, device = _entries(images, pairs, outs, inlier, min_score, min_length, conflicts)
    if device is None:          # no pair: the device of the images, if they have one
        device = next((im.device for im in images if hasattr(im, "device")), torch.device("cuda"))
    if device.type != "cuda":
        raise ValueError(f"build_tracks: the matches are on {device}: the tracks are built on the GPU, from device tensors")
    flat = [(a, b, *(None if t is None else t.reshape(-1).contiguous() for t in row)) for a, b, row in entries]
    with torch.cuda.device(device):
        track_of, out, counters, _, keep = hip.build_tracks(flat, counts, device, min_length=int(min_length), keep_conflicting=conflicts == "keep",
                                                            min_score=None if min_score is None else float(min_score))
        pin = torch.empty(8, dtype=torch.int32, pin_memory=True)
        pin.copy_(counters, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        done.synchronize()      # the one host synchronisation: the counters size the views below
    del keep
    stats = dict(zip(hip.TRACKS_COUNTERS, (int(v) for v in pin[:len(hip.TRACKS_COUNTERS)].tolist())))
    if stats["status"] != 0:
        raise GimsHipError(f"build_tracks: the device reported status {stats['status']} (a bounded retry loop ran out, or a parent chain was not descending)")
    n = sum(counts)
    o_ptr, o_img, o_kp, o_conf, _ = hip.tracks_out_layout(n)
    T, n_obs = stats["n_tracks"], stats["n_obs"]
    start = [0]
    for c in counts:
        start.append(start[-1] + c)
    return Tracks(track_of, out[o_ptr:o_ptr + T + 1], out[o_img:o_img + n_obs], out[o_kp:o_kp + n_obs],
                  out[o_conf:].view(torch.uint8)[:T], stats, start)
