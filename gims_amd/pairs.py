"""Which image pairs to match, decided on the device (kernels: gims_amd/csrc/pairs.hip, GIMS_AUX_SELECT_PAIRS).

``match_features`` is the dominant cost of an image set and grows with the number of pairs; ``select_pairs`` chooses the pairs from what
``encode_images`` already holds.  The ``per_image`` best-scored descriptors of every image are quantised to int8 with one scale and matched
coarsely against those of every other image; a row of image i *votes* for image j when its nearest row of j passes Lowe's ratio test against
the second nearest; S[i][j] = votes[i][j] + votes[j][i]; every image keeps its ``k`` partners with the largest S (at least ``min_votes``,
ties by index) and the result is the union, each pair once, ascending.  include/gims_hip.h has the specification in full and
tests/pairs_ref.py is its NumPy restatement; every decision is taken in integers, so the device and the restatement agree exactly."""
from __future__ import annotations

import math

import torch

from . import hip

ORDERS = ("score", "first")


class PairSelection:
    """The result of ``select_pairs``.  Immutable.  Device tensors: ``pairs`` int32 [cap, 2] and ``pair_votes`` int32 [cap] (the first
    n_pairs entries are the selection, ascending, and S of every pair), ``votes`` int32 [N, N], ``counters`` int32 [8]
    (``hip.PAIRS_COUNTERS``) and ``n_rows`` (int32 scalar: the rows that took part).  ``tolist()`` and ``stats`` read back; nothing else does."""
    __slots__ = ("pairs", "pair_votes", "votes", "counters", "n_rows", "n_images", "_host", "_keep")

    def __init__(self, pairs, pair_votes, votes, counters, n_images, keep=None):
        for name, v in (("pairs", pairs), ("pair_votes", pair_votes), ("votes", votes), ("counters", counters), ("n_rows", counters[1]),
                        ("n_images", int(n_images)), ("_host", {}), ("_keep", keep)):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError("PairSelection is immutable")

    __delattr__ = __setattr__

    def _read(self):
        if "pairs" not in self._host:
            c = [int(v) for v in self.counters.tolist()]
            self._host["stats"] = dict(zip(hip.PAIRS_COUNTERS, c))
            self._host["pairs"] = [(int(a), int(b)) for a, b in self.pairs[:c[0]].tolist()]
        return self._host

    def tolist(self) -> list:
        """[(i, j), ...] with i < j, ascending: what ``match_features`` takes.  Reads back once; cached."""
        return list(self._read()["pairs"])

    @property
    def stats(self) -> dict:
        """The op's counters: n_pairs, n_rows, n_short_images (fewer than two rows), n_bad_rows, n_nonfinite.  Reads back."""
        return dict(self._read()["stats"])

    def partners(self, i: int) -> list:
        """The images paired with image i, ascending (off the host list)."""
        if not 0 <= i < self.n_images:
            raise ValueError(f"PairSelection.partners: image {i} is out of range (0 .. {self.n_images - 1})")
        return sorted([b for a, b in self._read()["pairs"] if a == i] + [a for a, b in self._read()["pairs"] if b == i])

    def __len__(self):
        return len(self._read()["pairs"])

    def __repr__(self):
        return f"PairSelection(n_images={self.n_images}, cap={self.pairs.shape[0]})"


def _is_int(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, int)


def _checked(feats, k, per_image, ratio, min_votes, order, scale):
    """Everything select_pairs checks before the device is touched -> [(descriptors, scores or None)], D."""
    if order not in ORDERS:
        raise ValueError(f"select_pairs: order must be one of {ORDERS}, got {order!r}")
    if not _is_int(k) or k < 1:
        raise ValueError(f"select_pairs: k must be an integer >= 1, got {k!r}")
    if not _is_int(per_image) or not 1 <= per_image <= hip.PAIRS_MAX_ROWS:
        raise ValueError(f"select_pairs: per_image must be an integer in 1 .. {hip.PAIRS_MAX_ROWS}, got {per_image!r}")
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not 0.0 <= ratio <= 1.0:
        raise ValueError(f"select_pairs: ratio must lie in [0, 1], got {ratio!r}")
    if not _is_int(min_votes) or min_votes < 0:
        raise ValueError(f"select_pairs: min_votes must be an integer >= 0, got {min_votes!r}")
    if scale is not None and (isinstance(scale, bool) or not isinstance(scale, (int, float)) or not math.isfinite(scale) or scale < 0):
        raise ValueError(f"select_pairs: scale must be None or a finite number >= 0, got {scale!r}")
    feats = list(feats)
    if not 2 <= len(feats) <= hip.PAIRS_MAX_IMAGES:
        raise ValueError(f"select_pairs: {len(feats)} images: the op serves 2 .. {hip.PAIRS_MAX_IMAGES}")
    items, device, d = [], None, None
    for i, f in enumerate(feats):
        desc, sc = (f.descriptors, f.scores) if hasattr(f, "descriptors") else (f[0], f[1] if len(f) > 1 else None)
        if not isinstance(desc, torch.Tensor) or desc.dtype != torch.float32 or desc.dim() != 2:
            raise ValueError(f"select_pairs: image {i}: the descriptors must be a float32 [n, D] tensor")
        if sc is not None and (not isinstance(sc, torch.Tensor) or sc.dim() != 1 or sc.shape[0] != desc.shape[0]):
            raise ValueError(f"select_pairs: image {i}: the scores must be a [n] tensor, n = {desc.shape[0]}")
        device = desc.device if device is None else device
        for t in (desc, sc):
            if t is not None and t.device != device:
                raise ValueError(f"select_pairs: image {i}: a tensor is on {t.device}, the tensors before it on {device}")
        d = desc.shape[1] if d is None else d
        if desc.shape[1] != d:
            raise ValueError(f"select_pairs: image {i}: D = {desc.shape[1]}, the images before it have D = {d}")
        items.append((desc, sc))
    if d % 32 != 0 or not 32 <= d <= hip.PAIRS_MAX_D:
        raise ValueError(f"select_pairs: D = {d} is not served: the op takes a multiple of 32 in 32 .. {hip.PAIRS_MAX_D}")
    if device.type != "cuda":
        raise ValueError(f"select_pairs: the descriptors are on {device}: the pairs are selected on the GPU, from device tensors")
    if device.index is not None and device.index != torch.cuda.current_device():
        raise ValueError(f"select_pairs: the descriptors are on {device}, the current device is cuda:{torch.cuda.current_device()}")
    return items, d


def select_pairs(feats, k: int = 20, per_image: int = 512, ratio: float = 0.8, min_votes: int = 1, order: str = "score", scale=None) -> PairSelection:
    """Choose the image pairs worth matching, on the device.

    ``feats``: a list of ``ImageFeatures`` or of ``(descriptors [n, D] float32 device tensor, scores [n] or None)``.  ``order='score'``:
    the rows of an image are ``torch.sort(scores, descending=True, stable=True)[1][:per_image]``; ``'first'``, or no scores: its first
    rows.  ``scale=None``: 127 / the largest finite |value| among the selected rows; a number: that scale (values beyond +-127 / scale
    saturate).  ``match_features(feats, sel.tolist())`` consumes the result.

    ValueError, before the device is touched: fewer than two images (or more than 8192), tensors on different devices or not on the
    current one, differing D, a D that is no multiple of 32 in 32 .. 1024, k < 1, per_image outside 1 .. 4096, ratio outside [0, 1],
    min_votes < 0, a scale that is not finite and >= 0, an unknown order.

    Host synchronisation: none; ``tolist()`` and ``stats`` of the result read back."""
    items, d = _checked(feats, k, per_image, ratio, min_votes, order, scale)
    device = items[0][0].device
    images, keep = [], []
    for desc, sc in items:
        n = desc.shape[0]
        if desc.stride(1) != 1 and n > 0:
            desc = desc.contiguous()
        m, idx = min(n, per_image), None
        if order == "score" and sc is not None and n > 0:
            idx = torch.sort(sc, descending=True, stable=True)[1][:per_image].to(torch.int32)
        keep += [desc, idx]
        images.append((desc if n > 0 else None, max(desc.stride(0), d) if n > 0 else d, n, idx, m))
    votes, out, counters, alive = hip.select_pairs(images, d, device, k, per_image, hip.pairs_rq(ratio), min_votes,
                                                   None if scale is None else float(scale))
    o_pairs, o_votes, _, cap = hip.pairs_out_layout(len(images), k)
    return PairSelection(out[o_pairs:o_pairs + 2 * cap].view(cap, 2), out[o_votes:o_votes + cap], votes, counters, len(images), (keep, alive))
