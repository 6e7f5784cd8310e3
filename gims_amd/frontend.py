"""Device-side front end: patch extraction + CAR-HyNet descriptors on the GPU (SURVEY 8f, rows f4 + f1).

The reference's ``utils.common.sift_forward`` (utils/common.py:837-893) does, per image: OpenCV SIFT detection -> Gaussian
pyramid + one affine-warped 64x64 patch per keypoint (utils/library.py:84-110, 234-271, one CPU core: 3.2-3.9 s per image
at 15 k keypoints, README.md:151,155) -> CAR-HyNet on 32x32 patches -> 128-d descriptors duplicated to 256-d.  Here
everything after the detection runs on the MI355X: ``extract_patches`` (csrc/patches.hip) writes the patches straight in
the NHWC float layout the CAR-HyNet kernels read, so they never exist on the host.

``sift_forward_device`` has ``sift_forward``'s signature and can be handed to ``Matching`` as ``config['front_end']``.
Keypoint DETECTION stays what the caller provides: ``detector(img) -> keypoints`` (objects with cv2.KeyPoint's attributes
``pt, size, angle, response, octave``, or a structured array with those fields); by default OpenCV's SIFT with the
reference's parameters when ``cv2`` is importable.  The patch arithmetic restates OpenCV's uint8 fixed-point resampling;
it is PARITY UNPINNED against OpenCV itself (see csrc/patches.hip and DESIGN.md).

``sift_detect_device`` is the detector on the device (csrc/sift.hip, OpenCV 4.x SIFT detect restated): it returns
per image a dict of device tensors that ``keypoint_arrays``, ``filter_max_num``, ``pad_training_keypoints`` and
``extract_patches`` take without a host round trip.  ``device_front_end`` is ``sift_forward_device`` with that detector, batched
over ``data['image']``; ``Matching({'front_end': frontend.device_front_end})`` selects it (the default stays OpenCV's).

``sift_describe_device`` / ``sift_detect_and_compute_device`` add the 128-d SIFT descriptor of those keypoints over the detector's
pyramid (csrc/sift.hip), ``root_sift`` the reference's RootSIFT, and ``sift_baseline_front_end`` the front end of the
classical baseline (SIFT + NNDR / MNN, ``gims_amd.baselines``) that learned matchers are reported against.

``diou_nms_device`` / ``process_diou_nms`` are the reference's keypoint thinning ``process_diou_nms`` (utils/common.py:720-807; the line
it keeps commented out at 863) on the device (csrc/nms.hip).  Every front end applies it between detection and
``filter_max_num`` when ``data['diou_nms']`` is set: ``True`` for the reference's settings (radius 4, threshold 0.3) or a dict
``{'radius', 'iou_thresh'}``; absent, ``None`` or ``False`` leaves everything as it was.  ``with_diou_nms(front_end)`` sets the key.
"""
from __future__ import annotations

import numpy as np
import torch

from . import hip


def _is_device_dict(kps):
    return isinstance(kps, dict) and torch.is_tensor(kps.get("pt"))


def keypoint_arrays(kps):
    """cv2.KeyPoint-like objects (or a structured array / dict of arrays) -> (kp4 float32 [n, 4] = x, y, size, angle;
    octave int32 [n]; response float32 [n]).  A dict of tensors (what sift_detect_device returns) gives tensors on its device."""
    if _is_device_dict(kps):
        pt = kps["pt"].reshape(-1, 2).float()
        kp4 = torch.cat([pt, kps["size"].float()[:, None], kps["angle"].float()[:, None]], 1).contiguous()
        resp = kps.get("response")
        resp = resp.float() if resp is not None else torch.zeros(len(pt), dtype=torch.float32, device=pt.device)
        return kp4, kps["octave"].to(torch.int32).contiguous(), resp.contiguous()
    if isinstance(kps, dict):
        pt = np.asarray(kps["pt"], dtype=np.float32).reshape(-1, 2)
        kp4 = np.concatenate([pt, np.asarray(kps["size"], np.float32)[:, None], np.asarray(kps["angle"], np.float32)[:, None]], 1)
        return np.ascontiguousarray(kp4), np.asarray(kps["octave"], np.int32), np.asarray(kps.get("response", np.zeros(len(pt))), np.float32)
    n = len(kps)
    kp4 = np.empty((n, 4), dtype=np.float32)
    octv = np.empty(n, dtype=np.int32)
    resp = np.empty(n, dtype=np.float32)
    for i, k in enumerate(kps):
        kp4[i] = (k.pt[0], k.pt[1], k.size, k.angle)
        octv[i] = k.octave
        resp[i] = k.response
    return kp4, octv, resp


def extract_patches(img, kps, device=None):
    """buildGaussianPyramid + ComputePatches(radius_size=64) + INTER_AREA to 32x32 + / 255 (utils/common.py:882-884) on the
    device.  img: uint8 [H, W, 3] (NumPy or tensor); kps: see keypoint_arrays.  Returns float32 [n, 32, 32, 3] on the device.
    Keypoints whose octave / layer fall outside the pyramid raise IndexError, like the reference's list indexing would."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    t = torch.as_tensor(np.ascontiguousarray(img) if isinstance(img, np.ndarray) else img)
    if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
        raise ValueError("extract_patches takes a uint8 [H, W, 3] image (what sift_forward passes with graydesc=False)")
    t = t.to(dev).contiguous()
    kp4, octv, _ = keypoint_arrays(kps)
    pyr, levels, dev_levels = hip.pyramid_build(t)
    out, bad = hip.patch_extract(pyr, dev_levels, len(levels), _on(kp4, dev), _on(octv, dev))
    if len(kp4) and int(bad.item()):
        raise IndexError(f"{int(bad.item())} keypoint(s) reference a pyramid level that does not exist (octave / layer out of range)")
    return out


def _on(a, dev):
    return a.to(dev).contiguous() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def filter_max_num(kps, max_num):
    """filterMaxNumDesc (utils/common.py:710-718): the max_num keypoints with the largest response, in descending order.
    For a dict of device tensors (sift_detect_device) the order is descending response, equal responses in the detector's
    order (a stable sort; multi-orientation keypoints share a response).  The reference's np.argsort + fliplr leaves the
    order of equal responses to NumPy's unstable sort, so the two forms agree apart from ties."""
    if _is_device_dict(kps):
        n = len(kps["pt"])
        if 0 < max_num < n:
            idx = torch.sort(kps["response"], descending=True, stable=True)[1][:max_num]
            return {k: v[idx] for k, v in kps.items()}
        return kps
    if 0 < max_num < len(kps):
        responses = [k.response for k in kps]
        idxs = np.fliplr(np.reshape(np.argsort(responses), (1, -1))).reshape(-1)
        return [kps[idxs[n]] for n in range(max_num)]
    return kps


NMS_DEFAULT = (4, 0.3)        # the reference's gconfig: iou_borders, iou_thresh (utils/common.py:846-847)


def _nms_args(radius, iou_thresh):
    """The reference's argument rules -> (radius as the op takes it: 0.0 = boxes from the size, threshold), or None when radius == 0
    (the reference returns its input).  ValueError for a negative / non-finite radius or a threshold outside (0, 1)."""
    if radius is not None and radius == 0:
        return None
    thr = float(iou_thresh or 0.5)
    rad = 0.0 if radius is None else float(radius)
    if not np.isfinite(rad) or rad < 0:
        raise ValueError(f"diou_nms: radius = {radius!r} (a positive number, or None for boxes from the keypoint size)")
    if not 0.0 < thr < 1.0:
        raise ValueError(f"diou_nms: iou_thresh = {iou_thresh!r} is outside (0, 1)")
    return rad, thr


def _nms_settings(spec):
    """data['diou_nms'] -> None (off) or (radius, iou_thresh)."""
    if spec is None or spec is False:
        return None
    if spec is True:
        return NMS_DEFAULT
    if isinstance(spec, dict):
        return spec.get("radius", NMS_DEFAULT[0]), spec.get("iou_thresh", NMS_DEFAULT[1])
    raise TypeError("data['diou_nms'] is True or a dict {'radius', 'iou_thresh'}")


def _nms_rows(kp4s, resps, rad, thr, shape, dev):
    """One hip.diou_nms call for the keypoints of every image (kp4 [n_b, 4] and response [n_b] per image, on dev) -> per image the
    selected rows (int64, local) in the result's order.  The order handed to the op: descending response, equal responses with the
    higher row first; a non-finite response takes the keypoint out (the op counts the -1 left in its place as bad)."""
    counts = [int(k.shape[0]) for k in kp4s]
    n = sum(counts)
    if n == 0:
        return [torch.zeros(0, dtype=torch.int64, device=dev) for _ in counts]
    kp4 = torch.cat([k.float().reshape(-1, 4) for k in kp4s]).contiguous()
    resp = torch.cat([r.float().reshape(-1) for r in resps])
    bounds = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    order = torch.sort(resp, stable=True)[1].flip(0)                      # descending; NaN first, dropped below
    if len(counts) > 1:
        image = torch.repeat_interleave(torch.arange(len(counts), device=dev), torch.as_tensor(counts, device=dev), output_size=n)
        order = order[torch.sort(image[order], stable=True)[1]]
    order = torch.where(torch.isfinite(resp[order]), order, torch.full_like(order, -1)).to(torch.int32).contiguous()
    h, w = (1 << 30, 1 << 30) if shape is None else (max(int(shape[0]), 1), max(int(shape[1]), 1))
    keep, count = hip.diou_nms(kp4, order, hip.upload(bounds, dev), rad, thr, h, w)
    kept = count.cpu().numpy()                                            # the one host read of the call
    return [keep[bounds[b]:bounds[b] + int(kept[b])].long() - int(bounds[b]) for b in range(len(counts))]


def diou_nms_device(kps, radius=4, iou_thresh=0.3, shape=None, device=None):
    """The reference's ``process_diou_nms(keypoints, radius, iou_thresh)`` on the device (csrc/nms.hip) for one dict of
    device tensors (what ``sift_detect_device`` returns) or a list of them, which goes through the kernel as one batch.  Returns the
    dict(s) with every field indexed by the result: the surviving keypoints in descending response, as the reference returns them.
    ``radius=None``: boxes from the keypoint size; ``radius == 0`` returns the input unchanged and a falsy ``iou_thresh`` means 0.5
    (both rules are the reference's own); a threshold outside (0, 1) or a negative radius raises ValueError.  ``shape`` = (height,
    width) of the image(s) bounds the search grid; it changes the speed only.  Equal responses are processed higher row first (the
    reference leaves them to NumPy's sort); between identical boxes that cannot change the result.  One host synchronisation per call."""
    args = _nms_args(radius, iou_thresh)
    if args is None:
        return kps
    single = _is_device_dict(kps)
    lst = [kps] if single else list(kps)
    if not lst:
        return kps
    dev = torch.device(device) if device is not None else lst[0]["pt"].device
    parts = [keypoint_arrays(k) for k in lst]
    rows = _nms_rows([_on(p[0], dev) for p in parts], [_on(p[2], dev) for p in parts], args[0], args[1], shape, dev)
    out = [{name: v[r.to(v.device)] for name, v in k.items()} for k, r in zip(lst, rows)]
    return out[0] if single else out


def process_diou_nms(keypoints, radius=None, iou_thresh=0.3):
    """The reference's function with its signature, for a list (or array) of cv2.KeyPoint-like objects (``pt``, ``size``,
    ``response``): uploads them, runs the op on the current device and returns the selected objects as a list, in the reference's order.
    Differences: an empty input returns an empty list (the reference raises there), and equal responses of DIFFERENT boxes are
    processed higher row first, where the reference leaves the order to NumPy's sort."""
    args = _nms_args(radius, iou_thresh)
    if args is None:
        return keypoints
    if len(keypoints) == 0:
        return []
    dev = torch.device("cuda", torch.cuda.current_device())
    kp4 = np.array([[k.pt[0], k.pt[1], k.size, 0.0] for k in keypoints], dtype=np.float32)
    resp = np.array([k.response for k in keypoints], dtype=np.float32)
    rows = _nms_rows([_on(kp4, dev)], [_on(resp, dev)], args[0], args[1], None, dev)[0].cpu().tolist()
    return [keypoints[i] for i in rows]


def with_diou_nms(front_end, radius=4, iou_thresh=0.3):
    """A front end that runs ``front_end`` with ``data['diou_nms']`` set: ``Matching({'front_end': with_diou_nms(device_front_end)})``."""
    def thinned(data, device):
        return front_end({**data, "diou_nms": {"radius": radius, "iou_thresh": iou_thresh}}, device)
    return thinned


class PaddedKeyPoint:
    """What ``cv2.KeyPoint(x, y, 1)`` carries (utils/common.py:683): size 1, angle -1, response 0, octave 0, class_id -1."""
    __slots__ = ("pt", "size", "angle", "response", "octave", "class_id")

    def __init__(self, x, y):
        self.pt, self.size, self.angle, self.response, self.octave, self.class_id = (float(x), float(y)), 1.0, -1.0, 0.0, 0, -1


def pad_training_keypoints(kps, max_keypoints, img_shape):
    """The ``is_train`` branch of sift_forward (utils/common.py:866-880, ``copy=False``): an image with fewer than max_keypoints
    detections gets random extra locations -- x and y drawn with the reference's own sequence of ``np.random`` calls (a
    (n, 2) block scaled by the width, then the y column redrawn and scaled by the height), so a seeded run places them where
    the reference does -- as size-1 keypoints, so that every image of a training batch carries exactly max_keypoints
    (train.py:107-110 stacks them).  The reference passes the locations through ``cv2.SIFT.compute`` (682-685), which may
    drop points OpenCV considers too close to the border: NOT restated (OpenCV is not available here; parity unpinned).
    A dict of device tensors is padded on its device, with the same np.random sequence."""
    if _is_device_dict(kps):
        n = len(kps["pt"])
        if max_keypoints <= 0 or n >= max_keypoints:
            return kps
        to_add = max_keypoints - n
        coordinates = np.random.random((to_add, 2)) * img_shape[1]
        coordinates[:, 1] = np.random.random(to_add) * img_shape[0]
        dev = kps["pt"].device
        pad = {"pt": torch.from_numpy(coordinates.astype(np.float32)).to(dev), "size": torch.ones(to_add, device=dev),
               "angle": torch.full((to_add,), -1.0, device=dev), "response": torch.zeros(to_add, device=dev),
               "octave": torch.zeros(to_add, dtype=torch.int32, device=dev)}
        return {k: torch.cat([kps[k], pad[k].to(kps[k].dtype)]) for k in pad}
    kps = list(kps)
    if max_keypoints <= 0 or len(kps) >= max_keypoints:
        return kps
    to_add = max_keypoints - len(kps)
    coordinates = np.random.random((to_add, 2)) * img_shape[1]
    coordinates[:, 1] = np.random.random(to_add) * img_shape[0]
    return kps + [PaddedKeyPoint(x, y) for x, y in coordinates]


def _default_detector():
    try:
        import cv2
    except Exception as e:             # no OpenCV in this environment
        raise NotImplementedError("keypoint DETECTION needs OpenCV SIFT (cv2 is not importable here): pass detector=callable(img) -> "
                                  "keypoints (cv2.KeyPoint-like objects)") from e
    sift = cv2.SIFT_create(nfeatures=None, nOctaveLayers=3, contrastThreshold=0.001, edgeThreshold=80, sigma=1.6)   # common.py:838-857
    return lambda img: sift.detect(img, None)


def sift_detect_device(img_or_batch, device=None):
    """OpenCV SIFT detect (utils/common.py:838-857 parameters) on the device: uint8 [H, W, 3] (BGR) / [H, W] -> a dict of device
    tensors pt [n, 2], size, angle, response, octave; a batch [B, H, W(, 3)] (array, tensor or list of equal-size images) -> a
    list of such dicts.  Images of one size go through the kernels together."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if isinstance(img_or_batch, (list, tuple)):
        return [sift_detect_device(im, dev) for im in img_or_batch] if len({tuple(np.shape(im)) for im in img_or_batch}) > 1 else \
            sift_detect_device(torch.stack([torch.as_tensor(np.asarray(im) if not torch.is_tensor(im) else im) for im in img_or_batch]), dev)
    t = img_or_batch if torch.is_tensor(img_or_batch) else torch.from_numpy(np.ascontiguousarray(img_or_batch))
    single = t.dim() == 2 or (t.dim() == 3 and t.shape[2] == 3)       # [H, W, 3] is one BGR image, [B, H, W] a gray batch
    t = t.to(dev)
    out = hip.sift_detect(t.unsqueeze(0) if single else t)
    return out[0] if single else out


def _image_batch(img_or_batch, dev):
    """uint8 [H, W] / [H, W, 3] / [B, H, W(, 3)] (array, tensor or list of equal-size images) -> (tensor [B, ...] on dev, single)."""
    if isinstance(img_or_batch, (list, tuple)):
        img_or_batch = torch.stack([torch.as_tensor(np.asarray(im) if not torch.is_tensor(im) else im) for im in img_or_batch])
    t = img_or_batch if torch.is_tensor(img_or_batch) else torch.from_numpy(np.ascontiguousarray(img_or_batch))
    single = t.dim() == 2 or (t.dim() == 3 and t.shape[2] == 3)       # as sift_detect_device reads it
    return (t.unsqueeze(0) if single else t).to(dev), single


def _describe(pyr, h, w, kps, dev):
    """One hip.sift_describe call for the keypoints of every image of the pyramid buffer; raises IndexError on bad keypoints."""
    parts = [keypoint_arrays(k) for k in kps]
    counts = [len(p[0]) for p in parts]
    kp4 = torch.cat([_on(p[0], dev).float().reshape(-1, 4) for p in parts]).contiguous()
    octv = torch.cat([_on(p[1], dev).to(torch.int32).reshape(-1) for p in parts]).contiguous()
    image = torch.from_numpy(np.repeat(np.arange(len(kps), dtype=np.int32), counts)).to(dev) if len(kps) > 1 else None
    desc, bad = hip.sift_describe(pyr, h, w, len(kps), kp4, octv, image)
    if len(kp4) and int(bad.item()):
        raise IndexError(f"{int(bad.item())} keypoint(s) reference a pyramid level that does not exist (octave / layer out of range)")
    return list(torch.split(desc, counts))


def sift_describe_device(img_or_batch, keypoints, device=None):
    """128-d SIFT descriptors on the device (csrc/sift.hip, OpenCV 4.x calcSIFTDescriptor restated) for given keypoints:
    one dict of device tensors per image, as ``sift_detect_device`` returns, or anything ``keypoint_arrays`` accepts.  Returns float32
    [n, 128] (integer-valued, 0 .. 255) per image: a tensor for one image, a list for a batch.  The keypoints are described over the
    DETECTOR's pyramid of the image (what ``detectAndCompute`` does); ``cv2.SIFT.compute`` builds its pyramid from the octaves of the
    provided keypoints, which is not restated.  Keypoints whose octave / layer fall outside the pyramid raise IndexError with their
    count, like ``extract_patches``."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    t, single = _image_batch(img_or_batch, dev)
    kps = [keypoints] if single else list(keypoints)
    if len(kps) != t.shape[0]:
        raise ValueError(f"sift_describe_device: {t.shape[0]} image(s) but {len(kps)} keypoint set(s)")
    out = _describe(hip.sift_pyramid_buffer(t), int(t.shape[1]), int(t.shape[2]), kps, dev)
    return out[0] if single else out


def sift_detect_and_compute_device(img_or_batch, max_keypoints=-1, device=None, diou_nms=None):
    """``detectAndCompute``: ``sift_detect_device``, ``filter_max_num(max_keypoints)``, then ``sift_describe_device`` over the pyramid the
    detection built (it is built once).  Returns (keypoints, descriptors): a dict and a float32 [n, 128] tensor for one image, lists of
    them for a batch of equal-size images.  ``diou_nms`` (``True`` or ``{'radius', 'iou_thresh'}``, as ``data['diou_nms']``) thins the
    detections with ``diou_nms_device`` before ``filter_max_num``, the images as one batch."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    t, single = _image_batch(img_or_batch, dev)
    dets, pyr = hip.sift_detect(t, return_pyramid=True)
    nms = _nms_settings(diou_nms)
    if nms is not None:
        dets = diou_nms_device(dets, nms[0], nms[1], (int(t.shape[1]), int(t.shape[2])), dev)
    dets = [filter_max_num(d, max_keypoints) for d in dets]
    desc = _describe(pyr, int(t.shape[1]), int(t.shape[2]), dets, dev)
    return (dets[0], desc[0]) if single else (dets, desc)


def root_sift(desc, eps=1e-7, l2norm=False):
    """The reference's ``rootSIFT`` (utils/common.py:698-708) on tensors, [n, C]: L1-normalise with ``+ eps``, then the square root;
    ``l2norm=True`` then applies ``desc_l2norm`` (687-696): x / sqrt(sum x^2 + 1e-10).  Torch plumbing; the input is not modified."""
    d = desc / (desc.sum(dim=1, keepdim=True) + eps)
    d = torch.sqrt(d)
    if l2norm:
        d = d / d.pow(2).sum(dim=1, keepdim=True).add(1e-10).pow(0.5)
    return d


def sift_baseline_front_end(data, device):
    """The classical baseline's front end: SIFT keypoints and SIFT / RootSIFT descriptors, all on the device, no CAR-HyNet.
    data: {'image': uint8 [B, H, W, 3], 'max_keypoints': int (default -1), 'root': bool (default False), 'diou_nms': see
    ``sift_detect_and_compute_device`` (default off)}.  Returns {'keypoints',
    'scores', 'descriptors'}: lists with one tensor per image -- (n, 2), (n,), (128, n); ``baselines.nn_match_pairs`` reads the
    descriptors as ``descriptors0/1[None]``."""
    img = data["image"]
    dets, descs = sift_detect_and_compute_device(list(img) if not torch.is_tensor(img) and not isinstance(img, np.ndarray) else img,
                                                 data.get("max_keypoints", -1), device, **({"diou_nms": data["diou_nms"]} if "diou_nms" in data else {}))
    if isinstance(dets, dict):
        dets, descs = [dets], [descs]
    if data.get("root", False):
        descs = [root_sift(d) for d in descs]
    return {"keypoints": [d["pt"] for d in dets], "scores": [d["response"] for d in dets], "descriptors": [d.t().contiguous() for d in descs]}


def device_front_end(data, device):
    """``sift_forward_device`` with ``sift_detect_device`` as the detector, the detection batched over ``data['image']``.  Hand it to
    ``Matching`` as ``config['front_end']``.  With ``data['diou_nms']`` set the detections of all images are thinned in one
    ``diou_nms_device`` call before ``sift_forward_device`` sees them."""
    dets = sift_detect_device(list(data["image"]) if not torch.is_tensor(data["image"]) else data["image"], device)
    nms = _nms_settings(data.get("diou_nms"))
    if nms is not None:
        if isinstance(dets, dict):
            dets = [dets]
        sizes = {tuple(im.shape[:2]) for im in data["image"]}
        dets = diou_nms_device(dets, nms[0], nms[1], sizes.pop() if len(sizes) == 1 else None, device)
        data = {**data, "diou_nms": None}
    dets = iter(dets)
    return sift_forward_device(data, device, detector=lambda img: next(dets))


def sift_forward_device(data, device, detector=None):
    """``utils.common.sift_forward`` (common.py:837-893; ``data['is_train']``: pad_training_keypoints) with patches and descriptors on the device.
    data: {'image': uint8 [B, H, W, 3], 'max_keypoints': int, 'carhynet': gims_amd.carhynet.CARHyNet (or any object with
    ``_forward_nhwc`` / ``compute_des_batches``)}.  Returns {'keypoints', 'scores', 'descriptors'}: lists with one tensor per
    image -- (n, 2), (n,), (256, n) with the 128-d descriptor duplicated (common.py:890-892).  ``data['diou_nms']`` (``True`` or
    ``{'radius', 'iou_thresh'}``) thins every image's detections where the reference's commented-out line stands (common.py:863),
    before ``filter_max_num``: ``diou_nms_device`` for device detections, ``process_diou_nms`` for host keypoint lists."""
    det = detector or data.get("detector") or _default_detector()
    nms = _nms_settings(data.get("diou_nms"))
    net = data["carhynet"]
    kpts, descs, scores = [], [], []
    for img in data["image"]:
        img = np.asarray(img.cpu() if torch.is_tensor(img) else img)
        k = det(img)
        if nms is not None:
            k = diou_nms_device(k, nms[0], nms[1], img.shape[:2], device) if _is_device_dict(k) else process_diou_nms(list(k), nms[0], nms[1])
        k = filter_max_num(k if _is_device_dict(k) else list(k), data.get("max_keypoints", -1))
        if data.get("is_train", False):
            k = pad_training_keypoints(k, data.get("max_keypoints", -1), img.shape)
        kp4, _, resp = keypoint_arrays(k)
        patches = extract_patches(img, k, device)
        if hasattr(net, "_forward_nhwc"):                     # gims_amd.carhynet.CARHyNet: stays on the device
            with torch.no_grad():
                d = net._forward_nhwc(patches)[0]
        else:                                                 # the reference's HyNetnetFeature2D: NumPy in, NumPy out
            d = torch.from_numpy(np.asarray(net.compute_des_batches(patches.cpu().numpy(), True), dtype=np.float32)).to(device)
        kpts.append(_on(kp4[:, :2], device))
        descs.append(torch.cat([d, d], dim=1).permute(1, 0).to(device))
        scores.append(_on(resp, device))
    return {"keypoints": kpts, "scores": scores, "descriptors": descs}
