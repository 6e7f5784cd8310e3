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


def sift_detect_and_compute_device(img_or_batch, max_keypoints=-1, device=None):
    """``detectAndCompute``: ``sift_detect_device``, ``filter_max_num(max_keypoints)``, then ``sift_describe_device`` over the pyramid the
    detection built (it is built once).  Returns (keypoints, descriptors): a dict and a float32 [n, 128] tensor for one image, lists of
    them for a batch of equal-size images."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    t, single = _image_batch(img_or_batch, dev)
    dets, pyr = hip.sift_detect(t, return_pyramid=True)
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
    data: {'image': uint8 [B, H, W, 3], 'max_keypoints': int (default -1), 'root': bool (default False)}.  Returns {'keypoints',
    'scores', 'descriptors'}: lists with one tensor per image -- (n, 2), (n,), (128, n); ``baselines.nn_match_pairs`` reads the
    descriptors as ``descriptors0/1[None]``."""
    img = data["image"]
    dets, descs = sift_detect_and_compute_device(list(img) if not torch.is_tensor(img) and not isinstance(img, np.ndarray) else img,
                                                 data.get("max_keypoints", -1), device)
    if isinstance(dets, dict):
        dets, descs = [dets], [descs]
    if data.get("root", False):
        descs = [root_sift(d) for d in descs]
    return {"keypoints": [d["pt"] for d in dets], "scores": [d["response"] for d in dets], "descriptors": [d.t().contiguous() for d in descs]}


def device_front_end(data, device):
    """``sift_forward_device`` with ``sift_detect_device`` as the detector, the detection batched over ``data['image']``.  Hand it to
    ``Matching`` as ``config['front_end']``."""
    dets = iter(sift_detect_device(list(data["image"]) if not torch.is_tensor(data["image"]) else data["image"], device))
    return sift_forward_device(data, device, detector=lambda img: next(dets))


def sift_forward_device(data, device, detector=None):
    """``utils.common.sift_forward`` (common.py:837-893; ``data['is_train']``: pad_training_keypoints) with patches and descriptors on the device.
    data: {'image': uint8 [B, H, W, 3], 'max_keypoints': int, 'carhynet': gims_amd.carhynet.CARHyNet (or any object with
    ``_forward_nhwc`` / ``compute_des_batches``)}.  Returns {'keypoints', 'scores', 'descriptors'}: lists with one tensor per
    image -- (n, 2), (n,), (256, n) with the 128-d descriptor duplicated (common.py:890-892)."""
    det = detector or data.get("detector") or _default_detector()
    net = data["carhynet"]
    kpts, descs, scores = [], [], []
    for img in data["image"]:
        img = np.asarray(img.cpu() if torch.is_tensor(img) else img)
        k = det(img)
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
