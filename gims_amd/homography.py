"""Training and evaluation inputs from decoded images, on the device.

The reference builds every training batch from a COCO image (utils/dataset.py:40-66, train.py:100-140): a random homography,
``cv2.warpPerspective``, ``cv2.resize(INTER_AREA)`` to 640x480, SIFT + CAR-HyNet on the 2B images, then ``torch_find_matches``
per pair into the ``match_indexes`` rows the loss reads.  Here the random draws stay NumPy (the same ``np.random`` call sequence,
so a seeded run draws the reference's matrices), and every pixel and label is computed by HIP kernels: ``warp_perspective`` /
``resize`` (csrc/warp.hip, OpenCV 4.x's scalar arithmetic restated) and ``training_labels`` (csrc/eval.hip).  The pixels never
reach the host.  The albumentations colour augmentation (``apply_color_aug``) is restated as this library's own specification
(``augment.ColorAug``, csrc/augment.hip: documented behaviour, its own random draws, parity with albumentations itself unpinned) and is
applied by ``training_pair(..., color_aug=ColorAug(...))``.  Not restated: image decoding (``cv2.imread``).
"""
from __future__ import annotations

import numpy as np
import torch

from . import frontend, hip

INTER_LINEAR, INTER_AREA = hip.INTER_LINEAR, hip.INTER_AREA
_FLT_EPSILON = float(np.finfo(np.float32).eps)


# ------------------------------------------------------------------------------------------------ homographies (NumPy, host)
def get_rotmat(angle, as_3d=False, scale=1.0, center_x=0.0, center_y=0.0):
    """utils/preprocess_utils.py:6-17: a scaled rotation, as a 2x2 matrix or as the 3x3 rotation about (center_x, center_y)."""
    c, s = np.cos(angle) * scale, np.sin(angle) * scale
    rot = np.array([[c, s], [-s, c]])
    if not as_3d:
        return rot
    m = np.eye(3)
    m[:2, :2] = rot
    m[0, 2] = (1 - c) * center_x - s * center_y
    m[1, 2] = s * center_x + (1 - c) * center_y
    return m


def perspective_transform(points, m):
    """cv2.perspectiveTransform of float32 points (any shape ending in 2) through a float64 3x3 matrix: the projection in double,
    rounded to float32; a point whose |w| <= FLT_EPSILON maps to (0, 0)."""
    p = np.asarray(points, dtype=np.float32)
    m = np.asarray(m, dtype=np.float64).reshape(9)
    out = np.zeros(p.shape, dtype=np.float32)
    flat, res = p.reshape(-1, 2), out.reshape(-1, 2)
    for i, (x, y) in enumerate(flat.astype(np.float64)):
        w = x * m[6] + y * m[7] + m[8]
        if abs(w) > _FLT_EPSILON:
            w = 1.0 / w
            res[i, 0] = (x * m[0] + y * m[1] + m[2]) * w
            res[i, 1] = (x * m[3] + y * m[4] + m[5]) * w
    return out


def get_translation_mat(image_height, image_width, trans, transformed_corners):
    """utils/preprocess_utils.py:19-34: a random translation that moves the warped patch corners back towards the image
    (four np.random.uniform draws, in the reference's order)."""
    lt = np.min(transformed_corners, axis=0)
    rb = np.min(np.array([image_width, image_height]) - transformed_corners, axis=0)
    tx = int(np.random.uniform(0, trans) * image_width)
    ty = int(np.random.uniform(0, trans) * image_height)
    neg_x = lt[0] < 0 if np.random.uniform() > 0.5 else rb[0] > 0      # left edge, else right edge
    neg_y = lt[1] < 0 if np.random.uniform() > 0.5 else rb[1] > 0      # top edge, else bottom edge
    m = np.eye(3)
    m[0, 2] = tx if neg_x else -tx
    m[1, 2] = ty if neg_y else -ty
    return m


def get_perspective_mat(patch_ratio, center_x, center_y, pers_x, pers_y, shear_ratio, shear_angle, rotation_angle, scale, trans):
    """utils/preprocess_utils.py:36-72: perspective, shear about the centre, scaled rotation about the centre, then a translation
    that keeps the warped patch in view.  The np.random draws (normal x2, uniform for the shear branch, shear ratio, shear angle,
    rotation, scale, then get_translation_mat's four) follow the reference one for one."""
    shear_angle, rotation_angle = np.deg2rad(shear_angle), np.deg2rad(rotation_angle)
    h, w = center_y * 2, center_x * 2
    pw, ph = int(patch_ratio * w), int(patch_ratio * h)
    corners = np.array([[0, 0], [0, ph], [pw, ph], [pw, 0]], dtype=np.float32)
    px = np.random.normal(0, pers_x / 2)
    py = np.random.normal(0, pers_y / 2)
    pers = np.array([[1, 0, 0], [0, 1, 0], [px, py, 1]])
    if np.random.uniform() > 0.5:
        sx, sy = 1, 1 / np.random.uniform(1, 1 + shear_ratio)
    else:
        sx, sy = np.random.uniform(1 - shear_ratio, 1), 1
    a = np.random.uniform(-shear_angle, shear_angle)
    shear = get_rotmat(-a, True, center_x=center_x, center_y=center_y) @ np.diag([sx, sy, 1]) @ get_rotmat(a, True, center_x=center_x,
                                                                                                           center_y=center_y)
    r = np.random.uniform(-rotation_angle, rotation_angle)
    s = np.random.uniform(1, 1 + 2 * scale)
    hm = get_rotmat(r, True, scale=s, center_x=center_x, center_y=center_y) @ (shear @ pers)
    moved = perspective_transform(corners.reshape(-1, 1, 2), hm).reshape(-1, 2)
    return get_translation_mat(h, w, trans, moved) @ hm


def scale_homography(homo_matrix, src_height, src_width, dest_height, dest_width):
    """utils/preprocess_utils.py:134-143: the homography between the two images after both are resized the same way."""
    s = np.diag([dest_width / src_width, dest_height / src_height, 1.0])
    return s @ homo_matrix @ np.linalg.inv(s)


def process_resize(w, h, resize):
    """utils/common.py:318-334: the (w, h) an image is resized to for a --resize argument of one or two numbers (-1: unchanged)."""
    assert 0 < len(resize) <= 2
    if len(resize) == 1 and resize[0] > -1:
        f = resize[0] / max(h, w)
        return int(round(w * f)), int(round(h * f))
    if len(resize) == 1:
        return w, h
    return resize[0], resize[1]


# ------------------------------------------------------------------------------------------------ pixels (device)
def _device(device):
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def _as_batch(img, device):
    """(tensor uint8 [B, H, W(, 3)] on the device, was a single image).  [H, W, 3] is one colour image, [H, W] one grey image."""
    t = img if torch.is_tensor(img) else torch.from_numpy(np.ascontiguousarray(img))
    if t.dtype != torch.uint8:
        raise ValueError("image warps take uint8 images")
    single = t.dim() == 2 or (t.dim() == 3 and t.shape[2] == 3)
    t = t.to(_device(device) if not t.is_cuda else t.device)
    return (t.unsqueeze(0) if single else t).contiguous(), single


def _one(img, device):
    """One image as a device uint8 tensor of its own rank ([H, W, 3] or [H, W])."""
    t, single = _as_batch(img, device)
    assert single, "this takes one image"
    return t[0]


def warp_perspective(img, H, dsize, device=None):
    """cv2.warpPerspective(img, H, dsize) with the reference's defaults (INTER_LINEAR, BORDER_CONSTANT 0).  img: one uint8 image
    [H, W(, 3)] or a batch [B, H, W(, 3)], NumPy or tensor; H: 3x3 or [B, 3, 3] (host, any float type; inverted in double like
    cv::invert); dsize (w, h).  Returns device uint8 of the same rank."""
    t, single = _as_batch(img, device)
    m = np.asarray(H.detach().cpu() if torch.is_tensor(H) else H, dtype=np.float64).reshape(-1, 3, 3)
    if len(m) == 1 and t.shape[0] > 1:
        m = np.repeat(m, t.shape[0], 0)
    out = hip.warp_perspective(t, m, dsize)
    return out[0] if single else out


def resize(img, dsize, interpolation=INTER_LINEAR, device=None):
    """cv2.resize(img, dsize, interpolation=...) for INTER_LINEAR (cv2's default) and INTER_AREA.  Same inputs as warp_perspective."""
    t, single = _as_batch(img, device)
    out = hip.resize(t, dsize, interpolation)
    return out[0] if single else out


def resize_aspect_ratio(image, resize_h, resize_w, device=None):
    """utils/preprocess_utils.py:156-175: resize (INTER_LINEAR) to fit resize_h x resize_w with the aspect ratio kept, centred on a
    template filled with np.random.randint(0, 127)."""
    t = _one(image, device)
    h, w = t.shape[:2]
    m = max(h, w)
    nh, nw = int(resize_h * (h / m)), int(resize_w * (w / m))
    small = resize(t, (nw, nh), INTER_LINEAR)
    out = torch.full((resize_h, resize_w) + tuple(t.shape[2:]), np.random.randint(0, 127), dtype=torch.uint8, device=t.device)
    y0, x0 = (resize_h - nh) // 2, (resize_w - nw) // 2
    out[y0:y0 + nh, x0:x0 + nw] = small
    return out


def _aug_homography(shape, aug):
    h, w = shape[:2]
    return get_perspective_mat(aug['patch_ratio'], w // 2, h // 2, aug['perspective_x'], aug['perspective_y'], aug['shear_ratio'],
                               aug['shear_angle'], aug['rotation_angle'], aug['scale'], aug['translation'])


def training_pair(img, dataset_params, device=None, color_aug=None):
    """COCO_loader.__getitem__ (utils/dataset.py:40-66) from a decoded image: (original, warped) uint8 images of image_height x
    image_width on the device and the scaled homography (float32 NumPy 3x3).  color_aug: an ``augment.ColorAug``; after the resize it
    draws a plan for the original, then one for the warped image (the reference's order, utils/dataset.py:37), and augments both in one
    launch; the homography is untouched.  None (the default) augments nothing and draws nothing, whatever ``apply_color_aug`` in
    dataset_params says."""
    cfg = dataset_params
    th, tw = cfg['image_height'], cfg['image_width']
    image = _one(img, device)
    resize_both = True
    if cfg.get('resize_aspect', False):
        image = resize_aspect_ratio(image, th, tw)
        resize_both = False
    h, w = image.shape[:2]
    hm = _aug_homography((h, w), cfg['augmentation_params'])
    warped = warp_perspective(image, hm, (w, h))
    if resize_both:
        pair = resize(torch.stack([image, warped]), (tw, th), INTER_AREA)
        image, warped = pair[0], pair[1]
    if color_aug is not None:
        pair = color_aug.apply(pair if resize_both else torch.stack([image, warped]), [color_aug.draw(), color_aug.draw()])
        image, warped = pair[0], pair[1]
    return image, warped, scale_homography(hm, h, w, th, tw).astype(np.float32)


def validation_pair(img, H, dataset_params, device=None):
    """COCO_valloader.__getitem__ (utils/dataset.py:79-96): the image warped by the listed homography (cast to float32 first, as the
    reference does), both resized with INTER_AREA, and the scaled homography (float32)."""
    cfg = dataset_params
    th, tw = cfg['image_height'], cfg['image_width']
    image = _one(img, device)
    hm = np.asarray(H, dtype=np.float64).reshape(3, 3).astype(np.float32)
    h, w = image.shape[:2]
    warped = warp_perspective(image, hm, (w, h))
    pair = resize(torch.stack([image, warped]), (tw, th), INTER_AREA)
    return pair[0], pair[1], scale_homography(hm, h, w, th, tw).astype(np.float32)


def homography_pair(img, H, resize_arg=(640, 480)):
    """read_image_with_homography(..., color=True) (utils/common.py:364-390, rotation 0) from a decoded BGR image: (image0, image1,
    inp0, inp1, scales, scaled_homo) with the images device uint8 [h, w, 3] resized with cv2's default INTER_LINEAR and inp0 / inp1
    their [1, h, w, 3] batches -- what Matching (``image0`` / ``image1``) and evalh.evaluate_pairs (``h_gts``) take."""
    t, single = _as_batch(img, None)
    assert single and t.shape[3] == 3, "homography_pair takes one colour image"
    h, w = t.shape[1:3]
    warped = hip.warp_perspective(t, np.asarray(H, dtype=np.float64).reshape(1, 3, 3), (w, h))
    wn, hn = process_resize(w, h, list(resize_arg))
    pair = resize(torch.cat([t, warped]), (wn, hn), INTER_LINEAR)
    scales = (float(w) / float(wn), float(h) / float(hn))
    return pair[0], pair[1], pair[0:1], pair[1:2], scales, scale_homography(np.asarray(H), h, w, hn, wn).astype(np.float32)


def collate(pairs, device=None):
    """collate_batch (utils/dataset.py:98-104): the originals then the warped images as device uint8 [2B, H, W, 3], and the
    homographies as device float32 [B, 3, 3]."""
    dev = pairs[0][0].device if torch.is_tensor(pairs[0][0]) else _device(device)
    imgs = [p[0] for p in pairs] + [p[1] for p in pairs]
    batch = torch.stack([i if torch.is_tensor(i) else torch.from_numpy(np.ascontiguousarray(i)) for i in imgs]).to(dev)
    hs = torch.from_numpy(np.stack([np.asarray(p[2], dtype=np.float32) for p in pairs])).to(dev)
    return batch, hs


# ------------------------------------------------------------------------------------------------ labels and model inputs
def training_labels(kp0, kp1, Hs, dist_thresh=3, n_iters=1):
    """torch_find_matches(kp0[k], kp1[k], Hs[k], dist_thresh, n_iters) for every pair k, and the match_indexes rows of
    train.py:118-125: int64 [R, 3] on the device, [k, i0, i1] matches (i1 ascending, iteration after iteration), then [k, miss0, -1],
    then [k, -1, miss1], pair after pair.  kp0 / kp1: [B, n, 2] tensors or sequences of [n, 2] on the device; Hs: [B, 3, 3]."""
    hs = Hs if torch.is_tensor(Hs) else torch.from_numpy(np.asarray(Hs, dtype=np.float32))
    dev = kp0[0].device
    return hip.train_labels(list(kp0), list(kp1), hs.to(dev, torch.float32), float(dist_thresh), int(n_iters))


def training_inputs(batch, Hs, carhynet, max_keypoints=2048, device=None):
    """train.py:110-135 from a collated batch: SIFT over the 2B images in one batched detection (hip.sift_detect), then per image
    filter_max_num, pad_training_keypoints (the reference's np.random sequence, image after image), extract_patches, and CAR-HyNet
    over all patches at once; then training_labels.  Returns the ``gmodel_input`` dict ``model(data, mode='train')`` consumes, with
    ``matches`` and ``gt_vec``.  The images stay on the device."""
    dev = batch.device if device is None else torch.device(device)
    assert torch.is_tensor(batch) and batch.is_cuda and batch.dtype == torch.uint8 and batch.dim() == 4
    n = batch.shape[0]
    B = n // 2
    dets = hip.sift_detect(batch)
    kpts, scores, patches = [], [], []
    for i in range(n):
        k = frontend.filter_max_num(dets[i], max_keypoints)
        k = frontend.pad_training_keypoints(k, max_keypoints, tuple(batch.shape[1:]))
        kp4, _, resp = frontend.keypoint_arrays(k)
        patches.append(frontend.extract_patches(batch[i], k, dev))
        kpts.append(kp4[:, :2].contiguous())
        scores.append(resp)
    counts = [len(p) for p in patches]
    with torch.no_grad():
        desc = carhynet._forward_nhwc(torch.cat(patches))[0]
    descs = [torch.cat([d, d], dim=1).permute(1, 0) for d in torch.split(desc, counts)]
    keypoints, descriptors, scores = torch.stack(kpts), torch.stack(descs), torch.stack(scores)
    hs = Hs.to(dev, torch.float32)
    matches = training_labels(keypoints[:B], keypoints[B:], hs)
    return {'keypoints0': keypoints[:B], 'keypoints1': keypoints[B:], 'descriptors0': descriptors[:B], 'descriptors1': descriptors[B:],
            'image0': batch[:B], 'image1': batch[B:], 'scores0': scores[:B], 'scores1': scores[B:], 'matches': matches,
            'gt_vec': torch.ones(len(matches), dtype=torch.float32, device=dev), 'device': dev}
