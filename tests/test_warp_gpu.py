"""Device warps, resizes and training labels (csrc/warp.hip, csrc/eval.hip): known answers, bit equality with the
NumPy restatement tests/warp_ref.py, batching, a src/dst convention guard through SIFT, the label rows against the reference's
goldens, and one training step from images end to end."""
import os

import numpy as np
import pytest
import torch

from gims_amd import GMatcher, frontend, hip, synth
from gims_amd import homography as HG
from tests import warp_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
GOLD = os.path.join(os.path.dirname(__file__), "golden")
AUG = dict(patch_ratio=0.85, perspective_x=0.0, perspective_y=0.0, shear_ratio=0.04, shear_angle=10, rotation_angle=25, scale=0.6,
           translation=0.6)
STRONG = dict(AUG, perspective_x=0.0008, perspective_y=0.0008)
PARAMS = dict(image_height=480, image_width=640, resize_aspect=False, augmentation_params=AUG)


def _img(h, w, c=3, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)


def _warp(a, m, dsize):
    return HG.warp_perspective(a, m, dsize).cpu().numpy()


def _resize(a, dsize, ip):
    return HG.resize(a, dsize, ip).cpu().numpy()


def test_warp_known_answers():
    a = _img(48, 40)
    assert np.array_equal(_warp(a, np.eye(3), (40, 48)), a)
    o = _warp(a, np.array([[1, 0, 5], [0, 1, -3], [0, 0, 1.]]), (40, 48))
    assert np.array_equal(o[:-3, 5:], a[3:, :-5]) and (o[-3:] == 0).all() and (o[:, :5] == 0).all()
    assert np.array_equal(_warp(a, np.diag([0.5, 0.5, 1.0]), (20, 24)), a[::2, ::2])
    sq = _img(33, 33, seed=1)
    assert np.array_equal(_warp(sq, np.array([[0, 1, 0], [-1, 0, 32], [0, 0, 1.]]), (33, 33)), np.rot90(sq))
    assert (_warp(a, np.array([[1, 0, 5000], [0, 1, 0], [0, 0, 1.]]), (40, 48)) == 0).all()
    g = _img(48, 40, 1)[:, :, 0]
    assert np.array_equal(_warp(g, np.eye(3), (40, 48)), g)


def test_resize_known_answers():
    a = _img(48, 40)
    assert np.array_equal(_resize(a, (40, 48), HG.INTER_AREA), a)
    q = a.astype(np.int64)
    mean = ((q[::2, ::2] + q[1::2, ::2] + q[::2, 1::2] + q[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    assert np.array_equal(_resize(a, (20, 24), HG.INTER_AREA), mean)
    assert np.array_equal(_resize(a, (20, 24), HG.INTER_LINEAR), mean)
    k = np.full((37, 53, 3), 77, np.uint8)
    for d in [(20, 10), (100, 80), (26, 18), (60, 30), (53, 60), (17, 12)]:
        for ip in (HG.INTER_LINEAR, HG.INTER_AREA):
            assert (_resize(k, d, ip) == 77).all(), (d, ip)


def _homographies(w, h, n, seed):
    np.random.seed(seed)
    ms = []
    for i in range(n):
        aug = STRONG if i % 3 == 2 else AUG
        ms.append(HG.get_perspective_mat(aug['patch_ratio'], w // 2, h // 2, aug['perspective_x'], aug['perspective_y'], aug['shear_ratio'],
                                         aug['shear_angle'], aug['rotation_angle'], aug['scale'], aug['translation']))
    ms.append(np.array([[0.8, 0.1, 20.0], [-0.05, 1.1, 5.0], [1.5e-3, -8e-4, 1.0]]))       # strong perspective
    ms.append(np.array([[1.3, -0.4, -60.0], [0.3, 0.7, 40.0], [-1e-3, 2e-3, 1.0]]))
    return ms


@pytest.mark.parametrize("w,h", [(640, 480), (640, 427), (427, 640), (481, 639), (53, 37)])
@pytest.mark.parametrize("gray", [False, True])
def test_warp_equals_reference_bit_for_bit(w, h, gray):
    img = synth.make_textured_image(h, w, 11 + w, gray=gray)
    ms = _homographies(w, h, 21 if (w, h) == (640, 480) else 6, w * 7 + h)
    got = HG.warp_perspective(np.stack([img] * len(ms)), np.stack(ms), (w, h)).cpu().numpy()
    for i, m in enumerate(ms):
        assert np.array_equal(got[i], R.warp_perspective(img, m, (w, h))), (w, h, i)


@pytest.mark.parametrize("src,dst", [((640, 427), (640, 480)), ((427, 640), (640, 480)), ((1280, 960), (640, 480)), ((1000, 750), (640, 480)),
                                     ((481, 639), (640, 480)), ((53, 37), (640, 480)), ((640, 480), (53, 37)), ((900, 300), (640, 480)),
                                     ((1920, 1440), (640, 480)), ((640, 480), (1280, 960)), ((640, 480), (320, 240))])
@pytest.mark.parametrize("gray", [False, True])
def test_resize_equals_reference_bit_for_bit(src, dst, gray):
    img = synth.make_textured_image(src[1], src[0], 3 + src[0], gray=gray)
    for ip in (HG.INTER_AREA, HG.INTER_LINEAR):
        assert np.array_equal(_resize(img, dst, ip), R.resize(img, dst, ip)), (src, dst, ip)


def test_batch_equals_one_at_a_time():
    imgs = np.stack([synth.make_textured_image(480, 640, s) for s in range(4)])
    ms = _homographies(640, 480, 2, 99)
    batch = HG.warp_perspective(imgs, np.stack(ms), (640, 480))
    for i in range(4):
        assert torch.equal(batch[i], HG.warp_perspective(imgs[i], ms[i], (640, 480)))
    r = HG.resize(batch, (320, 213), HG.INTER_AREA)
    for i in range(4):
        assert torch.equal(r[i], HG.resize(batch[i], (320, 213), HG.INTER_AREA))


def test_convention_guard_true_h_beats_inverse():
    img = synth.make_textured_image(480, 640, 77)
    m = np.array([[0.95, -0.15, 40.0], [0.12, 0.9, 10.0], [1e-4, -5e-5, 1.0]])
    warped = HG.warp_perspective(img, m, (640, 480))
    d0, d1 = hip.sift_detect(torch.stack([torch.from_numpy(img).to(DEV), warped]))
    k0, k1 = d0["pt"].contiguous(), d1["pt"].contiguous()
    true = HG.training_labels([k0], [k1], torch.from_numpy(m.astype(np.float32))[None].to(DEV))
    inv = HG.training_labels([k0], [k1], torch.from_numpy(np.linalg.inv(m).astype(np.float32))[None].to(DEV))
    nt, ni = int((true[:, 1:] >= 0).all(1).sum()), int((inv[:, 1:] >= 0).all(1).sum())
    assert nt >= 5 * max(ni, 1), (nt, ni)


def test_labels_equal_golden_and_host_in_one_call():
    g = np.load(os.path.join(GOLD, "warp_labels.npz"))
    for iters in (1, 3):
        cases = [c for c in range(int(g["n_cases"])) if int(g[f"iters_{c}"]) == iters]
        while len(cases) < 3:
            cases = cases + cases
        cases = cases[:3]
        k0 = [torch.from_numpy(g[f"k0_{c}"]).to(DEV) for c in cases]
        k1 = [torch.from_numpy(g[f"k1_{c}"]).to(DEV) for c in cases]
        hs = torch.from_numpy(np.stack([g[f"H_{c}"] for c in cases])).to(DEV)
        got = HG.training_labels(k0, k1, hs, 3, iters).cpu().numpy()
        want = []
        for k, c in enumerate(cases):
            r = g[f"rows_{c}"].copy()
            r[:, 0] = k
            want.append(r)
        assert np.array_equal(got, np.concatenate(want)), iters
        host = R.label_rows([g[f"k0_{c}"] for c in cases], [g[f"k1_{c}"] for c in cases], [g[f"H_{c}"] for c in cases], 3, iters)
        assert np.array_equal(got, host)


def _net():
    from gims_amd.carhynet import CARHyNet
    net = CARHyNet().eval()
    net.load_state_dict(synth.make_carhynet_state_dict(321))
    return net


def _inputs(seed, net):
    np.random.seed(seed)
    pairs = [HG.training_pair(synth.make_textured_image(427, 640, 500 + k), PARAMS) for k in range(2)]
    batch, hs = HG.collate(pairs)
    return batch, hs, HG.training_inputs(batch, hs, net, max_keypoints=2048)


def test_training_inputs_end_to_end():
    net = _net()
    batch, hs, data = _inputs(31, net)
    assert batch.shape == (4, 480, 640, 3) and batch.is_cuda and hs.shape == (2, 3, 3)
    assert data['keypoints0'].shape == (2, 2048, 2) and data['descriptors0'].shape == (2, 256, 2048)
    # the same np.random state, the public pieces one image at a time
    np.random.seed(31)
    for k in range(2):
        HG.training_pair(synth.make_textured_image(427, 640, 500 + k), PARAMS)
    kp, sc, ds = [], [], []
    for i in range(4):
        k = frontend.sift_detect_device(batch[i], DEV)
        k = frontend.filter_max_num(k, 2048)
        k = frontend.pad_training_keypoints(k, 2048, tuple(batch.shape[1:]))
        kp4, _, resp = frontend.keypoint_arrays(k)
        with torch.no_grad():
            d = net._forward_nhwc(frontend.extract_patches(batch[i], k, DEV))[0]
        kp.append(kp4[:, :2]), sc.append(resp), ds.append(torch.cat([d, d], 1).permute(1, 0))
    kps = torch.stack(kp)
    assert torch.equal(torch.cat([data['keypoints0'], data['keypoints1']]), kps)
    assert torch.equal(torch.cat([data['scores0'], data['scores1']]), torch.stack(sc))
    assert torch.equal(torch.cat([data['descriptors0'], data['descriptors1']]), torch.stack(ds))
    want = R.label_rows(kps[:2].cpu().numpy(), kps[2:].cpu().numpy(), hs.cpu().numpy(), 3, 1)
    assert np.array_equal(data['matches'].cpu().numpy(), want)
    assert int((data['matches'][:, 1:] >= 0).all(1).sum()) > 50
    # one training step on the first pair (the reference trains with batch_size 1, configs/coco_config.yaml; two images of a batch
    # keep different numbers of keypoints after the graph build, which its torch.stack refuses)
    one = {k: v[:1] for k, v in data.items() if k.startswith(('keypoints', 'descriptors', 'scores', 'image'))}
    rows = data['matches'][data['matches'][:, 0] == 0]
    one.update(matches=rows, gt_vec=torch.ones(len(rows), device=DEV), device=DEV, radius=15, percentile=2, min_size=7)
    m = GMatcher({"sinkhorn_iterations": 20, "pos_loss_weight": 0.45, "neg_loss_weight": 1.0})
    m.load_state_dict(synth.make_state_dict(123))
    m = m.cuda().train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)
    with torch.enable_grad():
        loss, pos, neg = m(one, mode='train')
        loss.backward()
    assert torch.isfinite(loss).item()
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all().item() for g in grads)
    opt.step()
    # a second seeded run gives identical inputs
    _, _, again = _inputs(31, net)
    for key in ('keypoints0', 'keypoints1', 'descriptors0', 'descriptors1', 'scores0', 'scores1', 'matches', 'image0', 'image1'):
        assert torch.equal(data[key], again[key]), key
