"""GPU parity of the CAR-HyNet descriptor path: HIP kernels vs the CPU oracle and vs the reference's goldens.
Tolerance: the 3x3 / 8x8 convolutions run as split-bf16x3 GEMMs (2^-17 relative per product, seven of them in sequence with an
FRN normalisation after each), everything else in f32.  Descriptors are unit vectors (components up to ~0.4): the bar is
3e-5 absolute; measured worst case 2.3e-5 over 256 patches (tools/carhynet_bench.py), ~1e-5 typical."""
import glob
import os

import numpy as np
import pytest
import torch

from gims_amd import synth
from oracle import carhynet_oracle as CO

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
GOLD = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "carhynet_*.npz")))


def _model(seed_w):
    from gims_amd.carhynet import CARHyNet
    m = CARHyNet().eval()
    m.load_state_dict(synth.make_carhynet_state_dict(seed_w))
    return m


@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(g)[:-4] for g in GOLD])
def test_descriptors_vs_reference_golden(path):
    g = np.load(path)
    m = _model(int(g["seed_w"]))
    patches = synth.make_patches(int(g["n"]), int(g["seed_p"]))
    desc = m.compute_des_batches(patches, color=True)
    np.testing.assert_allclose(desc, g["desc"], atol=3e-5, rtol=0)
    x = torch.from_numpy(patches).permute(0, 3, 1, 2).cuda()              # the reference's NCHW forward()
    d2, raw = m(x, mode="train")
    np.testing.assert_allclose(d2.cpu().numpy(), g["desc"], atol=3e-5, rtol=0)
    np.testing.assert_allclose(raw.cpu().numpy(), g["raw"], atol=2e-4, rtol=1e-4)


def test_vs_oracle_ragged_batch():
    """A batch that is not a multiple of anything, and chunked processing (chunk smaller than the batch)."""
    m = _model(323)
    m.chunk = 37
    patches = synth.make_patches(101, 11)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_carhynet_state_dict(323).items()}
    ref, _ = CO.car_hynet_forward(sd, torch.from_numpy(patches))
    out = m.compute_des_batches(patches)
    np.testing.assert_allclose(out, ref.numpy(), atol=3e-5, rtol=0)
    np.testing.assert_allclose(np.linalg.norm(out, axis=1), 1.0, atol=1e-5)


def _sd64(seed_w):
    return {k: torch.from_numpy(np.asarray(v)).double() for k, v in synth.make_carhynet_state_dict(seed_w).items()}


def _hi_plus_lo(spl, shape):
    from gims_amd import hip
    hi, lo = hip.spl32_planes(spl)
    return (hi.double() + lo.double()).cpu().reshape(shape)


def _sandglass_case(hw, c, n, prefix):
    """Input and float64 reference of one SandGlass block test: (x [n, hw, hw, c] f32, x + CO.sandglass(x) as NHWC float64)."""
    x = torch.from_numpy(np.random.default_rng(7).standard_normal((n, hw, hw, c)).astype(np.float32))
    x[1] *= 8.0                                   # both ReLU6 stages saturate
    x[2] = 0.0
    xt = x.double().permute(0, 3, 1, 2)
    return x, (xt + CO.sandglass(xt, _sd64(321), prefix)).permute(0, 2, 3, 1).contiguous()


def _first_block_case():
    """Input and float64 reference of the first-layer test: (patches [5, 32, 32, 3] f32, layer 1 output as NHWC float64)."""
    patches = torch.from_numpy(synth.make_patches(5, 41).copy())
    patches[3] = 0.5
    patches[4] = 0.0                              # FRN on a zero statistic: eps decides the result
    sd = _sd64(321)
    x = CO.tlu(CO.frn(patches.double().permute(0, 3, 1, 2), sd, "layer1.0."), sd, "layer1.1.")
    x = torch.nn.functional.conv2d(x, sd["layer1.2.weight"], sd["layer1.2.bias"], padding=1)
    x = CO.tlu(CO.coord_att(CO.frn(x, sd, "layer1.3."), sd, "layer1.4."), sd, "layer1.5.")
    return patches, x.permute(0, 2, 3, 1).contiguous()


def _assert_within(got, ref, e_old, what):
    """The bar of the block tests: 4 * E_old + 2^-15 |ref| per element, where E_old is the largest absolute error against the same float64
    reference of the layer-by-layer kernels these fused kernels replaced (the same f32 terms summed in another association: errors of the
    same order, not ordered), and the relative term is the split-bf16 storage of the output."""
    err = (got - ref).abs()
    print(f"{what}: max abs err {err.max().item():.3e}, max err / bar {(err / (4 * e_old + 2.0 ** -15 * ref.abs())).max().item():.3f}")
    assert torch.isfinite(got).all()
    assert (err <= 4 * e_old + 2.0 ** -15 * ref.abs()).all(), (what, err.max().item())


@pytest.mark.parametrize("hw,c,n,prefix,e_old", [(16, 64, 5, "layer4_5.", 2.455e-4), (32, 32, 3, "layer2_5.", 2.462e-4), (32, 32, 259, "layer2_5.", 2.462e-4)])
def test_sandglass_vs_float64(hw, c, n, prefix, e_old):
    """gims_ch_sandglass alone against x + SandGlass(x) of the float64 oracle, on standard-normal input with one patch scaled by 8 (both ReLU6
    stages saturate) and one all-zero patch.  259 patches of 32 x 32 x 32 reach the persistent form (256 workgroups, three of them process a
    second patch).  E_old (the removed one-kernel-per-stage sequence -- depthwise 3x3, pools, gates, gated pointwise pair, depthwise 3x3 -- on
    these inputs, values up to 72): measured worst case 2.456e-4 at 16 x 16 x 64, 2.463e-4 at 32 x 32 x 32 (3 and 259 patches), all on the patch
    scaled by 8 (3e-5 .. 6e-5 on the others).  This kernel: measured worst case 2.68e-4 / 3.37e-4 / 3.37e-4, 0.13 / 0.16 / 0.16 of the bar
    4 E_old + 2^-15 |ref| (9.8e-4 plus up to 2.2e-3)."""
    from gims_amd import hip
    P = _model(321)._prepare(torch.device("cuda", torch.cuda.current_device()))
    x, ref = _sandglass_case(hw, c, n, prefix)
    out = hip.ch_sandglass(x.cuda(), P["sg2" if prefix == "layer2_5." else "sg4"], torch.empty((n * hw * hw, 2 * c), dtype=torch.bfloat16, device="cuda"))
    _assert_within(_hi_plus_lo(out, ref.shape), ref, e_old, f"sandglass {hw}x{hw}x{c} n={n}")


def test_first_block_vs_float64():
    """gims_ch_conv_block_first alone against the float64 oracle's TLU(FRN) -> conv2d -> FRN -> CoordAtt -> TLU with the layer1 weights: three
    synthetic patches, a constant 0.5 patch and an all-zero patch.  E_old: measured worst case 5.29e-5 (values up to 3.6) for BOTH removed
    paths (an input-block kernel + GEMM + an FRN-block kernel, and separate FRN kernels + materialised 3x3 neighbourhoods + GEMM + an apply
    kernel).  This kernel: measured worst case 5.29e-5 as well, 0.24 of the bar 4 E_old + 2^-15 |ref| (2.1e-4 plus up to 1.1e-4): all three
    carry the same split-bf16 rounding of the 27 products per output, which dominates."""
    from gims_amd import hip
    L = _model(321)._prepare(torch.device("cuda", torch.cuda.current_device()))["l1"]
    patches, ref = _first_block_case()
    out = hip.ch_conv_block_first(patches.cuda(), L["frn0"], L["tau0"], L["conv"], L["frn"], L["tau"], L["ca"],
                                  torch.empty((5 * 1024, 64), dtype=torch.bfloat16, device="cuda"))
    _assert_within(_hi_plus_lo(out, ref.shape), ref, 5.29e-5, "first block")


def test_conv_block_layer_vs_conv2d(monkeypatch):
    """One layer in isolation, every geometry: gims_ch_conv_block against torch's float64 conv2d + the FRN / TLU formulas on the
    SAME split-bf16 input (hi + lo) and split weights; layer 2's geometry (the one gated 3x3 layer after the first) also with CoordAtt gates
    (the oracle's coord_att between FRN and TLU), in its two-workgroups-per-CU form and with GIMS_CH_HALF=0.  The gates are sigmoids in (0, 1)
    applied after FRN: they scale the ungated error down and add one f32 rounding each, so the bar is the ungated one
    (measured worst case 1.8e-5 ungated, 4.7e-6 / 4.5e-6 with gates)."""
    from gims_amd import hip
    r = np.random.default_rng(5)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.float32))).cuda()      # noqa: E731
    for hin, cin, cout, stride, gates, half in ((32, 32, 32, 1, False, None), (32, 32, 64, 2, False, None), (16, 64, 64, 1, False, None),
                                                (16, 64, 128, 2, False, None), (8, 128, 128, 1, False, None),
                                                (32, 32, 32, 1, True, None), (32, 32, 32, 1, True, "0")):
        if half is not None:
            monkeypatch.setenv("GIMS_CH_HALF", half)
        n = 5
        x = r.normal(size=(n, hin, hin, cin)).astype(np.float32)
        w = (r.normal(size=(cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
        b = r.normal(size=cout).astype(np.float32) * 0.1
        fw, fb = (1 + 0.2 * r.normal(size=cout)).astype(np.float32), (0.1 * r.normal(size=cout)).astype(np.float32)
        tau = (-1 + 0.3 * r.normal(size=cout)).astype(np.float32)
        xs = hip.split_spl32(torch.from_numpy(x.reshape(-1, cin)).cuda())
        xh, xl = hip.spl32_planes(xs)
        x_seen = (xh.double() + xl.double()).cpu().reshape(n, hin, hin, cin)
        wp = hip.pack_conv3_fragments(torch.from_numpy(w))
        w_seen = (wp[:, :, 0].double() + wp[:, :, 1].double())            # [step][nb][lane][8] -> back to [cout][cin][3][3]
        w_seen = w_seen.reshape(9, cin // 16, cout // 32, 2, 32, 8).permute(2, 4, 1, 3, 5, 0).reshape(cout, cin, 3, 3)
        L = dict(wp=wp.cuda(), b=torch.from_numpy(b).cuda())
        F = dict(w=torch.from_numpy(fw).cuda(), b=torch.from_numpy(fb).cuda(), eps=1e-6)
        ho = (hin - 1) // stride + 1
        y = torch.empty((n, ho, ho, cout), dtype=torch.float32, device="cuda")
        G = gsd = None
        if gates:
            g = dict(w1=r.normal(size=(8, cout)) / 6, b1=r.normal(size=8) * 0.1, wh=r.normal(size=(cout, 8)) / 3, bh=r.normal(size=cout) * 0.1,
                     ww=r.normal(size=(cout, 8)) / 3, bw=r.normal(size=cout) * 0.1)
            G = {k: dev(v) for k, v in g.items()}
            g = {k: v.double().cpu() for k, v in G.items()}
            gsd = {"g.conv1.weight": g["w1"][:, :, None, None], "g.conv1.bias": g["b1"], "g.conv_h.weight": g["wh"][:, :, None, None], "g.conv_h.bias": g["bh"],
                   "g.conv_w.weight": g["ww"][:, :, None, None], "g.conv_w.bias": g["bw"],      # w1 / b1 are given with BatchNorm folded in: an identity bn1
                   "g.bn1.running_mean": torch.zeros(8).double(), "g.bn1.running_var": torch.full((8,), 1.0 - CO.BN_EPS).double(),
                   "g.bn1.weight": torch.ones(8).double(), "g.bn1.bias": torch.zeros(8).double()}
        hip.ch_conv_block(xs, n, hin, cin, cout, stride, L, F, torch.from_numpy(tau).cuda(), G, y=y)
        conv = torch.nn.functional.conv2d(x_seen.permute(0, 3, 1, 2), w_seen, torch.from_numpy(b).double(), stride=stride, padding=1)
        nu2 = (conv * conv).mean(dim=(2, 3), keepdim=True)
        ref = conv * torch.rsqrt(nu2 + 1e-6) * torch.from_numpy(fw).double()[None, :, None, None] + torch.from_numpy(fb).double()[None, :, None, None]
        if gates:
            ref = CO.coord_att(ref, gsd, "g.")
        ref = torch.maximum(ref, torch.from_numpy(tau).double()[None, :, None, None])
        err = (y.cpu().double() - ref.permute(0, 2, 3, 1)).abs().max().item()
        print(f"conv block {(hin, cin, cout, stride)} gates={gates} GIMS_CH_HALF={half}: max abs err {err:.3e}")
        assert err < 2e-5, (hin, cin, cout, stride, gates, half, err)


@pytest.mark.parametrize("geom", [(32, 32, 1, True), (32, 32, 1, False), (32, 64, 2, False)])
def test_conv_block_two_per_cu_equals_one_per_cu(monkeypatch, geom):
    """The 32 x 32 layers in their two-workgroups-per-CU form (ch_conv_block_half_kernel: the patch goes through LDS in two halves, the FRN /
    CoordAtt / TLU block runs on half images) against the one-workgroup kernel (GIMS_CH_HALF=0): same products in the same order; the FRN
    statistic and the column pools are summed over the two halves in a different association, so agreement is to f32 rounding (1e-5 of values
    of order 1), with and without CoordAtt gates, f32 and split-bf16 outputs, and a patch count that leaves workgroups of the last wave idle."""
    from gims_amd import hip
    cin, cout, stride, gates = geom
    r = np.random.default_rng(17)
    n, hin = 37, 32
    ho = (hin - 1) // stride + 1
    x = r.normal(size=(n, hin, hin, cin)).astype(np.float32)
    x[3] *= 40.0                                                       # one patch of a very different scale (per-patch statistics must not mix)
    w = (r.normal(size=(cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.float32))).cuda()      # noqa: E731
    L = dict(wp=hip.pack_conv3_fragments(torch.from_numpy(w)).cuda(), b=dev(r.normal(size=cout) * 0.1))
    F = dict(w=dev(1 + 0.2 * r.normal(size=cout)), b=dev(0.1 * r.normal(size=cout)), eps=1e-6)
    tau = dev(-1 + 0.3 * r.normal(size=cout))
    G = None
    if gates:
        G = dict(w1=dev(r.normal(size=(8, cout)) / 6), b1=dev(r.normal(size=8) * 0.1), wh=dev(r.normal(size=(cout, 8)) / 3), bh=dev(r.normal(size=cout) * 0.1),
                 ww=dev(r.normal(size=(cout, 8)) / 3), bw=dev(r.normal(size=cout) * 0.1))
    xs = hip.split_spl32(torch.from_numpy(x.reshape(-1, cin)).cuda())
    outs = {}
    for half in ("0", "1"):
        monkeypatch.setenv("GIMS_CH_HALF", half)
        y = torch.full((n, ho, ho, cout), float("nan"), dtype=torch.float32, device="cuda")
        ysp = torch.zeros((n * ho * ho, 2 * cout), dtype=torch.bfloat16, device="cuda")
        hip.ch_conv_block(xs, n, hin, cin, cout, stride, L, F, tau, G, y=y)
        hip.ch_conv_block(xs, n, hin, cin, cout, stride, L, F, tau, G, y_split=ysp)
        hi, lo = hip.spl32_planes(ysp)
        outs[half] = (y.cpu().numpy(), (hi.float() + lo.float()).cpu().numpy().reshape(n, ho, ho, cout))
    scale = np.abs(outs["0"][0]).max(axis=(1, 2, 3), keepdims=True)
    assert np.isfinite(outs["1"][0]).all()
    assert (np.abs(outs["1"][0] - outs["0"][0]) / scale).max() < 1e-5
    assert (np.abs(outs["1"][1] - outs["1"][0]) <= np.abs(outs["1"][0]) * 2.0 ** -15 + 1e-30).all()      # the split output carries the same values


def test_full_size_properties():
    """BASELINE config 5's size (descriptors for 2 x 8192 keypoints), where the CPU restatement is too slow: every patch is
    processed independently, so (1) the result does not depend on how the batch is chunked -- bit for bit --, (2) a patch
    gives the same descriptor wherever it sits in the batch, (3) all descriptors are unit vectors, (4) two runs agree bitwise."""
    m = _model(321)
    base = synth.make_patches(512, 21)
    patches = np.tile(base, (32, 1, 1, 1))                      # 16384 patches, period 512
    d1 = m.compute_des_batches(patches)
    assert d1.shape == (16384, 128)
    np.testing.assert_allclose(np.linalg.norm(d1, axis=1), 1.0, atol=1e-5)
    np.testing.assert_array_equal(d1[:512], d1[512 * 17:512 * 18])
    m.chunk = 1536                                              # does not divide the batch
    d2 = m.compute_des_batches(patches)
    np.testing.assert_array_equal(d1, d2)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_carhynet_state_dict(321).items()}
    ref, _ = CO.car_hynet_forward(sd, torch.from_numpy(base[:32]))
    np.testing.assert_allclose(d1[:32], ref.numpy(), atol=3e-5, rtol=0)


def test_state_dict_roundtrip_and_errors():
    from gims_amd.carhynet import CARHyNet
    m = _model(321)
    sd = m.state_dict()
    assert list(sd.keys()) == [n for n, _ in synth.carhynet_state_dict_spec()]
    m2 = CARHyNet().eval()
    m2.load_state_dict(sd)
    p = synth.make_patches(4, 2)
    np.testing.assert_array_equal(m.compute_des_batches(p), m2.compute_des_batches(p))
    with pytest.raises(RuntimeError):
        m2.load_state_dict({"layer1.0.weight": torch.zeros(1, 3, 1, 1)})
    with pytest.raises(Exception):
        m(torch.zeros(2, 3, 32, 32))                # CPU tensor: no CPU fallback
