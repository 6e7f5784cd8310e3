"""CAR-HyNet patch descriptor on MI355X -- host side.

Mirrors the reference's interface for this stage (carhynet/models.py):
  * ``CARHyNet`` is an ``nn.Module`` with the reference's 136 state tensors (``CAR_HyNet().state_dict()`` names and shapes,
    models.py:311-362), so ``load_state_dict(torch.load('car_hynet.pth'))`` works unchanged; ``forward(x)`` takes the
    reference's NCHW float input and returns L2-normalised [N, 128] descriptors (eval mode only, models.py:379-399);
  * ``compute_des_batches(patches, color=True)`` takes NHWC patches in [0, 1] like ``HyNetnetFeature2D`` (models.py:655-666)
    and returns a float32 NumPy array.
All arithmetic runs in libgims_hip.so, one per-patch kernel per block with the patch's activation resident in LDS: the first layer
(``gims_ch_conv_block_first``: FRN + TLU on the raw patch, 3x3 convolution, FRN + CoordAtt + TLU), the five other 3x3 layers
(``gims_ch_conv_block``: the convolution as an implicit split-bf16x3 GEMM on the matrix cores -- f32-class accuracy -- + FRN (+ CoordAtt)
+ TLU) and the two SandGlass blocks (``gims_ch_sandglass``, f32).  Between blocks an activation is NHWC f32 (in front of a SandGlass
block) or SPL32 split-bf16 pixel rows (in front of a convolution).  The 8x8 convolution is the split-bf16x3 GEMM (``gims_linear``) on the
flattened 8x8x128 rows of all patches at once, followed by ``gims_ch_l2norm``.  BatchNorm (eval) is folded into the neighbouring
weights.  No CPU fallback.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from . import hip
from .synth import carhynet_state_dict_spec

BN_EPS = 1e-5
EPS_L2_NORM = 1e-10


class CARHyNet(nn.Module):
    chunk = 8192                      # patches per pass (32 per CU and launch: the start-time stagger of the per-patch kernels and the launch tails amortise)

    def __init__(self):
        super().__init__()
        for name, shape in carhynet_state_dict_spec():
            t = torch.zeros(shape, dtype=torch.int64 if name.endswith("num_batches_tracked") else torch.float32)
            self.register_buffer(name.replace(".", "__"), t)
        self._names = [n for n, _ in carhynet_state_dict_spec()]
        self._pack = None

    # state_dict with the reference's dotted names
    def state_dict(self, *a, **k):
        return {n: getattr(self, n.replace(".", "__")) for n in self._names}

    def load_state_dict(self, sd, strict=True):
        missing = [n for n in self._names if n not in sd]
        extra = [n for n in sd if n not in self._names]
        if strict and (missing or extra):
            raise RuntimeError(f"CARHyNet.load_state_dict: missing {missing[:3]}..., unexpected {extra[:3]}...")
        for n in self._names:
            if n in sd:
                getattr(self, n.replace(".", "__")).copy_(torch.as_tensor(np.asarray(sd[n])) if not torch.is_tensor(sd[n]) else sd[n])
        self._pack = None

    # ------------------------------------------------------------------ weight preparation
    def _prepare(self, dev):
        if self._pack is not None and self._pack["dev"] == dev:
            return self._pack
        sd = {n: getattr(self, n.replace(".", "__")).detach().double().cpu() for n in self._names}
        f32 = lambda t: t.float().contiguous().to(dev)       # noqa: E731

        def bn_fold(p, affine=True):                # y = x * sc + sh
            sc = 1.0 / torch.sqrt(sd[p + "running_var"] + BN_EPS)
            if affine:
                sc = sc * sd[p + "weight"]
            sh = -sd[p + "running_mean"] * sc + (sd[p + "bias"] if affine else 0.0)
            return sc, sh

        def conv3(p):                               # [O][I][3][3] -> the MFMA fragment order of gims_ch_conv_block (I zero-padded to a 16-channel K step)
            w = sd[p + "weight"]
            w16 = torch.zeros(w.shape[0], (w.shape[1] + 15) // 16 * 16, 3, 3, dtype=torch.float64)
            w16[:, :w.shape[1]] = w
            return dict(wp=hip.pack_conv3_fragments(w16).to(dev), b=f32(sd[p + "bias"]))

        def frn(p):
            return dict(w=f32(sd[p + "weight"].reshape(-1)), b=f32(sd[p + "bias"].reshape(-1)), eps=float(sd[p + "eps"].abs()))

        def tau(p):
            return f32(sd[p + "tau"].reshape(-1))

        def coordatt(p):
            sc, sh = bn_fold(p + "bn1.")
            w1 = sd[p + "conv1.weight"][:, :, 0, 0] * sc[:, None]
            b1 = sd[p + "conv1.bias"] * sc + sh
            return dict(w1=f32(w1), b1=f32(b1), wh=f32(sd[p + "conv_h.weight"][:, :, 0, 0]), bh=f32(sd[p + "conv_h.bias"]),
                        ww=f32(sd[p + "conv_w.weight"][:, :, 0, 0]), bw=f32(sd[p + "conv_w.bias"]))

        def dw(pw, pbn):                            # depthwise [C][1][3][3] + BN -> wt [9][C], bias [C]
            sc, sh = bn_fold(pbn)
            w = sd[pw + "weight"][:, 0] * sc[:, None, None]
            return dict(wt=f32(w.permute(1, 2, 0).reshape(9, -1)), b=f32(sh))

        def pw(pconv, pbn):                         # 1x1 conv (no bias) + BN -> f32 [O][I], bias [O]
            sc, sh = bn_fold(pbn)
            return dict(w=f32(sd[pconv + "weight"][:, :, 0, 0] * sc[:, None]), b=f32(sh))

        def sandglass(p):                           # the 14 weight tensors of gims_ch_sandglass, in its order
            p0, p1 = pw(p + "conv.2.", p + "conv.3."), pw(p + "conv.4.0.", p + "conv.4.1.")
            d0, d1, ca = dw(p + "conv.0.0.", p + "conv.0.1."), dw(p + "conv.5.", p + "conv.6."), coordatt(p + "conv.1.")
            return dict(ptrs=[d0["wt"], d0["b"], ca["w1"], ca["b1"], ca["wh"], ca["bh"], ca["ww"], ca["bw"], p0["w"], p0["b"], p1["w"], p1["b"], d1["wt"], d1["b"]])

        sc7, sh7 = bn_fold("layer7.2.", affine=False)
        w7 = sd["layer7.1.weight"].permute(0, 2, 3, 1).reshape(128, 8 * 8 * 128) * sc7[:, None]      # column (y*8+x)*128 + c: NHWC flatten
        P = dict(dev=dev,
                 l1=dict(frn0=frn("layer1.0."), tau0=tau("layer1.1."), conv=conv3("layer1.2."), frn=frn("layer1.3."), ca=coordatt("layer1.4."),
                         tau=tau("layer1.5.")),
                 l2=dict(conv=conv3("layer2.0."), frn=frn("layer2.1."), ca=coordatt("layer2.2."), tau=tau("layer2.3.")),
                 sg2=sandglass("layer2_5."), sg4=sandglass("layer4_5."),
                 l3=dict(conv=conv3("layer3.0."), frn=frn("layer3.1."), tau=tau("layer3.2.")),
                 l4=dict(conv=conv3("layer4.0."), frn=frn("layer4.1."), tau=tau("layer4.2.")),
                 l5=dict(conv=conv3("layer5.0."), frn=frn("layer5.1."), tau=tau("layer5.2.")),
                 l6=dict(conv=conv3("layer6.0."), frn=frn("layer6.1."), tau=tau("layer6.2.")),
                 l7=dict(w=hip.split_spl32(f32(w7)), b=f32(sh7)))
        self._pack = P
        return P

    # ------------------------------------------------------------------ layers
    @staticmethod
    def _spl(rows, c, dev):
        """SPL32 split-bf16 pixel rows of an NHWC activation: [rows, 2c]."""
        return torch.empty((rows, 2 * c), dtype=torch.bfloat16, device=dev)

    @torch.no_grad()
    def _features(self, patches, out):
        """patches: [n, 32, 32, 3] f32 on the GPU -> layer 6 output (models.py:380-392) written into `out` [n*64, 256].  One per-patch kernel
        per block; the raw convolution outputs never reach HBM.  x1 + SandGlass(x1) = 2 x1 + conv-stack(x1): models.py:226-233 adds x1 inside,
        383-385 / 387-389 add it again."""
        if patches.device.type != "cuda":
            raise hip.GimsHipError("CARHyNet runs on the GPU only (no CPU fallback): move the patches to 'cuda'")
        P = self._prepare(patches.device)
        n, dev = patches.shape[0], patches.device
        nhwc = lambda hw, c: torch.empty((n, hw, hw, c), dtype=torch.float32, device=dev)      # noqa: E731
        L = P["l1"]
        xs = hip.ch_conv_block_first(patches.contiguous(), L["frn0"], L["tau0"], L["conv"], L["frn"], L["tau"], L["ca"], self._spl(n * 1024, 32, dev))
        L = P["l2"]
        x1 = hip.ch_conv_block(xs, n, 32, 32, 32, 1, L["conv"], L["frn"], L["tau"], L["ca"], y=nhwc(32, 32))
        xs = hip.ch_sandglass(x1, P["sg2"], self._spl(n * 1024, 32, dev))
        xs = hip.ch_conv_block(xs, n, 32, 32, 64, 2, P["l3"]["conv"], P["l3"]["frn"], P["l3"]["tau"], y_split=self._spl(n * 256, 64, dev))
        x1 = hip.ch_conv_block(xs, n, 16, 64, 64, 1, P["l4"]["conv"], P["l4"]["frn"], P["l4"]["tau"], y=nhwc(16, 64))
        xs = hip.ch_sandglass(x1, P["sg4"], self._spl(n * 256, 64, dev))
        xs = hip.ch_conv_block(xs, n, 16, 64, 128, 2, P["l5"]["conv"], P["l5"]["frn"], P["l5"]["tau"], y_split=self._spl(n * 64, 128, dev))
        return hip.ch_conv_block(xs, n, 8, 128, 128, 1, P["l6"]["conv"], P["l6"]["frn"], P["l6"]["tau"], y_split=out)

    def _head(self, xs, n):
        """layer7 + desc_l2norm over ALL patches at once.  The [n*64, 2*128] SPL32 pixel rows ARE the SPL32 layout of the
        flattened [n, 8*8*128] activation (32-channel blocks never straddle a pixel): the 8x8 convolution is one GEMM on a
        view (one launch for the whole batch: a chunk alone would fill 16 of the 256 CUs)."""
        P = self._pack
        raw = torch.empty((n, 128), dtype=torch.float32, device=xs.device)
        hip.linear(xs.view(n, 64 * 256), P["l7"]["w"], spl=True, bias=P["l7"]["b"], precision=hip.PREC_BF16X3, out=raw)
        desc = hip.ch_l2norm(raw, EPS_L2_NORM, torch.empty_like(raw))
        return desc, raw

    def _forward_nhwc(self, patches):
        """patches: [N, 32, 32, 3] f32 on the GPU -> (desc [N, 128], raw [N, 128]); the convolution stack runs in chunks."""
        n = patches.shape[0]
        if n == 0:
            z = torch.zeros((0, 128), dtype=torch.float32, device=patches.device)
            return z, z.clone()
        feats = torch.empty((n * 64, 256), dtype=torch.bfloat16, device=patches.device)
        for i in range(0, n, self.chunk):
            m = min(self.chunk, n - i)
            self._features(patches[i:i + m], feats[i * 64:(i + m) * 64])
        return self._head(feats, n)

    def forward(self, x, mode="eval"):
        """x: [N, 3, 32, 32] like the reference's CAR_HyNet.forward (models.py:379); eval mode only."""
        if self.training:
            raise NotImplementedError("CARHyNet: training mode (Dropout, batch statistics) is not on the HIP path")
        with torch.no_grad():
            desc, raw = self._forward_nhwc(x.permute(0, 2, 3, 1).float().contiguous())
        return (desc, raw) if mode == "train" else desc

    def compute_des_batches(self, patches, color=True):
        """HyNetnetFeature2D.compute_des_batches (models.py:655-666): NHWC patches in [0, 1] -> float32 [N, 128] NumPy array."""
        if not color:
            raise NotImplementedError("CARHyNet: the grey-level variant (HyNet, 1 input channel) is not built")
        dev = torch.device("cuda", torch.cuda.current_device())
        with torch.no_grad():
            p = torch.from_numpy(np.ascontiguousarray(patches, dtype=np.float32)).to(dev)
            return self._forward_nhwc(p)[0].cpu().numpy()

    def compute_sift(self, patches, kps, color=True):
        """HyNetnetFeature2D.compute_sift (models.py:668-671): what utils.common.sift_forward calls on ``data['carhynet']``
        (common.py:886) -- so an instance of this class can be handed to the reference's front end as its ``carhynet``."""
        if len(kps) == 0:
            return kps, []
        return kps, self.compute_des_batches(patches, color).astype(np.float32)
