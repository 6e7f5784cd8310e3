"""Drop-in ``GMatcher`` for the GIMS matcher hot path, running on MI355X through libgims_hip.so.

Mirrors the reference's operator interface (models/gmatcher.py):
  * ``GMatcher(config)`` with the same ``default_config`` keys (gmatcher.py:166-176) and checkpoint
    handling (``ema`` -> ``model`` -> raw state dict, gmatcher.py:208-217);
  * ``state_dict()`` / ``load_state_dict()`` use the reference's 348 parameter names (``bin_score``,
    ``kenc.encoder.*``, ``gnn.layers.*.attn.{merge,proj.N}``, ``gnn.layers.*.mlp.*``,
    ``gnn_encoder.layers.*.{fc_self,fc_neigh}``, ``final_proj``), both SAGEConv bias layouts accepted;
  * ``forward(data)`` consumes and MUTATES the same dict (gmatcher.py:219-307): kept keypoints /
    descriptors / scores, ``kept_kpts{0,1}_indices``, ``graph0/1``; returns the same result dict
    (int64 ``matches0/1`` with -1 for no match, f32 ``matching_scores0/1``, ``mdesc0/1`` ...).

Host code is Python on PyTorch-ROCm (device memory + streams); all arithmetic of the path runs in the
HIP kernels of ``gims_amd/csrc`` through the C ABI of ``include/gims_hip.h``.  No CPU fallback exists.
Internally activations are point-major ([rows, channels]); all images of a call are concatenated row-wise
so that every linear layer is ONE launch for the whole batch.
"""
from __future__ import annotations

import math
import os
import time
import weakref
from typing import Dict, List

import numpy as np
import torch
import torch.nn as nn

from . import hip
from .attention_tiers import MODE_NAMES, AttentionTiers

BN_EPS = 1e-5
LN_EPS = 1e-6          # the reference's LayerNorm (gmatcher.py:74-85)


class _Node(nn.Module):
    """Bare container used to reproduce the reference's parameter tree (names only, no forward)."""


def _register(root: nn.Module, dotted: str, tensor: torch.Tensor, buffer: bool):
    mod = root
    parts = dotted.split(".")
    for p in parts[:-1]:
        if not hasattr(mod, p):
            mod.add_module(p, _Node())
        mod = getattr(mod, p)
    if buffer:
        mod.register_buffer(parts[-1], tensor)
    else:
        mod.register_parameter(parts[-1], nn.Parameter(tensor))


def _stack(ts):
    """torch.stack for the reference-shaped outputs; a single pair (what eval_homography.py passes) gets a leading-axis VIEW instead
    of a copy kernel per output (the buffers behind it belong to this call alone)."""
    return ts[0][None] if len(ts) == 1 else torch.stack(ts)


class PairResults(list):
    """List of per-pair result dicts; ``.flat`` additionally exposes the batch-concatenated match tensors (what the
    per-pair entries are views of) so statistics can be reduced without touching each pair separately."""
    flat = None
    datas = None      # match_features: per pair the dict match_pairs would have left behind (None from match_pairs: its callers hold the dicts)


class GraphHandle:
    """What the reference hands back as ``data['graph0/1'][b]`` (a DGLGraph there): CSR of the adaptive
    graph over the kept keypoints (both edge directions), plus the node data the reference stores on it."""

    def __init__(self, indptr, indices, ndata):
        self.indptr, self.indices, self.ndata = indptr, indices, ndata

    def num_nodes(self):
        return int(self.indptr.numel() - 1)

    def num_edges(self):
        return int(self.indices.numel())

    def edges(self):
        deg = (self.indptr[1:] - self.indptr[:-1]).long()
        dst = torch.repeat_interleave(torch.arange(deg.numel(), device=deg.device), deg)
        return self.indices.long(), dst


class ImageFeatures:
    """One image as the matcher sees it behind its encoder stage (``GMatcher.encode_images``): everything of a match that does not depend
    on the partner image.  Immutable.  Device tensors: ``keypoints`` [n, 2], ``descriptors`` [n, 256] (point-major), ``scores`` [n] -- the
    kept ones --, ``kept`` (int32 indices into the input), ``graph`` (``GraphHandle``) and ``encoded`` f32 [n, 256], the residual stream the
    attentional layers start from.  Host values: ``n``, ``n_edges``, ``shape`` (the image's), ``setting`` = (radius, percentile, min_size,
    delaunay) and ``gen``, the generation of the weight pack the image was encoded with: features are valid for those weights only
    (``GMatcher.match_features`` refuses others)."""
    __slots__ = ("keypoints", "descriptors", "scores", "kept", "graph", "encoded", "n", "n_edges", "shape", "setting", "gen", "_owner")

    def __init__(self, **kw):
        for k in self.__slots__:
            object.__setattr__(self, k, kw[k])

    def __setattr__(self, name, value):
        raise AttributeError("ImageFeatures is immutable")

    __delattr__ = __setattr__

    @property
    def device(self):
        return self.encoded.device

    def __repr__(self):
        return f"ImageFeatures(n={self.n}, n_edges={self.n_edges}, shape={tuple(self.shape)}, setting={self.setting}, gen={self.gen}, device='{self.device}')"


class _ImageShape:
    """Stands where a data dict holds an image of which only ``.shape`` is read (``match_features``' ``datas``)."""

    def __init__(self, shape):
        self.shape = tuple(shape)


class GMatcher(nn.Module):
    default_config = {
        'descriptor_dim': 256,
        'weights_path': None,
        'keypoint_encoder': [32, 64, 128, 256],
        'transformer_layers': ['self', 'cross'] * 9,
        'sinkhorn_iterations': 100,
        'match_threshold': 0.2,
        'use_layernorm': False,
        'input_dim': 256,
        'num_heads': 4,
        # --- additions (defaults keep the reference behaviour) ---
        'linear_precision': 'bf16x3',   # 'bf16x3' (split-bf16 MFMA, ~2^-17) or 'f32' (exact-f32 MFMA)
        # 'bf16': plain bf16 MFMA attention (north_star's choice; meets the 1e-4 score bar for diffuse to moderately peaked
        # softmaxes -- mean row maximum up to ~0.2 measured).  'f16': the same kernels on IEEE-half operands
        # (v_mfma_f32_32x32x16_f16: same rate, 2^-12 instead of 2^-9 per operand; Q/K/V from the 3-pass projection, rounded to half in
        # its epilogue) -- holds the bar on the sharply peaked 'peaked' goldens (mean row maximum ~0.8) where bf16 does not.
        # 'bf16x3': Q, K, V and P as split-bf16 pairs, three MFMAs per product (GIMS_ATTN_X3): f32 class, no range limit.
        # 'auto' (default) picks PER LAYER from what the kernels measure about that layer (the stat accumulator of gims_attention): per head the mean
        # over the queries of max_k P[q, k] and the fraction of queries whose maximum exceeds 1/2 (the tail: a head with a few
        # one-hot rows among diffuse ones), and max |Q|, |K|, |V| as stored.  The first batch after the weights change runs every
        # layer at 'bf16x3' and measures; from then on a layer runs in plain bf16 while every head stays below
        # `attention_auto_threshold` (mean) and `attention_auto_tail` (fraction), in half above that while its operands stay
        # below `attention_f16_range` (half's finite range is 65504), else at 'bf16x3'.  EVERY batch is measured (round 5;
        # `attention_monitor_period` = 1) and the verdict is drawn ON THE DEVICE inside the same batch: behind every bf16 / half
        # attention launch of the table sit two GUARDED launches (gims_attn_guard) -- the 3-pass Q/K/V projection and the
        # split-bf16 attention of that layer -- that do nothing unless the statistic the cheap launch just produced is over the
        # thresholds (bf16 layer: peaked; half layer: out of range), and otherwise REDO the layer at f32-class accuracy before the
        # MLP consumes the message.  So the results of a batch never carry the cheap tier's error of a layer that sharpened on
        # THAT batch; the host reads the same statistic behind the next synchronisation and moves the layer up for good
        # (bf16 -> f16 -> bf16x3), after which the redo no longer fires.  Cost when nothing fires: 36 empty launches per batch.
        # `attention_auto_rowmax` (round 6): the guard of a bf16 layer also fires when a head's LARGEST row maximum reaches it -- one sharply
        # peaked row inside a diffuse layer (an outlier keypoint: mean and tail fraction stay far under their thresholds, the reference golden
        # raree2e_*_g10 shows 6e-4 of score error on plain bf16 operands).  That redo is per batch: the layer is NOT moved up (one outlier does
        # not cost every later batch the faster tier); forward() repeats such a batch with the device-side guards on.  The figure is complete
        # for every kernel and every row length: the running-maximum kernels report every row; the 8-wave kernel bounds every row's maximum by
        # its largest half-tile mass, reports that bound for rows of >= 512 keys and, for shorter rows (where half a tile is a large share of a
        # merely short row), has the waves whose bound reaches 1/2 measure their rows exactly (tests/test_attention_rowmax_gpu.py).  A batch
        # counts once towards `attention_auto_rare_batches`, also when forward() repeats it.  0 switches the criterion off.
        # `attention_auto_rare_batches`: a layer whose rows did that on this many batches is no outlier any more -- redoing it at three times the
        # matrix work every batch costs more than the half tier's 1.2 x -- and IS moved up (0: never).
        'attention_precision': 'auto',
        'attention_auto_threshold': 0.08,
        'attention_auto_tail': 0.02,
        'attention_auto_rowmax': 0.5,
        'attention_auto_rare_batches': 3,
        'attention_f16_range': 3.0e4,
        'attention_monitor_period': 1,
        # 0 (default): every call issues the encoder and the 18 layers as gims_run_ops tables.  > 0: only calls of up to this many keypoint rows
        # (both images of every pair) do, larger batches launch one by one from Python -- on some boxes 0.8-1.5 % faster for 4096 x 8, on
        # others 0.5 % slower, and with occasional 20-36 ms steps the tables never showed (GMatcher._replays)
        'launch_replay_rows': 0,
        'train_precision': 'bf16x6',      # products of the training step's forward (gims_amd/trainstep.py): 'bf16x6' (f32 class) | 'bf16x3'
        'train_backward_precision': 'bf16x3',      # products of its reverse pass: 'bf16x3' (default), 'bf16x6' or 'f32'.  The pass is linear in its operands, but the
                                                   # attention scores it recomputes carry 16 mantissa bits against the forward's exact-f32 lse: the error of
                                                   # the attention gradients grows with the logit magnitude, about 2.2e-6 |S| of the largest entry (6e-5 at
                                                   # |S| = 33, 6e-4 at 268: tests/test_train_kernels_gpu.py::test_train_attention_reverse_precision_at_large_logits);
                                                   # 'f32' keeps 2e-5 at any magnitude at 2.7 x the attention reverse time -- the setting for sharply peaked trained attention
        'verbose': False,               # the reference prints '>> ...' timing lines; off by default here
        # fold the attention 'merge' conv into the first MLP conv at load time:
        #   W0 [x ; Wm o + bm] + b0  ==  W0x x + (W0m Wm) o + (W0m bm + b0)        (gmatcher.py:114,125)
        # exact in real arithmetic (products formed in float64), removes one GEMM and one activation round trip per
        # layer; set False to run the reference's operation order
        'fuse_merge': True,
        # match_pairs can split a batch into independent sub-batches on separate HIP streams.  Measured on MI355X: no gain
        # (1840 vs 1874 pairs/s at 2x1024, 271 vs 267 at 2x4096) -- every stage already fills the chip -- so default 1.
        'streams': 1,
        # GMatcher.sweep runs its settings in sub-batches of at most this many keypoint rows (both images of every entry counted; one
        # entry at least): 65536 is the 8 pairs of 2 x 4096 the throughput numbers of match_pairs are quoted for -- larger sub-batches
        # gain nothing there, and every entry holds its own activations and score matrix ...
        'sweep_rows': 65536,
        # ... and of at most this much graph-build workspace (hip.agc_workspace_bytes: one 32-bit word per keypoint pair of an image)
        'sweep_workspace_mb': 4096,
    }

    def __init__(self, config):
        super().__init__()
        self.config = {**self.default_config, **config}
        cfg = self.config
        if cfg['input_dim'] != cfg['descriptor_dim']:
            raise NotImplementedError("input_proj is built but never called by the reference forward (gmatcher.py:198-201)")
        D = cfg['descriptor_dim']
        if D != 256:
            raise NotImplementedError("descriptor_dim must be 256 (4 heads x 64)")
        self.n_layers = len(cfg['transformer_layers'])
        self._heads = 4   # AttentionalGNN hard-codes 4 heads (gmatcher.py:131); config['num_heads'] is ignored there too
        from .synth import state_dict_spec
        spec = list(state_dict_spec(D, tuple(cfg['keypoint_encoder']), self.n_layers, use_layernorm=bool(cfg['use_layernorm'])))
        # the BatchNorm layers are real nn.BatchNorm1d modules (never called -- the kernels read their tensors by name): what
        # train.py:43-51 sorts into optimizer groups by isinstance, and what SyncBatchNorm conversion looks for
        bn_prefixes = {n[:-len(".running_mean")]: shape for n, shape in spec if n.endswith(".running_mean")}
        for prefix, shape in bn_prefixes.items():
            mod, parts = self, prefix.split(".")
            for q in parts[:-1]:
                if not hasattr(mod, q):
                    mod.add_module(q, _Node())
                mod = getattr(mod, q)
            mod.add_module(parts[-1], nn.BatchNorm1d(shape[0]))
        for name, shape in spec:
            if name.rsplit(".", 1)[0] in bn_prefixes:
                continue
            if name.endswith("num_batches_tracked"):
                _register(self, name, torch.zeros((), dtype=torch.int64), buffer=True)
            elif name.endswith("running_mean"):
                _register(self, name, torch.zeros(shape), buffer=True)
            elif name.endswith("running_var"):
                _register(self, name, torch.ones(shape), buffer=True)
            elif name == "bin_score" or name.endswith(".a_2"):
                _register(self, name, torch.tensor(1.0) if name == "bin_score" else torch.ones(shape), buffer=False)
            else:
                _register(self, name, torch.zeros(shape), buffer=False)
        self._pack = None
        self._pack_key = None
        if cfg['weights_path']:
            weights = torch.load(cfg['weights_path'], map_location="cpu", weights_only=False)
            if ('ema' in weights) and (weights['ema'] is not None):
                load_dict = weights['ema']
            elif 'model' in weights:
                load_dict = weights['model']
            else:
                load_dict = weights
            self.load_state_dict(load_dict)
            print('Loaded GMatcher model ("{}" weights)'.format(cfg['weights_path']))

    # ------------------------------------------------------------------ checkpoint compatibility
    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        sd = {}
        for k, v in state_dict.items():
            k = k[7:] if k.startswith("module.") else k          # DDP prefix (utils/common.py:107-114)
            # older DGL: SAGEConv keeps a separate ``bias`` parameter instead of ``fc_self.bias``
            if k.startswith("gnn_encoder.layers.") and k.endswith(".bias") and k.count(".") == 3:
                k = k[:-len("bias")] + "fc_self.bias"
            sd[k] = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))
        self._pack = None
        for k in ("_ops_cache", "_plist", "_train_params", "_train_buffers", "_fstate"):
            self.__dict__.pop(k, None)
        return super().load_state_dict(sd, strict=strict, **kw)

    def _apply(self, fn, *a, **kw):          # .to() / .cuda() / .half() replace the parameter tensors
        for k in ("_plist", "_train_params", "_train_buffers", "_fstate"):
            self.__dict__.pop(k, None)
        self._pack = None
        return super()._apply(fn, *a, **kw)

    def _float_state(self):
        """The floating entries of state_dict() -- parameters and BatchNorm running statistics, the tensors themselves -- in its order:
        what optim.ModelEMA averages.  Cached like _plist (walking the module tree per training step is host time)."""
        fs = self.__dict__.get("_fstate")
        if fs is None:
            fs = self.__dict__["_fstate"] = [v for v in self.state_dict(keep_vars=True).values() if v.dtype.is_floating_point]
        return fs

    # ------------------------------------------------------------------ weight packing
    def _packed(self, device):
        # (the parameter list is cached: walking the module tree for 348 parameters cost ~0.25 ms per call, twice per forward,
        # both times on the host's critical path in front of a launch; in-place updates are still seen through _version)
        plist = self.__dict__.get("_plist")
        if plist is None:
            plist = self.__dict__["_plist"] = list(self.parameters())
        key = (str(device), self.config['linear_precision'], bool(self.config['fuse_merge']),
               sum([p._version for p in plist]))
        if self._pack is not None and self._pack_key == key:
            return self._pack
        sd = {k: v.detach().to("cpu", torch.float32) for k, v in self.state_dict().items()}
        x3 = self.config['linear_precision'] == 'bf16x3'
        if self.config['linear_precision'] not in ('bf16x3', 'f32'):
            raise ValueError("linear_precision must be 'bf16x3' or 'f32'")
        ln = bool(self.config['use_layernorm'])
        P: Dict[str, object] = {"x3": x3, "ln": ln}

        def fold(w, b, prefix):   # Conv1d(k=1) followed by BatchNorm1d(eval)  (gmatcher.py:17-22)
            if ln:                # use_layernorm=True: LayerNorm sits there instead (gmatcher.py:19-20) -- nothing to fold
                return w, b
            g = sd[prefix + ".weight"] / torch.sqrt(sd[prefix + ".running_var"] + BN_EPS)
            return w * g[:, None], (b - sd[prefix + ".running_mean"]) * g + sd[prefix + ".bias"]

        def lnp(prefix):          # LayerNorm parameters (a_2, b_2) of the norm that follows a conv, on the device
            return (dev(sd[prefix + ".a_2"]), dev(sd[prefix + ".b_2"])) if ln else None

        def dev(t):
            return t.contiguous().to(device)

        def lin(w, b, spl=False):   # a linear layer in the configured precision (spl: SPL32 operands, LDS-DMA kernel)
            w = w.contiguous()
            e = {"b": dev(b), "n": w.shape[0], "k": w.shape[1], "spl": False}
            if x3 and spl:
                e.update(w=hip.split_spl32(dev(w)), w_lo=None, prec=hip.PREC_BF16X3, spl=True)
            elif x3 and w.shape[1] % 64 == 0:
                hi, lo = hip.split_bf16(dev(w))
                e.update(w=hi, w_lo=lo, prec=hip.PREC_BF16X3)
            else:
                e.update(w=dev(w), w_lo=None, prec=hip.PREC_F32)
            return e

        # keypoint encoder: Sequential indices conv 0,3,6,9,12 / BN 1,4,7,10 (gmatcher.py:92)
        nk = len(self.config['keypoint_encoder']) + 1
        w, b = fold(sd["kenc.encoder.0.weight"][:, :, 0], sd["kenc.encoder.0.bias"], "kenc.encoder.1")
        P["kenc_w1"], P["kenc_b1"] = dev(w), dev(b)
        P["kenc_ln"] = [lnp(f"kenc.encoder.{3 * i + 1}") for i in range(nk - 1)]       # norm after conv i (i < nk - 1)
        P["kenc"] = []
        for i in range(1, nk):
            w, b = sd[f"kenc.encoder.{3 * i}.weight"][:, :, 0], sd[f"kenc.encoder.{3 * i}.bias"]
            if i < nk - 1:
                w, b = fold(w, b, f"kenc.encoder.{3 * i + 1}")
            P["kenc"].append(lin(w, b, not ln))      # SPL32 operands (LDS-DMA GEMM); the LayerNorm variant keeps f32 activations
        # GraphSAGE: [W_self | W_neigh] on [h | mean(h)]  (gmatcher.py:149-151)
        P["sage"] = []
        for i in range(3):
            p = f"gnn_encoder.layers.{i}."
            P["sage"].append(lin(torch.cat([sd[p + "fc_self.weight"], sd[p + "fc_neigh.weight"]], 1), sd[p + "fc_self.bias"], True))
        # attentional GNN.  Heads are interleaved in the reference (channel c = d*H + h, gmatcher.py:111);
        # permute q/k/v output rows and merge input columns to head-blocked order c' = h*64 + d.
        H, D = self._heads, self.config['descriptor_dim']
        dh = D // H
        perm = torch.tensor([(c % dh) * H + (c // dh) for c in range(D)])   # new index c' -> old channel
        P["layers"] = []
        for l in range(self.n_layers):
            p = f"gnn.layers.{l}."
            wq, wk, wv = [sd[p + f"attn.proj.{j}.weight"][:, :, 0][perm] for j in range(3)]
            bq, bk, bv = [sd[p + f"attn.proj.{j}.bias"][perm] for j in range(3)]
            wm = sd[p + "attn.merge.weight"][:, :, 0][:, perm]
            w0, b0 = fold(sd[p + "mlp.0.weight"][:, :, 0], sd[p + "mlp.0.bias"], p + "mlp.1")
            w0f = b0f = None
            if self.config['fuse_merge']:
                w0m = w0[:, D:].double()
                w0f = torch.cat([w0[:, :D].double(), w0m @ wm.double()], 1).float()
                b0f = (b0.double() + w0m @ sd[p + "attn.merge.bias"].double()).float()
            # the softmax scale log2(e)/sqrt(dh) rides in the query projection (exact in f64, one rounding to f32): the
            # attention kernel then exponentiates the MFMA result as it is (hip.attention(..., q_prescaled=True))
            wq = (wq.double() * hip.ATTN_Q_SCALE).float()
            bq = (bq.double() * hip.ATTN_Q_SCALE).float()
            w1, b1 = sd[p + "mlp.3.weight"][:, :, 0], sd[p + "mlp.3.bias"]
            e0f = lin(w0f, b0f, True) if w0f is not None else None
            mlp_op = None
            if e0f is not None and x3 and not ln and D == 256:
                # the one-launch MLP (hip.op_mlp) reads [W0 ; W1 with its K axis in register order] and b0 | b1 as ONE buffer each; the
                # two-launch path keeps its own W1 and takes W0 / b0 as views of these (no second copy of the larger matrix)
                mlp_op = {"w": hip.split_spl32(dev(torch.cat([w0f, hip.mlp_w1_permute(w1)], 0))), "b": dev(torch.cat([b0f, b1]))}
                e0f.update(w=mlp_op["w"][:2 * D], b=mlp_op["b"][:2 * D])
            P["layers"].append({
                "mlp0_fused": e0f, "mlp_op": mlp_op,
                "qkv": lin(torch.cat([wq, wk, wv], 0), torch.cat([bq, bk, bv], 0), True),
                "merge": lin(wm, sd[p + "attn.merge.bias"], True),
                "mlp0": lin(w0, b0, True),
                "mlp1": lin(w1, b1, True),
                "ln": lnp(p + "mlp.1"),
                "cross": self.config['transformer_layers'][l] == 'cross',
            })
        P["final"] = lin(sd["final_proj.weight"][:, :, 0], sd["final_proj.bias"], True)
        P["alpha"] = float(sd["bin_score"])
        self._pack, self._pack_key = P, key
        # replay tables bake raw device pointers of the OLD pack's tensors: drop them with it, and identify packs by a
        # monotonically increasing generation (id() of a freed dict is readily reused by CPython)
        self._pack_gen = getattr(self, "_pack_gen", 0) + 1
        P["gen"] = self._pack_gen
        self.__dict__.pop("_ops_cache", None)
        return P

    # The Q/K/V projection feeds the bf16 attention kernel and is rounded to bf16 on the way out, so it runs as a plain bf16
    # product of the hi planes (one MFMA pass instead of three): end-to-end score error on the reference goldens 1.6e-5 /
    # 2.7e-5 against 1.1e-5 / 2.1e-5 with the split-bf16x3 projection (bar 1e-4).  GIMS_QKV_PREC=x3 restores the latter.
    _qkv_flags = 0 if os.environ.get("GIMS_QKV_PREC", "bf16") == "x3" else hip.LINEAR_HI_ONLY


    _use_graph = os.environ.get("GIMS_OPS_GRAPH", "0") == "1"      # opt-in: measured gain <= 3 % (tools/graph_probe.py)

    # The MLP of a layer as ONE launch (hip.op_mlp: the hidden activation stays in registers) from this many keypoint rows on --
    # the first measured size at which it beats the two launches (a lone 128-row workgroup is a serial chain of 48 stages, where the two
    # launches switch to smaller tiles).  Its second product sums in another order than the MLP1 launch, so WHICH of the two a call takes
    # shows in the last bits -- like the attention kernel families that 'auto', 'bf16' and 'f16' select by launch shape.
    # attention_precision='bf16x3' is the configuration whose results do not depend on what shares a batch with a pair
    # (tests/test_sweep_gpu.py::test_sub_batch_size_does_not_change_the_results): it keeps the two launches at every size.
    # GIMS_MLP_FUSED=0 | 1 (never | wherever the kernel serves the shape, at every size) overrides for A/B runs; read per call.
    mlp_fused_rows = 24576

    def _mlp_fused(self, P, n_tot):
        if not P["layers"] or P["layers"][0]["mlp_op"] is None:      # linear_precision='f32', fuse_merge=False, LayerNorm, another width
            return False
        env = os.environ.get("GIMS_MLP_FUSED")
        if env in ("0", "1"):
            return env == "1"
        return self.config['attention_precision'] != 'bf16x3' and n_tot >= self.mlp_fused_rows

    @staticmethod
    def _lin(e, a0, **kw):
        return hip.linear(a0, e["w"], w_lo=e["w_lo"], bias=e["b"], precision=e["prec"], spl=e["spl"], **kw)

    def _act(self, name, rows, cols, dtype):
        """Layer activation that never leaves this object ([rows, cols] of dtype): a view of a per-lane arena, so its
        address is the same from call to call and the recorded launch sequence of the GNN layers can be replayed."""
        nbytes = rows * cols * torch.empty((), dtype=dtype).element_size()
        return self._buf("act_" + name, nbytes)[:nbytes].view(dtype).view(rows, cols)

    # ------------------------------------------------------------------ attention_precision='auto'
    _tiers = None          # the AttentionTiers of the current weight pack (None before the first 'auto' batch)

    def _attention_modes(self, P, repeat):
        """Per layer the attention kernel family -- 0: bf16 operands, 1: IEEE half (GIMS_ATTN_F16), 2: split-bf16 pairs
        (GIMS_ATTN_X3) -- and the device accumulator [layers][heads + 1][4] int64 the kernels report the softmax peakedness and the
        operand range into (None when nothing is measured).  repeat: forward()'s repeat of a batch that was counted already."""
        mode, L = self.config['attention_precision'], self.n_layers
        if mode != 'auto' or not P["x3"]:          # (linear_precision='f32' has no split Q/K/V planes: 'auto' means bf16 there)
            return [MODE_NAMES.index(mode) if mode in MODE_NAMES and P["x3"] else 0] * L, None
        self._attention_stats_consume(self._lane)
        tiers = self._tiers
        if tiers is None or tiers.gen != P["gen"]:      # new weights: measure every layer at the accurate precision first
            tiers = self._tiers = AttentionTiers(L, self._heads, P["gen"], self.config)
        if not tiers.measured(self._lane, repeat):
            return list(tiers.mode), None
        nbytes = L * (self._heads + 1) * 4 * 8
        stat = self._buf("attn_stat", nbytes)[:nbytes].view(torch.int64).view(L, self._heads + 1, 4)
        return list(tiers.mode), stat.zero_()

    def _attention_stats_enqueue(self, stat):
        """Asynchronous read-back of this batch's statistics (consumed behind the next host synchronisation of this lane) into the lane's
        slot: [pinned buffer, event behind the copy (None once consumed), generation of the tier table the batch ran on]."""
        pend = self.__dict__.setdefault("_attn_pending", {})
        slot = pend.get(self._lane)
        if slot is None or slot[0].numel() != stat.numel():
            slot = pend[self._lane] = [torch.empty(stat.shape, dtype=torch.int64, pin_memory=True), None, 0]
        slot[0].copy_(stat, non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record()
        slot[2] = self._tiers.gen

    def _attention_stats_consume(self, lane=None, repeat=False):
        """Fold the finished read-back of `lane` (None: of every lane) into the tier table (AttentionTiers.fold; `repeat` as there); a
        read-back of an older generation of the weights is dropped.  Called by a lane right after the host synchronisation of its next
        batch's graph build -- its previous batch, read-back included, has finished by then, so WHEN a measurement takes effect does not
        depend on timing -- and after forward()'s final synchronisation.  Returns the number of layers a SETTLED table moved up by in this
        call (forward() repeats its batch then; match_pairs' batches were redone on the device already)."""
        tiers, moved = self._tiers, 0
        if tiers is not None:
            tiers.begin()
        for ln, slot in list(self.__dict__.get("_attn_pending", {}).items()):
            if slot[1] is None or (lane is not None and ln != lane):
                continue
            slot[1].synchronize()
            raw, slot[1] = slot[0].numpy().copy(), None
            if tiers is not None and slot[2] == tiers.gen:
                moved += tiers.fold(raw, repeat)
        return moved

    def _keep_attention_tiers(self, device):
        """TEST HOOK: carry the settled per-layer tier table over a change of the weights (which normally starts a new calibration), so that a
        test can hand a model whose layers all sit on plain bf16 a batch whose attention is peaked -- the situation the device-side redo exists
        for (a trained model meeting an input that sharpens a layer)."""
        assert self._tiers is not None and self._tiers.calibrated, "settle the model first"
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:        # (the pack is keyed by the full device name the batches arrive on)
            device = torch.device("cuda", torch.cuda.current_device())
        self._tiers.rebind(self._packed(device)["gen"])

    def attention_report(self):
        """What 'auto' decided: per layer 'bf16' / 'f16' / 'bf16x3', the last measured peakedness (mean row maximum) and tail
        fraction (row maximum above 1/2) per (layer, head), max |Q|, |K|, |V| per layer, layers moved up after the first measurement.
        None before the first batch or with a fixed attention_precision."""
        self._attention_stats_consume()
        return None if self._tiers is None else self._tiers.report()

    # ------------------------------------------------------------------ stage timing (HIP events on the launch stream)
    def enable_timing(self, on: bool = True, stepwise: bool = False):
        """Record a (start, end) HIP-event pair around every stage on the stream the kernels are launched on;
        read them back with ``stage_times_ms()`` after a synchronize.  The GNN layers keep running through the replayed
        launch table (the production path): the library records an event after each of its launches
        (gims_run_ops_timed).  ``stepwise=True`` issues the encoder and layer tables launch by launch instead (_issue)."""
        self._timers = {} if on else None
        self._stepwise = bool(stepwise)

    _stepwise = False

    def stage_times_ms(self):
        out = {}
        for name, evs in (self._timers or {}).items():
            if not name.startswith("_"):
                out[name] = [a.elapsed_time(b) for a, b, _ in evs]
        for pool, labels in (self._timers or {}).get("_ops", []):       # per-op events of the replayed layers
            for lab, ms in zip(labels, pool.elapsed_ms()):
                out.setdefault(lab, []).append(ms)
        return out

    def stage_host_ms(self):
        """Host wall time spent inside each stage (enqueue cost), same keys as stage_times_ms()."""
        return {name: [h for _, _, h in evs] for name, evs in (self._timers or {}).items() if not name.startswith("_")}

    class _Stage:
        def __init__(self, owner, name):
            self.o, self.name = owner, name

        def __enter__(self):
            if self.o._timers is not None:
                self.a = torch.cuda.Event(enable_timing=True)
                self.a.record()
                self.t0 = time.perf_counter()

        def __exit__(self, *exc):
            if self.o._timers is not None:
                b = torch.cuda.Event(enable_timing=True)
                b.record()
                self.o._timers.setdefault(self.name, []).append((self.a, b, 1e3 * (time.perf_counter() - self.t0)))

    _timers = None

    # ------------------------------------------------------------------ persistent scratch (grown on demand, reused across calls)
    def _buf(self, name: str, nbytes: int) -> torch.Tensor:
        dev = torch.device("cuda", torch.cuda.current_device())
        arena = self.__dict__.setdefault("_arena", {})
        key = (name, dev, self._lane)              # one scratch set per stream lane (lanes run concurrently)
        t = arena.get(key)
        if t is None or t.numel() < nbytes:
            t = torch.empty(((int(nbytes * 1.25) + 511) // 256) * 256, dtype=torch.uint8, device=dev)   # multiple of 256 bytes
            arena[key] = t
        return t

    _lane = 0

    # ------------------------------------------------------------------ ragged core: 2P images -> P pair results
    def _run_build(self, images, radius, percentile, min_size, robust=False, delaunay=False, each=None):
        """Phase 1: enqueue the adaptive graph construction (asynchronous; no host sync).  images: list of dicts {kp (N,2) f32, de (N,D) f32
        point-major, sc (N,), shape}; consecutive entries (2p, 2p+1) form pair p.  Every pair may keep a different number of keypoints
        (ragged batch).  Returns the context of the call, which _run_rest takes: the caller adds its mode to it -- `guards` (device-side
        redo launches behind the 'auto' attention tiers), `repeat` (forward()'s repeat of a batch that was counted already), `streamed`
        (other stream lanes run next to this one), `skip_empty` (sweep); each False where it is absent.  robust: the graph build histograms every
        similarity instead of predicting where the percentile lies (the repeat after a build reported a missed prediction).
        delaunay: D-GIMS -- the Delaunay triangulation of the keypoints instead (gims_delaunay_build: every keypoint kept; radius,
        percentile and min_size have no effect); it fills the same kept / indptr / indices / info slots.
        each: one (radius, percentile, min_size, delaunay) per image instead of the four values above (match_pairs(per_pair_graph=True),
        sweep): the adaptive images go through ONE agc_build_each call, the Delaunay images through ONE delaunay_build call."""
        cfg = self.config
        dev = images[0]["kp"].device
        D = cfg['descriptor_dim']
        St = lambda name: GMatcher._Stage(self, name)   # noqa: E731

        # ---- adaptive graph construction: every stage ONE launch for all images; ONE host sync for the counts
        with St("agc"):
            ns = [g["kp"].shape[0] for g in images]
            if min(ns) < 2:
                raise ValueError("need at least one array to concatenate")               # what the reference raises (agc.py:701)
            # capacity of the adaptive graph in directed edges per node (the reference has no limit: its percentile keeps
            # (100 - p) % of the radius pairs, agc.py:378-380, 445-447; dense keypoints at radius 25 can exceed any fixed guess):
            # starts at 64 and grows for good when a build reports an overflow (see _run_rest)
            ec = self._edge_cap
            pool = torch.empty(sum((ec + 2) * n + 4 for n in ns), dtype=torch.int32, device=dev)   # kept | indptr | indices per image
            o = 0
            for g, n in zip(images, ns):
                g["kept"], g["indptr"], g["indices"] = pool[o:o + n], pool[o + n:o + 2 * n + 1], pool[o + 2 * n + 4:o + (ec + 2) * n + 4]
                o += (ec + 2) * n + 4
            info_all = torch.empty((len(images), 8), dtype=torch.int32, device=dev)
            slots = [dict(kpts=g["kp"], desc=g["de"], kept=g["kept"], indptr=g["indptr"], indices=g["indices"], info=info_all[i])
                     for i, g in enumerate(images)]
            aflags = hip.AGC_ROBUST if robust else 0        # (the default flow never stores the N x N half matrix: half the workspace)
            if each is not None:
                assert len(each) == len(images)
                tri = [i for i, e in enumerate(each) if e[3]]
                ada = [i for i, e in enumerate(each) if not e[3]]
                if tri:
                    tri_imgs = hip.make_agc_images([slots[i] for i in tri])
                    hip.delaunay_build(tri_imgs, self._buf("delaunay", hip.delaunay_workspace_bytes(tri_imgs)))
                if ada:
                    ada_imgs = hip.make_agc_images([slots[i] for i in ada])
                    hip.agc_build_each(ada_imgs, [each[i][:3] for i in ada], self._buf("agc", hip.agc_workspace_bytes(ada_imgs, aflags)),
                                       flags=aflags)
                delaunay = False
            elif delaunay:
                agc_imgs = hip.make_agc_images(slots)
                hip.delaunay_build(agc_imgs, self._buf("delaunay", hip.delaunay_workspace_bytes(agc_imgs)))
            else:
                agc_imgs = hip.make_agc_images(slots)
                hip.agc_build(agc_imgs, radius, percentile, min_size, self._buf("agc", hip.agc_workspace_bytes(agc_imgs, aflags)), flags=aflags)
            # everything of the next stage that does not depend on the kept counts is prepared NOW, while the GPU builds the
            # graphs: after the host sync only two cumsums stand between the counts and the next launch
            ptab = hip.pack_table([(g["kp"].data_ptr(), g["de"].data_ptr(), g["de"].stride(0), g["sc"].data_ptr(),
                                    g["kept"].data_ptr(), g["indptr"].data_ptr(), g["indices"].data_ptr()) for g in images])
            # normalize_keypoints parameters (gmatcher.py:26-33) in float32 arithmetic, like the reference's tensors.
            # NHWC callers => (height, width) = (W, 3): the reference's quirk, kept verbatim.
            hw = np.asarray([[g["shape"][3], g["shape"][2]] for g in images], dtype=np.float32)   # size = [width, height]
            norm3 = np.concatenate([hw / np.float32(2), (hw.max(axis=1, keepdims=True) * np.float32(0.7))], axis=1).astype(np.float32)
            norm3_host, norm3 = norm3, hip.upload(norm3, dev)
            n_up = sum(ns)                                  # upper bounds: kept <= n, edges <= capacity * n
            bufs = dict(feat=torch.empty((n_up, D), dtype=torch.float32, device=dev),
                        kpts=torch.empty((n_up, 2), dtype=torch.float32, device=dev),
                        score=torch.empty((n_up,), dtype=torch.float32, device=dev),
                        seg=torch.empty((n_up,), dtype=torch.int32, device=dev),
                        indptr=torch.empty((n_up + 1,), dtype=torch.int32, device=dev),
                        indices=torch.empty((ec * n_up + 1,), dtype=torch.int32, device=dev))
        return dict(images=images, info_all=info_all, pool=pool, ptab=ptab, norm3=norm3, bufs=bufs, params=(radius, percentile, min_size),
                    robust=robust, delaunay=delaunay, each=each, norm3_host=norm3_host)

    _edge_cap = 64

    @staticmethod
    def _agc_retry(flags, robust, delaunay=False):
        """What to do with the flag words (info[7]) of a graph build: 'robust' -- some image's predicted percentile window was missed: ALL its
        outputs are void, its overflow bit included (a void threshold can keep any number of edges), so this comes first; 'grow' -- an edge
        buffer overflowed; None -- the build stands.  A robust build cannot report a miss.  A Delaunay build (delaunay=True) is never
        repeated as robust: a degenerate image raises ValueError (the reference raises scipy's QhullError there), stars that disagree raise."""
        flags = np.asarray(flags)
        if delaunay:
            bad = np.nonzero(flags & hip.DT_INFO_DEGENERATE)[0]
            if len(bad):
                i = int(bad[0])
                raise ValueError(f"delaunay: image {i} of the batch (pair {i // 2}, keypoints{i % 2}) has fewer than 3 distinct keypoints, "
                                 "all its keypoints on one line, or a non-finite coordinate: it has no Delaunay triangulation")
            if (flags & (hip.DT_INFO_ASYMMETRIC | hip.AGC_INFO_WINDOW_MISSED)).any():
                raise hip.GimsHipError("delaunay graph: the per-point stars of a build did not agree (asymmetric adjacency)")
        if (flags & hip.AGC_INFO_WINDOW_MISSED).any():
            if robust:
                raise hip.GimsHipError("adaptive graph: the robust flow reported a missed percentile window")
            return "robust"
        if (flags & hip.AGC_INFO_OVERFLOW).any():
            return "grow"
        return None

    def _gather(self, ctx):
        """Read the kept counts (the one host sync of a batch) and compact the kept keypoints of all images into merged
        row-major arrays + one merged CSR (gmatcher.py:244-249).  Returns None after growing the edge capacity (the caller
        repeats the build), else a dict of the merged arrays."""
        images, info_all = ctx["images"], ctx["info_all"]
        cfg = self.config
        dev = images[0]["kp"].device
        D = cfg['descriptor_dim']
        ts0 = time.perf_counter()
        # the one host sync of the build: into a pinned staging buffer (a pageable .cpu() goes through the runtime's own
        # pin / copy / unpin path and costs ~0.1 ms more per call, which a single pair through forward() feels)
        pin = self.__dict__.get("_info_pin")
        if pin is None or pin.shape[0] < info_all.shape[0]:
            pin = self.__dict__["_info_pin"] = torch.empty((max(64, info_all.shape[0]), 8), dtype=torch.int32, pin_memory=True)
        pin[:info_all.shape[0]].copy_(info_all, non_blocking=True)
        early = self._kenc_early(ctx)       # (the keypoint encoder over all input keypoints, enqueued BEHIND the read-back: it runs while the host waits)
        if early is None:
            torch.cuda.current_stream().synchronize()
        else:
            early["event"].synchronize()    # the read-back has landed; everything enqueued before it (the previous batch of this lane too) has finished
        infos = pin[:info_all.shape[0]].numpy().copy()
        self._sync_ms = 1e3 * (time.perf_counter() - ts0)
        each = ctx.get("each")
        if each is None:
            action = self._agc_retry(infos[:, 7], bool(ctx.get("robust")), bool(ctx.get("delaunay")))
        else:       # per-image graph kinds: every image's flag word is read by the rules of its own build (the other kind's masked out)
            tri = np.asarray([bool(e[3]) for e in each])
            acts = [self._agc_retry(np.where(tri, infos[:, 7], 0), bool(ctx.get("robust")), True) if tri.any() else None,
                    self._agc_retry(np.where(tri, 0, infos[:, 7]), bool(ctx.get("robust")), False)]
            action = "robust" if "robust" in acts else ("grow" if "grow" in acts else None)
        if action == "robust":
            # the percentile window predicted from the similarity sample did not provably hold the threshold (gims_agc_build): the
            # outputs of this build are void; the repeat histograms every similarity
            ctx["params"] = tuple(ctx["params"][:3]) + (True,)
            self._agc_window_misses = getattr(self, "_agc_window_misses", 0) + 1
            return None
        if action == "grow":
            # more edges than the buffers hold: repeat the graph build of this batch with room for what it reported (the
            # directed-edge total of the densest image, rounded up to a power of two per node), and keep the larger capacity
            ns = np.asarray([g["kp"].shape[0] for g in images], dtype=np.float64)
            # info[1]: directed edges of the final graph, info[2]: undirected edges of the coarse graph (both counted in full
            # even when they did not fit); the isolated-node fix-up adds at most one edge per node
            tot = np.maximum(infos[:, 1].astype(np.float64), 2.0 * infos[:, 2] + 2.0 * ns)
            need = int(np.ceil(max(2.0 * self._edge_cap, float((tot / ns).max()) * 1.1)))
            cap = 1 << (need - 1).bit_length()
            if cap > 16384 or cap <= self._edge_cap:
                raise hip.GimsHipError(f"adaptive graph exceeded the edge capacity ({self._edge_cap} directed edges per node) and cannot grow further")
            self._edge_cap = cap
            ctx["params"] = tuple(ctx["params"][:3]) + (bool(ctx.get("robust")),)      # a robust build stays robust when it is repeated for room
            return None
        norm3 = ctx["norm3"]
        if (infos[:, 0] == 0).any():
            if not ctx.get("skip_empty"):
                raise ValueError("need at least one array to concatenate")               # np.vstack([]) in agc.py:701
            # sweep: a pair with an image that keeps nothing leaves the batch here, before the compaction (the reference raises for that
            # setting alone, and parameter_search.py records it as a row without matches)
            gone = (infos[:, 0].reshape(-1, 2) == 0).any(axis=1)
            ctx["dropped"] = np.nonzero(gone)[0].tolist()
            keep = np.repeat(~gone, 2)
            images = ctx["images"] = [g for g, k in zip(images, keep) if k]
            infos, ctx["ptab"] = infos[keep], ctx["ptab"][keep]
            if not images:
                return dict(n_tot=0)
            norm3 = hip.upload(ctx["norm3_host"][keep], dev)

        # ---- kept-keypoint compaction (gmatcher.py:244-249): rows of all images concatenated, one launch
        row_off = np.concatenate([[0], np.cumsum(infos[:, 0], dtype=np.int64)])
        e_off = np.concatenate([[0], np.cumsum(infos[:, 1], dtype=np.int64)])
        n_tot, e_tot = int(row_off[-1]), int(e_off[-1])
        with GMatcher._Stage(self, "gather"):
            ptab, b = ctx["ptab"], ctx["bufs"]
            ptab["n_kept"], ptab["n_edges"], ptab["row_off"], ptab["edge_off"] = infos[:, 0], infos[:, 1], row_off[:-1], e_off[:-1]
            feat, kpts_all, score_all, seg = b["feat"][:n_tot], b["kpts"][:n_tot], b["score"][:n_tot], b["seg"][:n_tot]
            indptr_all, indices_all = b["indptr"][:n_tot + 1], b["indices"][:max(e_tot, 1)]
            hip.pack_graphs_table(ptab, D, feat, kpts_all, score_all, seg, indptr_all, indices_all, n_tot, e_tot)
        row_off, e_off = row_off.tolist(), e_off.tolist()
        for g, inf, ro in zip(images, infos, row_off):
            g["n_kept"], g["n_edges"], g["info_host"] = int(inf[0]), int(inf[1]), inf
            g["rows"] = (ro, g["n_kept"])
        return dict(feat=feat, kpts_all=kpts_all, score_all=score_all, seg=seg, indptr_all=indptr_all, indices_all=indices_all,
                    norm3=norm3, n_tot=n_tot, e_tot=e_tot, early=early)

    # The keypoint encoder reads (x, y), the image size and the folded weights only -- nothing of the graph build -- so with the default configuration
    # (linear_precision='bf16x3', no LayerNorm) it runs over ALL input keypoints of the batch while the host waits for the kept counts, where the
    # device used to idle.  GraphSAGE's last layer then adds the rows of the kept keypoints as its residual (linear_args
    # residual_rows, filled by the gather kernel) and writes desc (+ dpl): sage + kenc in place of kenc + sage, the same bits; a GEMM row does not depend
    # on the rows that share its launch.  The GraphSAGE output alone is not materialised in this order (`sage` of the results is None).
    # kenc_early = False or GIMS_KENC_EARLY=0 keeps the encoder behind the synchronisation.
    kenc_early = True

    def _kenc_early(self, ctx):
        """Enqueue the read-back event and, behind it, the keypoint encoder over all input keypoints of ctx's batch.  Returns None where that order
        does not apply (a caller other than _run_rest, configuration, switch, or keypoints that do not lie back to back in one buffer), else dict(event, out: f32 [n_in, D],
        src_row: int32 [n_in], filled by the gather kernel with the input row of every kept keypoint).  This runs before the build's flag words
        are read: a build that _run_rest repeats (missed window, edge capacity) throws the work away and it is enqueued again with the repeat.
        A sweep's sub-batch of several settings repeats the base images, fails the back-to-back test and keeps the old order."""
        if not ctx.get("kenc_early") or not self.kenc_early or os.environ.get("GIMS_KENC_EARLY", "1") == "0":
            return None
        images = ctx["images"]
        kp0 = images[0]["kp"]
        dev = kp0.device
        P = self._packed(dev)
        if not P["x3"] or P["ln"]:
            return None
        starts, off = [], 0
        for g in images:
            kp = g["kp"]
            if kp.dtype != torch.float32 or not kp.is_contiguous() or kp.data_ptr() != kp0.data_ptr() + 8 * off:
                return None
            starts.append(off)
            off += kp.shape[0]
        n_in = off
        bf, f32 = torch.bfloat16, torch.float32
        A = lambda name, cols, dt: self._act(name, n_in, cols, dt)                      # noqa: E731
        c1 = P["kenc_w1"].shape[0]
        kmax = max([c1] + [e["n"] for e in P["kenc"]])
        b = dict(xk=A("kenc_in_x", c1, f32), xs0=A("kenc_in_xs0", 2 * kmax, bf), xs1=A("kenc_in_xs1", 2 * kmax, bf), desc=A("kenc_in_out", P["kenc"][-1]["n"], f32))
        src_row = self._act("kenc_src_row", n_in, 1, torch.int32)
        ev = torch.cuda.Event()
        ev.record()
        starts_dev = hip.upload(np.asarray(starts, dtype=np.int32), dev)
        batch = dict(n=n_in, kpts=kp0.data_ptr(), norm3=ctx["norm3"].data_ptr(), seg=starts_dev.data_ptr(), n_img=len(images))
        key = (P["gen"],) + tuple(t.data_ptr() for t in b.values())
        cache = self.__dict__.setdefault("_kenc_cache", {})
        ent = cache.get(key)
        if ent is None:
            if len(cache) > 4:
                cache.clear()
            lst, slots = self._encoder_ops(P, b, None, batch, part="kenc")
            ent = cache[key] = self._table(lst, (P, b), slots)
        self._patch(ent, batch)
        self._issue("encoder", ent, n_in)
        ctx["ptab"]["src_row"], ctx["ptab"]["in_off"] = src_row.data_ptr(), starts
        return dict(event=ev, out=b["desc"], src_row=src_row, starts=starts_dev)

    @staticmethod
    def _patch(ent, batch):
        """Write the per-call values `batch` into the slots the builder of table `ent` recorded."""
        ops = ent[0]
        for k, field, j, what in ent[6]:
            if j is None:
                setattr(ops[k].u.lin, field, batch[what])
            else:
                getattr(ops[k].u.aux, field)[j] = batch[what]

    @staticmethod
    def _finish_graphs(images, G):
        """Per-image views and graph handles (host-only bookkeeping, done after everything is enqueued)."""
        for g in images:
            ro, nk = g["rows"]
            g["kept"] = g["kept"][:nk]
            g["indptr"] = g["indptr"][:nk + 1]
            g["indices"] = g["indices"][:g["n_edges"]]
            g["graph"] = GraphHandle(g["indptr"], g["indices"],
                                     {"point": G["kpts_all"][ro:ro + nk], "feat": G["feat"][ro:ro + nk], "score": G["score_all"][ro:ro + nk]})

    def _replays(self, part, n_tot):
        """Whether `part` ("encoder" | "layers") of this call is issued as one gims_run_ops table or launch by launch.

        The table removes the host's per-launch cost, which is what bounds small calls (one pair: 2.1 vs 2.4 ms).  Large batches hide
        the host behind the GPU either way; launch-by-launch issue measured 0.8-1.5 % faster there on four boxes and 0.5 % slower on a
        fifth, where it also produced 3 runs in 32 with a 21-36 ms step against none in 32 with the tables (DESIGN.md section 4.5:
        same kernels, same order, bit-equal results) -- so the tables are the default at every size, and `launch_replay_rows` > 0
        restricts them to calls of at most that many keypoint rows.  GIMS_NO_REPLAY=1 | 2 | 3 (nothing | only the layers | only the
        encoder replayed) and GIMS_REPLAY=1 (always) override for A/B runs."""
        if self._stepwise:
            return False
        env = os.environ.get("GIMS_NO_REPLAY")
        if env is not None:
            return env == ("3" if part == "encoder" else "2")
        rows = int(self.config['launch_replay_rows'])
        return os.environ.get("GIMS_REPLAY") == "1" or rows <= 0 or n_tot <= rows

    def _run_rest(self, ctx):
        """Phase 2: read the kept counts (the one host sync; a build that asks for it is repeated), then enqueue everything else.  Returns the
        results of the batch: items (per pair the score matrix, matches and potentials), pairs (their row ranges), mdesc, desc, sage (None where _kenc_early applied),
        images, flat, outputs (every device buffer of the batch), status_offs (where in outputs[4] each pair's Sinkhorn status word lies),
        dropped (sweep: the pairs that kept nothing) and repeats (of the graph build)."""
        ctx["kenc_early"] = True        # (the encoder stage of _run_batch knows that order; the training step gathers for its own encoder and does not ask)
        G = self._gather(ctx)
        if G is None:
            again = self._run_build(ctx["images"], *ctx["params"], delaunay=bool(ctx.get("delaunay")), each=ctx.get("each"))
            again.update({k: ctx[k] for k in ("guards", "repeat", "streamed", "skip_empty") if k in ctx}, repeats=ctx.get("repeats", 0) + 1)
            return self._run_rest(again)
        # (a sweep's sub-batch may have lost the pairs that kept nothing, all of them even)
        # self._last: a reference to the most recent result, for sinkhorn_status(), the probes under tools/ and the tests -- valid until the
        # next call on the same lane
        res = self._last = self._run_batch(ctx, G) if ctx["images"] else dict(items=[], pairs=[], mdesc=None, images=[], outputs=[], status_offs=np.zeros(0, dtype=np.int64))
        res.update(dropped=ctx.get("dropped", []), repeats=ctx.get("repeats", 0))
        return res

    def _run_batch(self, ctx, G):
        """_run_rest for the batch gathered in G: encoder, layers, scores, Sinkhorn and selection, all enqueued without a host sync."""
        images = ctx["images"]
        P = self._packed(images[0]["kp"].device)
        feat, kpts_all, score_all, n_tot = G["feat"], G["kpts_all"], G["score_all"], G["n_tot"]
        # ---- GraphSAGE over the merged CSR of all images (gmatcher.py:145-162, 268-269) and keypoint encoder (gmatcher.py:26-33, 87-97);
        #      desc = sage + kenc (gmatcher.py:270-271)
        sage, desc = self._encoder(P, G)
        pairs = [(images[2 * p]["rows"], images[2 * p + 1]["rows"]) for p in range(len(images) // 2)]
        res = self._match_rows(P, desc, n_tot, pairs, max(g["n_kept"] for g in images), ctx)
        self._finish_graphs(images, G)
        res.update(sage=sage, images=images, outputs=res["outputs"] + [feat, kpts_all, score_all, ctx["pool"]])
        return res

    def _match_rows(self, P, desc, n_tot, pairs, max_nq, ctx):
        """Everything behind the encoder stage, for _run_batch and match_features alike: the residual stream desc [n_tot, D] (and, with
        linear_precision='bf16x3', its SPL32 copy self._act('dpl')) hold the encoded rows of the batch, pairs = [((o0, n0), (o1, n1))] are the row
        ranges of every pair's two images, max_nq the longest of them.  Layers, final projection, scores, Sinkhorn and selection, all enqueued
        without a host sync; ctx: the mode of the call (guards, repeat, streamed; see _run_build)."""
        cfg = self.config
        dev = desc.device
        D = cfg['descriptor_dim']
        St = lambda name: GMatcher._Stage(self, name)   # noqa: E731
        # ---- attentional GNN (gmatcher.py:99-143): per layer QKV -> flash attention -> merge -> MLP -> residual
        # problem tables travel as kernel arguments (hip.upload): a pageable torch.tensor(..., device=) would block this
        # thread until the stream drains and stop the host from running ahead of the GPU
        # (problem tables and layer activations live in per-lane arenas: stable addresses let the launch tables be cached)
        spr = np.asarray([[o, n, o, n] for pr in pairs for (o, n) in pr], dtype=np.int32)
        cpr = np.asarray([q for (o0, n0), (o1, n1) in pairs for q in ((o0, n0, o1, n1), (o1, n1, o0, n0))], dtype=np.int32)
        # (ONE upload for both tables: a launch and ~15 us of host time less per call on the single-pair path)
        both = hip.upload(np.concatenate([spr, cpr]), dev, out=self._buf("attn_pr", spr.nbytes + cpr.nbytes + 32))
        stat = self._layers(P, desc, n_tot, max_nq, both[:spr.shape[0]], both[spr.shape[0]:], bool(ctx.get("guards")), bool(ctx.get("repeat")))
        if stat is not None:
            self._attention_stats_enqueue(stat)
        # ---- final projection, score matrix, Sinkhorn, selection (gmatcher.py:273-294)
        with St("final_scores"):
            mdesc = self._lin(P["final"], self._act("dpl", n_tot, 2 * D, torch.bfloat16) if P["x3"] else desc)
            items, largs = [], []
            tot0, tot1 = sum(n0 for (_, n0), _ in pairs), sum(n1 for _, (_, n1) in pairs)
            m0_all = torch.empty(tot0, dtype=torch.int64, device=dev)
            m1_all = torch.empty(tot1, dtype=torch.int64, device=dev)
            s0_all = torch.empty(tot0, dtype=torch.float32, device=dev)
            s1_all = torch.empty(tot1, dtype=torch.float32, device=dev)
            uv_all = torch.empty(tot0 + tot1 + 3 * len(pairs), dtype=torch.float32, device=dev)
            c0 = c1 = cu = 0
            # the score GEMM keeps f32 accuracy: three-way bf16 split operands (six MFMAs per product) unless
            # GIMS_SCORE_PREC=f32 asks for the exact-f32 MFMA kernel
            sprec = hip.PREC_BF16X6 if (D % 32 == 0 and os.environ.get("GIMS_SCORE_PREC", "x6") != "f32") else hip.PREC_F32
            sdesc = hip.split_spl3(mdesc) if sprec == hip.PREC_BF16X6 else mdesc
            for (o0, n0), (o1, n1) in pairs:
                ld = (n1 + 3) // 4 * 4
                scores = torch.empty((n0, ld), dtype=torch.float32, device=dev)
                largs.append(hip.linear_args(sdesc[o0:o0 + n0], sdesc[o1:o1 + n1], out=scores, precision=sprec,
                                             scale=1.0 / math.sqrt(D), n=n1))
                items.append(dict(scores=scores, n=n0, m=n1, matches0=m0_all[c0:c0 + n0], matches1=m1_all[c1:c1 + n1],
                                  mscores0=s0_all[c0:c0 + n0], mscores1=s1_all[c1:c1 + n1], uv=uv_all[cu:cu + n0 + n1 + 3]))
                c0, c1, cu = c0 + n0, c1 + n1, cu + n0 + n1 + 3
            hip.linear_batch(largs, self._buf("score_args", 256 * len(largs)), sprec)
        with St("sinkhorn"):
            probs = hip.make_ot_problems(items)
            work = self._buf("ot", hip.sinkhorn_workspace_bytes(probs))
            otf = hip.OT_STREAMED if ctx.get("streamed") else 0
            self.sinkhorn_plan_last = hip.sinkhorn_plan(probs, cfg['sinkhorn_iterations'], otf)   # 0 streamed / k resident launches
            # (a resident solve that gives up -- status 2: its 256 workgroups were not co-resident, e.g. next to another
            # process's kernels -- is re-solved inside this call by a dependency-free kernel before the selection runs, so the
            # matches of THIS batch are valid when the call returns; see ot_rescue_kernel.  The status words stay readable:
            # `sinkhorn_status()` after a synchronise.)
            hip.sinkhorn_match(probs, P["alpha"], cfg['sinkhorn_iterations'], cfg['match_threshold'], work, otf)
            status_offs = np.cumsum([it["n"] + it["m"] + 3 for it in items]) - 1
        return dict(items=items, pairs=pairs, mdesc=mdesc, desc=desc,
                    flat=dict(matches0=m0_all, scores0=s0_all, n0=[n0 for (_, n0), _ in pairs], n1=[n1 for _, (_, n1) in pairs]),
                    outputs=[m0_all, m1_all, s0_all, s1_all, uv_all, mdesc], status_offs=status_offs)

    # ------------------------------------------------------------------ encoder and layer stages: launch tables
    # Each stage's launches are spelled ONCE, by its builder (_encoder_ops, _layer_ops), as a list of (stage-timer label, gims_op); the list is
    # cached as a gims_run_ops table and _issue runs it -- in one call into the library, or launch by launch as slices of the same table.
    @staticmethod
    def _lin_op(e, a0, **kw):
        """Linear layer `e` of the weight pack applied to a0, as an op of a launch table."""
        return hip.op_linear(hip.linear_args(a0, e["w"], w_lo=e["w_lo"], bias=e["b"], precision=e["prec"], spl=e["spl"], **kw))

    @staticmethod
    def _norm_args(x, a2b2, rows, out=None, out_split=None):
        """hip.op_aux arguments of LayerNorm + ReLU over the channels of x[:rows] (use_layernorm=True: conv -> LayerNorm -> ReLU, gmatcher.py:17-23)."""
        return (hip.AUX_LAYERNORM_ACT, [x, a2b2[0], a2b2[1], out, out_split, None if out_split is None else out_split.data_ptr() + 64],
                [x.stride(0), rows, x.shape[1], hip.ACT_RELU, 0 if out is None else out.stride(0), 0 if out_split is None else out_split.stride(0)],
                [LN_EPS])

    @staticmethod
    def _table(lst, keep, *extra):
        """Cache entry of the launch sequence lst = [(label, gims_op)], a list: [0] the table, [1] its HIP graph (GIMS_OPS_GRAPH=1), [2] the number
        of times it was issued in ONE call, [3] `keep`, references to every tensor whose address is baked into the table, [4] its labels, [5] the
        maximal runs of equal consecutive labels as [label, start, count] (the stage brackets of launch-by-launch issue), then `extra`."""
        runs = []
        for k, (lab, _) in enumerate(lst):
            if runs and runs[-1][0] == lab:
                runs[-1][2] += 1
            else:
                runs.append([lab, k, 1])
        return [hip.make_ops([o for _, o in lst]), None, 0, keep, [lab for lab, _ in lst], runs, *extra]

    def _issue(self, part, ent, n_tot):
        """Run the cached table `ent` of `part` ("encoder" | "layers").  Where _replays says so, in one call: gims_run_ops; for the layers
        under stage timers gims_run_ops_timed (an event after every op), under GIMS_OPS_GRAPH=1 on a non-default stream ONE graph launch from
        the second use on (the first initialises inside the library).  Otherwise launch by launch: one gims_run_ops call per run of equal
        labels, inside that label's stage bracket -- the same ops in the same order, so the results are bit-equal by construction.  The
        replayed encoder under stage timers is issued that way too (two brackets: an event after each of its ops -- and their creation -- sat
        in the host-bound stretch behind the synchronisation and cost a timed 1024 x 32 step 3 %)."""
        ops, labels, runs = ent[0], ent[4], ent[5]
        if self._replays(part, n_tot) and (part == "layers" or self._timers is None):
            ent[2] += 1
            if (part == "layers" and ent[1] is None and ent[2] >= 2 and self._use_graph
                    and torch.cuda.current_stream().cuda_stream != 0):        # (the encoder table is patched per call: never a graph)
                ent[1] = hip.OpsGraph(ops)
            if self._timers is not None:
                pool = hip.EventPool(len(ops) + 1)
                hip.run_ops_timed(ops, pool)
                self._timers.setdefault("_ops", []).append((pool, labels))
            elif ent[1] is not None:
                ent[1].launch()
            else:
                hip.run_ops(ops)
            return
        for label, start, count in runs:
            with GMatcher._Stage(self, label):
                hip.run_ops(ops, start, count)

    def _encoder(self, P, G):
        """GraphSAGE + keypoint encoder of the batch gathered in G.  Every intermediate lives in the per-lane arena, so its address does not
        change from call to call: the table is CACHED and PATCHED per call with what does change -- the row count and the six pointers of the
        batch (kept descriptors, CSR, keypoints, image index per row, normalisation constants), at the slots the builder recorded.  Between a
        batch's one host synchronisation and its layers the device waits for the host: on a cache hit no gims_op is built or copied
        (DESIGN.md 4.5).  Returns (sage, desc); with linear_precision='bf16x3' dpl, the SPL32 copy of desc, is self._act('dpl').  Where the keypoint
        encoder ran ahead of the synchronisation (G['early'], _kenc_early) only GraphSAGE is left here: its last layer adds the encoder's rows and
        writes desc, and sage is None."""
        D, n_tot = self.config['descriptor_dim'], G["n_tot"]
        bf, f32 = torch.bfloat16, torch.float32
        x3, spl = P["x3"], P["x3"] and not P["ln"]            # spl: the keypoint encoder's hidden activations exist as SPL32 planes only
        A = lambda name, cols, dt: self._act(name, n_tot, cols, dt)                     # noqa: E731
        c1 = P["kenc_w1"].shape[0]
        wmax = max([D] + [e["n"] for e in P["sage"]])                                    # (one width per arena buffer: the widest layer that uses it)
        kmax = max([c1] + [e["n"] for e in P["kenc"]])
        early = G.get("early")                                  # the keypoint encoder ran before the synchronisation (_kenc_early): GraphSAGE only, its last layer adds it
        b = dict(hf0=A("sage_h0", wmax, f32), hf1=A("sage_h1", wmax, f32), agg=A("sage_agg", 2 * wmax, bf) if x3 else A("sage_agg", wmax, f32),
                 desc=A("desc", P["kenc"][-1]["n"], f32))
        if early is None:
            b.update(sage=A("sage_out", P["sage"][-1]["n"], f32), xk=A("kenc_x", c1, f32))
        if x3:
            b.update(hs0=A("sage_hs0", 2 * wmax, bf), hs1=A("sage_hs1", 2 * wmax, bf), dpl=A("dpl", 2 * D, bf))
        if early is None and spl:
            b.update(xs0=A("kenc_xs0", 2 * kmax, bf), xs1=A("kenc_xs1", 2 * kmax, bf))
        elif early is None:
            b.update(xf0=A("kenc_xf0", kmax, f32), xf1=A("kenc_xf1", kmax, f32))
        batch = dict(n=n_tot, feat=G["feat"].data_ptr(), ldf=G["feat"].stride(0), indptr=G["indptr_all"].data_ptr(), indices=G["indices_all"].data_ptr(),
                     kpts=G["kpts_all"].data_ptr(), norm3=G["norm3"].data_ptr(), seg=G["seg"].data_ptr())
        if early is not None:
            batch.update(kenc_all=early["out"].data_ptr(), src_row=early["src_row"].data_ptr())
        key = (P["gen"], early is not None) + tuple(t.data_ptr() for t in b.values())
        cache = self.__dict__.setdefault("_enc_cache", {})
        ent = cache.get(key)
        if ent is None:
            if len(cache) > 4:
                cache.clear()
            lst, slots = self._encoder_ops(P, b, G["feat"], batch, part="all" if early is None else "sage", early=early)
            ent = cache[key] = self._table(lst, (P, b), slots)
        self._patch(ent, batch)
        self._issue("encoder", ent, n_tot)
        return b.get("sage"), b["desc"]

    def _encoder_ops(self, P, b, feat, batch, part="all", early=None):
        """The launches of GraphSAGE (label 'sage') and the keypoint encoder ('kenc') on the arena buffers b, for the configuration of pack P:
        [(label, gims_op)], and the slots _encoder patches per call as (op, field, index | None, name in `batch`) -- an argument given here by its
        name in `batch` is such a slot.  part: 'all' -- both, the encoder's last layer adds `sage`; 'kenc' -- the encoder alone over whole images
        (_kenc_early: no residual, b['desc'] is its output); 'sage' -- GraphSAGE alone, its last layer adds the rows early['src_row'] of early['out']
        and writes desc (+ dpl)."""
        x3, ln, spl = P["x3"], P["ln"], P["x3"] and not P["ln"]
        lst, slots = [], []
        V = lambda t, cols: t[:, :cols]                                              # noqa: E731  (a view of the arena buffer with the layer's width)

        def aux(label, fn, ptrs, ints, floats=()):
            for field, args in (("p", ptrs), ("i", ints)):
                slots.extend((len(lst), field, j, a) for j, a in enumerate(args) if isinstance(a, str))
            lst.append((label, hip.op_aux(fn, [batch[a] if isinstance(a, str) else a for a in ptrs],
                                          [batch[a] if isinstance(a, str) else a for a in ints], floats)))

        def lin(label, e, a0, **kw):
            slots.append((len(lst), "m", None, "n"))
            if kw.get("residual_rows") is not None:
                slots.extend([(len(lst), "residual", None, "kenc_all"), (len(lst), "residual_rows", None, "src_row")])
            if feat is not None and a0 is feat:
                slots.extend([(len(lst), "a0", None, "feat"), (len(lst), "lda0", None, "ldf")])
            lst.append((label, self._lin_op(e, a0, **kw)))
        # GraphSAGE, per layer mean(h) over the neighbours and the GEMM on [h | mean(h)].  bf16x3: both operands as SPL32 planes (the producing
        # GEMM writes the planes of the next layer's h itself; the aggregation reads h in f32); f32: both in f32
        if part != "kenc":
            self._sage_ops(P, b, feat, aux, lin, V, early)
        if part != "sage":
            self._kenc_ops(P, b, aux, lin, V, part == "kenc")
        return lst, slots

    @staticmethod
    def _sage_ops(P, b, feat, aux, lin, V, early):
        x3 = P["x3"]
        dims = [feat.shape[1]] + [e["n"] for e in P["sage"]]                           # 256, 128, 128, 256
        h, ldh, hop = "feat", "ldf", feat
        if x3:
            aux("sage", hip.AUX_SPLIT_SPL32, ["feat", b["hs0"]], ["ldf", b["hs0"].stride(0), "n", dims[0]])
            hop = V(b["hs0"], 2 * dims[0])
        for i, e in enumerate(P["sage"]):
            last = i == len(P["sage"]) - 1
            aggv = V(b["agg"], (2 if x3 else 1) * dims[i])
            aux("sage", hip.AUX_SAGE_MEAN_SPLIT if x3 else hip.AUX_SAGE_MEAN, [h, "indptr", "indices", aggv], [ldh, "n", dims[i], aggv.stride(0)])
            if last and early is not None:     # sage + kenc: the encoder's rows of the kept keypoints as the residual
                lin("sage", e, hop, a1=aggv, act=hip.ACT_NONE, out=b["desc"], out_split=b.get("dpl"), residual=early["out"], residual_rows=early["src_row"])
                break
            h = b["sage"] if last else V(b["hf%d" % (i & 1)], dims[i + 1])
            hs = V(b["hs%d" % ((i + 1) & 1)], 2 * dims[i + 1]) if x3 and not last else None
            lin("sage", e, hop, a1=aggv, act=hip.ACT_NONE if last else hip.ACT_RELU, out=h, out_split=hs)
            ldh, hop = h.stride(0), hs if x3 else h

    def _kenc_ops(self, P, b, aux, lin, V, images):
        """images: the rows are whole images back to back (the batch's 'seg' holds their first rows, 'n_img' their number) and nothing is added."""
        ln, spl = P["ln"], P["x3"] and not P["ln"]
        # keypoint encoder: first layer on normalised coordinates, then the MLP (LayerNorm variant: conv -> norm kernel -> ReLU); the last layer
        # adds `sage` and writes desc (+ dpl)
        c1, xk = b["xk"].shape[1], b["xk"]
        aux("kenc", hip.AUX_KENC_FIRST_LINEAR if ln else hip.AUX_KENC_FIRST, ["kpts", "norm3", "seg", P["kenc_w1"], P["kenc_b1"], xk],
            [c1, "n"] + (["n_img"] if images else []))
        if ln:
            aux("kenc", *self._norm_args(xk, P["kenc_ln"][0], "n", out=xk))
        cur = xk
        if spl:
            aux("kenc", hip.AUX_SPLIT_SPL32, [xk, b["xs0"]], [xk.stride(0), b["xs0"].stride(0), "n", c1])
            cur = V(b["xs0"], 2 * c1)
        for i, e in enumerate(P["kenc"]):
            if i == len(P["kenc"]) - 1:
                if images:
                    lin("kenc", e, cur, out=b["desc"])
                else:
                    lin("kenc", e, cur, residual=b["sage"], out=b["desc"], out_split=b.get("dpl"))
            elif spl:
                cur, prev = V(b["xs%d" % ((i + 1) & 1)], 2 * e["n"]), cur
                lin("kenc", e, prev, act=hip.ACT_RELU, out_split=cur)
            else:
                cur, prev = V(b["xf%d" % (i & 1)], e["n"]), cur
                lin("kenc", e, prev, act=hip.ACT_NONE if ln else hip.ACT_RELU, out=cur)
                if ln:
                    aux("kenc", *self._norm_args(cur, P["kenc_ln"][i + 1], "n", out=cur))

    def _layers(self, P, desc, n_tot, max_nq, self_pr, cross_pr, guards, repeat):
        """The 18 attentional layers on the residual stream desc (and its SPL32 copy self._act('dpl')): their launches depend only on the buffer
        addresses, the batch geometry and the per-layer attention tiers, which repeat from call to call in steady state -- one cached table per
        such key.  guards, repeat: the mode of the call (_run_build).  Returns the accumulator the attention statistic of this batch went to (None:
        nothing was measured)."""
        cfg, D = self.config, self.config['descriptor_dim']
        x3 = P["x3"]
        if cfg['attention_precision'] not in ('auto', 'bf16', 'f16', 'bf16x3'):
            raise ValueError("attention_precision must be 'auto', 'bf16', 'f16' or 'bf16x3'")
        if cfg['attention_precision'] in ('f16', 'bf16x3') and not x3:
            raise ValueError(f"attention_precision='{cfg['attention_precision']}' needs linear_precision='bf16x3' (the 3-pass Q/K/V projection)")
        # per-layer choice of the attention kernel family (0 bf16, 1 half, 2 split-bf16) and, in 'auto' mode, the accumulator its
        # statistic goes to
        amode, stat = self._attention_modes(P, repeat)
        calibrated = self._tiers is not None and self._tiers.calibrated
        # the device-side verdict of 'auto' (see default_config): guarded redo launches behind every bf16 / half attention launch
        # (match_pairs returns without a host synchronisation: its verdict is drawn on the device, by guarded launches; forward() ends in one and
        # repeats the batch itself when the statistic it reads back there moved a layer up -- no extra launches on the latency path)
        guarded = stat is not None and cfg['attention_precision'] == 'auto' and calibrated and guards
        bf, f32 = torch.bfloat16, torch.float32
        A = lambda name, cols, dt: self._act(name, n_tot, cols, dt)                     # noqa: E731
        # bf16x3: all GEMM operands travel as split-bf16 SPL32 buffers written by the producing kernel's epilogue; only the residual stream `desc`
        # also exists in f32 (dpl: its SPL32 copy) -- and, with LayerNorm, the hidden activations in front of the norm kernel.  f32: all in f32.
        # msg: attention output, mrg: merged message (fuse_merge=False), hid: MLP hidden layer as the second conv reads it
        one_mlp = self._mlp_fused(P, n_tot)        # (then no hidden-layer buffer: it is part of the key through hid = None)
        self.linear_launches_per_layer = 2 if one_mlp else (3 if cfg['fuse_merge'] else 4)
        b = dict(desc=desc, src=A("dpl", 2 * D, bf) if x3 else desc, stat=stat, self_pr=self_pr, cross_pr=cross_pr,
                 msg=A("mpl", 2 * D, bf) if x3 else A("msg", D, f32), mrg=A("gpl", 2 * D, bf) if x3 else A("mrg", D, f32),
                 hid=None if one_mlp else (A("hpl", 4 * D, bf) if x3 else A("hid", 2 * D, f32)), hid_ln=A("hid_ln", 2 * D, f32) if (x3 and P["ln"]) else None,
                 # bf16 / half attention: Q|K|V as one 16-bit buffer [rows][768] (a layer writes and reads it in its own format); x3 attention (and the
                 # guarded redo): the same three matrices as SPL32 hi/lo planes
                 qkv_b=A("qkv", 3 * D, bf) if not all(a == 2 for a in amode) else None,
                 qkv_s=A("qkv6", 6 * D, bf) if (guarded or any(a == 2 for a in amode)) else None)
        key = (P["gen"], n_tot, max_nq) + tuple(0 if t is None else t.data_ptr() for t in b.values()) + (
            (float(cfg['attention_auto_threshold']), float(cfg['attention_auto_tail']), float(cfg['attention_f16_range']),
             float(cfg['attention_auto_rowmax'])) if guarded else None,
            self_pr.shape[0], cross_pr.shape[0], self._qkv_flags, tuple(amode))
        cache = self.__dict__.setdefault("_ops_cache", {})
        ent = cache.get(key)
        if ent is None:
            if len(cache) > 8:
                cache.clear()
            ent = cache[key] = self._table(self._layer_ops(P, b, n_tot, max_nq, amode, calibrated, guarded), (P, b))
        self._issue("layers", ent, n_tot)
        return stat

    def _layer_ops(self, P, b, n_tot, max_nq, amode, calibrated, guarded):
        """The launches of the attentional layers on the buffers b (see _layers) as [(label, gims_op)]: per layer the Q/K/V projection ('qkv'),
        the attention ('attn_self' | 'attn_cross'; both with a suffix that names the tier), for a guarded layer the two redo launches ('guard'),
        and the MLP with the residual update ('mlp': two launches, three with fuse_merge=False, one more with LayerNorm; ONE, hip.op_mlp,
        when the table has no hidden-layer buffer: b["hid"] is None, see _mlp_fused)."""
        cfg, D, H = self.config, self.config['descriptor_dim'], self._heads
        x3, ln, stat = P["x3"], P["ln"], b["stat"]
        desc, src, msg, mrg, hid, qkv_b, qkv_s = b["desc"], b["src"], b["msg"], b["mrg"], b["hid"], b["qkv_b"], b["qkv_s"]
        to = (lambda t: dict(out_split=t)) if x3 else (lambda t: dict(out=t))           # where a GEMM's result goes: SPL32 planes | f32
        lst = []
        for l, L in enumerate(P["layers"]):
            pr = b["cross_pr"] if L["cross"] else b["self_pr"]
            sfx = ("", "_f16", "_x3")[amode[l]]                  # stage-timer labels tell the attention kernels apart
            # (a settled split-bf16 layer is the top tier: nothing left to decide, nothing measured)
            st = None if (stat is None or (calibrated and amode[l] == 2)) else stat[l]
            # the half tier rounds the THREE-pass projection (f32 class) to half in the epilogue -- which also reports the operand range
            # (range_stat) instead of a scan of the Q | K | V buffer, 25 us per layer at 2 x 4096 x 8; the bf16 tier multiplies hi planes only
            if amode[l] == 2:
                qkv, qkv_out = qkv_s, dict(out_split=qkv_s)
            elif amode[l] == 1:
                qkv, qkv_out = qkv_b, dict(out_bf16=qkv_b, flags=hip.LINEAR_OUT_F16, range_stat=None if st is None else stat[l][H])
            else:
                qkv, qkv_out = qkv_b, (dict(out_bf16=qkv_b, flags=self._qkv_flags) if x3 else dict(out_bf16=qkv_b))
            lst.append(("qkv" + sfx, self._lin_op(L["qkv"], src, **qkv_out)))
            lst.append((("attn_cross" if L["cross"] else "attn_self") + sfx,
                        hip.op_attention(qkv, pr, max_nq, H, None if x3 else msg, 0, D, 2 * D, out_split=msg if x3 else None, q_prescaled=True,
                                         x3=amode[l] == 2, f16=amode[l] == 1, stat=st, no_range=amode[l] == 1)))
            if guarded and amode[l] != 2:      # the redo of this layer at split-bf16, launched always, executed only when the guard fires
                gd = (hip.attn_guard(stat[l], hip.GUARD_PEAKED, H, mean_thr=cfg['attention_auto_threshold'], tail_thr=cfg['attention_auto_tail'],
                                     max_thr=cfg['attention_auto_rowmax']) if amode[l] == 0
                      else hip.attn_guard(stat[l], hip.GUARD_RANGE, H, range_limit=cfg['attention_f16_range']))
                lst.append(("guard", self._lin_op(L["qkv"], src, out_split=qkv_s, guard=gd)))
                lst.append(("guard", hip.op_attention(qkv_s, pr, max_nq, H, None, 0, D, 2 * D, out_split=msg, q_prescaled=True, x3=True, guard=gd)))
            m, e0 = msg, L["mlp0_fused"]
            if hid is None:                    # desc += MLP([desc | message]) in one launch; dpl follows
                lst.append(("mlp", hip.op_mlp(src, msg, L["mlp_op"]["w"], L["mlp_op"]["b"], desc, src, residual=desc)))
                continue
            if e0 is None:                     # fuse_merge=False: the reference's operation order
                lst.append(("mlp", self._lin_op(L["merge"], msg, **to(mrg))))
                m, e0 = mrg, L["mlp0"]
            if ln:                             # LayerNorm between the two MLP convs: hidden activations in f32, normalised (+ split) by the norm kernel
                hf = b["hid_ln"] if x3 else hid
                lst.append(("mlp", self._lin_op(e0, src, a1=m, out=hf)))
                lst.append(("mlp", hip.op_aux(*self._norm_args(hf, L["ln"], n_tot, **to(hid)))))
            else:
                lst.append(("mlp", self._lin_op(e0, src, a1=m, act=hip.ACT_RELU, **to(hid))))
            lst.append(("mlp", self._lin_op(L["mlp1"], hid, residual=desc, out=desc, **(dict(out_split=src) if x3 else {}))))   # desc += delta (gmatcher.py:142)
        return lst

    def _ingest(self, raw):
        """raw: list of (kp (N,2), desc (D,N) channel-major, scores (N,), image shape).  ONE launch transposes the whole
        batch into point-major descriptors (no per-image torch ops); per-image views share the big buffers."""
        dev = raw[0][0].device
        D = self.config['descriptor_dim']
        ns = [int(r[0].shape[0]) for r in raw]
        offs = np.cumsum([0] + ns).tolist()
        tot = offs[-1]
        arena = self._buf("ingest", tot * (D + 3) * 4).view(torch.float32)
        de_all = arena[:tot * D].view(tot, D)
        kp_all = arena[tot * D:tot * (D + 2)].view(tot, 2)
        sc_all = arena[tot * (D + 2):tot * (D + 3)]
        items, keep = [], []
        for (kp, de, sc, _), n, off in zip(raw, ns, offs):
            kp = kp if (kp.dtype == torch.float32 and kp.is_contiguous()) else kp.to(torch.float32).contiguous()
            de = de if (de.dtype == torch.float32 and de.stride(1) == 1) else de.to(torch.float32).contiguous()
            sc = sc if (sc.dtype == torch.float32 and sc.is_contiguous()) else sc.to(torch.float32).contiguous()
            keep.append((kp, de, sc))
            items.append(hip.IngestImage(kp.data_ptr(), de.data_ptr(), de.stride(0), sc.data_ptr(), n, off))
        keep.append(hip.ingest_images(items, D, de_all, kp_all, sc_all))
        images = []
        for (_, _, _, shape), n, off in zip(raw, ns, offs):
            images.append({"kp": kp_all[off:off + n], "de": de_all[off:off + n], "sc": sc_all[off:off + n], "shape": tuple(shape)})
        images[0]["_keep"] = keep
        return images

    def sinkhorn_status(self):
        """Status word of every pair of the LAST batch of this lane (0 ok, 1 a marginal left the finite range -> that pair's
        matches are all -1); synchronises.  Status 2 (on-chip solve gave up) never survives a call: it is rescued inside."""
        uv, offs = self._last["outputs"][4], self._last["status_offs"]
        return uv[torch.from_numpy(offs).to(uv.device)].cpu().numpy()

    def _check_call(self, data, kwargs):
        if data.get('delaunay', False) and kwargs.get('mode', 'test') == "train":
            raise NotImplementedError("D-GIMS training (delaunay=True with mode='train') is not supported")
        if data['keypoints0'].device.type != "cuda":
            raise hip.GimsHipError("GMatcher runs on the GPU only (no CPU fallback): move the inputs to 'cuda'")

    # ------------------------------------------------------------------ reference-shaped forward (gmatcher.py:219-307)
    def forward(self, data, **kwargs):
        """gmatcher.py:219-307.  ``mode='train'`` on a module in train() mode is one differentiable training step (train.py:136:
        batch-statistics BatchNorm, running statistics updated, ``loss.backward()`` fills every parameter's .grad --
        gims_amd/trainstep.py); ``mode='train'`` on a module in eval() mode returns the forward value of the loss on running
        statistics, without a graph."""
        self._check_call(data, kwargs)
        if kwargs.get('mode', 'test') == "train" and self.training:
            from . import trainstep
            return trainstep.train_forward(self, data)
        if (kwargs.get('mode', 'test') == "train" and torch.is_grad_enabled() and not self.__dict__.get("_warned_eval_train")
                and any(p.requires_grad for p in self.parameters())):
            import warnings
            self.__dict__["_warned_eval_train"] = True
            warnings.warn("GMatcher.forward(mode='train') on a module in eval() mode returns the loss VALUE only (running-statistics BatchNorm, no "
                          "autograd graph): loss.backward() will raise.  Call model.train() first for a differentiable training step.", stacklevel=2)
        with hip.pinned_stream():                 # one stream lookup for the ~150 launches of a call
            return self._forward_eval(data, **kwargs)

    def _forward_once(self, data, B, radius, percentile, min_size, guards, last_attempt):
        """One pass of forward()'s batch up to its host synchronisation; guards: a repeat of the batch, run with the device-side guards.
        Returns the batch's results (_run_rest) and the pinned views of its kept-index lists, or None: the statistic this batch produced
        moved a layer of a SETTLED 'auto' table up -- the batch ran that layer on operands that did not suffice and the caller repeats it on
        the new table."""
        images = self._ingest([(data['keypoints' + side][b], data['descriptors' + side][b], data['scores' + side][b],
                                data['image' + side].shape) for b in range(B) for side in ("0", "1")])
        ctx = self._run_build(images, radius, percentile, min_size, delaunay=bool(data.get('delaunay', False)))
        ctx.update(guards=guards, repeat=guards)      # the same batch again: measured like the first attempt, its outlier rows counted once
        res = self._run_rest(ctx)
        items = res["items"]
        # what the host needs back -- the kept-index lists the reference returns as Python lists, and the Sinkhorn status words --
        # travels in asynchronous copies into one pinned buffer behind ONE stream synchronisation (three blocking read-backs cost
        # ~0.1 ms of a 5 ms single-pair call)
        n_int = sum(g["n_kept"] for g in images)
        pin = self.__dict__.get("_out_pin")
        if pin is None or pin.numel() < n_int + len(items):
            pin = self.__dict__["_out_pin"] = torch.empty(max(1 << 16, 2 * (n_int + len(items))), dtype=torch.int32, pin_memory=True)
        o, views = 0, []
        for g in images:
            v = pin[o:o + g["n_kept"]]
            v.copy_(g["kept"], non_blocking=True)
            views.append(v)
            o += g["n_kept"]
        uv = res["outputs"][4]
        st = pin[o:o + len(items)].view(torch.float32)
        for i, so in enumerate(res["status_offs"].tolist()):        # (an index tensor would be a pageable upload in the middle of the stream)
            st[i:i + 1].copy_(uv[so:so + 1], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        # 'auto' attention: the statistic of THIS batch is in (the first call's measurement decides the next call's kernels)
        moved = self._attention_stats_consume(self._lane, repeat=guards)
        rare = self._tiers is not None and self._tiers.rare_last and not guards
        if (moved or rare) and not last_attempt:
            return None
        if (st.numpy() == 2.0).any():        # cannot happen (rescued inside gims_sinkhorn_match); never return silently wrong
            raise hip.GimsHipError("the Sinkhorn solve of this batch gave up and was not rescued")
        return res, views

    def _forward_batch(self, data):
        """forward()'s batch: run it (twice where the 'auto' attention tiers ask for it), mutate `data` as the reference does, return its results."""
        radius, percentile, min_size = data.get('radius', 25), data.get('percentile', 7), data.get('min_size', 8)
        B = data['keypoints0'].shape[0]
        # forward() ends in a host synchronisation, so its 'auto' verdict is drawn THERE (no guarded launches on the latency path): a batch
        # whose statistic moves a settled layer up is repeated on the new table before anything is returned.  Tiers only move up, twice per
        # layer at most: the loop is short and a repeat is rare (a layer sharpening for the first time).
        for attempt in range(4):
            # the LAST attempt cannot be repeated: it runs with the device-side guards (like match_pairs), so a layer whose statistic moves up
            # once more inside it is redone at f32-class accuracy on the device -- no batch is ever returned from an under-precision tier
            # ... and so does every REPEAT: a repeat was asked for either by a layer that moved up (then the guards are idle) or by a sharply
            # peaked row inside a diffuse layer, which only the device-side redo answers (the layer is not moved up for one outlier)
            done = self._forward_once(data, B, radius, percentile, min_size, attempt >= 1, attempt == 3)
            if done is not None:
                break
            self._attn_forward_repeats = getattr(self, "_attn_forward_repeats", 0) + 1
        res, views = done
        # the reference's in-place dict mutation (gmatcher.py:244-252); torch.stack raises for ragged B>1, as there
        for s, side in enumerate(("0", "1")):
            gs = [res["images"][2 * b + s]["graph"] for b in range(B)]
            data['keypoints' + side] = _stack([h.ndata['point'] for h in gs])
            data['descriptors' + side] = _stack([h.ndata['feat'] for h in gs]).permute(0, 2, 1)
            data['scores' + side] = _stack([h.ndata['score'] for h in gs])
            data['kept_kpts%s_indices' % side] = [views[2 * b + s].tolist() for b in range(B)]
            data['graph' + side] = gs
        return res

    @torch.no_grad()
    def _forward_eval(self, data, **kwargs):
        res = self._forward_batch(data)
        items, pairs, mdesc = res["items"], res["pairs"], res["mdesc"]
        if kwargs.get('mode', 'test') == "train":        # gmatcher.py:254
            return self._forward_train(data, res["images"], items)
        md0 = _stack([mdesc[o0:o0 + n0] for (o0, n0), _ in pairs])
        md1 = _stack([mdesc[o1:o1 + n1] for _, (o1, n1) in pairs])
        return {
            'keypoints0': data['keypoints0'], 'keypoints1': data['keypoints1'],
            'descriptors0': data['descriptors0'], 'descriptors1': data['descriptors1'],
            'matches0': _stack([it["matches0"] for it in items]),
            'matches1': _stack([it["matches1"] for it in items]),
            'matching_scores0': _stack([it["mscores0"] for it in items]),
            'matching_scores1': _stack([it["mscores1"] for it in items]),
            'mdesc0': md0.squeeze(), 'mdesc1': md1.squeeze(),
        }

    def _forward_train(self, data, images, items):
        """Forward value of the reference's training loss (gmatcher.py:309-386) on the potentials the Sinkhorn kernels just
        produced: kept-index remap of data['matches'] (340-367), gather of the OT log-scores at the ground-truth cells --
        negatives read the corner cell OT[N, M], the reference's scores[b, -1, -1] (368-372) --, clamp, scatter_mean per
        batch element, weights (373-385).  Returns (loss, pos_loss, neg_loss) as 0-dim tensors.  This is the eval()-mode
        value (running-statistics BatchNorm) and carries no autograd graph -- .backward() on it raises, it does not silently
        no-op; the differentiable training step (train() mode: batch statistics, full reverse pass on the HIP path) is
        gims_amd/trainstep.py, which forward() routes to when the module is in train() mode."""
        gt = data['matches']
        dev = images[0]["kp"].device
        gt = gt.to(device=dev, dtype=torch.int64).contiguous()
        B = len(items)
        out3, _ = hip.train_loss(items, [images[2 * b]["kept"] for b in range(B)], [images[2 * b + 1]["kept"] for b in range(B)], gt,
                                 self._packed(dev)["alpha"], self.config['pos_loss_weight'], self.config['neg_loss_weight'])
        return out3[0], out3[1], out3[2]

    @torch.no_grad()
    def loss_and_score_gradients(self, data):
        """``forward(data, mode='train')`` plus the first stage of its backward pass: the gradient of the loss
        with respect to the score matrix of every pair and to ``bin_score``, by reverse mode through the unrolled Sinkhorn
        iterations (what autograd does in the reference, gmatcher.py:41-69, 372-385).  Returns
        ``{'loss', 'pos_loss', 'neg_loss', 'dscores': [per pair, (n_kept0, n_kept1)], 'dbin_score'}``.  A diagnostic of the
        Sinkhorn reverse sweep for a module in eval() mode; the complete backward pass (final projection, attention layers,
        encoders, GraphSAGE) is the training step of gims_amd/trainstep.py (``model.train(); model(data, mode='train')``)."""
        res = self._forward_batch(data)
        items = res["items"]
        loss, pos, neg = self._forward_train(data, res["images"], items)
        dscores, dalpha = hip.sinkhorn_score_gradients(items, self._packed(items[0]["scores"].device)["alpha"], self.config['sinkhorn_iterations'],
                                                       self.config['pos_loss_weight'], self.config['neg_loss_weight'], hip.train_loss.last)
        return {"loss": loss, "pos_loss": pos, "neg_loss": neg, "dscores": dscores, "dbin_score": dalpha}

    # ------------------------------------------------------------------ ragged batch of independent pairs
    @torch.no_grad()
    def match_pairs(self, datas: List[dict], *, per_pair_graph=False, **kwargs):
        """Throughput API: a list of single-pair dicts (each exactly what ``forward`` takes with B == 1) is
        matched in ONE batched pass even when every pair keeps a different number of keypoints (the reference's
        ``forward`` can only stack equal-sized pairs, gmatcher.py:244-249).  Each dict is mutated like ``forward``
        does and a list of per-pair result dicts (same keys as ``forward``) is returned.

        All pairs of a call share radius / percentile / min_size and ``delaunay`` (ValueError otherwise) unless
        ``per_pair_graph=True``: then every dict's own values (defaults 25 / 7 / 8, False) are honoured inside the same single pass --
        the graph build takes its parameters per image (gims_agc_build with one gims_agc_params each), the Delaunay pairs go through one Delaunay build."""
        tm0 = time.perf_counter()
        n_lanes = int(self.config.get('streams', 1))
        if n_lanes < 2 or len(datas) < 2 * n_lanes:
            n_lanes = 1
        cuts = [round(i * len(datas) / n_lanes) for i in range(n_lanes + 1)]
        groups = [datas[cuts[i]:cuts[i + 1]] for i in range(n_lanes)]
        for data in datas:
            self._check_call(data, kwargs)
            if data['keypoints0'].shape[0] != 1:
                raise ValueError("match_pairs takes single-pair dicts (B == 1)")
        d0 = datas[0]
        params = (d0.get('radius', 25), d0.get('percentile', 7), d0.get('min_size', 8))
        for i, data in enumerate(() if per_pair_graph else datas):        # one graph-build launch serves the whole batch: its parameters are the batch's
            if (data.get('radius', 25), data.get('percentile', 7), data.get('min_size', 8)) != params:
                raise ValueError(f"match_pairs: pair {i} asks for radius / percentile / min_size = "
                                 f"{(data.get('radius', 25), data.get('percentile', 7), data.get('min_size', 8))}, pair 0 for {params}; "
                                 "all pairs of one call share the adaptive-graph parameters (call match_pairs once per setting)")
        delaunay = bool(d0.get('delaunay', False))
        for i, data in enumerate(() if per_pair_graph else datas):
            if bool(data.get('delaunay', False)) != delaunay:
                raise ValueError(f"match_pairs: pair {i} asks for delaunay={bool(data.get('delaunay', False))}, pair 0 for delaunay={delaunay}; "
                                 "all pairs of one call share the graph construction (call match_pairs once per setting)")
        cur = torch.cuda.current_stream()
        if n_lanes > 1:
            # independent sub-batches on separate HIP streams: the HBM-bound stages of one lane (Sinkhorn, epilogues) overlap
            # the MFMA-bound stages of the other, and the host sync of one lane's graph build hides behind the other's work
            lanes = self.__dict__.setdefault("_lanes", {}).setdefault((cur.device, n_lanes), [torch.cuda.Stream() for _ in range(n_lanes)])
            for L in lanes:
                L.wait_stream(cur)
        else:
            lanes = [cur]
        try:
            ctxs = []
            for gi, grp in enumerate(groups):
                with torch.cuda.stream(lanes[gi]), hip.pinned_stream():
                    self._lane = gi
                    raw = [(data['keypoints' + side][0], data['descriptors' + side][0], data['scores' + side][0], data['image' + side].shape)
                           for data in grp for side in ("0", "1")]
                    each = [self._graph_setting(data) for data in grp for _ in ("0", "1")] if per_pair_graph else None
                    ctxs.append(self._run_build(self._ingest(raw), *params, delaunay=delaunay, each=each))
                    # no host synchronisation at the end of this call: the 'auto' verdict is drawn on the device.  Stream lanes run concurrently,
                    # and the on-chip Sinkhorn kernels need every CU of the device to themselves: next to another lane's kernels they cannot get
                    # their workgroups co-resident, give up and fall to the slow rescue -- so such a call plans the streamed kernels up front
                    ctxs[gi].update(guards=True, streamed=n_lanes > 1)
            tm1 = time.perf_counter()
            outs, flats = [], []
            for gi, grp in enumerate(groups):
                with torch.cuda.stream(lanes[gi]), hip.pinned_stream():
                    self._lane = gi
                    res = self._run_rest(ctxs[gi])
                    items, pairs, mdesc, images = res["items"], res["pairs"], res["mdesc"], res["images"]
                    flats.append(res["flat"])
                    if n_lanes > 1:
                        for t_ in res["outputs"]:
                            t_.record_stream(cur)
                    for p, (data, it) in enumerate(zip(grp, items)):
                        for s, side in enumerate(("0", "1")):
                            g = images[2 * p + s]["graph"]
                            data['keypoints' + side] = g.ndata['point'][None]
                            data['descriptors' + side] = g.ndata['feat'].t()[None]
                            data['scores' + side] = g.ndata['score'][None]
                            data['kept_kpts%s_indices' % side] = [images[2 * p + s]["kept"]]      # device tensor (no host sync here)
                            data['graph' + side] = [g]
                        (o0, n0), (o1, n1) = pairs[p]
                        outs.append({
                            'keypoints0': data['keypoints0'], 'keypoints1': data['keypoints1'],
                            'descriptors0': data['descriptors0'], 'descriptors1': data['descriptors1'],
                            'matches0': it["matches0"][None], 'matches1': it["matches1"][None],
                            'matching_scores0': it["mscores0"][None], 'matching_scores1': it["mscores1"][None],
                            'mdesc0': mdesc[o0:o0 + n0], 'mdesc1': mdesc[o1:o1 + n1],
                        })
        finally:
            self._lane = 0          # (_buf hands out the scratch arena of the current lane)
        if n_lanes > 1:
            for L in lanes:
                cur.wait_stream(L)
        tm2 = time.perf_counter()
        outs = PairResults(outs)
        outs.flat = flats
        self.n_lanes_last = n_lanes
        if self._timers is not None:
            self._timers.setdefault("_host_marks", []).append((None, None, (1e3 * (tm1 - tm0), 1e3 * (tm2 - tm1), 1e3 * (time.perf_counter() - tm2),
                                                                            getattr(self, "_sync_ms", 0.0))))
        return outs

    @staticmethod
    def _graph_setting(s):
        """(radius, percentile, min_size, delaunay) of a data dict or of one entry of a sweep's grid (a triple, or a dict that may carry
        ``delaunay``); the defaults are forward()'s."""
        if isinstance(s, dict):
            return (s.get('radius', 25), s.get('percentile', 7), s.get('min_size', 8), bool(s.get('delaunay', False)))
        radius, percentile, min_size = s
        return (radius, percentile, min_size, False)

    # ------------------------------------------------------------------ image sets: encode each image once, match many pairs
    @torch.no_grad()
    def encode_images(self, images: List[dict], *, radius=25, percentile=7, min_size=8, delaunay=False, each=None) -> List[ImageFeatures]:
        """Everything of a match that belongs to ONE image -- graph build, kept-keypoint compaction, GraphSAGE, keypoint encoder -- for a list
        of images in one batched pass.  ``images``: dicts ``{'keypoints': (1, N, 2) | (N, 2), 'descriptors': (1, 256, N) |
        (256, N), 'scores': (1, N) | (N,), 'image': anything with the image's .shape}`` -- what a front end returns per image, plus the image;
        any number of them.  ``each``: one ``(radius, percentile, min_size[, delaunay])`` per image instead of the four keyword values.
        Returns one ``ImageFeatures`` per image, in order, for ``match_features``; they are valid for the current weights.  One host
        synchronisation (the kept counts).  An image that keeps nothing raises ``ValueError`` like ``forward``.  Evaluation only."""
        if self.training:
            raise NotImplementedError("encode_images serves evaluation only: call model.eval() first (training runs through forward(mode='train'))")
        if not images:
            raise ValueError("encode_images: the image list is empty")
        if each is not None:
            if len(each) != len(images):
                raise ValueError(f"encode_images: each holds {len(each)} settings for {len(images)} images")
            each = [self._graph_setting(e) if isinstance(e, dict) or len(e) == 3 else (e[0], e[1], e[2], bool(e[3])) for e in each]
        raw = []
        for k, im in enumerate(images):
            kp, de, sc = im['keypoints'], im['descriptors'], im['scores']
            kp, de, sc = (kp[0] if kp.dim() == 3 else kp), (de[0] if de.dim() == 3 else de), (sc[0] if sc.dim() == 2 else sc)
            if kp.device.type != "cuda":
                raise hip.GimsHipError("GMatcher runs on the GPU only (no CPU fallback): move the inputs to 'cuda'")
            if kp.dim() != 2 or kp.shape[1] != 2 or de.dim() != 2 or de.shape[1] != kp.shape[0] or sc.shape != (kp.shape[0],):
                raise ValueError(f"encode_images: image {k}: keypoints {tuple(kp.shape)}, descriptors {tuple(de.shape)} and scores {tuple(sc.shape)} "
                                 "are not (N, 2), (256, N) and (N,)")
            raw.append((kp, de, sc, tuple(im['image'].shape)))
        with hip.pinned_stream():
            ctx = self._run_build(self._ingest(raw), radius, percentile, min_size, delaunay=bool(delaunay), each=each)
            while True:
                ctx["kenc_early"] = True            # the encoder stage in the order _run_rest gives it
                G = self._gather(ctx)
                if G is not None:
                    break
                ctx = self._run_build(ctx["images"], *ctx["params"], delaunay=bool(ctx.get("delaunay")), each=ctx.get("each"))
            batch = ctx["images"]
            P = self._packed(batch[0]["kp"].device)
            _, desc = self._encoder(P, G)
            with GMatcher._Stage(self, "store"):
                encoded = desc.clone()               # out of the lane arena: the next call overwrites it, and the layers update it in place
            self._finish_graphs(batch, G)
        owner = weakref.ref(self)
        feats = []
        for k, g in enumerate(batch):
            ro, nk = g["rows"]
            h = g["graph"]
            feats.append(ImageFeatures(keypoints=h.ndata["point"], descriptors=h.ndata["feat"], scores=h.ndata["score"], kept=g["kept"], graph=h,
                                       encoded=encoded[ro:ro + nk], n=nk, n_edges=g["n_edges"], shape=g["shape"],
                                       setting=tuple(each[k]) if each is not None else (radius, percentile, min_size, bool(delaunay)),
                                       gen=P["gen"], _owner=owner))
        return feats

    @torch.no_grad()
    def match_features(self, feats: List[ImageFeatures], pairs) -> PairResults:
        """Match the index pairs ``pairs = [(i, j), ...]`` over the encoded images ``feats`` (``encode_images``) in ONE batched pass: the batch
        has the layout ``match_pairs`` gives the same pairs in the same order, its residual stream is filled from the features by one
        launch (hip.assemble_rows; every entry gets its own copy of its images' rows, the layers update them in place), and the layers,
        scores, Sinkhorn and selection run as they do there -- the results are bit for bit ``match_pairs``'.  ``i == j`` is allowed.  No
        graph build, no encoder, and no host synchronisation on this call's work (with ``attention_precision='auto'`` the call folds in
        the statistic of the PREVIOUS batch like every batch does, which waits for that batch's read-back).

        Returns the ``PairResults`` of ``match_pairs`` (``keypoints0/1`` and ``descriptors0/1`` are views of the features; ``.flat`` as
        there) with ``.datas``: per pair a dict shaped like the one ``match_pairs`` leaves behind (kept keypoints, descriptors, scores,
        ``kept_kpts0/1_indices``, ``graph0/1``, ``image0/1`` as objects with the image's ``.shape``), for ``verify_pairs``,
        ``evalh.evaluate_pairs`` and ``shard.pair_stats``.  ``ValueError``: an empty pair list, an index out of range, features of another
        device, of another matcher, or of other weights (after ``load_state_dict`` / ``.to()``)."""
        if self.training:
            raise NotImplementedError("match_features serves evaluation only: call model.eval() first")
        feats = list(feats)
        pairs = [(int(i), int(j)) for i, j in pairs]
        if not pairs:
            raise ValueError("match_features: the pair list is empty")
        for p, (i, j) in enumerate(pairs):
            if not (0 <= i < len(feats) and 0 <= j < len(feats)):
                raise ValueError(f"match_features: pair {p} = ({i}, {j}) has an index out of range (there are {len(feats)} images)")
        used = sorted({k for pr in pairs for k in pr})
        dev = feats[used[0]].device
        for k in used:
            f = feats[k]
            if not isinstance(f, ImageFeatures):
                raise TypeError(f"match_features: feats[{k}] is {type(f).__name__}, not ImageFeatures")
            if f.device != dev or dev.index != torch.cuda.current_device():
                raise ValueError(f"match_features: feats[{k}] lives on another device ({f.device}) than the batch runs on "
                                 f"(cuda:{torch.cuda.current_device()}, with feats[{used[0]}] on {dev})")
            if f._owner() is not self:
                raise ValueError(f"match_features: feats[{k}] was encoded by another matcher")
        D = self.config['descriptor_dim']
        St = lambda name: GMatcher._Stage(self, name)   # noqa: E731
        with hip.pinned_stream():
            self._lane = 0
            P = self._packed(dev)
            for k in used:
                if feats[k].gen != P["gen"]:
                    raise ValueError(f"match_features: feats[{k}] was encoded with weight generation {feats[k].gen}, the matcher now holds "
                                     f"generation {P['gen']} (the weights changed or moved): encode the images again")
            rows, segs, o = [], [], 0
            for i, j in pairs:
                ni, nj = feats[i].n, feats[j].n
                rows.append(((o, ni), (o + ni, nj)))
                segs += [(feats[i].encoded, o), (feats[j].encoded, o + ni)]
                o += ni + nj
            n_tot = o
            desc = self._act("desc", n_tot, D, torch.float32)
            dpl = self._act("dpl", n_tot, 2 * D, torch.bfloat16) if P["x3"] else None
            with St("assemble"):
                table = hip.assemble_rows(segs, desc, dpl, D)
            res = self._last = self._match_rows(P, desc, n_tot, rows, max(feats[k].n for k in used), dict(guards=True))
            res.update(images=[], table=table, dropped=[], repeats=0)
        outs, datas = [], []
        for (i, j), it, ((o0, n0), (o1, n1)) in zip(pairs, res["items"], rows):
            data = {}
            for side, f in (("0", feats[i]), ("1", feats[j])):
                data['keypoints' + side] = f.keypoints[None]
                data['descriptors' + side] = f.descriptors.t()[None]
                data['scores' + side] = f.scores[None]
                data['kept_kpts%s_indices' % side] = [f.kept]
                data['graph' + side] = [f.graph]
                data['image' + side] = _ImageShape(f.shape)
            datas.append(data)
            outs.append({
                'keypoints0': data['keypoints0'], 'keypoints1': data['keypoints1'],
                'descriptors0': data['descriptors0'], 'descriptors1': data['descriptors1'],
                'matches0': it["matches0"][None], 'matches1': it["matches1"][None],
                'matching_scores0': it["mscores0"][None], 'matching_scores1': it["mscores1"][None],
                'mdesc0': res["mdesc"][o0:o0 + n0], 'mdesc1': res["mdesc"][o1:o1 + n1],
            })
        outs = PairResults(outs)
        outs.flat = [res["flat"]]
        outs.datas = datas
        return outs

    # ------------------------------------------------------------------ one pair under a grid of graph parameters
    @torch.no_grad()
    def sweep(self, data, grid, *, rows=None, outputs="all", verify=None):
        """One image pair matched under every graph setting of ``grid`` (what the reference's tools/parameter_search.py does with one
        ``forward`` per setting).  ``data``: a single-pair dict as ``forward`` takes it (B == 1; not mutated).  ``grid``: an iterable of
        ``(radius, percentile, min_size)`` triples or of dicts with those keys that may also carry ``delaunay``.

        The two images are ingested ONCE; every setting is an entry of a batch whose images point at the same keypoint / descriptor /
        score buffers, and the entries run like the pairs of ``match_pairs(per_pair_graph=True)``, in sub-batches of at most
        ``rows`` keypoint rows (default ``config['sweep_rows']``) and ``config['sweep_workspace_mb']`` of graph-build workspace.  One
        host synchronisation per sub-batch (the kept counts), none per setting.

        Returns one record per setting, in grid order: ``radius, percentile, min_size, delaunay, kept0, kept1`` (host numbers),
        ``n_matches`` (a 0-dim device tensor: ``(matches0 > -1).sum()``), ``error`` (None) and ``result``: the per-pair dict of
        ``match_pairs`` plus ``kept_kpts0_indices`` / ``kept_kpts1_indices`` (device tensors; ``outputs='matches'`` leaves out keypoints,
        descriptors and mdesc, which are 16 MB per setting at 2 x 4096).  A setting under which an image keeps nothing does not raise
        (``forward`` and ``match_pairs`` do, like the reference): its record has ``error='ValueError: need at least one array to
        concatenate'``, ``kept0 = kept1 = 0``, ``n_matches = 0`` and ``result=None``, the way parameter_search.py writes such a row.

        ``verify``: None, or a dict with any of ``thresh``, ``iters``, ``lo_iters``, ``seed``, ``model`` (the keywords of
        ``gims_amd.verify.verify_pairs``).  When given, every record also carries ``correct_matches`` (a 0-dim device tensor: the inliers of
        the verified homography, the quantity parameter_search.py:161-165 records), ``homography`` [3, 3] and ``inlier`` [kept0] uint8 -- one
        ``verify_pairs`` call per sub-batch, no extra host synchronisation; ``0 / None / None`` on a record with ``error``.  With
        ``model='fundamental'`` (a camera that moved through a 3-D scene) the inliers are those of the fundamental matrix and the record
        carries it as ``fundamental`` in place of ``homography``.  With ``model='pose'`` and ``intrinsics=(K0, K1)`` (calibrated cameras)
        the inliers are those of the essential matrix, carried as ``essential``, and the record also has the relative pose ``R`` [3, 3]
        and ``t`` [3] (``gims_amd.verify.verify_pairs``)."""
        if verify is not None and (not isinstance(verify, dict) or set(verify) - {"thresh", "iters", "lo_iters", "seed", "model", "intrinsics"}):
            raise ValueError("verify must be None or a dict with keys among thresh, iters, lo_iters, seed, model, intrinsics")
        vmodel = verify.get("model", "homography") if verify is not None else "homography"
        if isinstance(vmodel, bool) or vmodel not in ("homography", "fundamental", "pose", 0, 1, 3):
            raise ValueError("verify['model'] must be 'homography', 'fundamental' or 'pose'")
        vpose = vmodel in ("pose", 3)
        if verify is not None and vpose != (verify.get("intrinsics") is not None):
            raise ValueError("verify['intrinsics'] = (K0, K1) goes with verify['model'] = 'pose', and only with it")
        vkey = "essential" if vpose else "fundamental" if vmodel in ("fundamental", 1) else "homography"
        self._check_call(data, {})
        if data['keypoints0'].shape[0] != 1:
            raise ValueError("sweep takes one single-pair dict (B == 1)")
        if outputs not in ("all", "matches"):
            raise ValueError("outputs must be 'all' or 'matches'")
        settings = [self._graph_setting(s) for s in grid]
        if not settings:
            return []
        cfg = self.config
        records = [None] * len(settings)
        stats = self.sweep_stats_last = dict(settings=len(settings), ingests=0, sub_batches=0, build_repeats=0)
        with hip.pinned_stream():
            base = self._ingest([(data['keypoints' + side][0], data['descriptors' + side][0], data['scores' + side][0], data['image' + side].shape)
                                 for side in ("0", "1")])
            stats["ingests"] += 1
            dev = base[0]["kp"].device
            n_rows = base[0]["kp"].shape[0] + base[1]["kp"].shape[0]
            per = max(1, int(rows if rows is not None else cfg['sweep_rows']) // max(n_rows, 1))     # a pair without keypoints: the build's check speaks
            if min(g["kp"].shape[0] for g in base) >= 2 and not all(s[3] for s in settings):
                # the workspace of one entry's two images (the slots are never written by this call: it only sizes)
                z = torch.empty(8, dtype=torch.int32, device=dev)
                one = hip.agc_workspace_bytes(hip.make_agc_images([dict(kpts=g["kp"], desc=g["de"], kept=z, indptr=z, indices=z, info=z) for g in base]), 0)
                per = max(1, min(per, (int(cfg['sweep_workspace_mb']) << 20) // max(one, 1)))
            for c0 in range(0, len(settings), per):
                chunk = settings[c0:c0 + per]
                images = [dict(kp=g["kp"], de=g["de"], sc=g["sc"], shape=g["shape"]) for _ in chunk for g in base]
                ctx = self._run_build(images, None, None, None, each=[s for s in chunk for _ in (0, 1)])
                ctx.update(skip_empty=True, guards=True)      # as in match_pairs: no host synchronisation at the end, the 'auto' verdict is drawn on the device
                out = self._run_rest(ctx)
                items, pairs, mdesc = out["items"], out["pairs"], out["mdesc"]
                stats["sub_batches"] += 1
                stats["build_repeats"] += out["repeats"]
                images, dropped = out["images"], set(out["dropped"])
                if items:       # matches per entry: one segmented count for the sub-batch
                    m0_all = out["flat"]["matches0"]
                    ends = np.cumsum(out["flat"]["n0"], dtype=np.int64)
                    csum = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), (m0_all > -1).cumsum(0)])
                    n_matches = csum[hip.upload(ends, dev)] - csum[hip.upload(ends - np.asarray(out["flat"]["n0"], dtype=np.int64), dev)]
                p = 0
                live = []
                for j, (radius, percentile, min_size, delaunay) in enumerate(chunk):
                    rec = dict(radius=radius, percentile=percentile, min_size=min_size, delaunay=delaunay, kept0=0, kept1=0, n_matches=0,
                               error=None, result=None)
                    if verify is not None:
                        rec.update({'correct_matches': 0, vkey: None, 'inlier': None})
                        if vpose:
                            rec.update({'R': None, 't': None})
                    records[c0 + j] = rec
                    if j in dropped:
                        rec["error"] = "ValueError: need at least one array to concatenate"
                        continue
                    g0, g1, it = images[2 * p], images[2 * p + 1], items[p]
                    (o0, n0), (o1, n1) = pairs[p]
                    rec.update(kept0=n0, kept1=n1, n_matches=n_matches[p])
                    res = {'matches0': it["matches0"][None], 'matches1': it["matches1"][None],
                           'matching_scores0': it["mscores0"][None], 'matching_scores1': it["mscores1"][None],
                           'kept_kpts0_indices': [g0["kept"]], 'kept_kpts1_indices': [g1["kept"]]}
                    if outputs == "all":
                        res.update({'keypoints0': g0["graph"].ndata['point'][None], 'keypoints1': g1["graph"].ndata['point'][None],
                                    'descriptors0': g0["graph"].ndata['feat'].t()[None], 'descriptors1': g1["graph"].ndata['feat'].t()[None],
                                    'mdesc0': mdesc[o0:o0 + n0], 'mdesc1': mdesc[o1:o1 + n1]})
                    rec["result"] = res
                    live.append((rec, g0["graph"].ndata['point'][None], g1["graph"].ndata['point'][None]))
                    p += 1
                if verify is not None and live:
                    from .verify import verify_pairs
                    v = verify_pairs([dict(keypoints0=k0, keypoints1=k1) for _, k0, k1 in live],
                                     [{'matches0': r["result"]['matches0']} for r, _, _ in live], **verify)
                    col = hip.VERIFY_FIELDS.index("n_inliers")
                    for q, (rec, _, _) in enumerate(live):
                        rec.update({'correct_matches': v["records"][q, col], vkey: v["models"][q], 'inlier': v["inlier"][q]})
                        if vpose:
                            rec.update({'R': v["R"][q], 't': v["t"][q]})
        return records
