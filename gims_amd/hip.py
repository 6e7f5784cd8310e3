"""ctypes binding of libgims_hip.so (C ABI declared in include/gims_hip.h).

PyTorch is plumbing only: tensors own the device memory, ``torch.cuda.current_stream()`` provides the
hipStream_t.  There is NO CPU fallback: if the shared library is missing or a call fails this module
raises -- the product path never routes around the HIP kernels.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import threading

import numpy as np
import torch

from . import _abi
from ._abi import GimsHipError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgims_hip.so")

ABI = _abi.parse()          # include/gims_hip.h as ctypes: every struct, prototype and `#define GIMS_X <int>` below comes from it
_K = ABI.constants
EXPORTS = tuple(ABI.signatures)
ABI_VERSION = _K["GIMS_ABI_VERSION"]
GIMS_OK, GIMS_EINVAL, GIMS_EHIP, GIMS_ENUMERIC = _K["GIMS_OK"], _K["GIMS_EINVAL"], _K["GIMS_EHIP"], _K["GIMS_ENUMERIC"]

PREC_F32, PREC_BF16X3, PREC_BF16X6 = _K["GIMS_PREC_F32"], _K["GIMS_PREC_BF16X3"], _K["GIMS_PREC_BF16X6"]
LINEAR_UPPER = _K["GIMS_LINEAR_UPPER"]
LINEAR_HI_ONLY = _K["GIMS_LINEAR_HI_ONLY"]
LINEAR_OUT_F16 = _K["GIMS_LINEAR_OUT_F16"]      # out_bf16 receives IEEE half (saturated) instead of bf16
ACT_NONE, ACT_RELU = _K["GIMS_ACT_NONE"], _K["GIMS_ACT_RELU"]

# The structs of the header under their Python names; every pointer member is a c_void_p (an address, or None).
AttnGuard = ABI.structs["gims_attn_guard"]      # a launch that only runs when the statistic of the launch before it asks for the redo
LinearArgs = ABI.structs["gims_linear_args"]
AttnArgs = ABI.structs["gims_attn_args"]
AuxArgs = ABI.structs["gims_aux_args"]          # one of the small kernels as an op of gims_run_ops (fn = AUX_*; p / i / f: its arguments)
Op = ABI.structs["gims_op"]
AgcImage = ABI.structs["gims_agc_image"]
AgcParams = ABI.structs["gims_agc_params"]
PackImage = ABI.structs["gims_pack_image"]
IngestImage = ABI.structs["gims_ingest_image"]
OtProblem = ABI.structs["gims_ot_problem"]
PyrLevel = ABI.structs["gims_pyr_level"]
SiftInfo = ABI.structs["gims_sift_info"]        # what gims_sift_layout reports for one image size
LossPair = ABI.structs["gims_loss_pair"]
Gemm = ABI.structs["gims_gemm"]
TrainAttnProblem = ABI.structs["gims_train_attn_problem"]
TrainAttnArgs = ABI.structs["gims_train_attn_args"]
Segments = ABI.structs["gims_segments"]
AdamTensor = ABI.structs["gims_adam_tensor"]
AdamGroup = ABI.structs["gims_adam_group"]
SgdTensor = ABI.structs["gims_sgd_tensor"]
SgdGroup = ABI.structs["gims_sgd_group"]
EmaTensor = ABI.structs["gims_ema_tensor"]
EvalPair = ABI.structs["gims_eval_pair"]
VerifySet = ABI.structs["gims_verify_set"]      # one set of correspondences for gims_verify_pairs
LabelPair = ABI.structs["gims_label_pair"]
NnPair = ABI.structs["gims_nn_pair"]
AugPlan = ABI.structs["gims_aug_plan"]          # one image's colour augmentation

GUARD_PEAKED, GUARD_RANGE = _K["GIMS_GUARD_PEAKED"], _K["GIMS_GUARD_RANGE"]
AUX_SPLIT_SPL32, AUX_SAGE_MEAN_SPLIT, AUX_KENC_FIRST = _K["GIMS_AUX_SPLIT_SPL32"], _K["GIMS_AUX_SAGE_MEAN_SPLIT"], _K["GIMS_AUX_KENC_FIRST"]
AUX_SAGE_MEAN, AUX_KENC_FIRST_LINEAR, AUX_LAYERNORM_ACT = _K["GIMS_AUX_SAGE_MEAN"], _K["GIMS_AUX_KENC_FIRST_LINEAR"], _K["GIMS_AUX_LAYERNORM_ACT"]
AUX_SIFT_DESCRIBE = _K["GIMS_AUX_SIFT_DESCRIBE"]     # SIFT descriptors: reached through gims_run_ops only (no entry point of its own)
AUX_DIOU_NMS = _K["GIMS_AUX_DIOU_NMS"]               # DIoU-NMS keypoint thinning: likewise
AUX_ASSEMBLE_ROWS = _K["GIMS_AUX_ASSEMBLE_ROWS"]     # desc / dpl of a batch of pairs from per-image stores of encoded rows: likewise
AUX_BUILD_TRACKS = _K["GIMS_AUX_BUILD_TRACKS"]       # multi-view tracks from the matches of an image set: likewise
TRACKS_TABLE_WORDS, TRACKS_KEEP_CONFLICTING = _K["GIMS_TRACKS_TABLE_WORDS"], _K["GIMS_TRACKS_KEEP_CONFLICTING"]
TRACKS_SCAN_TILE = _K["GIMS_TRACKS_SCAN_TILE"]           # elements per workgroup of the op's scans: N around its multiples are the seams
TRACKS_SHORT_SEGMENT = _K["GIMS_TRACKS_SHORT_SEGMENT"]   # components up to this size are ranked by one lane, larger ones by a wave
TRACKS_LONG_SEGMENT = _K["GIMS_TRACKS_LONG_SEGMENT"]     # ... and above max(this, N / 1024) -- tracks_huge(N) -- by a prefix count over the nodes
TRACKS_COUNTERS = ("n_tracks", "n_obs", "n_conflicting", "n_edges", "n_bad", "status")      # the first words of the op's int32 [8] counters
AUX_TRIANGULATE_TRACKS = _K["GIMS_AUX_TRIANGULATE_TRACKS"]   # robust multi-view triangulation of tracks from known cameras: likewise
TRI_CAMERA_WORDS, TRI_MAX_OBS = _K["GIMS_TRI_CAMERA_WORDS"], _K["GIMS_TRI_MAX_OBS"]
TRI_SHORT_TRACK = _K["GIMS_TRI_SHORT_TRACK"]             # tracks up to this length are served by that many lanes, up to 64 by a wave: the seams
TRI_COUNTERS = ("n_ok", "n_low_angle", "n_no_model", "n_too_short", "n_too_long", "n_bad_obs", "n_inlier_obs")
TRI_TOO_SHORT, TRI_NO_MODEL, TRI_LOW_ANGLE, TRI_TOO_LONG = 1, 2, 4, 8      # the bits of the op's per-track status
AUX_RESECT_IMAGES = _K["GIMS_AUX_RESECT_IMAGES"]             # absolute poses from 2-D to 3-D matches (resection): likewise
RESECT_CAMERA_WORDS = _K["GIMS_RESECT_CAMERA_WORDS"]
RESECT_HB = _K["GIMS_RESECT_HB"]                             # hypotheses per workgroup of the scoring kernel: the seam of `iters`
RESECT_COUNTERS = ("n_ok", "n_failed", "n_corr_total", "n_inlier_total")
AUX_BUNDLE_ADJUST = _K["GIMS_AUX_BUNDLE_ADJUST"]             # joint refinement of cameras and points (bundle adjustment): likewise; 12 is unassigned
BA_TABLE_WORDS, BA_MAX_FREE_CAMERAS, BA_MAX_REJECTS = _K["GIMS_BA_TABLE_WORDS"], _K["GIMS_BA_MAX_FREE_CAMERAS"], _K["GIMS_BA_MAX_REJECTS"]
AUX_BUNDLE_ADJUST_PCG = _K["GIMS_AUX_BUNDLE_ADJUST_PCG"]     # the same with a matrix-free conjugate-gradient reduced solve: no 128-camera cap
BA_PCG_MAX_FREE_CAMERAS, BA_PCG_MAX_CG_ITERS = _K["GIMS_BA_PCG_MAX_FREE_CAMERAS"], _K["GIMS_BA_PCG_MAX_CG_ITERS"]
AUX_BUNDLE_ADJUST_FOCAL = _K["GIMS_AUX_BUNDLE_ADJUST_FOCAL"]  # the conjugate-gradient form with a focal scale per group of images; 15 is unassigned
AUX_SELECT_PAIRS = _K["GIMS_AUX_SELECT_PAIRS"]               # which image pairs to match, from a coarse int8 pre-match: likewise
PAIRS_TABLE_WORDS, PAIRS_SCALE_GIVEN = _K["GIMS_PAIRS_TABLE_WORDS"], _K["GIMS_PAIRS_SCALE_GIVEN"]
PAIRS_MAX_IMAGES, PAIRS_MAX_ROWS, PAIRS_MAX_D = _K["GIMS_PAIRS_MAX_IMAGES"], _K["GIMS_PAIRS_MAX_ROWS"], _K["GIMS_PAIRS_MAX_D"]
PAIRS_QUERY_TILE = _K["GIMS_PAIRS_QUERY_TILE"]               # pooled rows per workgroup of the vote kernel, 32 per wave: the seams of m_i
PAIRS_COUNTERS = ("n_pairs", "n_rows", "n_short_images", "n_bad_rows", "n_nonfinite")
AUX_GUIDED_MATCH = _K["GIMS_AUX_GUIDED_MATCH"]               # the descriptor match again under a verified pair's model: likewise
GUIDED_TABLE_WORDS = _K["GIMS_GUIDED_TABLE_WORDS"]
GUIDED_INFO = ("fallback_rows0", "fallback_rows1", "n_fixed", "n_bad_prior", "n_dup_prior", "no_model", "n_added")
BA_COUNTERS = ("n_free", "n_fixed", "n_held", "n_points", "n_active_obs", "n_bad_obs", "rounds_taken", "status")
BA_BAD_CAMERA, BA_BAD_START = 1, 2                           # the bits of the status counter
BA_ABSENT, BA_FIXED, BA_FREE = 0, 1, 2                       # the modes of a camera
SIFT_MAX_OCTAVES, SIFT_MAX_RADIUS, SIFT_SLOTS = _K["GIMS_SIFT_MAX_OCTAVES"], _K["GIMS_SIFT_MAX_RADIUS"], _K["GIMS_SIFT_SLOTS"]


def attn_guard(stat, kind, n_heads, mean_thr=0.0, tail_thr=0.0, range_limit=0.0, max_thr=0.0) -> AttnGuard:
    assert stat.dtype == torch.int64 and stat.is_cuda and stat.is_contiguous() and stat.numel() >= 4 * (n_heads + 1)
    return AttnGuard(stat.data_ptr(), float(mean_thr), float(tail_thr), float(range_limit), int(n_heads), int(kind), float(max_thr))


_lib = None


def load(path: str | None = None):
    """dlopen the kernel library and type its entry points.  Raises if it is not there."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise GimsHipError(f"{p} is missing: build it with `python -m gims_amd.build` "
                           "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = C.CDLL(p)
    for name, (res, args) in ABI.signatures.items():
        fn = getattr(lib, name)           # AttributeError if the .so does not export a declared symbol
        fn.restype, fn.argtypes = res, args
    if lib.gims_abi_version() != ABI_VERSION:
        raise GimsHipError(f"ABI version mismatch: library {lib.gims_abi_version()} != binding {ABI_VERSION} (rebuild: python -m gims_amd.build)")
    if path is None:
        _lib = lib
    return lib



def _check(rc: int, what: str):
    if rc != 0:
        msg = load().gims_last_error()
        raise GimsHipError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


_TLS = threading.local()    # per thread: .pin = the raw hipStream_t pinned by pinned_stream(), .gemm_prec = gemm()'s default precision


def _stream() -> int:
    pin = getattr(_TLS, "pin", None)
    return pin if pin is not None else torch.cuda.current_stream().cuda_stream


class on_stream:
    """``with on_stream(handle):`` -- launches of the calling thread go to the raw HIP stream `handle` inside the block (the side stream of
    the training step's parameter-gradient work).  Ordering against the surrounding stream and the lifetime of the tensors involved are
    the caller's business (events; references held until the streams have joined)."""

    def __init__(self, handle: int):
        self._h = int(handle)

    def __enter__(self):
        self._prev = getattr(_TLS, "pin", None)
        _TLS.pin = self._h
        return self

    def __exit__(self, *exc):
        _TLS.pin = self._prev
        return False


class pinned_stream:
    """``with pinned_stream():`` -- look the current torch stream up ONCE for a run of launches (torch.cuda.current_stream() costs a
    few microseconds per call; a training step makes ~1 800 launches).  The pin belongs to the calling THREAD (other threads
    keep resolving their own current stream), and the stream must not be switched inside the block: leaving it with a
    different current stream raises instead of having launched on the wrong one silently."""

    def __enter__(self):
        self._prev = getattr(_TLS, "pin", None)
        _TLS.pin = torch.cuda.current_stream().cuda_stream
        return self

    def __exit__(self, exc_type, *exc):
        pin, _TLS.pin = _TLS.pin, self._prev
        if exc_type is None and torch.cuda.current_stream().cuda_stream != pin:
            raise GimsHipError("the current CUDA stream changed inside a pinned_stream() block: launches went to the stream that was current on entry")
        return False


def _p(t) -> int | None:
    return None if t is None else t.data_ptr()


_NP2TORCH = {"float32": torch.float32, "int32": torch.int32, "int64": torch.int64, "uint8": torch.uint8}


def upload(arr, device="cuda", out=None) -> torch.Tensor:
    """Small host table (numpy array) -> device tensor, asynchronously and in stream order (gims_upload_table): the
    bytes ride in kernel arguments, so unlike ``torch.tensor(..., device=...)`` / ``.to(device)`` from pageable memory
    the calling thread never waits for the stream to drain."""
    a = np.ascontiguousarray(arr)
    dt = _NP2TORCH[a.dtype.name]
    nbytes = a.nbytes
    if out is not None:      # caller-owned uint8 arena (stable address from call to call); stream order protects earlier readers
        assert out.dtype == torch.uint8 and out.numel() >= nbytes + 16
        buf = out
    else:
        buf = torch.empty(((nbytes + 15) // 16 * 16 + 16,), dtype=torch.uint8, device=device)   # caching allocator: 512-B aligned
    if nbytes:
        _check(load().gims_upload_table(a.ctypes.data, nbytes, buf.data_ptr(), _stream()), "gims_upload_table")
    return buf[:nbytes].view(dt).view(a.shape)


def _dev(t: torch.Tensor, dtype=None):
    if not t.is_cuda:
        raise GimsHipError("expected a device tensor")
    if dtype is not None and t.dtype != dtype:
        raise GimsHipError(f"expected {dtype}, got {t.dtype}")
    return t


def linear_args(a0, w, *, bias=None, a1=None, w_lo=None, residual=None, out=None, out_bf16=None, act=ACT_NONE,
                precision=PREC_F32, scale=1.0, n=None, spl=False, out_split=None, flags=0, guard=None, range_stat=None, residual_rows=None):
    """Build the C struct.
    spl=False: a0/a1 f32 [m,k*]; w f32 [n,K] (PREC_F32) or bf16 hi plane with w_lo (PREC_BF16X3).
    spl=True : a0/a1/w are SPL32 bf16 buffers [rows, 2*k] (see include/gims_hip.h), precision BF16X3.
    out_split: SPL32 bf16 buffer [m, >= 2n] receiving the result split into hi/lo.
    residual_rows (spl=True): int32 [m], row r adds residual[residual_rows[r]] -- `residual` may then have any number of rows."""
    m = a0.shape[0]
    if precision == PREC_BF16X6:
        # a0 / w are SPL3 bf16 buffers [rows, 3k] (split_spl3); plain f32 output only
        assert a0.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and a1 is None and not spl
        k0 = k = a0.shape[1] // 3
        assert w.shape[1] == 3 * k, (w.shape, k)
        a0_lo = a1_lo = w_lo = None
    elif spl:
        assert a0.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and precision == PREC_BF16X3
        k0 = a0.shape[1] // 2
        k = k0 + (a1.shape[1] // 2 if a1 is not None else 0)
        assert w.shape[1] == 2 * k, (w.shape, k)
        # (the lo planes sit 32 elements = 64 bytes behind the hi planes of the same buffers: plain pointer arithmetic -- a sliced view per
        # operand cost a single-pair forward() ~8 us of Python per GEMM launch)
        p_a0, p_a1, p_w = a0.data_ptr(), (a1.data_ptr() if a1 is not None else None), w.data_ptr()
        return _linear_struct(p_a0, a0.stride(0), p_a1, a1.stride(0) if a1 is not None else 0, p_w, p_w + 64, w, bias, residual, out, out_bf16, m, n,
                              k, k0, act, precision, scale, p_a0 + 64, (p_a1 + 64) if p_a1 is not None else None, out_split, flags, guard, range_stat, residual_rows)
    else:
        _dev(a0, torch.float32)
        k0 = a0.shape[1]
        k = k0 + (a1.shape[1] if a1 is not None else 0)
        assert w.shape[1] == k, (w.shape, k)
        a0_lo = a1_lo = None
    return _linear_struct(_p(a0), a0.stride(0), _p(a1), a1.stride(0) if a1 is not None else 0, _p(w), _p(w_lo), w, bias, residual, out, out_bf16, m, n,
                          k, k0, act, precision, scale, _p(a0_lo), _p(a1_lo), out_split, flags, guard, range_stat, residual_rows)


def _linear_struct(p_a0, lda0, p_a1, lda1, p_w, p_w_lo, w, bias, residual, out, out_bf16, m, n, k, k0, act, precision, scale, p_a0_lo, p_a1_lo, out_split,
                   flags, guard, range_stat, residual_rows=None) -> LinearArgs:
    n = w.shape[0] if n is None else n
    assert w.stride(1) == 1
    if residual is not None:
        assert out is not None and residual.stride(0) == out.stride(0)
    if out_split is not None:
        assert out_split.dtype == torch.bfloat16 and out_split.shape[1] >= 2 * n and out_split.stride(1) == 1
    return LinearArgs(p_a0, lda0, p_a1, lda1, p_w, p_w_lo, w.stride(0), _p(bias), _p(residual), _p(out),
                      out.stride(0) if out is not None else 0, _p(out_bf16),
                      out_bf16.stride(0) if out_bf16 is not None else 0, m, n, k, k0, act, precision, float(scale),
                      p_a0_lo, p_a1_lo, _p(out_split), (out_split.data_ptr() + 64) if out_split is not None else None,
                      out_split.stride(0) if out_split is not None else 0, int(flags), residual_rows=_p(residual_rows),
                      guard=guard if guard is not None else AttnGuard(), range_stat=_p(range_stat))


def linear_batch(arg_list, dev_args: torch.Tensor, precision=PREC_F32):
    """Many independent problems in one launch; dev_args: uint8 device scratch of >= len * sizeof(LinearArgs)."""
    lib = load()
    sz = C.sizeof(LinearArgs)
    assert dev_args.numel() * dev_args.element_size() >= sz * len(arg_list)
    st = _stream()
    arr = (LinearArgs * len(arg_list))(*arg_list)
    _check(lib.gims_linear_put_many(arr, len(arg_list), dev_args.data_ptr(), st), "gims_linear_put_many")
    _check(lib.gims_linear_batch(dev_args.data_ptr(), len(arg_list), max(a.m for a in arg_list), max(a.n for a in arg_list),
                                 precision, st), "gims_linear_batch")


def linear(a0, w, *, out=None, out_bf16=None, out_split=None, **kw):
    """C = act(scale * [a0 | a1] @ w[:n].T + bias) (+ residual); see linear_args / include/gims_hip.h."""
    lib = load()
    if out is None and out_bf16 is None and out_split is None:
        n = kw.get("n") or w.shape[0]
        out = torch.empty((a0.shape[0], n), dtype=torch.float32, device=a0.device)
    args = linear_args(a0, w, out=out, out_bf16=out_bf16, out_split=out_split, **kw)
    _check(lib.gims_linear(C.byref(args), _stream()), "gims_linear")
    return out if out is not None else (out_bf16 if out_bf16 is not None else out_split)


def split_spl32(x: torch.Tensor, out: torch.Tensor | None = None):
    """f32 [rows, k] -> SPL32 bf16 [rows, 2k] (32 hi | 32 lo per 32-channel block)."""
    lib = load()
    rows, k = x.shape
    assert x.stride(1) == 1 and k % 32 == 0
    if out is None:
        out = torch.empty((rows, 2 * k), dtype=torch.bfloat16, device=x.device)
    _check(lib.gims_split_spl32(_p(_dev(x, torch.float32)), x.stride(0), _p(out), out.stride(0), rows, k, _stream()), "gims_split_spl32")
    return out


def op_linear(args: LinearArgs) -> Op:
    o = Op()
    o.kind = 0
    o.u.lin = args
    return o


OP_MLP = _K["GIMS_OP_MLP"]
# where channel c of a 32-channel block of W1's K axis sits in the copy GIMS_OP_MLP reads: position 16 s + 8 h + j holds channel
# (r & 3) + 8 (r >> 2) + 4 h, r = 8 s + j (include/gims_hip.h)
MLP_W1_ORDER = tuple((r & 3) + 8 * (r >> 2) + 4 * h for s in range(2) for h in range(2) for r in range(8 * s, 8 * s + 8))


def mlp_w1_permute(w1: torch.Tensor) -> torch.Tensor:
    """W1 [n, hidden] with its K axis reordered inside every 32-channel block as GIMS_OP_MLP reads it (MLP_W1_ORDER)."""
    n, k = w1.shape
    assert k % 32 == 0
    return w1.reshape(n, k // 32, 32)[:, :, list(MLP_W1_ORDER)].reshape(n, k).contiguous()


def op_mlp(a0, a1, w, bias, out, out_split, residual=None) -> Op:
    """One layer's MLP in one launch (include/gims_hip.h GIMS_OP_MLP): out = residual + W1 relu(W0 [a0 | a1] + b0) + b1 on SPL32 operands;
    w = SPL32 of [W0 ; mlp_w1_permute(W1)] (3n rows), bias = b0 | b1."""
    n = a0.shape[1] // 2
    assert w.shape[0] == 3 * n and bias.numel() == 3 * n and bias.dtype == torch.float32 and bias.is_contiguous()
    o = Op()
    o.kind = OP_MLP
    o.u.lin = linear_args(a0, w, bias=bias, a1=a1, residual=residual, out=out, act=ACT_RELU, precision=PREC_BF16X3, n=n, spl=True, out_split=out_split)
    return o


def _attn_flags(q_prescaled, x3, f16, no_range=False):
    assert not (x3 and f16)
    return (1 if q_prescaled else 0) | (ATTN_X3 if x3 else 0) | (ATTN_F16 if f16 else 0) | (ATTN_NO_RANGE if no_range else 0)


def op_attention(qkv, problems, max_n_q, n_heads, out=None, q_col=0, k_col=256, v_col=512, out_split=None, q_prescaled=False, x3=False,
                 stat=None, f16=False, guard=None, no_range=False) -> Op:
    assert qkv.dtype == torch.bfloat16 and problems.dtype == torch.int32 and problems.is_cuda
    if stat is not None:
        assert stat.dtype == torch.int64 and stat.is_contiguous() and stat.numel() >= 4 * (n_heads + 1) and stat.is_cuda
    o = Op()
    o.kind = 1
    o.u.att = AttnArgs(_p(qkv), qkv.stride(0), q_col, k_col, v_col, _p(problems), problems.shape[0], max_n_q, n_heads, _p(out),
                       out.stride(0) if out is not None else 0, _p(out_split), (out_split.data_ptr() + 64) if out_split is not None else None,
                       out_split.stride(0) if out_split is not None else 0, _attn_flags(q_prescaled, x3, f16, no_range), _p(stat),
                       guard if guard is not None else AttnGuard())
    return o


def op_aux(fn: int, ptrs, ints, floats=()) -> Op:
    """One small kernel as an op (include/gims_hip.h GIMS_OP_AUX): ptrs = tensors or raw addresses (None -> NULL), ints = integers,
    floats = the entry point's floating-point arguments."""
    o = Op()
    o.kind = 2
    o.u.aux.fn = int(fn)
    for k, t in enumerate(ptrs):
        o.u.aux.p[k] = t if (t is None or isinstance(t, int)) else t.data_ptr()
    for k, v in enumerate(ints):
        o.u.aux.i[k] = int(v)
    for k, v in enumerate(floats):
        o.u.aux.f[k] = float(v)
    return o


def make_ops(ops):
    """A replayable launch sequence (see gims_run_ops): returns the ctypes array; keep the tensors it points to alive."""
    return (Op * len(ops))(*ops)


def run_ops(op_array, start: int = 0, count: int | None = None):
    """Replay ops[start : start + count] (default: all of them) in one call."""
    n = len(op_array) - start if count is None else count
    assert 0 <= start and start + n <= len(op_array)
    _check(load().gims_run_ops(C.byref(op_array, start * C.sizeof(Op)) if start else op_array, n, _stream()), "gims_run_ops")


class EventPool:
    """n HIP events owned by the library (gims_events_*): per-op timing of a replayed launch sequence."""

    def __init__(self, n):
        self.n = n
        self._ev = (C.c_void_p * n)()
        _check(load().gims_events_create(n, self._ev), "gims_events_create")

    def elapsed_ms(self):
        """The n - 1 intervals between consecutive events (ms); synchronise the stream first."""
        out = (C.c_float * (self.n - 1))()
        _check(load().gims_events_elapsed(self._ev, self.n, out), "gims_events_elapsed")
        return list(out)

    def __del__(self):
        try:
            load().gims_events_destroy(self._ev, self.n)
        except Exception:
            pass


def run_ops_timed(op_array, pool: EventPool):
    assert pool.n == len(op_array) + 1
    _check(load().gims_run_ops_timed(op_array, len(op_array), _stream(), pool._ev), "gims_run_ops_timed")


class OpsGraph:
    """The launch sequence as an instantiated HIP graph (gims_ops_graph_*); capture needs a non-default stream."""

    def __init__(self, op_array):
        self._ops = op_array          # keeps the host table alive
        h = C.c_void_p()
        _check(load().gims_ops_graph_create(op_array, len(op_array), _stream(), C.byref(h)), "gims_ops_graph_create")
        self._h = h

    def launch(self):
        _check(load().gims_ops_graph_launch(self._h, _stream()), "gims_ops_graph_launch")

    def __del__(self):
        try:
            if self._h:
                load().gims_ops_graph_destroy(self._h)
        except Exception:
            pass


def split_spl3(x: torch.Tensor, out: torch.Tensor | None = None):
    """f32 [rows, k] -> SPL3 bf16 [rows, 3k]: the exact three-way split x = a1 + a2 + a3 (32 a1 | 32 a2 | 32 a3 per
    32-channel block), the operand layout of PREC_BF16X6."""
    lib = load()
    rows, k = x.shape
    assert x.stride(1) == 1 and k % 32 == 0
    if out is None:
        out = torch.empty((rows, 3 * k), dtype=torch.bfloat16, device=x.device)
    _check(lib.gims_split_spl3(_p(_dev(x, torch.float32)), x.stride(0), _p(out), out.stride(0), rows, k, _stream()), "gims_split_spl3")
    return out


def spl32_planes(buf: torch.Tensor):
    """Decode an SPL32 buffer [rows, 2k] into (hi, lo) bf16 tensors [rows, k] (test / debug helper)."""
    rows, k2 = buf.shape
    v = buf.reshape(rows, k2 // 64, 2, 32)
    return v[:, :, 0, :].reshape(rows, k2 // 2), v[:, :, 1, :].reshape(rows, k2 // 2)


def split_bf16(x: torch.Tensor):
    lib = load()
    x = x.contiguous()
    hi = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    lo = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    _check(lib.gims_split_bf16(_p(_dev(x, torch.float32)), _p(hi), _p(lo), x.numel(), _stream()), "gims_split_bf16")
    return hi, lo


ATTN_Q_SCALE = 0.125 * 1.4426950408889634      # log2(e) / sqrt(64): what q_prescaled=True expects folded into Q


ATTN_X3 = _K["GIMS_ATTN_X3"]
ATTN_NO_RANGE = _K["GIMS_ATTN_NO_RANGE"]   # a measured launch leaves the range row alone (the projection reported it: linear_args(range_stat=...))
ATTN_F16 = _K["GIMS_ATTN_F16"]        # qkv holds IEEE half (gims_linear with LINEAR_OUT_F16); v_mfma_f32_32x32x16_f16 kernels


ATTN_STAT_SCALE = float(1 << 24)       # fixed point of the row maxima in gims_attention's stat accumulator


def attention(qkv: torch.Tensor, problems: torch.Tensor, max_n_q: int, n_heads: int, out=None,
              q_col=0, k_col=256, v_col=512, out_split=None, q_prescaled=False, x3=False, stat=None, f16=False, guard=None, no_range=False):
    """qkv bf16 [rows, ld]; problems int32 [P,4] (q_off, n_q, kv_off, n_kv) on device; out f32 [rows, ld_out]
    and/or out_split = SPL32 bf16 buffer [rows, >= 512].  q_prescaled: Q already carries ATTN_Q_SCALE.
    x3: qkv is the SPL32 split-bf16 buffer [rows, >= 1536] of the 3-pass projection (GIMS_ATTN_X3).
    f16: the 16-bit values of qkv are IEEE half, not bf16 (GIMS_ATTN_F16; the tensor's dtype stays torch.bfloat16: raw storage).
    stat: int64 [n_heads + 1, 4] accumulator of the softmax peakedness and the operand range (gims_attn_args.stat; zero it before the
    first use)."""
    # (guard: an x3 launch that is a no-op unless the guard's statistic asks for the redo)
    op = op_attention(qkv, problems, max_n_q, n_heads, out, q_col, k_col, v_col, out_split, q_prescaled, x3, stat, f16, guard, no_range)
    _check(load().gims_attention(C.byref(op.u.att), _stream()), "gims_attention")
    return out if out is not None else out_split


def kenc_first(kpts, norm3, seg_of_row, w1, b1, out, relu=True):
    lib = load()
    c1 = w1.shape[0]
    fn = lib.gims_kenc_first if relu else lib.gims_kenc_first_linear
    _check(fn(_p(_dev(kpts, torch.float32)), _p(norm3), _p(seg_of_row), _p(w1), _p(b1), c1,
              _p(out), kpts.shape[0], _stream()), "gims_kenc_first")
    return out


def layernorm_act(x, a2, b2, out=None, out_split=None, act=ACT_RELU, eps=1e-6):
    """LayerNorm over the channels of every row (unbiased std, eps on the std; gmatcher.py:74-85) + activation.
    out: f32 [rows, c] (may be x itself) and/or out_split: SPL32 bf16 [rows, >= 2c]."""
    lib = load()
    rows, c = x.shape
    assert x.dtype == torch.float32 and x.stride(1) == 1 and (out is not None or out_split is not None)
    _check(lib.gims_layernorm_act(_p(x), x.stride(0), rows, c, _p(a2), _p(b2), float(eps), act, _p(out),
                                  out.stride(0) if out is not None else 0, _p(out_split),
                                  (out_split.data_ptr() + 64) if out_split is not None else None,
                                  out_split.stride(0) if out_split is not None else 0, _stream()), "gims_layernorm_act")
    return out if out is not None else out_split


def sage_mean_split(h, indptr, indices, out_spl, n=None, c=None):
    """mean over CSR neighbours, written as SPL32 split-bf16 planes (out_spl: bf16 [rows, 2 * c])."""
    lib = load()
    n = h.shape[0] if n is None else n
    c = h.shape[1] if c is None else c
    _check(lib.gims_sage_mean_split(_p(_dev(h, torch.float32)), h.stride(0), _p(indptr), _p(indices), n, c, _p(out_spl),
                                    out_spl.stride(0), _stream()), "gims_sage_mean_split")
    return out_spl


def sage_mean(h, indptr, indices, out, n=None, c=None):
    lib = load()
    n = h.shape[0] if n is None else n
    c = h.shape[1] if c is None else c
    _check(lib.gims_sage_mean(_p(_dev(h, torch.float32)), h.stride(0), _p(indptr), _p(indices), n, c, _p(out),
                              out.stride(0), _stream()), "gims_sage_mean")
    return out


def pair_stats(matches0, scores0, table):
    """[n_pairs, 5] f32 records {pair_id, n0, n1, n_matches, mean_score} from batch-concatenated outputs; table: int32
    [n_pairs, 4] = {pair_id, n0, n1, row offset} on the device (gims_pair_stats)."""
    lib = load()
    n = table.shape[0]
    out = torch.empty((n, 5), dtype=torch.float32, device=matches0.device)
    _check(lib.gims_pair_stats(_p(_dev(matches0, torch.int64)), _p(_dev(scores0, torch.float32)), _p(_dev(table, torch.int32)), n, _p(out),
                               _stream()), "gims_pair_stats")
    return out


def gather_rows(src, idx, out):
    lib = load()
    _check(lib.gims_gather_rows(_p(_dev(src, torch.float32)), src.stride(0), _p(idx), idx.shape[0], src.shape[1],
                                _p(out), out.stride(0), _stream()), "gims_gather_rows")
    return out


def make_agc_images(items):
    """items: dicts with kpts [n,2], desc [n,d] (point-major f32), kept [n], indptr [n+1], indices [cap], info [8].
    desc may be None for delaunay_build (which reads keypoints only)."""
    arr = (AgcImage * len(items))()
    for i, it in enumerate(items):
        de = it.get("desc")
        assert it["kpts"].is_contiguous()
        if de is None:
            arr[i] = AgcImage(_p(_dev(it["kpts"], torch.float32)), None, 0, it["kpts"].shape[0], 0,
                              _p(it["kept"]), _p(it["indptr"]), _p(it["indices"]), it["indices"].numel(), _p(it["info"]))
            continue
        assert de.stride(1) == 1
        arr[i] = AgcImage(_p(_dev(it["kpts"], torch.float32)), _p(_dev(de, torch.float32)), de.stride(0), de.shape[0], de.shape[1],
                          _p(it["kept"]), _p(it["indptr"]), _p(it["indices"]), it["indices"].numel(), _p(it["info"]))
    return arr


def agc_max_keypoints() -> int:
    """Largest image the graph build takes (32768; include/gims_hip.h says what bounds it)."""
    return int(load().gims_agc_max_keypoints())


def agc_workspace_bytes(images, flags=None) -> int:
    """Scratch bytes of agc_build(images, ..., flags=flags); flags=None: enough for either flow (the robust one stores the half N x N matrix)."""
    nmax = max(int(im.n) for im in images)
    if nmax > agc_max_keypoints():
        raise GimsHipError(f"adaptive graph: an image has {nmax} keypoints, more than the library's limit of {agc_max_keypoints()} per image "
                           "(gims_agc_max_keypoints; the reference has none) -- reduce max_keypoints or split the image")
    return int(load().gims_agc_workspace_bytes(images, len(images), AGC_ROBUST if flags is None else int(flags)))


AGC_ROBUST = _K["GIMS_AGC_ROBUST"]               # gims_agc_build flags
AGC_INFO_OVERFLOW, AGC_INFO_WINDOW_MISSED = 1, 2     # bits of info[7]


def agc_build(images, radius, percentile, min_size, work: torch.Tensor, flags=0):
    """Asynchronous adaptive-graph build for a batch of images; see include/gims_hip.h.  An image whose info[7] has AGC_INFO_WINDOW_MISSED
    set after the call must be rebuilt with flags=AGC_ROBUST."""
    one = AgcParams(float(radius), float(percentile), int(min_size), 0)
    _check(load().gims_agc_build(images, len(images), C.byref(one), 1, int(flags), _p(work), work.numel() * work.element_size(), _stream()),
           "gims_agc_build")


def agc_build_each(images, params, work: torch.Tensor, flags=0):
    """agc_build with each image's own parameters: params[i] = (radius, percentile, min_size) of images[i]."""
    params = list(params)
    if len(params) != len(images):
        raise ValueError(f"agc_build_each: {len(images)} images but {len(params)} parameter triples")
    arr = (AgcParams * len(params))(*[AgcParams(float(r), float(t), int(m), 0) for r, t, m in params])
    _check(load().gims_agc_build(images, len(images), arr, len(params), int(flags), _p(work), work.numel() * work.element_size(), _stream()),
           "gims_agc_build")


DT_INFO_DEGENERATE, DT_INFO_ASYMMETRIC = _K["GIMS_DT_INFO_DEGENERATE"], _K["GIMS_DT_INFO_ASYMMETRIC"]     # bits of info[7] set by delaunay_build (bit 0: AGC_INFO_OVERFLOW, same meaning)


def delaunay_workspace_bytes(images) -> int:
    """Scratch bytes of delaunay_build(images, ...)."""
    nmax = max(int(im.n) for im in images)
    if nmax > agc_max_keypoints():
        raise GimsHipError(f"delaunay graph: an image has {nmax} keypoints, more than the library's limit of {agc_max_keypoints()} per image "
                           "(gims_agc_max_keypoints) -- reduce max_keypoints or split the image")
    return int(load().gims_delaunay_workspace_bytes(images, len(images)))


def delaunay_build(images, work: torch.Tensor):
    """Asynchronous Delaunay-graph build (D-GIMS) for a batch of images made by make_agc_images; see include/gims_hip.h.  After the stream
    is synchronised, info[7] must be checked: DT_INFO_DEGENERATE / DT_INFO_ASYMMETRIC / AGC_INFO_OVERFLOW void the image's graph."""
    lib = load()
    _check(lib.gims_delaunay_build(images, len(images), _p(work), work.numel() * work.element_size(), _stream()), "gims_delaunay_build")


def _upload_structs(arr, device):
    """ctypes descriptor table -> device through gims_upload_table (stream-ordered, never blocks the host)."""
    nbytes = C.sizeof(arr)
    buf = torch.empty(((nbytes + 15) // 16 * 16 + 16,), dtype=torch.uint8, device=device)
    _check(load().gims_upload_table(C.addressof(arr), nbytes, buf.data_ptr(), _stream()), "gims_upload_table")
    return buf


def ingest_images(items, d, desc_out, kpts_out, score_out):
    """items: list of IngestImage (host).  One launch for the batch; none, and None back, when every image is empty (the entry point
    refuses max_n = 0, and the caller's own check of the keypoint counts is what has to speak then)."""
    lib = load()
    if not any(i.n > 0 for i in items):
        return None
    arr = (IngestImage * len(items))(*items)
    dev_arr = _upload_structs(arr, desc_out.device)
    _check(lib.gims_ingest_images(_p(dev_arr), len(items), max(i.n for i in items), d, _p(desc_out), desc_out.stride(0),
                                  _p(kpts_out), _p(score_out), _stream()), "gims_ingest_images")
    return dev_arr


PACK_DTYPE = np.dtype(PackImage)


def pack_table(images_ptrs):
    """numpy structured array of gims_pack_image records (one per image) with the pointer columns filled;
    the count/offset columns are filled after the graph build's host sync (vectorised: no per-image Python work then)."""
    t = np.zeros(len(images_ptrs), dtype=PACK_DTYPE)
    for i, r in enumerate(images_ptrs):
        t[i] = tuple(r) + (0,) * (len(PACK_DTYPE.names) - len(r))
    return t


def pack_graphs_table(table, d, feat, kpts_out, score_out, seg, indptr_out, indices_out, n_rows, n_edges):
    """One launch for the batch (gims_pack_graphs); table: the descriptor records as the numpy array of pack_table()."""
    lib = load()
    nbytes = table.nbytes
    dev_arr = torch.empty(((nbytes + 15) // 16 * 16 + 16,), dtype=torch.uint8, device=feat.device)
    st = _stream()
    _check(lib.gims_upload_table(table.ctypes.data, nbytes, dev_arr.data_ptr(), st), "gims_upload_table")
    _check(lib.gims_pack_graphs(_p(dev_arr), len(table), int(table["n_kept"].max()), max(int(table["n_edges"].max()), 1), d,
                                _p(feat), feat.stride(0), _p(kpts_out), _p(score_out), _p(seg), _p(indptr_out),
                                _p(indices_out), n_rows, n_edges, st), "gims_pack_graphs")
    return dev_arr


def make_ot_problems(items):
    """items: list of dicts with scores (f32 [n, ld>=m] view), n, m, matches0/1, mscores0/1, uv tensors."""
    arr = (OtProblem * len(items))()
    for i, it in enumerate(items):
        s = it["scores"]
        arr[i] = OtProblem(_p(s), s.stride(0), it["n"], it["m"], _p(it["matches0"]), _p(it["matches1"]),
                           _p(it["mscores0"]), _p(it["mscores1"]), _p(it["uv"]))
    return arr


def sinkhorn_workspace_bytes(problems) -> int:
    return int(load().gims_sinkhorn_workspace_bytes(problems, len(problems)))


OT_STREAMED = _K["GIMS_OT_STREAMED"]      # flag of sinkhorn_plan / sinkhorn_match: never an on-chip kernel (concurrent streams on one GPU)


def sinkhorn_plan(problems, iters: int, flags: int = 0) -> int:
    """0: streamed kernels (one launch per iteration); k > 0: on-chip resident kernel in k launches."""
    return int(load().gims_sinkhorn_plan(problems, len(problems), int(iters), int(flags)))


ATTN_KERNEL_KINDS = ("wave4", "split", "wave8", "wave8_f16", "x3", "x3_guarded")


def attention_launch_counts(reset: bool = False) -> dict:
    """Attention launches of this process per kernel family since the last reset (include/gims_hip.h GIMS_ATTN_KERNEL_*)."""
    buf = (C.c_uint64 * len(ATTN_KERNEL_KINDS))()
    _check(load().gims_attention_launch_counts(buf, len(ATTN_KERNEL_KINDS), int(reset)), "gims_attention_launch_counts")
    return dict(zip(ATTN_KERNEL_KINDS, (int(x) for x in buf)))


# GIMS_LINEAR_KERNEL_* of the header, in value order, under their lower-case names ("f32", "x6_batch", "x3p_128x128_w4_s2", ...)
LINEAR_KERNEL_NAMES = tuple(k[len("GIMS_LINEAR_KERNEL_"):].lower() for k, _ in sorted(
    ((k, v) for k, v in _K.items() if k.startswith("GIMS_LINEAR_KERNEL_") and k != "GIMS_LINEAR_KERNEL_KINDS"), key=lambda kv: kv[1]))
assert len(LINEAR_KERNEL_NAMES) == _K["GIMS_LINEAR_KERNEL_KINDS"]


def linear_launch_counts(reset: bool = False) -> dict:
    """GEMM launches of this process per kernel instance since the last reset (include/gims_hip.h GIMS_LINEAR_KERNEL_*)."""
    buf = (C.c_uint64 * len(LINEAR_KERNEL_NAMES))()
    _check(load().gims_linear_launch_counts(buf, len(LINEAR_KERNEL_NAMES), int(reset)), "gims_linear_launch_counts")
    return dict(zip(LINEAR_KERNEL_NAMES, (int(x) for x in buf)))


def sinkhorn_rescues() -> int:
    """On-chip solves of this process that gave up and were re-solved by a rescue path on the current device (synchronises)."""
    n = int(load().gims_sinkhorn_rescues())
    if n < 0:
        _check(GIMS_EHIP, "gims_sinkhorn_rescues")
    return n


def sinkhorn_match(problems, alpha: float, iters: int, match_threshold: float, work: torch.Tensor, flags: int = 0):
    lib = load()
    _check(lib.gims_sinkhorn_match(problems, len(problems), float(alpha), int(iters), float(match_threshold), _p(work),
                                   work.numel() * work.element_size(), int(flags), _stream()), "gims_sinkhorn_match")


def ot_matrix(scores, n, m, alpha, uv):
    lib = load()
    out = torch.empty((n + 1, m + 1), dtype=torch.float32, device=scores.device)
    _check(lib.gims_ot_matrix(_p(scores), scores.stride(0), n, m, float(alpha), _p(uv), _p(out), _stream()),
           "gims_ot_matrix")
    return out


# ------------------------------------------------------------------------------------------------ evaluation
EVAL_FIELDS = ("n_valid", "n_gt", "n_correct", "n_fn", "precision", "recall", "n_inliers", "err_dlt", "err_ransac", "dlt_ok",
               "ransac_ok")


def eval_pairs(items, dist_thresh=3.0, n_iters=3, ransac_thresh=3.0, ransac_iters=3000, seed=0, work=None):
    """items: list of dicts with device tensors kpts0 [n0,2] f32, kpts1 [n1,2] f32, matches0 [n0] int64, mscores0 [n0] f32,
    h_gt (3x3 array-like), height, width, and outputs gt0 [n0] int32, inlier [n0] uint8, record [16] f32,
    homographies [18] f32.  One batched asynchronous call; see include/gims_hip.h."""
    lib = load()
    arr = (EvalPair * len(items))()
    for i, it in enumerate(items):
        k0, k1 = it["kpts0"], it["kpts1"]
        assert k0.dtype == torch.float32 and k1.dtype == torch.float32 and k0.is_contiguous() and k1.is_contiguous()
        assert it["matches0"].dtype == torch.int64 and it["mscores0"].dtype == torch.float32
        assert it["gt0"].dtype == torch.int32 and it["inlier"].dtype == torch.uint8
        h = np.asarray(it["h_gt"], dtype=np.float32).reshape(9)
        arr[i] = EvalPair(_p(k0), _p(k1), _p(it["matches0"]), _p(it["mscores0"]), k0.shape[0], k1.shape[0], int(it["height"]),
                          int(it["width"]), (C.c_float * 9)(*h.tolist()), _p(it["gt0"]), _p(it["inlier"]), _p(it["record"]),
                          _p(it["homographies"]))
    need = int(lib.gims_eval_workspace_bytes(arr, len(items), int(ransac_iters)))
    if work is None or work.numel() * work.element_size() < need:
        work = torch.empty(need, dtype=torch.uint8, device=items[0]["kpts0"].device)
    _check(lib.gims_eval_pairs(arr, len(items), float(dist_thresh), int(n_iters), float(ransac_thresh), int(ransac_iters),
                               int(seed) & 0xFFFFFFFFFFFFFFFF, _p(work), work.numel() * work.element_size(), _stream()),
           "gims_eval_pairs")
    return work


# ------------------------------------------------------------------------------------------------ geometric verification
VERIFY_FIELDS = ("n_valid", "ok", "n_inliers", "best_hyp", "best_hyp_inliers", "lo_rounds", "err_corner")
VERIFY_MODELS = {"homography": _K["GIMS_VERIFY_MODEL_HOMOGRAPHY"], "fundamental": _K["GIMS_VERIFY_MODEL_FUNDAMENTAL"],
                 "pose": _K["GIMS_VERIFY_MODEL_POSE"]}
VERIFY_POSE_FLOATS = 24                  # what the `homography` output of a pose set receives: E[9], R[9], t[3], n_front, root, 0


def verify_model(model) -> int:
    """GIMS_VERIFY_MODEL_* of a model given by name or by number."""
    if isinstance(model, str) and model in VERIFY_MODELS:
        return VERIFY_MODELS[model]
    if isinstance(model, (int, np.integer)) and not isinstance(model, bool) and int(model) in VERIFY_MODELS.values():
        return int(model)
    raise GimsHipError(f"verify_pairs: model must be 'homography' (0), 'fundamental' (1) or 'pose' (3), not {model!r}")


def verify_pairs(items, thresh=3.0, iters=3000, lo_iters=8, seed=0, work=None):
    """items: list of dicts with device tensors kpts0 [n0,2] f32, kpts1 [n1,2] f32, matches0 [n0] int64 or None (identity pairing, n0 == n1),
    optionally h_ref (3x3 array-like) with height / width, optionally model ('homography' / 0, the default, 'fundamental' / 1 or 'pose' / 3;
    per item, one call may mix them; h_ref with 'fundamental' is refused by the library), and outputs inlier [n0] uint8, record [8] f32 (VERIFY_FIELDS), homography [9] f32
    (the fundamental matrix F, x1^T F x0 = 0, when that is the model).  An item with model 'pose' carries intrinsics=(K0, K1), two 3x3
    array-likes, in the place of h_ref, and its `homography` output has VERIFY_POSE_FLOATS = 24 floats: E[9], R[9], t[3], n_front, root, 0.
    One batched asynchronous call; returns the workspace (keep it alive until the stream has passed the call).  See include/gims_hip.h."""
    lib = load()
    arr = (VerifySet * len(items))()
    for i, it in enumerate(items):
        k0, k1, m0 = it["kpts0"], it["kpts1"], it.get("matches0")
        for k in (k0, k1):
            if k.dtype != torch.float32 or not k.is_contiguous() or k.dim() != 2 or k.shape[1] != 2 or not k.is_cuda:
                raise GimsHipError("verify_pairs: kpts0 / kpts1 must be contiguous float32 [n, 2] device tensors")
        n0, n1 = int(k0.shape[0]), int(k1.shape[0])
        if m0 is not None and (m0.dtype != torch.int64 or m0.numel() != n0 or not m0.is_contiguous()):
            raise GimsHipError("verify_pairs: matches0 must be a contiguous int64 tensor of n0 elements")
        if it["inlier"].dtype != torch.uint8 or it["inlier"].numel() < n0 or it["record"].dtype != torch.float32 or it["record"].numel() < 8 \
                or it["homography"].dtype != torch.float32 or it["homography"].numel() < 9:
            raise GimsHipError("verify_pairs: outputs are inlier uint8 [n0], record float32 [8], homography float32 [9]")
        h_ref = it.get("h_ref")
        model = verify_model(it.get("model", 0))
        h = np.asarray(h_ref, dtype=np.float32).reshape(9) if h_ref is not None else np.zeros(9, dtype=np.float32)
        if model == VERIFY_MODELS["pose"]:
            if h_ref is not None or it.get("intrinsics") is None or len(it["intrinsics"]) != 2:
                raise GimsHipError("verify_pairs: model 'pose' takes intrinsics=(K0, K1) and no h_ref")
            if it["homography"].numel() < VERIFY_POSE_FLOATS or not it["homography"].is_contiguous():
                raise GimsHipError("verify_pairs: the homography output of model 'pose' has 24 contiguous floats (E, R, t, n_front, root, 0)")
            k0m, k1m = (np.asarray(k, dtype=np.float64).reshape(3, 3) for k in it["intrinsics"])
            h = np.array([k0m[0, 0], k0m[1, 1], k0m[0, 2], k0m[1, 2], k1m[0, 0], k1m[1, 1], k1m[0, 2], k1m[1, 2], 0.0], dtype=np.float32)
        elif it.get("intrinsics") is not None:
            raise GimsHipError("verify_pairs: intrinsics are read with model 'pose' only")
        arr[i] = VerifySet(_p(k0) if n0 else None, _p(k1) if n1 else None, _p(m0), n0, n1, int(it.get("height", 0)), int(it.get("width", 0)),
                           int(h_ref is not None), model, (C.c_float * 9)(*h.tolist()), _p(it["inlier"]) if n0 else None, _p(it["record"]),
                           _p(it["homography"]))
    need = int(lib.gims_verify_workspace_bytes(arr, len(items), int(iters)))
    if work is None or work.numel() * work.element_size() < need:
        work = torch.empty(max(need, 256), dtype=torch.uint8, device=items[0]["record"].device)
    _check(lib.gims_verify_pairs(arr, len(items), float(thresh), int(iters), int(lo_iters), int(seed) & 0xFFFFFFFFFFFFFFFF, _p(work),
                                 work.numel() * work.element_size(), _stream()), "gims_verify_pairs")
    return work


# ------------------------------------------------------------------------------------------------ descriptor baselines
NN_EXHAUSTIVE = _K["GIMS_NN_EXHAUSTIVE"]            # gims_nn_match flag: every row through the exhaustive float64 path
NN_OUTPUTS = (("nn1", torch.int32), ("nn2", torch.int32), ("d1", torch.float32), ("d2", torch.float32), ("ratio", torch.float32),
              ("match", torch.uint8), ("matches0", torch.int64), ("scores0", torch.float32))


def nn_match(items, flags: int = 0, work=None):
    """items: list of dicts with device tensors a [n0, d] / b [n1, d] (float32, rows contiguous), `mutual` (bool), `threshold`, and the output
    tensors of include/gims_hip.h's gims_nn_pair: nn1, nn2 (int32), d1, d2, ratio (float32), match (uint8), matches0 (int64), scores0 (float32),
    all [n0]; info int32 [4]; with `mutual` also matches1 int64 [n1] and optionally cnn1 int32 [n1]; optionally debug float32 [n0, 4].
    One batched asynchronous call; returns the workspace (keep it alive until the stream has passed the call)."""
    lib = load()
    arr = (NnPair * len(items))()
    for i, it in enumerate(items):
        a, b = it["a"], it["b"]
        if a.dtype != torch.float32 or b.dtype != torch.float32 or a.dim() != 2 or b.dim() != 2 or a.stride(1) != 1 or b.stride(1) != 1:
            raise GimsHipError("nn_match: a / b must be float32 [n, d] with contiguous rows")
        n0, n1 = int(a.shape[0]), int(b.shape[0])
        for name, dt in NN_OUTPUTS:
            if it[name].dtype != dt or it[name].numel() < n0 or not it[name].is_contiguous():
                raise GimsHipError(f"nn_match: output {name} must be a contiguous {dt} tensor of n0 elements")
        mutual = bool(it.get("mutual", False))
        if mutual and (it["matches1"].dtype != torch.int64 or it["matches1"].numel() < n1):
            raise GimsHipError("nn_match: matches1 must be int64 [n1]")
        if it.get("cnn1") is not None and (it["cnn1"].dtype != torch.int32 or it["cnn1"].numel() < n1):
            raise GimsHipError("nn_match: cnn1 must be int32 [n1]")
        if it["info"].dtype != torch.int32 or it["info"].numel() < 4:
            raise GimsHipError("nn_match: info must be int32 [4]")
        if it.get("debug") is not None and (it["debug"].dtype != torch.float32 or it["debug"].numel() < 4 * n0):
            raise GimsHipError("nn_match: debug must be float32 [n0, 4]")
        lda, ldb = (a.stride(0) if n0 > 1 else a.shape[1]), (b.stride(0) if n1 > 1 else b.shape[1])      # a single row has no meaningful stride
        arr[i] = NnPair(_p(a), _p(b), lda, ldb, n0, n1, int(a.shape[1]), int(mutual), float(it.get("threshold", 0.8)), 0,
                        *[_p(it[name]) for name, _ in NN_OUTPUTS], _p(it.get("cnn1")) if mutual else None,
                        _p(it["matches1"]) if mutual else None, _p(it["info"]), _p(it.get("debug")))
    need = int(lib.gims_nn_workspace_bytes(arr, len(items), int(flags)))
    if need == 0:           # bad arguments: let the call itself name them
        _check(lib.gims_nn_match(arr, len(items), int(flags), None, 0, _stream()), "gims_nn_match")
    if work is None or work.numel() * work.element_size() < need:
        work = torch.empty(need, dtype=torch.uint8, device=items[0]["a"].device)
    _check(lib.gims_nn_match(arr, len(items), int(flags), _p(work), work.numel() * work.element_size(), _stream()), "gims_nn_match")
    return work


# ------------------------------------------------------------------------------------------------ guided matching
GUIDED_OUTPUTS = (("nn1", torch.int32), ("nn2", torch.int32), ("d1", torch.float32), ("d2", torch.float32), ("ratio", torch.float32),
                  ("n_admissible", torch.int32), ("matches0", torch.int64), ("scores0", torch.float32), ("added0", torch.uint8))
_GUIDED_WORDS = ("a", "b", "lda", "ldb", "n0", "n1", "d", "kpts0", "kpts1", "model", "kind", "ok", "prior", "prior_mask", "prior_scores", "mutual",
                 "nn1", "nn2", "d1", "d2", "ratio", "n_admissible", "matches0", "scores0", "added0", "cnn1", "matches1", "info", "thresh", "threshold",
                 "max_distance", "reserved")
GUIDED_WORD = {name: k for k, name in enumerate(_GUIDED_WORDS)}       # the words of one pair in the table of GIMS_AUX_GUIDED_MATCH


def guided_layout(sizes, flags: int = 0) -> dict:
    """The workspace of GIMS_AUX_GUIDED_MATCH (include/gims_hip.h has the formula; csrc/nn.hip gd_layout carves it and gims_aux_layout sizes
    it).  sizes: (n0, n1, mutual) per pair.  -> {'bytes', 'csplit' (per problem, pair by pair: A against B, with mutual then B against A),
    'items' (workgroups of the candidate pass)}.  'csplit' and 'items' are a restatement of the library's plan, kept for the tests that
    check it: nothing sizes a buffer from them."""
    cd = lambda a, b: -(-a // b)                                       # noqa: E731
    probs = []
    for n0, n1, mutual in sizes:
        probs.append((int(n0), int(n1), 0))
        if mutual:
            probs.append((int(n1), int(n0), 1))
    want = min(max(cd(512, sum(cd(nx, 128) for nx, _, _ in probs)), 1), 8)
    csplits, items = [], 0
    for nx, ny, second in probs:
        tiles = cd(ny, 128)
        tiles_per = cd(tiles, min(want, tiles))
        csplit = cd(tiles, tiles_per)
        csplits.append(csplit)
        items += cd(nx, 128) * csplit
    total = _aux_layout(AUX_GUIDED_MATCH, (flags, len(sizes), *(int(v) for s in sizes for v in s)))[2]
    return dict(bytes=total, csplit=csplits, items=items)


def _f32_bits(v) -> int:
    return int(np.float32(v).view(np.uint32))


def guided_table(items) -> np.ndarray:
    """The HOST table of GIMS_AUX_GUIDED_MATCH (include/gims_hip.h): int64 [P, GUIDED_TABLE_WORDS].  items: dicts keyed by the words of
    GUIDED_WORD -- device tensors or raw addresses for the pointers (None -> 0), numbers for the rest; `thresh`, `threshold` (the ratio) and
    `max_distance` (None: +inf) are stored as the bits of a float32.  The array must stay alive during the call."""
    tab = np.zeros((len(items), GUIDED_TABLE_WORDS), dtype=np.int64)
    addr = lambda t: 0 if t is None else (int(t) if isinstance(t, (int, np.integer)) else t.data_ptr())      # noqa: E731
    for p, it in enumerate(items):
        for name, k in GUIDED_WORD.items():
            v = it.get(name)
            if name in ("lda", "ldb", "n0", "n1", "d", "kind", "reserved"):
                tab[p, k] = int(v or 0)
            elif name == "mutual":
                tab[p, k] = int(bool(v))
            elif name in ("thresh", "threshold", "max_distance"):
                tab[p, k] = _f32_bits(float("inf") if (v is None and name == "max_distance") else v)
            else:
                tab[p, k] = addr(v)
    return tab


def op_guided_match(table: np.ndarray, work, work_bytes: int, flags: int = 0) -> Op:
    """GIMS_AUX_GUIDED_MATCH as an op of gims_run_ops (include/gims_hip.h): the one way to reach it.  table: guided_table's HOST array (keep
    it alive while the op is run); work: uint8 [work_bytes] on the device, 256-byte aligned."""
    return op_aux(AUX_GUIDED_MATCH, (int(table.ctypes.data), work, None, None, None, None), (table.shape[0], flags, work_bytes, 0, 0, 0), (0.0, 0.0))


def guided_match(items, flags: int = 0, work=None):
    """Guided matching of a batch of pairs on the device (csrc/nn.hip).  items: dicts with device tensors a [n0, d] / b [n1, d]
    (float32, rows contiguous), kpts0 [n0, 2] / kpts1 [n1, 2] (float32, contiguous), model float32 [9] (or [3, 3]), kind ('homography' / 0 or
    'fundamental' / 1), optionally ok (a float32 tensor whose first element is read), prior int64 [n0], prior_mask uint8 [n0], prior_scores
    float32 [n0]; `mutual`, `thresh`, `threshold`, `max_distance`; and the outputs of GUIDED_OUTPUTS [n0], info int32 [8], with `mutual` also
    cnn1 int32 [n1] and matches1 int64 [n1].  One asynchronous call; returns (workspace, table): keep both alive until the stream has passed."""
    rows = []
    for it in items:
        a, b = it["a"], it["b"]
        if a.dtype != torch.float32 or b.dtype != torch.float32 or a.dim() != 2 or b.dim() != 2 or a.stride(1) != 1 or b.stride(1) != 1:
            raise GimsHipError("guided_match: a / b must be float32 [n, d] with contiguous rows")
        n0, n1 = int(a.shape[0]), int(b.shape[0])
        for k, n in ((it["kpts0"], n0), (it["kpts1"], n1)):
            if k.dtype != torch.float32 or not k.is_contiguous() or tuple(k.shape) != (n, 2):
                raise GimsHipError("guided_match: kpts0 / kpts1 must be contiguous float32 [n0, 2] / [n1, 2]")
        if it["model"].dtype != torch.float32 or it["model"].numel() != 9 or not it["model"].is_contiguous():
            raise GimsHipError("guided_match: model must be 9 contiguous float32")
        kind = verify_model(it.get("kind", "fundamental"))
        mutual = bool(it.get("mutual", True))
        for name, dt in GUIDED_OUTPUTS + ((("cnn1", torch.int32), ("matches1", torch.int64)) if mutual else ()):
            n = n1 if name in ("cnn1", "matches1") else n0
            if it[name].dtype != dt or it[name].numel() < n or not it[name].is_contiguous():
                raise GimsHipError(f"guided_match: output {name} must be a contiguous {dt} tensor of {n} elements")
        if it["info"].dtype != torch.int32 or it["info"].numel() < 8:
            raise GimsHipError("guided_match: info must be int32 [8]")
        for name, dt in (("prior", torch.int64), ("prior_mask", torch.uint8), ("prior_scores", torch.float32)):
            t = it.get(name)
            if t is not None and (t.dtype != dt or t.numel() != n0 or not t.is_contiguous()):
                raise GimsHipError(f"guided_match: {name} must be a contiguous {dt} tensor of n0 elements")
        if it.get("ok") is not None and it["ok"].dtype != torch.float32:
            raise GimsHipError("guided_match: ok must be a float32 tensor")
        lda, ldb = (a.stride(0) if n0 > 1 else a.shape[1]), (b.stride(0) if n1 > 1 else b.shape[1])
        rows.append(dict(it, lda=lda, ldb=ldb, n0=n0, n1=n1, d=int(a.shape[1]), kind=kind, mutual=mutual, thresh=it.get("thresh", 3.0),
                         threshold=it.get("threshold", 0.8), max_distance=it.get("max_distance"), reserved=0))
    need = guided_layout([(r["n0"], r["n1"], r["mutual"]) for r in rows], flags)["bytes"]
    if work is None or work.numel() * work.element_size() < need:
        work = torch.empty(need, dtype=torch.uint8, device=items[0]["a"].device)
    tab = guided_table(rows)
    run_ops(make_ops([op_guided_match(tab, work, work.numel() * work.element_size(), flags)]))
    return work, tab


# ------------------------------------------------------------------------------------------------ CAR-HyNet ops (NHWC f32)
def pack_conv3_fragments(w: torch.Tensor) -> torch.Tensor:
    """[cout][cin][3][3] float64/float32 (CPU) -> the bf16 fragment layout of gims_ch_conv_block:
    [step = (ky*3+kx) * cin/16 + ks][nb][plane hi|lo][lane = lh*32 + li][8]."""
    o, i = w.shape[0], w.shape[1]
    assert o % 32 == 0 and i % 16 == 0 and w.shape[2:] == (3, 3)
    x = w.double().permute(2, 3, 1, 0).reshape(9, i // 16, 2, 8, o // 32, 32)         # [tap][ks][lh][e][nb][li]
    x = x.permute(0, 1, 4, 2, 5, 3).reshape(9 * (i // 16), o // 32, 64, 8).float()     # [step][nb][lane][e]
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return torch.stack([hi, lo], dim=2).contiguous()                                   # [step][nb][plane][lane][8]


def _gate_table(G):
    """CoordAtt gate weights G = dict(w1, b1, wh, bh, ww, bw) as the host array of six device pointers of gims_ch_conv_block*; None: no gates."""
    return (C.c_void_p * 6)(*[G[k].data_ptr() for k in ("w1", "b1", "wh", "bh", "ww", "bw")]) if G is not None else None


def ch_conv_block(xs, n, hin, cin, cout, stride, L, F, tau, G=None, y=None, y_split=None):
    """Fused 3x3 convolution + FRN (+ CoordAtt gates G) + TLU, one workgroup per patch (gims_ch_conv_block).
    xs: SPL32 pixel rows [n*hin*hin, >= 2 cin]; L: dict(wp=packed fragments on the device, b=bias)."""
    _check(load().gims_ch_conv_block(_p(xs), xs.stride(0), n, hin, cin, cout, stride, _p(L["wp"]), _p(L["b"]), _p(F["w"]), _p(F["b"]), float(F["eps"]), _gate_table(G),
                                     _p(tau), _p(y), _p(y_split), y_split.stride(0) if y_split is not None else 0, _stream()), "gims_ch_conv_block")
    return y if y is not None else y_split


def ch_conv_block_first(patches, F0, tau0, L, F, tau, G, y_split):
    """Layer 1 in one kernel: patches [n, 32, 32, 3] f32 -> FRN(3) + TLU(3) -> conv 3->32 -> FRN + CoordAtt + TLU -> SPL32 rows.
    L: dict(wp=fragments of the weights with the input channels zero-padded to 16, b=bias)."""
    n = patches.shape[0]
    _check(load().gims_ch_conv_block_first(_p(_dev(patches, torch.float32)), n, _p(F0["w"]), _p(F0["b"]), float(F0["eps"]), _p(tau0), _p(L["wp"]), _p(L["b"]),
                                           _p(F["w"]), _p(F["b"]), float(F["eps"]), _gate_table(G), _p(tau), None, _p(y_split), y_split.stride(0), _stream()),
           "gims_ch_conv_block_first")
    return y_split


def ch_sandglass(x, S, out_split):
    """S: dict with the 14 weight tensors of gims_ch_sandglass in order (key 'ptrs': list of tensors)."""
    n, h, w, c = x.shape
    arr = (C.c_void_p * 14)(*[t.data_ptr() for t in S["ptrs"]])
    _check(load().gims_ch_sandglass(_p(_dev(x, torch.float32)), n, h, c, arr, _p(out_split), out_split.stride(0), _stream()), "gims_ch_sandglass")
    return out_split


def ch_l2norm(x, eps, y):
    rows, c = x.shape
    _check(load().gims_ch_l2norm(_p(_dev(x, torch.float32)), rows, c, float(eps), _p(y), _stream()), "gims_ch_l2norm")
    return y


def train_loss(items, kept0, kept1, gt: torch.Tensor, alpha: float, pos_weight: float, neg_weight: float):
    """forward_train's loss from the solved potentials (gims_train_loss).  items: the per-pair dicts given to make_ot_problems
    (scores, n, m, uv); kept0 / kept1: per pair the int32 device tensors of kept original ids; gt: [K, 3] int64 device tensor
    (b, i0, i1).  Returns (out3 f32 [3] = loss, pos, neg; per-row loss vector [K])."""
    dev = gt.device
    assert gt.dtype == torch.int64 and gt.is_contiguous() and (gt.numel() == 0 or gt.shape[1] == 3)
    B = len(items)
    arr = (LossPair * B)()
    for i, (it, k0, k1) in enumerate(zip(items, kept0, kept1)):
        assert k0.dtype == torch.int32 and k1.dtype == torch.int32 and k0.numel() == it["n"] and k1.numel() == it["m"]
        arr[i] = LossPair(_p(it["scores"]), it["scores"].stride(0), it["n"], it["m"], _p(it["uv"]), _p(k0), _p(k1))
    tab = upload(np.frombuffer(bytes(arr), dtype=np.uint8), dev)
    K = int(gt.shape[0])
    loss_vec = torch.empty(max(K, 1), dtype=torch.float32, device=dev)
    tag = torch.empty(max(K, 1) + 2 * B, dtype=torch.int32, device=dev)      # row classes, then 2 group sizes per batch element
    out3 = torch.empty(3, dtype=torch.float32, device=dev)
    _check(load().gims_train_loss(_p(tab), B, _p(gt), K, float(alpha), float(pos_weight), float(neg_weight), _p(loss_vec), _p(tag), _p(out3),
                                  _stream()), "gims_train_loss")
    train_loss.last = dict(table=tab, tag=tag, gt=gt, K=K, B=B)          # what the gradient entry points need again
    return out3, loss_vec[:K]


def sinkhorn_history(items, alpha: float, iters: int):
    """The streamed Sinkhorn solve with the potentials after every iteration recorded (gims_sinkhorn_history): returns the list
    of history buffers; every item's ``uv`` holds the final potentials afterwards (what gims_train_loss reads)."""
    lib = load()
    dev = items[0]["scores"].device
    probs = make_ot_problems(items)
    work = torch.empty(sinkhorn_workspace_bytes(probs), dtype=torch.uint8, device=dev)
    hists = [torch.zeros(int(lib.gims_sinkhorn_history_floats(it["n"], it["m"], iters)), dtype=torch.float32, device=dev) for it in items]
    hp = (C.c_void_p * len(items))(*[h.data_ptr() for h in hists])
    _check(lib.gims_sinkhorn_history(probs, len(items), float(alpha), int(iters), hp, _p(work), work.numel(), _stream()), "gims_sinkhorn_history")
    return hists


def sinkhorn_score_gradients(items, alpha: float, iters: int, pos_weight: float, neg_weight: float, loss_state, hists=None):
    """d loss / d scores (list of [n, m] views with pitch m + 1) and d loss / d bin_score (0-dim tensor) for the loss of
    ``train_loss`` (whose ``last`` state is passed in): a recorded streamed forward solve (``hists`` from sinkhorn_history, made
    here when absent), the loss gradient scattered into zeroed (n+1) x (m+1) buffers (gims_train_loss_grad), the reverse sweep
    through the unrolled iterations (gims_sinkhorn_backward)."""
    lib = load()
    dev = items[0]["scores"].device
    probs = make_ot_problems(items)
    if hists is None:
        hists = sinkhorn_history(items, alpha, iters)
    hp = (C.c_void_p * len(items))(*[h.data_ptr() for h in hists])
    dzs = [torch.zeros((it["n"] + 1, it["m"] + 1), dtype=torch.float32, device=dev) for it in items]
    dz_tab = upload(np.asarray([d.data_ptr() for d in dzs], dtype=np.int64), dev)
    st = loss_state
    _check(lib.gims_train_loss_grad(_p(st["table"]), st["B"], _p(st["gt"]), st["K"], float(alpha), _p(st["tag"]), float(pos_weight), float(neg_weight),
                                    _p(dz_tab), _stream()), "gims_train_loss_grad")
    bw = torch.empty(int(lib.gims_sinkhorn_backward_workspace_bytes(probs, len(items))), dtype=torch.uint8, device=dev)
    dalpha = torch.empty(len(items), dtype=torch.float32, device=dev)
    dp = (C.c_void_p * len(items))(*[d.data_ptr() for d in dzs])
    _check(lib.gims_sinkhorn_backward(probs, len(items), float(alpha), int(iters), hp, dp, _p(dalpha), _p(bw), bw.numel(), _stream()),
           "gims_sinkhorn_backward")
    return [d[:it["n"], :it["m"]] for d, it in zip(dzs, items)], dalpha.sum()


def pyramid_layout(h: int, w: int, c: int = 3):
    """(levels [(offset, h, w)], pyramid bytes, scratch bytes) of gims_pyramid_layout."""
    n, pb, sb = C.c_int32(), C.c_size_t(), C.c_size_t()
    _check(load().gims_pyramid_layout(h, w, c, None, 0, C.byref(n), C.byref(pb), C.byref(sb)), "gims_pyramid_layout")
    arr = (PyrLevel * n.value)()
    _check(load().gims_pyramid_layout(h, w, c, arr, n.value, C.byref(n), C.byref(pb), C.byref(sb)), "gims_pyramid_layout")
    return arr, int(pb.value), int(sb.value)


def pyramid_build(img: torch.Tensor):
    """img uint8 [H, W, 3] on the device -> (pyramid buffer uint8, ctypes level table, device level table)."""
    assert img.dtype == torch.uint8 and img.is_cuda and img.dim() == 3 and img.is_contiguous()
    h, w, c = img.shape
    levels, pb, sb = pyramid_layout(h, w, c)
    pyr = torch.empty(pb, dtype=torch.uint8, device=img.device)
    scratch = torch.empty(sb, dtype=torch.uint8, device=img.device)
    _check(load().gims_pyramid_build(_p(img), h, w, c, _p(pyr), _p(scratch), _stream()), "gims_pyramid_build")
    dev_levels = upload(np.frombuffer(bytes(levels), dtype=np.uint8), img.device)
    return pyr, levels, dev_levels


def patch_extract(pyr: torch.Tensor, dev_levels: torch.Tensor, n_levels: int, kp4: torch.Tensor, kp_octave: torch.Tensor):
    """kp4 f32 [N, 4] (x, y, size, angle), kp_octave int32 [N] on the device -> (patches f32 [N, 32, 32, 3], bad-count tensor)."""
    assert kp4.dtype == torch.float32 and kp_octave.dtype == torch.int32 and kp4.is_contiguous() and kp4.is_cuda and kp_octave.is_cuda
    n = int(kp4.shape[0])
    out = torch.empty((n, 32, 32, 3), dtype=torch.float32, device=pyr.device)
    bad = torch.empty(1, dtype=torch.int32, device=pyr.device)
    _check(load().gims_patch_extract(_p(pyr), _p(dev_levels), n_levels, _p(kp4), _p(kp_octave), n, _p(out), _p(bad), _stream()), "gims_patch_extract")
    return out, bad

def sift_layout(h: int, w: int) -> SiftInfo:
    """gims_sift_layout (host only): octave sizes, level offsets, blur sigmas, kernel sizes and half kernels for an h x w image."""
    info = SiftInfo()
    _check(load().gims_sift_layout(int(h), int(w), C.byref(info)), "gims_sift_layout")
    return info


def _sift_images(images: torch.Tensor):
    t = images if torch.is_tensor(images) else torch.as_tensor(images)
    if t.dtype != torch.uint8 or t.dim() not in (3, 4) or (t.dim() == 4 and t.shape[3] not in (1, 3)):
        raise ValueError("SIFT detection takes uint8 [B, H, W, 3] (BGR) or [B, H, W] (gray) images")
    if t.dim() == 3:
        t = t.unsqueeze(-1)
    return t.contiguous()


def sift_pyramid(images: torch.Tensor):
    """The Gaussian and DoG levels gims_sift_detect works on (a test hook): images uint8 [B, H, W, 3] / [B, H, W] on the device ->
    (gauss, dog) with gauss[b][o][i] float32 [h_o, w_o] (6 per octave) and dog[b][o][i] (5 per octave), views of one buffer."""
    t = _sift_images(images)
    assert t.is_cuda
    B, H, W, c = t.shape
    L = sift_layout(H, W)
    pyr = sift_pyramid_buffer(t)
    gauss, dog = [], []
    for b in range(B):
        base = b * L.image_floats
        gb, db = [], []
        for o in range(L.n_octaves):
            h, w = L.oct_h[o], L.oct_w[o]
            gb.append([pyr[base + L.gauss_offset[o] + i * h * w: base + L.gauss_offset[o] + (i + 1) * h * w].view(h, w) for i in range(6)])
            db.append([pyr[base + L.dog_offset[o] + i * h * w: base + L.dog_offset[o] + (i + 1) * h * w].view(h, w) for i in range(5)])
        gauss.append(gb)
        dog.append(db)
    return gauss, dog


def sift_detect(images: torch.Tensor, cand_cap: int | None = None, return_pyramid: bool = False):
    """OpenCV SIFT detect on the device for a batch of equal-size images: uint8 [B, H, W, 3] (BGR) or [B, H, W] ->
    one dict per image of device tensors pt f32 [n, 2], size, angle, response f32 [n], octave int32 [n], in OpenCV's output order.
    Every pixel and keypoint is computed by the HIP kernels; the stable key sorts between them are torch plumbing.  The one host
    read per call is the final count (with the extremum count: when it exceeds the candidate capacity the buffers grow and the
    call repeats, so nothing is dropped).  return_pyramid=True: (that list, pyr) with the float pyramid buffer [B * image_floats] the
    call filled, which sift_describe reads (gims_sift_layout has its layout)."""
    t = _sift_images(images)
    assert t.is_cuda
    B, H, W, c = t.shape
    L = sift_layout(H, W)
    dev = t.device
    lib = load()
    pyr = torch.empty(B * L.image_floats, dtype=torch.float32, device=dev)
    scratch = torch.empty(B * L.scratch_floats, dtype=torch.float32, device=dev)
    cap = int(cand_cap) if cand_cap else B * max(4096, H * W // 16)
    stat = torch.empty(B + 1, dtype=torch.int32, device=dev)          # counts per image, then the extremum count
    while True:
        S = cap * SIFT_SLOTS
        cand = torch.empty(cap * 4, dtype=torch.int32, device=dev)
        sf = torch.empty(5 * S, dtype=torch.float32, device=dev)
        sk = torch.empty(3 * S, dtype=torch.int64, device=dev)
        si = torch.empty(2 * S, dtype=torch.int32, device=dev)
        stat.zero_()
        _check(lib.gims_sift_detect(_p(t), B, H, W, c, _p(pyr), _p(scratch), _p(cand), cap, _p(stat[B:]), _p(sf), _p(sk), _p(si), _stream()),
               "gims_sift_detect")
        perm = torch.sort(sk[:S], stable=True)[1]                           # octave desc, response desc
        for key in (sk[S:2 * S], sk[2 * S:], si[S:]):                        # size desc, angle asc; x asc, y asc; image
            perm = perm[torch.sort(key[perm], stable=True)[1]]
        keep = torch.empty(S, dtype=torch.int32, device=dev)
        _check(lib.gims_sift_compact(_p(perm), S, B, cap, _p(sf), _p(sk), _p(si), _p(keep), None, None, None, None, None, None, None,
                                     _stream()), "gims_sift_compact")
        pos = torch.cumsum(keep, 0)
        pt = torch.empty((S, 2), dtype=torch.float32, device=dev)
        size, angle, resp = (torch.empty(S, dtype=torch.float32, device=dev) for _ in range(3))
        octave = torch.empty(S, dtype=torch.int32, device=dev)
        _check(lib.gims_sift_compact(_p(perm), S, B, cap, _p(sf), _p(sk), _p(si), _p(keep), _p(pos), _p(pt), _p(size), _p(angle), _p(resp),
                                     _p(octave), _p(stat), _stream()), "gims_sift_compact")
        host = stat.cpu().tolist()
        if host[B] <= cap:
            break
        cap = host[B] + host[B] // 4 + 1024
    out, off = [], 0
    for b in range(B):
        n = host[b]
        out.append({"pt": pt[off:off + n], "size": size[off:off + n], "angle": angle[off:off + n], "response": resp[off:off + n],
                    "octave": octave[off:off + n]})
        off += n
    return (out, pyr) if return_pyramid else out


def sift_pyramid_buffer(images: torch.Tensor):
    """gims_sift_pyramid alone: images uint8 [B, H, W, 3] / [B, H, W] on the device -> the float pyramid buffer [B * image_floats] that
    sift_detect(return_pyramid=True) also hands back (bit for bit: detection runs the same call first)."""
    t = _sift_images(images)
    assert t.is_cuda
    B, H, W, c = t.shape
    L = sift_layout(H, W)
    pyr = torch.empty(B * L.image_floats, dtype=torch.float32, device=t.device)
    scratch = torch.empty(B * L.scratch_floats, dtype=torch.float32, device=t.device)
    _check(load().gims_sift_pyramid(_p(t), B, H, W, c, _p(pyr), _p(scratch), _stream()), "gims_sift_pyramid")
    return pyr


def op_sift_describe(pyr, h, w, n_images, kp4, octave, image, out, bad) -> Op:
    """The descriptor stage as an op of gims_run_ops (include/gims_hip.h GIMS_AUX_SIFT_DESCRIBE): the one way to reach it."""
    return op_aux(AUX_SIFT_DESCRIBE, (pyr, kp4, octave, image, out, bad), (kp4.shape[0], n_images, h, w, out.stride(0), 0))


def sift_describe(pyr: torch.Tensor, h: int, w: int, n_images: int, kp4: torch.Tensor, octave: torch.Tensor, image: torch.Tensor | None = None):
    """OpenCV's calcSIFTDescriptor over the detector's pyramid (csrc/sift.hip sift_describe_kernel): pyr from
    sift_detect(return_pyramid=True) / sift_pyramid_buffer for n_images images of h x w; kp4 f32 [n, 4] (x, y, size, angle), octave
    int32 [n] and image int32 [n] (None: one image) as detection returns them -> (desc f32 [n, 128], integer-valued 0 .. 255;
    bad int32 [1] on the device: keypoints whose octave / layer / image is outside the pyramid, described as zeros).  This is the
    detectAndCompute descriptor: cv2.SIFT.compute would rebuild a pyramid from the keypoints' octaves, which is not restated.
    Asynchronous; no host read."""
    assert pyr.dtype == torch.float32 and pyr.is_cuda and pyr.is_contiguous()
    assert kp4.dtype == torch.float32 and kp4.is_cuda and kp4.is_contiguous() and kp4.dim() == 2 and kp4.shape[1] == 4
    assert octave.dtype == torch.int32 and octave.is_cuda and octave.is_contiguous() and octave.shape[0] == kp4.shape[0]
    assert image is None or (image.dtype == torch.int32 and image.is_cuda and image.is_contiguous() and image.shape[0] == kp4.shape[0])
    L = sift_layout(h, w)
    assert pyr.numel() >= n_images * L.image_floats, "the pyramid buffer is smaller than n_images pyramids of this image size"
    out = torch.empty((kp4.shape[0], 128), dtype=torch.float32, device=pyr.device)
    bad = torch.zeros(1, dtype=torch.int32, device=pyr.device)
    run_ops(make_ops([op_sift_describe(pyr, h, w, n_images, kp4, octave, image, out, bad)]))
    return out, bad


def _aux_layout(fn: int, sizes):
    """gims_aux_layout (include/gims_hip.h): where the layout routine of auxiliary function fn puts every region of its caller-allocated
    buffer, for the sizes that routine takes.  -> (byte offset of every region, number of output regions, bytes in all).  Host arithmetic
    inside the library: no device is needed."""
    lib = load()
    arr = (C.c_int64 * max(len(sizes), 1))(*[int(s) for s in sizes])
    n_regions, n_outputs, total = C.c_int32(), C.c_int32(), C.c_size_t()
    _check(lib.gims_aux_layout(fn, arr, len(sizes), None, 0, C.byref(n_regions), C.byref(n_outputs), C.byref(total)), "gims_aux_layout")
    offsets = (C.c_int64 * max(n_regions.value, 1))()
    _check(lib.gims_aux_layout(fn, arr, len(sizes), offsets, n_regions.value, C.byref(n_regions), C.byref(n_outputs), C.byref(total)), "gims_aux_layout")
    return list(offsets[:n_regions.value]), n_outputs.value, total.value


# The output regions of the ops that write into one caller-allocated buffer, in the order their layout routines take them: (name, dtype,
# shape) for the sizes gims_aux_layout takes.  The offsets come from the library; these tables only name and type the regions.
def _tri_regions(T, n_obs):
    return (("xyz", torch.float64, (T, 3)), ("max_angle", torch.float32, (T,)), ("rms_error", torch.float32, (T,)), ("n_inliers", torch.int32, (T,)),
            ("obs_error", torch.float32, (n_obs,)), ("status", torch.uint8, (T,)), ("obs_inlier", torch.uint8, (n_obs,)), ("counters", torch.int32, (8,)))


def _resect_regions(m, S, iters):
    return (("pose", torch.float64, (m, 12)), *((k, torch.int32, (m,)) for k in ("n_corr", "ok", "n_inliers", "best_hyp", "best_hyp_inliers", "lo_rounds")),
            ("rms_error", torch.float32, (m,)), ("kp_inlier", torch.uint8, (S,)), ("kp_error", torch.float32, (S,)), ("counters", torch.int32, (8,)))


def _ba_regions(T, n_obs, n_images, iters, n_free):
    return (("xyz", torch.float64, (T, 3)), ("cams", torch.float64, (n_images, TRI_CAMERA_WORDS)), ("obs_error", torch.float32, (n_obs,)),
            ("cam_obs", torch.int32, (n_images,)), ("history", torch.float64, (iters + 1, 2)), ("taken", torch.uint8, (iters,)), ("counters", torch.int32, (8,)))


def _ba_pcg_regions(T, n_obs, n_images, iters, n_free):
    return _ba_regions(T, n_obs, n_images, iters, n_free) + (("cg_used", torch.int32, (iters,)), ("cg_res", torch.float64, (iters,)))


def _ba_focal_regions(T, n_obs, n_images, iters, n_free, n_groups):
    return _ba_pcg_regions(T, n_obs, n_images, iters, n_free) + (("focal_scale", torch.float64, (n_groups,)), ("group_obs", torch.int32, (n_groups,)))


_AUX_REGIONS = {AUX_TRIANGULATE_TRACKS: _tri_regions, AUX_RESECT_IMAGES: _resect_regions, AUX_BUNDLE_ADJUST: _ba_regions,
                AUX_BUNDLE_ADJUST_PCG: _ba_pcg_regions, AUX_BUNDLE_ADJUST_FOCAL: _ba_focal_regions}


def _out_layout(fn: int, sizes) -> dict:
    """BYTE offsets into the one buffer of auxiliary function fn: the name of every output region of _AUX_REGIONS -> its offset, 'outputs' =
    'scratch' = the offset of the kernels' scratch behind the outputs, 'bytes' = the whole buffer.  All numbers are the library's
    (_aux_layout); a region whose extent there is not that of its dtype and shape here raises, so that a table that has drifted from the
    layout routine fails where the buffer is allocated."""
    regions = _AUX_REGIONS[fn](*sizes)
    offsets, n_outputs, total = _aux_layout(fn, sizes)
    if n_outputs != len(regions) or n_outputs >= len(offsets):
        raise GimsHipError(f"auxiliary function {fn}: the library lays out {n_outputs} output regions of {len(offsets)}, the binding names {len(regions)}")
    off = {}
    for r, (name, dt, shape) in enumerate(regions):
        want, got = (math.prod(shape) * dt.itemsize + 255) & ~255, offsets[r + 1] - offsets[r]
        if got != want:
            raise GimsHipError(f"auxiliary function {fn}: region {name}: {got} bytes in the library's layout, {want} for {dt} {list(shape)}")
        off[name] = offsets[r]
    off["outputs"] = off["scratch"] = offsets[n_outputs]
    off["bytes"] = total
    return off


def _out_views(fn: int, sizes, out: torch.Tensor) -> dict:
    """The typed views of the output regions of fn's buffer, by _out_layout."""
    o = _out_layout(fn, sizes)
    return {name: out[o[name]:o[name] + math.prod(shape) * dt.itemsize].view(dt).view(shape) for name, dt, shape in _AUX_REGIONS[fn](*sizes)}


def diou_nms_workspace_bytes(n: int, n_images: int) -> int:
    """The workspace of GIMS_AUX_DIOU_NMS for n keypoints in n_images images (include/gims_hip.h has the formula; the library evaluates it
    with the routine that carves the workspace, csrc/nms.hip nms_layout)."""
    return _aux_layout(AUX_DIOU_NMS, (n, n_images))[2]


def op_diou_nms(kp4, order, offsets, keep, count, work, n_images, height, width, radius, iou_thresh) -> Op:
    """The keypoint thinning as an op of gims_run_ops (include/gims_hip.h GIMS_AUX_DIOU_NMS): the one way to reach it.  radius 0: boxes
    from the keypoint size."""
    return op_aux(AUX_DIOU_NMS, (kp4, order, offsets, keep, count, work), (kp4.shape[0], n_images, height, width, work.numel() * work.element_size(), 0),
                  (radius, iou_thresh))


def diou_nms(kp4: torch.Tensor, order: torch.Tensor, offsets: torch.Tensor, radius: float, iou_thresh: float, height: int, width: int):
    """The reference's process_diou_nms (utils/common.py:720-807) for a batch of images on the device (csrc/nms.hip): kp4
    f32 [n, 4] (x, y, size, angle) of all images, image b holding rows offsets[b] .. offsets[b + 1] - 1 (offsets int32 [n_images + 1] on
    the device); order int32 [n]: per image a permutation of its own (global) rows, the processing order -- descending score.  radius > 0:
    fixed boxes of that side, 0: boxes from the keypoint size; 0 < iou_thresh < 1; height, width: the extent of the search grid (speed
    only).  -> (keep int32 [n]: per image its result rows, global, then -1; count int32 [n_images + 1]: kept per image, then the number
    of bad keypoints -- non-finite, negative size in size mode, order entries outside their image).  Asynchronous; no host read."""
    assert kp4.dtype == torch.float32 and kp4.is_cuda and kp4.is_contiguous() and kp4.dim() == 2 and kp4.shape[1] == 4
    assert order.dtype == torch.int32 and order.is_cuda and order.is_contiguous() and order.shape == (kp4.shape[0],)
    assert offsets.dtype == torch.int32 and offsets.is_cuda and offsets.is_contiguous() and offsets.dim() == 1 and offsets.numel() >= 2
    n, n_images = kp4.shape[0], offsets.numel() - 1
    keep = torch.empty(n, dtype=torch.int32, device=kp4.device)
    count = torch.zeros(n_images + 1, dtype=torch.int32, device=kp4.device)
    work = torch.empty(diou_nms_workspace_bytes(n, n_images), dtype=torch.uint8, device=kp4.device)
    run_ops(make_ops([op_diou_nms(kp4, order, offsets, keep, count, work, n_images, height, width, radius, iou_thresh)]))
    return keep, count


def assemble_table(segments, n_rows: int, k: int, device) -> np.ndarray:
    """The segment table of GIMS_AUX_ASSEMBLE_ROWS (include/gims_hip.h) as a host array int64 [n_seg, 4] = {source address, source pitch
    in floats, rows, first destination row}, ascending by first destination row.  segments: (source f32 [rows, >= k] with unit stride along
    the row, first destination row) each; the same source may appear any number of times.  Checks what the device cannot: dtype, layout,
    alignment and device of every source, and that the destination ranges are disjoint and inside 0 .. n_rows - 1 (ValueError)."""
    device = torch.device(device)
    tab = np.empty((len(segments), 4), dtype=np.int64)
    for s, (src, first) in enumerate(segments):
        if src.dtype != torch.float32:
            raise ValueError(f"assemble_rows: segment {s}: the source is {src.dtype}, not float32")
        if src.dim() != 2 or src.shape[1] < k or (src.shape[1] > 1 and src.stride(1) != 1):
            raise ValueError(f"assemble_rows: segment {s}: the source must be [rows, >= {k}] with unit stride along the row, got {tuple(src.shape)} / {src.stride()}")
        if src.device != device and not (src.device.type == device.type and None in (src.device.index, device.index)):
            raise ValueError(f"assemble_rows: segment {s}: the source is on {src.device}, the outputs on {device}")
        pitch = src.stride(0) if src.shape[0] > 1 else max(src.stride(0), k)
        if src.data_ptr() % 16 or pitch % 4 or pitch < 0:
            raise ValueError(f"assemble_rows: segment {s}: the source must be 16-byte aligned with a row pitch that is a multiple of 4 floats")
        if first < 0 or first + src.shape[0] > n_rows:
            raise ValueError(f"assemble_rows: segment {s}: destination rows {first} .. {first + src.shape[0] - 1} lie outside the {n_rows} rows of the output")
        tab[s] = (src.data_ptr(), pitch, src.shape[0], first)
    tab = tab[np.argsort(tab[:, 3], kind="stable")]
    ends = tab[:-1, 3] + tab[:-1, 2]
    bad = np.nonzero(ends > tab[1:, 3])[0]
    if len(bad):
        raise ValueError(f"assemble_rows: the destination rows {tab[bad[0], 3]} .. {ends[bad[0]] - 1} and those from {tab[bad[0] + 1, 3]} on overlap")
    return tab


def op_assemble_rows(table, n_seg: int, n_rows: int, k: int, out, out_split) -> Op:
    """GIMS_AUX_ASSEMBLE_ROWS as an op of gims_run_ops (include/gims_hip.h): the one way to reach it.  table: the device copy of
    assemble_table's array; out f32 [n_rows, >= k] and / or out_split SPL32 bf16 [n_rows, >= 2 k]."""
    return op_aux(AUX_ASSEMBLE_ROWS, (table, out, out_split), (n_seg, n_rows, k, 0 if out is None else out.stride(0),
                                                               0 if out_split is None else out_split.stride(0), 0))


def upload_large(arr: np.ndarray, device) -> torch.Tensor:
    """upload() for a table of any size: in pieces of at most 1 MiB (what one gims_upload_table call takes) into one device buffer."""
    a = np.ascontiguousarray(arr).reshape(-1)
    raw = a.view(np.uint8)
    step = 1 << 20
    if raw.nbytes <= step:
        return upload(arr, device)
    buf = torch.empty(((raw.nbytes + 15) // 16 * 16 + 16,), dtype=torch.uint8, device=device)
    for o in range(0, raw.nbytes, step):
        upload(raw[o:o + step], device, out=buf[o:])
    return buf[:raw.nbytes].view(_NP2TORCH[a.dtype.name]).view(arr.shape)


def assemble_rows(segments, out, out_split, k: int):
    """Fill rows of out (f32 [n_rows, >= k], or None) and out_split (its SPL32 copy, bf16 [n_rows, >= 2 k], or None) from stores of encoded
    rows in ONE launch (csrc/features.hip): segments = [(source f32 [rows, >= k], first destination row)], see
    assemble_table.  Rows that no segment covers are left as they are.  Asynchronous; returns what must stay alive until the launch has
    run: the device table (the sources and outputs are the caller's)."""
    ref = out if out is not None else out_split
    if ref is None:
        raise ValueError("assemble_rows: out and out_split are both None")
    n_rows = ref.shape[0]
    if out is not None and (out.dtype != torch.float32 or out.dim() != 2 or out.shape[1] < k or out.stride(1) != 1):
        raise ValueError("assemble_rows: out must be float32 [n_rows, >= k] with unit stride along the row")
    if out_split is not None and (out_split.dtype != torch.bfloat16 or out_split.dim() != 2 or out_split.shape[0] != n_rows or out_split.shape[1] < 2 * k
                                  or out_split.stride(1) != 1):
        raise ValueError("assemble_rows: out_split must be bfloat16 [n_rows, >= 2 k] with unit stride along the row")
    tab = assemble_table(segments, n_rows, k, ref.device)
    dev_tab = upload_large(tab, ref.device) if len(tab) else None
    run_ops(make_ops([op_assemble_rows(dev_tab, len(tab), n_rows, k, out, out_split)]))
    return dev_tab


def _same_device(t: torch.Tensor, device: torch.device) -> bool:
    return t.device == device or (t.device.type == device.type and None in (t.device.index, device.index))


def tracks_table(entries, counts, device) -> np.ndarray:
    """The pair table of GIMS_AUX_BUILD_TRACKS (include/gims_hip.h) as a host array int64 [n_pairs + 1, 8] = {address of matches0, of the
    scores or 0, of the mask or 0, n_a, n_b, start_a, start_b, first row}, the last entry holding the total number of rows.  entries:
    (a, b, matches0, scores or None, mask or None) each -- image indices into counts (the keypoint count of every image) and 1-D contiguous
    tensors of counts[a] elements, int64 / float32 / uint8.  Checks what the device cannot (ValueError): the indices, dtype, layout, length
    and device of every tensor, and that all rows together stay below 2^31."""
    device = torch.device(device)
    counts = [int(c) for c in counts]
    if any(c < 0 for c in counts):
        raise ValueError("build_tracks: a keypoint count is negative")
    start = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
    tab = np.zeros((len(entries) + 1, TRACKS_TABLE_WORDS), dtype=np.int64)
    row = 0
    for p, (a, b, m0, sc, mask) in enumerate(entries):
        if not (0 <= a < len(counts) and 0 <= b < len(counts)):
            raise ValueError(f"build_tracks: pair {p}: the image index of ({a}, {b}) is out of range (0 .. {len(counts) - 1})")
        for name, t, dt in (("matches0", m0, torch.int64), ("matching_scores0", sc, torch.float32), ("the inlier mask", mask, torch.uint8)):
            if t is None and name != "matches0":
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != dt:
                raise ValueError(f"build_tracks: pair {p}: {name} must be a {dt} tensor, got {getattr(t, 'dtype', type(t).__name__)}")
            if t.dim() != 1 or (t.numel() > 1 and t.stride(0) != 1):
                raise ValueError(f"build_tracks: pair {p}: {name} must be 1-D with unit stride, got {tuple(t.shape)} / {t.stride()}")
            if t.numel() != counts[a]:
                raise ValueError(f"build_tracks: pair {p}: {name} has {t.numel()} elements, image {a} has {counts[a]} keypoints")
            if not _same_device(t, device):
                raise ValueError(f"build_tracks: pair {p}: {name} is on {t.device}, the outputs on {device}")
        tab[p] = (m0.data_ptr(), 0 if sc is None else sc.data_ptr(), 0 if mask is None else mask.data_ptr(), counts[a], counts[b], start[a], start[b], row)
        row += counts[a]
    if row > 2 ** 31 - 1 or start[-1] > 2 ** 30:
        raise ValueError(f"build_tracks: {row} rows / {start[-1]} keypoints in all: at most 2^31 - 1 rows and 2^30 keypoints")
    tab[len(entries), TRACKS_TABLE_WORDS - 1] = row
    return tab


def tracks_work_bytes(n_pairs: int, n_images: int, n: int) -> int:
    """The workspace of GIMS_AUX_BUILD_TRACKS for n keypoints in all (include/gims_hip.h has the formula; csrc/tracks.hip trk_layout carves
    it and, through gims_aux_layout, sizes it).  It depends on neither n_pairs nor n_images: the pair table is read where it lies."""
    return _aux_layout(AUX_BUILD_TRACKS, (n,))[2]


def tracks_huge(n: int) -> int:
    """The component size above which GIMS_AUX_BUILD_TRACKS ranks a component by a prefix count over the nodes (H of include/gims_hip.h)."""
    return max(TRACKS_LONG_SEGMENT, n // 1024)


def tracks_out_layout(n: int):
    """Word offsets into the int32 output buffer of GIMS_AUX_BUILD_TRACKS (include/gims_hip.h): (indptr, obs_image, obs_keypoint, conflict,
    total words); conflict is uint8 [n // 2] packed into its words."""
    cap_t = n // 2
    return 0, cap_t + 1, cap_t + 1 + n, cap_t + 1 + 2 * n, cap_t + 1 + 2 * n + (cap_t + 3) // 4


def op_build_tracks(table, start, track_of, out, counters, work, n_pairs: int, n_images: int, n: int, min_length: int = 2,
                    keep_conflicting: bool = False, min_score: float = 0.0) -> Op:
    """GIMS_AUX_BUILD_TRACKS as an op of gims_run_ops (include/gims_hip.h): the one way to reach it.  table: the device copy of
    tracks_table's array; start int32 [n_images + 1]; track_of int32 [n]; out int32 [tracks_out_layout(n)[-1]]; counters int32 [8]; work
    uint8 [tracks_work_bytes(...)]."""
    return op_aux(AUX_BUILD_TRACKS, (table, start, track_of, out, counters, work),
                  (n_pairs, n_images, n, int(min_length) | (TRACKS_KEEP_CONFLICTING if keep_conflicting else 0),
                   0 if work is None else work.numel() * work.element_size(), 0), (min_score,))


def build_tracks(entries, counts, device, min_length: int = 2, keep_conflicting: bool = False, min_score: float | None = None):
    """Multi-view tracks from the matches of an image set on the device (csrc/tracks.hip): entries and counts as
    tracks_table takes them; min_score None: no entry's scores are read.  -> (track_of int32 [N], out int32 -- see tracks_out_layout --,
    counters int32 [8] -- TRACKS_COUNTERS --, start int32 [n_images + 1], and what must stay alive until the launches have run).
    Asynchronous; no host read: the caller reads the counters to size its views."""
    if min_score is None:
        entries = [(a, b, m0, None, mask) for a, b, m0, _, mask in entries]
    tab = tracks_table(entries, counts, device)
    n_images, n = len(counts), int(sum(int(c) for c in counts))
    start = upload(np.concatenate([[0], np.cumsum([int(c) for c in counts])]).astype(np.int32), device)
    dev_tab = upload_large(tab, device)
    track_of = torch.full((n,), -1, dtype=torch.int32, device=device)       # (the op leaves it alone when there is nothing to join)
    out = torch.empty(tracks_out_layout(n)[-1], dtype=torch.int32, device=device)
    counters = torch.empty(8, dtype=torch.int32, device=device)
    work = torch.empty(tracks_work_bytes(len(entries), n_images, n), dtype=torch.uint8, device=device)
    run_ops(make_ops([op_build_tracks(dev_tab, start, track_of, out, counters, work, len(entries), n_images, n, min_length, keep_conflicting,
                                      0.0 if min_score is None else min_score)]))
    return track_of, out, counters, start, (dev_tab, work, entries)


def pairs_pool(ms) -> int:
    """Rows of the pooled int8 matrix of GIMS_AUX_SELECT_PAIRS for images of ms selected rows each (include/gims_hip.h): every image on a
    multiple of 32 rows, the whole on a multiple of PAIRS_QUERY_TILE."""
    rows = max(sum((int(m) + 31) // 32 * 32 for m in ms), 1)
    return (rows + PAIRS_QUERY_TILE - 1) // PAIRS_QUERY_TILE * PAIRS_QUERY_TILE


def pairs_work_bytes(ms, d: int) -> int:
    """The workspace of GIMS_AUX_SELECT_PAIRS (include/gims_hip.h has the formula; csrc/pairs.hip prs_layout carves it and, through
    gims_aux_layout, sizes it)."""
    return _aux_layout(AUX_SELECT_PAIRS, (d, len(ms), *ms))[2]


def pairs_out_layout(n: int, k: int):
    """Word offsets into the int32 output buffer of GIMS_AUX_SELECT_PAIRS: (pairs, pair_votes, total words, cap); cap = min(n k, n (n - 1) / 2)
    pairs at the most, pairs is [cap][2]."""
    cap = min(n * k, n * (n - 1) // 2)
    return 0, 2 * cap, 3 * cap, cap


def pairs_rq(ratio) -> int:
    """The ratio test of GIMS_AUX_SELECT_PAIRS in integers: rint(ratio^2 * 65536) of the float32 ratio, the products in float64."""
    r = float(np.float32(ratio))
    return int(np.rint(r * r * 65536.0))


def pairs_table(images, rq: int, work_bytes: int, scale_given: bool = False) -> np.ndarray:
    """The HOST table of GIMS_AUX_SELECT_PAIRS (include/gims_hip.h): int64 [N + 1, 8].  images: (descriptors, row stride in floats, n, index
    list or None, m) each; descriptors and the index list are device tensors or raw addresses.  The array must stay alive during the call."""
    tab = np.zeros((len(images) + 1, PAIRS_TABLE_WORDS), dtype=np.int64)
    addr = lambda t: 0 if t is None else (int(t) if isinstance(t, int) else t.data_ptr())
    for i, (desc, ld, n, idx, m) in enumerate(images):
        tab[i, :5] = (addr(desc), int(ld), int(n), addr(idx), int(m))
    tab[len(images), :3] = (int(rq), PAIRS_SCALE_GIVEN if scale_given else 0, int(work_bytes))
    return tab


def op_select_pairs(table: np.ndarray, votes, out, counters, work, n: int, d: int, per_image: int, k: int, min_votes: int, scale: float = 0.0) -> Op:
    """GIMS_AUX_SELECT_PAIRS as an op of gims_run_ops (include/gims_hip.h): the one way to reach it.  table: pairs_table's HOST array (keep it
    alive while the op is run); votes int32 [n, n]; out int32 [pairs_out_layout(n, k)[2]]; counters int32 [8]; work uint8 [pairs_work_bytes]."""
    return op_aux(AUX_SELECT_PAIRS, (int(table.ctypes.data), votes, out, counters, work, None), (n, d, per_image, k, min_votes, 0), (scale,))


def select_pairs(images, d: int, device, k: int, per_image: int, rq: int, min_votes: int, scale: float | None = None, out=None):
    """The pair selection of an image set on the device (csrc/pairs.hip): images as pairs_table takes them.  -> (votes int32
    [N, N], out int32 -- see pairs_out_layout --, counters int32 [8], and what must stay alive until the launches have run).  out: a buffer
    to write into instead of a new one.  Asynchronous; no host read."""
    n, ms = len(images), [int(im[4]) for im in images]
    work = torch.empty(pairs_work_bytes(ms, d), dtype=torch.uint8, device=device)
    tab = pairs_table(images, rq, work.numel(), scale is not None)
    votes = torch.empty((n, n), dtype=torch.int32, device=device)
    if out is None:
        out = torch.zeros(max(pairs_out_layout(n, k)[2], 1), dtype=torch.int32, device=device)
    counters = torch.empty(8, dtype=torch.int32, device=device)
    run_ops(make_ops([op_select_pairs(tab, votes, out, counters, work, n, d, per_image, k, min_votes, 0.0 if scale is None else scale)]))
    return votes, out, counters, (work, images)


def triangulate_out_layout(T: int, n_obs: int) -> dict:
    """BYTE offsets into the one buffer of GIMS_AUX_TRIANGULATE_TRACKS (include/gims_hip.h; csrc/triangulate.hip tri_layout carves it and
    gims_aux_layout reports it): xyz float64 [T, 3], max_angle / rms_error float32 [T], n_inliers int32 [T], obs_error float32 [n_obs], status
    uint8 [T], obs_inlier uint8 [n_obs], counters int32 [8]; 'outputs' = the bytes of all of these, 'scratch' = the offset of the kernels'
    scratch behind them (the same value), 'bytes' = the whole buffer.  Every region starts on a 256-byte boundary."""
    return _out_layout(AUX_TRIANGULATE_TRACKS, (T, n_obs))


def triangulate_cameras(K, R, t, counts) -> np.ndarray:
    """The camera records of GIMS_AUX_TRIANGULATE_TRACKS as a host array float64 [n_images, 18] = {fx, fy, cx, cy, R row-major, t, first node,
    n_k}: K [n, 3, 3], R [n, 3, 3], t [n, 3] (world to camera: x_c = R X + t) and the keypoint count of every image."""
    K, R, t = (np.asarray(x, dtype=np.float64) for x in (K, R, t))
    n = len(counts)
    rec = np.zeros((n, TRI_CAMERA_WORDS), dtype=np.float64)
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3] = K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]
    rec[:, 4:13], rec[:, 13:16] = R.reshape(n, 9), t.reshape(n, 3)
    rec[:, 16] = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])[:-1]
    rec[:, 17] = counts
    return rec


def op_triangulate_tracks(indptr, obs_image, obs_keypoint, kpts, cams, out, T: int, n_obs: int, n_images: int, n: int, thresh: float = 4.0,
                          min_angle: float = 1.5, max_hyp: int = 64, refine_iters: int = 10) -> Op:
    """GIMS_AUX_TRIANGULATE_TRACKS as an op of gims_run_ops (include/gims_hip.h): the one way to reach it.  indptr int32 [T + 1], obs_image /
    obs_keypoint int32 [n_obs], kpts float32 [n, 2], cams float64 [n_images, 18], out uint8 [triangulate_out_layout(T, n_obs)['bytes']]."""
    if not (0 <= int(max_hyp) <= 65535 and 0 <= int(refine_iters) <= 255):
        raise ValueError(f"triangulate_tracks: max_hyp = {max_hyp} must be 0 .. 65535 and refine_iters = {refine_iters} 0 .. 255")
    return op_aux(AUX_TRIANGULATE_TRACKS, (indptr, obs_image, obs_keypoint, kpts, cams, out),
                  (T, n_obs, n_images, n, int(max_hyp) | (int(refine_iters) << 16), 0), (thresh, min_angle))


def triangulate_views(out: torch.Tensor, T: int, n_obs: int) -> dict:
    """The typed views of the op's buffer, by triangulate_out_layout."""
    return _out_views(AUX_TRIANGULATE_TRACKS, (T, n_obs), out)


def triangulate_tracks(indptr, obs_image, obs_keypoint, kpts, cams: np.ndarray, thresh: float = 4.0, min_angle: float = 1.5, max_hyp: int = 64,
                       refine_iters: int = 10):
    """Robust triangulation of every track on the device (csrc/triangulate.hip): device tensors as op_triangulate_tracks takes
    them, cams the HOST records of triangulate_cameras, or the same records as a device tensor.  -> (the views of triangulate_views, and
    what must stay alive until the launches have run).  Asynchronous; no host read."""
    device = indptr.device
    T, n_obs, n = indptr.numel() - 1, obs_image.numel(), kpts.shape[0]
    if isinstance(cams, torch.Tensor):                           # the records already on the device (Adjusted.records of bundle_adjust): used where they lie
        if cams.dtype != torch.float64 or cams.device != device or not cams.is_contiguous() or cams.numel() % TRI_CAMERA_WORDS:
            raise ValueError(f"triangulate_tracks: device camera records must be a contiguous float64 tensor [n_images, 18] on {device}")
        rec, dev_cams = cams.view(-1, TRI_CAMERA_WORDS), cams
    else:
        rec = np.ascontiguousarray(cams, dtype=np.float64).reshape(-1, TRI_CAMERA_WORDS)
        dev_cams = upload_large(rec.view(np.uint8).reshape(-1), device).view(torch.float64) if rec.size else torch.zeros(0, dtype=torch.float64, device=device)
    out = torch.empty(triangulate_out_layout(T, n_obs)["bytes"], dtype=torch.uint8, device=device)
    run_ops(make_ops([op_triangulate_tracks(indptr, obs_image, obs_keypoint, kpts, dev_cams, out, T, n_obs, len(rec), n, thresh, min_angle, max_hyp,
                                            refine_iters)]))
    return triangulate_views(out, T, n_obs), (dev_cams, out, indptr, obs_image, obs_keypoint, kpts)


def resect_cameras(K, counts, which=None) -> np.ndarray:
    """The entry records of GIMS_AUX_RESECT_IMAGES as a host array float64 [m, 6] = {fx, fy, cx, cy, first node, n_k}: K [n, 3, 3] and the
    keypoint count of every image of the set, which = the images to resect in the caller's order (default: all of them)."""
    K = np.asarray(K, dtype=np.float64).reshape(-1, 3, 3)
    start = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
    which = np.arange(len(counts), dtype=np.int64) if which is None else np.asarray(which, dtype=np.int64).reshape(-1)
    rec = np.zeros((len(which), RESECT_CAMERA_WORDS), dtype=np.float64)
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3] = K[which, 0, 0], K[which, 1, 1], K[which, 0, 2], K[which, 1, 2]
    rec[:, 4], rec[:, 5] = start[which], np.asarray(counts, dtype=np.int64)[which]
    return rec


def _resect_slots(cams) -> np.ndarray:
    rec = np.asarray(cams, dtype=np.float64).reshape(-1, RESECT_CAMERA_WORDS)
    n_k = rec[:, 5]
    if len(rec) and not (np.isfinite(n_k).all() and (n_k >= 0).all() and (n_k <= 2 ** 30).all() and (n_k == np.floor(n_k)).all() and n_k.sum() <= 2 ** 30):
        raise ValueError("resect_images: every n_k must be an integer in 0 .. 2^30, and their sum at most 2^30")
    return np.concatenate([[0], np.cumsum(n_k.astype(np.int64))])


def resect_out_layout(cams, iters: int = 0) -> dict:
    """BYTE offsets into the one buffer of GIMS_AUX_RESECT_IMAGES (include/gims_hip.h; csrc/resect.hip rs_layout carves it and
    gims_aux_layout reports it) for the host records cams [m, 6]: pose float64 [m, 12], n_corr / ok / n_inliers / best_hyp / best_hyp_inliers / lo_rounds int32 [m], rms_error float32
    [m], kp_inlier uint8 [S], kp_error float32 [S], counters int32 [8], S = the sum of n_k; 'outputs' = the bytes of all of these = 'scratch',
    the offset of the kernels' scratch (which holds iters counters per entry), 'bytes' = the whole buffer; 'slots' = the m + 1 offsets of
    the entries in kp_inlier / kp_error.  Every region starts on a 256-byte boundary."""
    slots = _resect_slots(cams)
    off = _out_layout(AUX_RESECT_IMAGES, (len(slots) - 1, int(slots[-1]), int(iters)))
    off["slots"] = [int(s) for s in slots]
    return off


def op_resect_images(track_of, xyz, use, kpts, cams: np.ndarray, out, n: int, T: int, thresh: float = 4.0, iters: int = 1024, lo_iters: int = 8,
                     min_inliers: int = 12, seed: int = 0) -> Op:
    """GIMS_AUX_RESECT_IMAGES as an op of gims_run_ops (include/gims_hip.h): the one way to reach it.  track_of int32 [n], xyz float64 [T, 3],
    use uint8 [T], kpts float32 [n, 2] on the device; cams the HOST records float64 [m, 6] (C-contiguous; the caller keeps the array alive
    for as long as the op is run); out uint8 [resect_out_layout(cams, iters)['bytes']]."""
    if not (0 <= int(iters) <= 65535 and 0 <= int(lo_iters) <= 255 and 0 <= int(min_inliers) <= 2 ** 30):
        raise ValueError(f"resect_images: iters = {iters} must be 0 .. 65535, lo_iters = {lo_iters} 0 .. 255 and min_inliers = {min_inliers} 0 .. 2^30")
    if not (isinstance(cams, np.ndarray) and cams.dtype == np.float64 and cams.flags["C_CONTIGUOUS"] and cams.size % RESECT_CAMERA_WORDS == 0):
        raise ValueError("resect_images: cams must be a C-contiguous float64 host array [m, 6] (resect_cameras)")
    m = cams.size // RESECT_CAMERA_WORDS
    s64 = int(seed) & 0xFFFFFFFFFFFFFFFF                      # the seed's 64 bits, as the signed word of the table
    return op_aux(AUX_RESECT_IMAGES, (track_of, xyz, use, kpts, cams.ctypes.data if m else None, out),
                  (m, n, T, int(iters) | (int(lo_iters) << 16) | (int(min_inliers) << 24), s64 - (1 << 64) if s64 >> 63 else s64, 0), (thresh, 0.0))


def resect_views(out: torch.Tensor, cams, iters: int = 0) -> dict:
    """The typed views of the op's buffer, by resect_out_layout."""
    slots = [int(s) for s in _resect_slots(cams)]
    return dict(_out_views(AUX_RESECT_IMAGES, (len(slots) - 1, slots[-1], int(iters)), out), slots=slots)


def resect_images(track_of, xyz, use, kpts, cams: np.ndarray, thresh: float = 4.0, iters: int = 1024, lo_iters: int = 8, min_inliers: int = 12,
                  seed: int = 0, n: int | None = None, T: int | None = None):
    """Absolute poses of the entries of cams on the device (csrc/resect.hip): device tensors as op_resect_images takes them,
    cams the HOST records of resect_cameras; n, T: the sizes to state when a tensor is a stand-in for an empty one (default: the tensors' own).
    -> (the views of resect_views, and what must stay alive until the launches have run).
    Asynchronous; no host read."""
    device = track_of.device
    rec = np.ascontiguousarray(cams, dtype=np.float64).reshape(-1, RESECT_CAMERA_WORDS)
    out = torch.empty(max(resect_out_layout(rec, iters)["bytes"], 16), dtype=torch.uint8, device=device)
    run_ops(make_ops([op_resect_images(track_of, xyz, use, kpts, rec, out, track_of.numel() if n is None else n, use.numel() if T is None else T, thresh, iters, lo_iters,
                                       min_inliers, seed)]))
    return resect_views(out, rec, iters), (rec, out, track_of, xyz, use, kpts)


def ba_out_layout(T: int, n_obs: int, n_images: int, iters: int, n_free: int) -> dict:
    """BYTE offsets into the one buffer of GIMS_AUX_BUNDLE_ADJUST (include/gims_hip.h; csrc/ba.hip ba_layout carves it and gims_aux_layout
    reports it): xyz float64 [T, 3], cams float64 [n_images, 18], obs_error float32 [n_obs], cam_obs int32 [n_images], history float64 [iters + 1, 2], taken uint8 [iters],
    counters int32 [8]; 'outputs' = the bytes of all of these = 'scratch', the offset of the kernels' scratch (which holds the 6 n_free square
    reduced system), 'bytes' = the whole buffer.  Every region starts on a 256-byte boundary."""
    return _out_layout(AUX_BUNDLE_ADJUST, (T, n_obs, n_images, iters, n_free))


def ba_pcg_out_layout(T: int, n_obs: int, n_images: int, iters: int, n_free: int) -> dict:
    """BYTE offsets into the one buffer of GIMS_AUX_BUNDLE_ADJUST_PCG (include/gims_hip.h; csrc/ba.hip ba_pcg_layout carves it): the seven
    output regions of ba_out_layout at the same offsets, then cg_used int32 [iters] and cg_res float64 [iters]; 'outputs' = 'scratch' =
    the offset of the kernels' scratch, which is linear in every size (no reduced system is stored), 'bytes' = the whole buffer."""
    return _out_layout(AUX_BUNDLE_ADJUST_PCG, (T, n_obs, n_images, iters, n_free))


def ba_focal_out_layout(T: int, n_obs: int, n_images: int, iters: int, n_free: int, n_groups: int) -> dict:
    """BYTE offsets into the one buffer of GIMS_AUX_BUNDLE_ADJUST_FOCAL (include/gims_hip.h; csrc/ba.hip ba_focal_layout carves it): the nine
    output regions of ba_pcg_out_layout at the same offsets, then focal_scale float64 [n_groups] and group_obs int32 [n_groups]; 'outputs'
    = 'scratch' = the offset of the kernels' scratch, which is linear in every size, 'bytes' = the whole buffer."""
    return _out_layout(AUX_BUNDLE_ADJUST_FOCAL, (T, n_obs, n_images, iters, n_free, n_groups))


def ba_table(indptr, obs_image, obs_keypoint, obs_use, point_use, cg_iters: int = 0, cg_tol: float = 0.0, group=None) -> np.ndarray:
    """The HOST table of GIMS_AUX_BUNDLE_ADJUST, int64 [8]: the addresses of the five device arrays (tensors, raw addresses, or None) and
    three reserved zeros.  For GIMS_AUX_BUNDLE_ADJUST_PCG word 5 is cg_iters and word 6 the bit pattern of the double cg_tol (the
    defaults leave both 0).  For GIMS_AUX_BUNDLE_ADJUST_FOCAL word 7 is the address of ``group``, a C-contiguous int32 HOST array
    [n_images] (or a raw address).  The caller keeps it, the group array and the tensors alive for as long as the op is run."""
    tab = np.zeros(BA_TABLE_WORDS, dtype=np.int64)
    for k, t in enumerate((indptr, obs_image, obs_keypoint, obs_use, point_use)):
        tab[k] = 0 if t is None else t if isinstance(t, int) else t.data_ptr()
    tab[5] = int(cg_iters)
    tab[6:7] = np.array([cg_tol], dtype=np.float64).view(np.int64)
    if group is not None:
        if not isinstance(group, int) and not (isinstance(group, np.ndarray) and group.dtype == np.int32 and group.flags["C_CONTIGUOUS"] and group.ndim == 1):
            raise ValueError("bundle_adjust: group must be a C-contiguous int32 host array [n_images]")
        tab[7] = group if isinstance(group, int) else group.ctypes.data if group.size else 0
    return tab


def op_bundle_adjust(table: np.ndarray, kpts, xyz, cams, mode: np.ndarray, out, T: int, n_obs: int, n: int, iters: int = 20, huber: float = 0.0,
                     lambda0: float = 1e-4) -> Op:
    """GIMS_AUX_BUNDLE_ADJUST as an op of gims_run_ops (include/gims_hip.h): the one way to reach it.  table: the HOST int64 [8] of ba_table;
    kpts float32 [n, 2], xyz float64 [T, 3], cams float64 [n_images, 18] on the device; mode: HOST int32 [n_images] (0 absent, 1 fixed,
    2 free; C-contiguous; the caller keeps both host arrays alive for as long as the op is run); out uint8
    [ba_out_layout(T, n_obs, n_images, iters, n_free)['bytes']]."""
    if not (isinstance(table, np.ndarray) and table.dtype == np.int64 and table.flags["C_CONTIGUOUS"] and table.size == BA_TABLE_WORDS):
        raise ValueError("bundle_adjust: table must be a C-contiguous int64 host array [8] (ba_table)")
    if not (isinstance(mode, np.ndarray) and mode.dtype == np.int32 and mode.flags["C_CONTIGUOUS"] and mode.ndim == 1):
        raise ValueError("bundle_adjust: mode must be a C-contiguous int32 host array [n_images]")
    return op_aux(AUX_BUNDLE_ADJUST, (table.ctypes.data, kpts, xyz, cams, mode.ctypes.data if mode.size else None, out),
                  (T, n_obs, mode.size, n, int(iters), 0), (huber, lambda0))


def ba_views(out: torch.Tensor, T: int, n_obs: int, n_images: int, iters: int, n_free: int) -> dict:
    """The typed views of the op's buffer, by ba_out_layout."""
    return _out_views(AUX_BUNDLE_ADJUST, (T, n_obs, n_images, iters, n_free), out)


def op_bundle_adjust_pcg(table: np.ndarray, kpts, xyz, cams, mode: np.ndarray, out, T: int, n_obs: int, n: int, iters: int = 20, huber: float = 0.0,
                         lambda0: float = 1e-4) -> Op:
    """GIMS_AUX_BUNDLE_ADJUST_PCG as an op of gims_run_ops (include/gims_hip.h): the arguments of op_bundle_adjust, with the table of
    ba_table(..., cg_iters=, cg_tol=) and out uint8 [ba_pcg_out_layout(T, n_obs, n_images, iters, n_free)['bytes']]."""
    op = op_bundle_adjust(table, kpts, xyz, cams, mode, out, T, n_obs, n, iters, huber, lambda0)      # (the same checks of the host arrays)
    op.u.aux.fn = AUX_BUNDLE_ADJUST_PCG
    return op


def ba_pcg_views(out: torch.Tensor, T: int, n_obs: int, n_images: int, iters: int, n_free: int) -> dict:
    """The typed views of the buffer of GIMS_AUX_BUNDLE_ADJUST_PCG, by ba_pcg_out_layout: those of ba_views, cg_used and cg_res."""
    return _out_views(AUX_BUNDLE_ADJUST_PCG, (T, n_obs, n_images, iters, n_free), out)


def op_bundle_adjust_focal(table: np.ndarray, kpts, xyz, cams, mode: np.ndarray, out, T: int, n_obs: int, n: int, iters: int = 20, huber: float = 0.0,
                           lambda0: float = 1e-4) -> Op:
    """GIMS_AUX_BUNDLE_ADJUST_FOCAL as an op of gims_run_ops (include/gims_hip.h): the arguments of op_bundle_adjust_pcg, with the table of
    ba_table(..., cg_iters=, cg_tol=, group=) and out uint8 [ba_focal_out_layout(T, n_obs, n_images, iters, n_free, n_groups)['bytes']]."""
    op = op_bundle_adjust(table, kpts, xyz, cams, mode, out, T, n_obs, n, iters, huber, lambda0)      # (the same checks of the host arrays)
    op.u.aux.fn = AUX_BUNDLE_ADJUST_FOCAL
    return op


def ba_focal_groups(mode: np.ndarray, group: np.ndarray) -> int:
    """n_groups as the op counts it: 1 + the largest id among the posed images (0 when every id is -1)."""
    ids = np.asarray(group)[np.asarray(mode) != BA_ABSENT]
    return int(ids.max()) + 1 if ids.size and ids.max() >= 0 else 0


def ba_focal_views(out: torch.Tensor, T: int, n_obs: int, n_images: int, iters: int, n_free: int, n_groups: int) -> dict:
    """The typed views of the buffer of GIMS_AUX_BUNDLE_ADJUST_FOCAL, by ba_focal_out_layout: those of ba_pcg_views, focal_scale, group_obs."""
    return _out_views(AUX_BUNDLE_ADJUST_FOCAL, (T, n_obs, n_images, iters, n_free, n_groups), out)


def bundle_adjust(indptr, obs_image, obs_keypoint, obs_use, point_use, kpts, xyz, cams, mode: np.ndarray, iters: int = 20, huber: float = 0.0,
                  lambda0: float = 1e-4, T: int | None = None, n_obs: int | None = None, n: int | None = None, solver: str = "dense",
                  cg_iters: int = 64, cg_tol: float = 1e-6, group: np.ndarray | None = None):
    """Joint refinement of the free cameras and the active points on the device (csrc/ba.hip): device tensors as
    op_bundle_adjust takes them (cams the DEVICE records float64 [n_images, 18]), mode the HOST int32 [n_images]; T, n_obs, n: the sizes to
    state when a tensor is a stand-in for an empty one (default: the tensors' own).  -> (the views of ba_views, and what must stay alive
    until the launches have run).  Asynchronous; no host read.  solver='pcg': GIMS_AUX_BUNDLE_ADJUST_PCG with cg_iters and cg_tol
    (DESIGN.md 4.21), the views of ba_pcg_views; with 'dense' the two are not used.  group (HOST int32 [n_images], solver='pcg' only):
    GIMS_AUX_BUNDLE_ADJUST_FOCAL, the views of ba_focal_views."""
    if solver not in ("dense", "pcg"):
        raise ValueError(f"bundle_adjust: solver must be 'dense' or 'pcg', got {solver!r}")
    if group is not None and solver != "pcg":
        raise ValueError("bundle_adjust: focal groups need solver='pcg'")
    mode = np.ascontiguousarray(mode, dtype=np.int32).reshape(-1)
    T = indptr.numel() - 1 if T is None else T
    n_obs = obs_image.numel() if n_obs is None else n_obs
    n = kpts.shape[0] if n is None else n
    n_free = int((mode == BA_FREE).sum())
    if group is not None:
        group = np.ascontiguousarray(group, dtype=np.int32).reshape(-1)
        n_groups = ba_focal_groups(mode, group)
        table = ba_table(indptr, obs_image, obs_keypoint, obs_use, point_use, cg_iters=cg_iters, cg_tol=cg_tol, group=group)
        out = torch.empty(ba_focal_out_layout(T, n_obs, mode.size, iters, n_free, n_groups)["bytes"], dtype=torch.uint8, device=xyz.device)
        run_ops(make_ops([op_bundle_adjust_focal(table, kpts, xyz, cams, mode, out, T, n_obs, n, iters, huber, lambda0)]))
        return (ba_focal_views(out, T, n_obs, mode.size, iters, n_free, n_groups),
                (table, mode, group, out, indptr, obs_image, obs_keypoint, obs_use, point_use, kpts, xyz, cams))
    if solver == "pcg":
        table = ba_table(indptr, obs_image, obs_keypoint, obs_use, point_use, cg_iters=cg_iters, cg_tol=cg_tol)
        out = torch.empty(ba_pcg_out_layout(T, n_obs, mode.size, iters, n_free)["bytes"], dtype=torch.uint8, device=xyz.device)
        run_ops(make_ops([op_bundle_adjust_pcg(table, kpts, xyz, cams, mode, out, T, n_obs, n, iters, huber, lambda0)]))
        return ba_pcg_views(out, T, n_obs, mode.size, iters, n_free), (table, mode, out, indptr, obs_image, obs_keypoint, obs_use, point_use, kpts, xyz, cams)
    table = ba_table(indptr, obs_image, obs_keypoint, obs_use, point_use)
    out = torch.empty(ba_out_layout(T, n_obs, mode.size, iters, n_free)["bytes"], dtype=torch.uint8, device=xyz.device)
    run_ops(make_ops([op_bundle_adjust(table, kpts, xyz, cams, mode, out, T, n_obs, n, iters, huber, lambda0)]))
    return ba_views(out, T, n_obs, mode.size, iters, n_free), (table, mode, out, indptr, obs_image, obs_keypoint, obs_use, point_use, kpts, xyz, cams)


def patch_affine(kp4: torch.Tensor, kp_octave: torch.Tensor):
    """The 2x3 warp matrix (f64 [N, 2, 3]) and pyramid level (int32 [N]) gims_patch_extract derives per keypoint (library.py:96-106)."""
    assert kp4.dtype == torch.float32 and kp_octave.dtype == torch.int32 and kp4.is_contiguous() and kp4.is_cuda and kp_octave.is_cuda
    n = int(kp4.shape[0])
    A = torch.empty((n, 2, 3), dtype=torch.float64, device=kp4.device)
    level = torch.empty(n, dtype=torch.int32, device=kp4.device)
    _check(load().gims_patch_affine(_p(kp4), _p(kp_octave), n, _p(A), _p(level), _stream()), "gims_patch_affine")
    return A, level


# ------------------------------------------------------------------------------------------------ training step
EW_SCALE, EW_ADD, EW_RELU_MASK, EW_RELU, EW_ACC = (_K["GIMS_EW_" + k] for k in ("SCALE", "ADD", "RELU_MASK", "RELU", "ACC"))


def _operand(x: torch.Tensor):
    """A 2-D (or batched 3-D) f32 tensor VIEW as a GEMM operand [rows][k]: (transposed flag, pitch, batch stride, rows, k, dims).
    The view must be contiguous along one of its last two dimensions -- `w.t()`, column slices and head slices all qualify.
    (shape and strides are fetched once: this runs ~1 300 times per training step)"""
    sh, sd = x.shape, x.stride()
    nd = len(sh)
    if x.dtype != torch.float32 or not x.is_cuda or nd not in (2, 3):
        raise GimsHipError("gemm operands are 2-D / 3-D f32 device tensors")
    st = sd[0] if nd == 3 else 0
    r, k, s2, s1 = sh[-2], sh[-1], sd[-2], sd[-1]
    if s1 == 1 or k == 1:
        return 0, (s2 if r > 1 else max(k, s2)), st, r, k, nd
    if s2 == 1 or r == 1:
        return 1, (s1 if k > 1 else max(r, s1)), st, r, k, nd
    raise GimsHipError("gemm operand is contiguous along neither of its last two dimensions")


_gemm_work = {}
_gemm_fn = None


GEMM_PRECISION = PREC_BF16X6          # default precision of gemm() outside a gemm_precision() block


class gemm_precision:
    """``with gemm_precision(PREC_BF16X3):`` -- default precision of gemm() for the calling thread inside the block (the training
    step sets it per pass from config['train_precision']); restored on exit, so two models with different settings, or a direct
    gemm() user, never see each other's choice."""

    def __init__(self, precision: int):
        self.precision = int(precision)

    def __enter__(self):
        self._prev = getattr(_TLS, "gemm_prec", None)
        _TLS.gemm_prec = self.precision
        return self

    def __exit__(self, *exc):
        _TLS.gemm_prec = self._prev
        return False


def gemm(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor | None = None, *, alpha=1.0, beta=0.0, bias=None, residual=None, act=ACT_NONE,
         precision=None):
    """out = alpha * a @ b^T + beta * out (+ bias over the last dimension) (+ residual), then act (gims_gemm_f32, split-bf16 MFMA,
    f32 class by default).  a: [.., m, k], b: [.., n, k] views (either may be a transposed view), out: [.., m, n] with unit
    stride along n.  Batched when the tensors are 3-D."""
    global _gemm_fn
    ta, lda, sa, m, k, nda = _operand(a)
    tb, ldb, sb, n, kb, ndb = _operand(b)
    if kb != k or nda != ndb:
        raise GimsHipError(f"gemm: shapes {tuple(a.shape)} x {tuple(b.shape)}^T do not agree")
    batch = a.shape[0] if nda == 3 else 1
    if out is None:
        out = torch.empty((batch, m, n) if nda == 3 else (m, n), dtype=torch.float32, device=a.device)
    osh, osd = out.shape, out.stride()
    if osh[-2] != m or osh[-1] != n or (osd[-1] != 1 and n > 1) or out.dtype != torch.float32:
        raise GimsHipError("gemm: bad output tensor")
    ldr = sr = 0
    if residual is not None:
        rsd = residual.stride()
        ldr, sr = rsd[-2], (rsd[0] if len(rsd) == 3 else 0)
    g = Gemm(a.data_ptr(), b.data_ptr(), out.data_ptr(), _p(bias), _p(residual), lda, ldb, osd[-2] if m > 1 else max(n, osd[-2]), ldr, sa, sb,
             osd[0] if len(osd) == 3 else 0, sr, m, n, k, batch, ta, tb, int(act), 0, float(alpha), float(beta))
    if precision is None:
        precision = getattr(_TLS, "gemm_prec", None)
    g.precision = GEMM_PRECISION if precision is None else int(precision)
    stream = _stream()
    if k >= 512:                                  # split-K workspace (one arena per device and stream; stream order protects it)
        key = (a.device, stream)
        w = _gemm_work.get(key)
        if w is None:
            w = _gemm_work[key] = torch.empty(32 << 20, dtype=torch.float32, device=a.device)
        g.work, g.work_floats = w.data_ptr(), w.numel()
    if _gemm_fn is None:
        _gemm_fn = load().gims_gemm_f32
    rc = _gemm_fn(C.byref(g), stream)
    if rc != 0:
        _check(rc, "gims_gemm_f32")
    return out


def segments(ranges) -> Segments:
    """ranges: [(first row, rows)] -- the rows every call of a module covers in the reference (image 0 of the batch, image 1)."""
    sg = Segments()
    sg.n = len(ranges)
    for i, (o, r) in enumerate(ranges):
        sg.off[i], sg.rows[i] = int(o), int(r)
    return sg


def batchnorm_train_forward(x, sg: Segments, gamma, beta, eps, momentum, running_mean, running_var, relu: bool, y=None):
    """nn.BatchNorm1d in train() mode (+ ReLU) on x [rows, c]; returns (y, save).  Running statistics are updated in place."""
    c = x.shape[1]
    y = torch.empty_like(x) if y is None else y
    save = torch.empty((sg.n, c, 2), dtype=torch.float32, device=x.device)
    work = torch.empty(int(load().gims_batchnorm_workspace_floats(C.byref(sg), c)), dtype=torch.float32, device=x.device)
    _check(load().gims_batchnorm_train_forward(_p(x), x.stride(0), c, C.byref(sg), _p(gamma), _p(beta), float(eps), float(momentum), _p(running_mean),
                                               _p(running_var), _p(save), _p(y), y.stride(0), int(relu), _p(work), _stream()), "gims_batchnorm_train_forward")
    return y, save


def batchnorm_train_backward(x, dy, sg: Segments, save, gamma, beta, relu: bool, dx=None):
    """Returns (dx, dgamma, dbeta) for the module of batchnorm_train_forward; dy: gradient of its (post-ReLU) output."""
    c = x.shape[1]
    dx = torch.empty_like(x) if dx is None else dx
    dg = torch.empty(c, dtype=torch.float32, device=x.device)
    db = torch.empty(c, dtype=torch.float32, device=x.device)
    work = torch.empty(int(load().gims_batchnorm_workspace_floats(C.byref(sg), c)), dtype=torch.float32, device=x.device)
    _check(load().gims_batchnorm_train_backward(_p(x), x.stride(0), _p(dy), dy.stride(0), c, C.byref(sg), _p(save), _p(gamma), _p(beta), int(relu),
                                                _p(dx), dx.stride(0), _p(dg), _p(db), _p(work), _stream()), "gims_batchnorm_train_backward")
    return dx, dg, db


def softmax_rows_(s: torch.Tensor, cols: int):
    """In-place softmax over the first `cols` entries of every row of s [batch, rows, ld]."""
    assert s.dim() == 3 and s.stride(2) == 1
    _check(load().gims_softmax_rows(_p(s), s.stride(1), s.shape[1], int(cols), s.shape[0], s.stride(0), _stream()), "gims_softmax_rows")
    return s


def softmax_rows_backward_(prob: torch.Tensor, dp: torch.Tensor, cols: int):
    assert prob.shape == dp.shape and prob.stride() == dp.stride() and prob.dim() == 3
    _check(load().gims_softmax_rows_backward(_p(prob), _p(dp), prob.stride(1), prob.shape[1], int(cols), prob.shape[0], prob.stride(0), _stream()),
           "gims_softmax_rows_backward")
    return dp


_tattn_work = {}


def train_attn_problems(problems):
    """[(q_off, nq, k_off, nk)] -> (ctypes array, n): problem i attends the query rows [q_off, q_off + nq) to the source rows [k_off, k_off + nk)."""
    arr = (TrainAttnProblem * len(problems))()
    for i, (qo, nq, ko, nk) in enumerate(problems):
        arr[i].q_off, arr[i].nq, arr[i].k_off, arr[i].nk = int(qo), int(nq), int(ko), int(nk)
    return arr, len(problems)


TRAIN_ATTN_REVERSE_F32, TRAIN_ATTN_REVERSE_BF16X3 = _K["GIMS_TRAIN_ATTN_REVERSE_F32"], _K["GIMS_TRAIN_ATTN_REVERSE_BF16X3"]


def _train_attn_args(qkv, problems, heads, o, lse, d_o=None, d_qkv=None, reverse_precision=1):
    rows, d = qkv.shape[0], qkv.shape[1] // 3
    assert qkv.dtype == torch.float32 and qkv.stride(1) == 1 and o.stride(1) == 1 and lse.is_contiguous() and lse.shape == (heads, rows)
    need = int(load().gims_train_attention_workspace_floats(rows, heads))
    key = (qkv.device, _stream())
    w = _tattn_work.get(key)
    if w is None or w.numel() < need:
        if w is not None:
            _colsum_retired.append(w)                 # (see colsum: a launch on a non-torch stream may still read the outgrown buffer)
        w = _tattn_work[key] = torch.empty(need, dtype=torch.float32, device=qkv.device)
    arr, n = problems if isinstance(problems, tuple) else train_attn_problems(problems)
    g = TrainAttnArgs(qkv.data_ptr(), qkv.stride(0), rows, d, heads, 1.0 / math.sqrt(d // heads), n, C.addressof(arr), o.data_ptr(), o.stride(0), lse.data_ptr(),
                      _p(d_o), d_o.stride(0) if d_o is not None else 0, _p(d_qkv), d_qkv.stride(0) if d_qkv is not None else 0, w.data_ptr(), w.numel(),
                      int(reverse_precision))
    return g, arr


def train_attention_forward(qkv: torch.Tensor, problems, heads: int, o: torch.Tensor | None = None, lse: torch.Tensor | None = None):
    """o = softmax(Q K^T / sqrt(64)) V for every problem and head of one layer (qkv [rows, 3 d]: packed Q | K | V, heads contiguous), and the
    row statistic lse [heads, rows] the reverse pass recomputes the probabilities from.  Returns (o, lse)."""
    rows, d = qkv.shape[0], qkv.shape[1] // 3
    o = torch.empty((rows, d), dtype=torch.float32, device=qkv.device) if o is None else o
    lse = torch.empty((heads, rows), dtype=torch.float32, device=qkv.device) if lse is None else lse
    g, keep = _train_attn_args(qkv, problems, heads, o, lse)
    _check(load().gims_train_attention_forward(C.byref(g), _stream()), "gims_train_attention_forward")
    return o, lse


def train_attention_backward(qkv, o, lse, d_o, problems, heads: int, d_qkv: torch.Tensor | None = None, precision=None):
    """d_qkv [rows, 3 d] from the gradient d_o of train_attention_forward's output.  precision: PREC_BF16X3 (three bf16 passes; also the default
    inside a gemm_precision(PREC_BF16X3) block, as the training step's reverse pass is) or anything else = exact f32 products."""
    if precision is None:
        precision = getattr(_TLS, "gemm_prec", None)
    rp = TRAIN_ATTN_REVERSE_BF16X3 if precision == PREC_BF16X3 else TRAIN_ATTN_REVERSE_F32
    d_qkv = torch.empty_like(qkv) if d_qkv is None else d_qkv
    assert d_o.stride(1) == 1 and d_qkv.stride(1) == 1
    g, keep = _train_attn_args(qkv, problems, heads, o, lse, d_o, d_qkv, rp)
    _check(load().gims_train_attention_backward(C.byref(g), _stream()), "gims_train_attention_backward")
    return d_qkv


_colsum_work = {}
_colsum_retired = []


def colsum(x: torch.Tensor, out: torch.Tensor | None = None, beta=0.0):
    """out[c] = beta * out[c] + sum_rows x[row, c] (fixed summation order)."""
    rows, c = x.shape
    if out is None:
        out = torch.empty(c, dtype=torch.float32, device=x.device)
    need = int(load().gims_colsum_workspace_floats(rows, c))
    key = (x.device, _stream())
    w = _colsum_work.get(key)
    if w is None or w.numel() < need:
        if w is not None:
            # a kernel enqueued on this (possibly non-torch) stream may still be reading the outgrown workspace, and torch's allocator orders
            # re-use only against ITS streams: the old buffer is kept alive for the life of the process (regrowth is rare, the buffers small)
            _colsum_retired.append(w)
        w = _colsum_work[key] = torch.zeros(max(need, 1 << 16), dtype=torch.float32, device=x.device)
        if getattr(_TLS, "pin", None) is not None:
            torch.cuda.current_stream(x.device).synchronize()      # the zero fill ran on torch's stream, the kernel may run on another (on_stream)
    # (the kernel leaves its counters -- the first 64 words -- zeroed; partials are overwritten before they are read)
    _check(load().gims_colsum(_p(x), x.stride(0), rows, c, float(beta), _p(out), _p(w), _stream()), "gims_colsum")
    return out


def elementwise(op: int, out, a, b=None, alpha=1.0):
    rows, cols = a.shape
    _check(load().gims_elementwise(int(op), _p(out), out.stride(0), _p(a), a.stride(0), _p(b), (b.stride(0) if b is not None else 0), rows, cols,
                                   float(alpha), _stream()), "gims_elementwise")
    return out


def permute3(dst, src, shape, dstrides, sstrides, accumulate=False):
    _check(load().gims_permute3(_p(dst), _p(src), *[int(v) for v in shape], *[int(v) for v in dstrides], *[int(v) for v in sstrides], int(accumulate),
                                _stream()), "gims_permute3")
    return dst


def sage_mean_transposed(g, indptr, indices, out=None):
    n, c = g.shape
    out = torch.empty_like(g) if out is None else out
    _check(load().gims_sage_mean_transposed(_p(g), g.stride(0), _p(indptr), _p(indices), n, c, _p(out), out.stride(0), _stream()),
           "gims_sage_mean_transposed")
    return out


def normalize_keypoints(kpts, norm3, seg):
    out = torch.empty_like(kpts)
    _check(load().gims_normalize_keypoints(_p(kpts), _p(norm3), _p(seg), kpts.shape[0], _p(out), _stream()), "gims_normalize_keypoints")
    return out


def layernorm_backward(x, dy, a2, b2, relu: bool, eps=1e-6):
    """Reverse pass of layernorm_act on x [rows, c]: returns (dx, d a_2, d b_2)."""
    rows, c = x.shape
    dx = torch.empty_like(x)
    gb = torch.empty((rows, c), dtype=torch.float32, device=x.device)
    ga = torch.empty((rows, c), dtype=torch.float32, device=x.device)
    _check(load().gims_layernorm_backward(_p(x), x.stride(0), _p(dy), dy.stride(0), rows, c, _p(a2), _p(b2), float(eps), int(relu), _p(dx), dx.stride(0),
                                          _p(gb), _p(ga), _stream()), "gims_layernorm_backward")
    return dx, colsum(ga), colsum(gb)


def head_pack(proj_w, proj_b, merge_w, wqkv, bqkv, wm, heads: int, to_params: bool):
    """All head-interleave permutations of one attention layer in one launch (gims_head_pack): parameters -> packed tensors, or
    packed gradients -> parameter-layout gradients."""
    pw = (C.c_void_p * 3)(*[t.data_ptr() for t in proj_w])
    pb = (C.c_void_p * 3)(*[t.data_ptr() for t in proj_b])
    _check(load().gims_head_pack(pw, pb, _p(merge_w), _p(wqkv), _p(bqkv), _p(wm), merge_w.shape[0], int(heads), int(to_params), _stream()), "gims_head_pack")


ADAM_TENSOR_DTYPE = np.dtype(AdamTensor)


def adam_step(table, groups):
    """One fused Adam step (gims_adam_step).  table: C-contiguous NumPy structured array of dtype ADAM_TENSOR_DTYPE (= gims_adam_tensor:
    device pointers of contiguous float32 tensors, element count, group index); groups: at most 8 dicts with lr, beta1, beta2, eps,
    weight_decay, step (1-based, after the increment)."""
    assert table.dtype == ADAM_TENSOR_DTYPE and table.flags["C_CONTIGUOUS"]
    gt = (AdamGroup * max(len(groups), 1))()
    for i, g in enumerate(groups):
        gt[i].lr, gt[i].beta1, gt[i].beta2, gt[i].eps, gt[i].weight_decay, gt[i].step = (float(g["lr"]), float(g["beta1"]), float(g["beta2"]), float(g["eps"]),
                                                                                      float(g["weight_decay"]), int(g["step"]))
    _check(load().gims_adam_step(table.ctypes.data, len(table), gt, len(groups), _stream()), "gims_adam_step")


SGD_TENSOR_DTYPE = np.dtype(SgdTensor)
EMA_TENSOR_DTYPE = np.dtype(EmaTensor)


def sgd_step(table, groups):
    """One fused SGD step (gims_sgd_step).  table: C-contiguous NumPy structured array of dtype SGD_TENSOR_DTYPE (= gims_sgd_tensor: device
    pointers of contiguous float32 tensors, element count, group index, first = the momentum buffer holds nothing yet); groups: 1 to 8
    dicts with lr, momentum, dampening, weight_decay, nesterov."""
    assert table.dtype == SGD_TENSOR_DTYPE and table.flags["C_CONTIGUOUS"]
    gt = (SgdGroup * max(len(groups), 1))()
    for i, g in enumerate(groups):
        gt[i].lr, gt[i].momentum, gt[i].dampening, gt[i].weight_decay, gt[i].nesterov = (float(g["lr"]), float(g["momentum"]), float(g["dampening"]),
                                                                                         float(g["weight_decay"]), int(bool(g["nesterov"])))
    _check(load().gims_sgd_step(table.ctypes.data, len(table), gt, len(groups), _stream()), "gims_sgd_step")


def ema_update(table, decay):
    """ema = ema * decay + (1 - decay) * model over a table of tensors (gims_ema_update).  table: C-contiguous NumPy structured array of
    dtype EMA_TENSOR_DTYPE (= gims_ema_tensor: device pointers of contiguous float32 tensors and their element count)."""
    assert table.dtype == EMA_TENSOR_DTYPE and table.flags["C_CONTIGUOUS"]
    _check(load().gims_ema_update(table.ctypes.data, len(table), float(decay), _stream()), "gims_ema_update")


# ------------------------------------------------------------------------------------------------ training data from images
INTER_LINEAR, INTER_AREA = _K["GIMS_INTER_LINEAR"], _K["GIMS_INTER_AREA"]          # cv2's values


def _image_batch(images: torch.Tensor):
    if images.dtype != torch.uint8 or images.dim() not in (3, 4) or not images.is_cuda or (images.dim() == 4 and images.shape[3] not in (1, 3)):
        raise ValueError("image warps take device uint8 [B, H, W, 3] or [B, H, W] images")
    t = images.contiguous()
    return t if t.dim() == 4 else t.unsqueeze(-1)


def warp_perspective(images: torch.Tensor, ms, dsize, out=None):
    """cv2.warpPerspective(img, M, dsize) (INTER_LINEAR, BORDER_CONSTANT 0) for a batch: images uint8 [B, H, W(, 3)] on the device,
    ms float64-convertible [B, 3, 3] (host), dsize (w, h) -> uint8 [B, h, w(, 3)] on the device.  One launch for the batch."""
    t = _image_batch(images)
    B, H, W, c = t.shape
    dw, dh = int(dsize[0]), int(dsize[1])
    m = np.ascontiguousarray(np.asarray(ms, dtype=np.float64).reshape(B, 9))
    res = out if out is not None else torch.empty((B, dh, dw, c), dtype=torch.uint8, device=t.device)
    assert res.shape == (B, dh, dw, c) and res.dtype == torch.uint8 and res.is_contiguous()
    work = torch.empty(9 * B, dtype=torch.float64, device=t.device)
    _check(load().gims_warp_perspective(_p(t), B, H, W, c, m.ctypes.data, _p(res), dh, dw, _p(work), _stream()), "gims_warp_perspective")
    return res if images.dim() == 4 else res.squeeze(-1)


def resize(images: torch.Tensor, dsize, interpolation=INTER_LINEAR, out=None):
    """cv2.resize(img, dsize, interpolation) for INTER_LINEAR / INTER_AREA on a batch of device uint8 [B, H, W(, 3)] images."""
    t = _image_batch(images)
    B, H, W, c = t.shape
    dw, dh = int(dsize[0]), int(dsize[1])
    res = out if out is not None else torch.empty((B, dh, dw, c), dtype=torch.uint8, device=t.device)
    assert res.shape == (B, dh, dw, c) and res.dtype == torch.uint8 and res.is_contiguous()
    _check(load().gims_resize(_p(t), B, H, W, c, _p(res), dh, dw, int(interpolation), _stream()), "gims_resize")
    return res if images.dim() == 4 else res.squeeze(-1)


def color_aug(images: torch.Tensor, plans, out=None):
    """gims_color_aug: every image of a device uint8 batch [n, h, w, c] (or [n, h, w]) under its own plan (a ctypes array of n AugPlan, or
    a sequence of them) into a separate tensor of the same shape; one launch for the batch, asynchronous on the current stream.  The
    library checks the arguments (channels, kernel sizes, blur with noise, out overlapping images) and raises GimsHipError."""
    if not torch.is_tensor(images) or not images.is_cuda or images.dtype != torch.uint8 or images.dim() not in (3, 4):
        raise ValueError("color_aug takes device uint8 [n, h, w, c] or [n, h, w] images")
    t = images.contiguous()
    n, h, w = t.shape[:3]
    c = t.shape[3] if t.dim() == 4 else 1
    if len(plans) != n:
        raise ValueError(f"color_aug: {len(plans)} plans for {n} images")
    arr = plans if isinstance(plans, C.Array) else (AugPlan * max(n, 1))(*plans)
    res = out if out is not None else torch.empty_like(t)
    assert res.shape == t.shape and res.dtype == torch.uint8 and res.is_cuda and res.is_contiguous()
    lib = load()
    need = int(lib.gims_color_aug_workspace_bytes(n))
    work = torch.empty(max(need, 16), dtype=torch.uint8, device=t.device)
    _check(lib.gims_color_aug(_p(t), n, h, w, c, arr, _p(res), _p(work), need, _stream()), "gims_color_aug")
    return res


def train_labels(kpts0, kpts1, homographies: torch.Tensor, dist_thresh=3.0, n_iters=1):
    """torch_find_matches per pair + the match_indexes rows of train.py:118-125 (gims_train_labels): kpts0 / kpts1 sequences of device
    float32 [n, 2] (or [B, n, 2] tensors), homographies device float32 [B, 3, 3] -> int64 [R, 3] on the device.  The row count is the one
    host read."""
    B = len(kpts0)
    assert len(kpts1) == B and homographies.shape[0] == B
    k0 = [k.float().contiguous() for k in kpts0]
    k1 = [k.float().contiguous() for k in kpts1]
    hs = homographies.to(torch.float32).reshape(B, 9).contiguous()
    dev = hs.device
    arr = (LabelPair * B)()
    for i in range(B):
        assert k0[i].is_cuda and k1[i].is_cuda and k0[i].shape[-1] == 2 and k1[i].shape[-1] == 2
        arr[i] = LabelPair(_p(k0[i]), _p(k1[i]), k0[i].shape[0], k1[i].shape[0])
    lib = load()
    need = int(lib.gims_train_labels_workspace_bytes(arr, B))
    work = torch.empty(need, dtype=torch.uint8, device=dev)
    cap = sum(int(k0[i].shape[0]) + int(k1[i].shape[0]) for i in range(B))
    rows = torch.empty((cap, 3), dtype=torch.int64, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    _check(lib.gims_train_labels(arr, B, _p(hs), float(dist_thresh), int(n_iters), _p(rows), _p(total), _p(work), need, _stream()),
           "gims_train_labels")
    return rows[:int(total.item())]
