"""Plain NumPy references (float64 / int64) of the small kernels of gims_amd/csrc/misc.hip and gims_amd/csrc/train.hip, and the input
builders their tests share -- TEST INFRASTRUCTURE.  Every reference is the operation's formula in vectorised form; tests/test_small_kernels_cpu.py
checks each against a second formulation (a loop).  Used by tests/test_small_kernels_gpu.py."""
import numpy as np

# degrees the sage_mean graph must contain (the kernel fetches 64 neighbour indices per pass and adds four rows per step)
SAGE_DEGREES = (0, 1, 3, 4, 5, 63, 64, 65, 67, 128, 131, 200)
SAGE_N = 79                                    # not a multiple of 4: the last workgroup has one idle wave


def roundup(x, m):
    return (x + m - 1) // m * m


# ------------------------------------------------------------------------------------------------ graphs
def sage_graph(seed=5):
    """CSR graph of SAGE_N nodes, neighbours drawn with repetition; node 0 has degree 200, the last node 131, every degree of
    SAGE_DEGREES occurs, the rest are 0 .. 8.  Returns (indptr int32 [n + 1], indices int32 [E])."""
    rng = np.random.default_rng(seed)
    n = SAGE_N
    deg = rng.integers(0, 9, size=n)
    deg[0], deg[n - 1] = 200, 131
    rest = [d for d in SAGE_DEGREES if d not in (200, 131)]
    deg[np.arange(len(rest)) * 7 + 3] = rest              # nodes 3, 10, 17, ...: spread over the workgroups
    indptr = np.r_[0, np.cumsum(deg)].astype(np.int32)
    indices = rng.integers(0, n, size=int(indptr[-1])).astype(np.int32)
    return indptr, indices


def sym_graph(seed=6):
    """Symmetric multigraph of SAGE_N nodes: every undirected edge stands in both rows.  Node 0 is a hub of degree 131 (edges with
    repetition), node 40 has no edge, node 41 has exactly one.  Returns (indptr, indices)."""
    rng = np.random.default_rng(seed)
    n = SAGE_N
    others = np.array([i for i in range(1, n) if i not in (40, 41)])
    edges = [(0, int(v)) for v in rng.choice(others, size=130)] + [(0, 41)]
    while len(edges) < 131 + 150:
        u, v = (int(t) for t in rng.choice(others, size=2))
        if u != v:
            edges.append((u, v))
    rows = [[] for _ in range(n)]
    for u, v in edges:
        rows[u].append(v)
        rows[v].append(u)
    indptr = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int32)
    indices = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows if r]).astype(np.int32)
    return indptr, indices


def _row_of_edge(indptr):
    return np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))


# ------------------------------------------------------------------------------------------------ GraphSAGE mean
def sage_sum(h, indptr, indices):
    """sum over the CSR neighbours, in h's dtype widened (int64 for integers, float64 otherwise); [n, c]."""
    wide = np.int64 if np.issubdtype(np.asarray(h).dtype, np.integer) else np.float64
    out = np.zeros((len(indptr) - 1, h.shape[1]), dtype=wide)
    np.add.at(out, _row_of_edge(indptr), h[indices].astype(wide))
    return out


def sage_mean_exact(h_int, indptr, indices):
    """The f32 result for integer-valued h whose sums are exact in f32: float32(sum) / float32(deg), one correctly rounded division;
    zero for a node without neighbours."""
    s = sage_sum(h_int, indptr, indices)
    assert np.abs(s).max() < 2 ** 24
    deg = np.diff(indptr).astype(np.float32)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(deg > 0, s.astype(np.float32) / deg, np.float32(0)).astype(np.float32)


def sage_mean(h, indptr, indices):
    """float64 mean over the neighbours; zero for a node without neighbours."""
    deg = np.diff(indptr).astype(np.float64)[:, None]
    return sage_sum(np.asarray(h, dtype=np.float64), indptr, indices) / np.maximum(deg, 1.0)


def sage_mean_transposed(g, indptr, indices):
    """(out, mag): out_j = sum_{i in N(j)} g_i / deg_i in float64, and mag_j = sum_i |g_i| / deg_i, what the error bar scales with."""
    g = np.asarray(g, dtype=np.float64)
    deg = np.diff(indptr).astype(np.float64)
    q = g[indices] / deg[indices][:, None]
    out, mag = np.zeros_like(g), np.zeros_like(g)
    np.add.at(out, _row_of_edge(indptr), q)
    np.add.at(mag, _row_of_edge(indptr), np.abs(q))
    return out, mag


# ------------------------------------------------------------------------------------------------ copies
def gather_rows(src, idx):
    return src[idx]


def ingest(images, d, total_rows):
    """images: list of (kpts [n, 2], desc [d, n] channel-major, score [n] or None, row_off).  Returns (desc_out [total, d], kpts_out
    [total, 2], score_out [total], written [total] bool); rows no image owns stay zero and unwritten.  A missing score reads as 0."""
    desc_out, kpts_out = np.zeros((total_rows, d), np.float32), np.zeros((total_rows, 2), np.float32)
    score_out, written = np.zeros(total_rows, np.float32), np.zeros(total_rows, bool)
    for kpts, desc, score, off in images:
        n = kpts.shape[0]
        desc_out[off:off + n] = desc[:, :n].T
        kpts_out[off:off + n] = kpts
        score_out[off:off + n] = 0 if score is None else score
        written[off:off + n] = True
    return desc_out, kpts_out, score_out, written


def pack(images, d):
    """images: list of dicts kpts [N, 2], desc [N, d], score [N] or None, kept [k], indptr [k + 1], indices [e] (local rows).  The
    row-concatenated layout of gims_pack_graphs: dict feat, kpts, score, has_score (rows whose score is written), seg, indptr
    (with the closing entry), indices."""
    ks = [len(im["kept"]) for im in images]
    es = [len(im["indices"]) for im in images]
    ro, eo = np.r_[0, np.cumsum(ks)], np.r_[0, np.cumsum(es)]
    out = dict(feat=np.zeros((ro[-1], d), np.float32), kpts=np.zeros((ro[-1], 2), np.float32), score=np.zeros(ro[-1], np.float32),
               has_score=np.zeros(ro[-1], bool), seg=np.zeros(ro[-1], np.int32), indptr=np.zeros(ro[-1] + 1, np.int32),
               indices=np.zeros(eo[-1], np.int32))
    for i, im in enumerate(images):
        r, e = slice(ro[i], ro[i + 1]), slice(eo[i], eo[i + 1])
        if ks[i]:
            out["feat"][r] = im["desc"][im["kept"]][:, :d]
            out["kpts"][r] = im["kpts"][im["kept"]]
            if im["score"] is not None:
                out["score"][r] = im["score"][im["kept"]]
                out["has_score"][r] = True
            out["seg"][r] = i
            out["indptr"][r] = im["indptr"][:-1] + eo[i]
        if es[i]:
            out["indices"][e] = im["indices"] + ro[i]
    out["indptr"][ro[-1]] = eo[-1]
    return out


def permute3_offsets(shape, strides):
    """flat offsets [n0, n1, n2] of a strided 3-D view."""
    i0, i1, i2 = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    return i0 * strides[0] + i1 * strides[1] + i2 * strides[2]


def permute3(dst, src, shape, dstrides, sstrides, accumulate=False):
    """dst (flat, float64 / int64 copy returned) with dst[i . dstrides] (=|+=) src[i . sstrides]."""
    out = np.array(dst, copy=True)
    d, s = permute3_offsets(shape, dstrides).ravel(), permute3_offsets(shape, sstrides).ravel()
    assert len(np.unique(d)) == len(d)
    out[d] = (out[d] if accumulate else 0) + src[s]
    return out


# ------------------------------------------------------------------------------------------------ norms and the keypoint encoder
def layernorm_act(x, a2, b2, eps, relu):
    """float64: a2 * (x - mean) / (std + eps) + b2 over the channels of a row, UNBIASED std, eps added to the std; then ReLU."""
    x = np.asarray(x, dtype=np.float64)
    mean = x.mean(-1, keepdims=True)
    std = np.sqrt(((x - mean) ** 2).sum(-1, keepdims=True) / (x.shape[-1] - 1))
    y = np.asarray(a2, np.float64) * (x - mean) / (std + eps) + np.asarray(b2, np.float64)
    return np.maximum(y, 0) if relu else y


def normalize_keypoints_f32(kpts, norm3, seg):
    """(k - centre) / scale in float32: one subtraction and one division, both correctly rounded."""
    nm = np.asarray(norm3, np.float32)[seg]
    return ((np.asarray(kpts, np.float32) - nm[:, :2]) / nm[:, 2:3]).astype(np.float32)


def kenc_first(kpts, norm3, seg, w1, b1, relu):
    """float64: normalize_keypoints, then Conv1d(2 -> c1) with its bias, then ReLU."""
    nm = np.asarray(norm3, np.float64)[seg]
    kn = (np.asarray(kpts, np.float64) - nm[:, :2]) / nm[:, 2:3]
    y = kn @ np.asarray(w1, np.float64).T + np.asarray(b1, np.float64)
    return np.maximum(y, 0) if relu else y


# ------------------------------------------------------------------------------------------------ split-bf16 planes
def spl_col(k):
    """SPL32: column of channel k's hi value inside a row of [32 hi | 32 lo] blocks; its lo value is 32 further."""
    k = np.asarray(k)
    return ((k >> 5) << 6) + (k & 31)


def bf16_bits(x):
    """round-to-nearest-even float32 -> bfloat16, as uint16 bit patterns (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


# ------------------------------------------------------------------------------------------------ training helpers
def colsum(x_int, out_prev=None, beta=0.0):
    """int64 column sums (+ beta * out_prev in float64): exact for the integer-valued inputs of the tests."""
    s = np.asarray(x_int).astype(np.int64).sum(0)
    return s if out_prev is None or beta == 0 else s + beta * np.asarray(out_prev, np.float64)


def softmax(x):
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def softmax_backward(p, dp):
    p, dp = np.asarray(p, np.float64), np.asarray(dp, np.float64)
    return p * (dp - (p * dp).sum(-1, keepdims=True))


def elementwise(op, a, b=None, alpha=1.0, out_prev=None):
    """float64 values of the five operations as the kernel writes them: scale alpha * a; add a + alpha * b; relu_mask b > 0 ? a : 0;
    relu fmaxf(a, 0) (a NaN gives 0: fmaxf returns its other operand); acc out + alpha * a."""
    a = np.asarray(a, np.float64)
    if op == "scale":
        return alpha * a
    if op == "add":
        return a + alpha * np.asarray(b, np.float64)
    if op == "relu_mask":
        return np.where(np.asarray(b) > 0, a, 0.0)
    if op == "relu":
        return np.where(a > 0, a, 0.0)
    if op == "acc":
        return np.asarray(out_prev, np.float64) + alpha * a
    raise ValueError(op)
