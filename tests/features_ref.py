"""NumPy restatement of GIMS_AUX_ASSEMBLE_ROWS (include/gims_hip.h; gims_amd/csrc/features.hip), written from that specification -- TEST
INFRASTRUCTURE.  Integer arithmetic on the bit patterns for the bf16 roundings (round to nearest, ties to even), one float32 subtraction
for the low part, the SPL32 column rule for the placement."""
import numpy as np


def f2bf(x):
    """float32 -> bf16 bit patterns (uint16), round to nearest even.  (No NaN handling: the tests feed none.)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf2f(b):
    """bf16 bit patterns -> float32 (exact)."""
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def spl_col(c):
    c = np.asarray(c)
    return 64 * (c // 32) + c % 32


def split(x):
    """f32 [rows, k] -> SPL32 bit patterns uint16 [rows, 2 k]: hi = bf16(x), lo = bf16(x - hi), per 32-channel block 32 hi then 32 lo."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    rows, k = x.shape
    assert k % 32 == 0
    hi = f2bf(x)
    lo = f2bf(x - bf2f(hi))                                  # float32 subtraction (NumPy keeps float32 for float32 operands)
    out = np.zeros((rows, 2 * k), dtype=np.uint16)
    cols = spl_col(np.arange(k))
    out[:, cols] = hi
    out[:, cols + 32] = lo
    return out


def assemble(segments, k, out=None, out_split=None):
    """segments: [(source f32 [rows, >= k], first destination row)], ascending by first row and disjoint.  out: f32 [n_rows, >= k] or None;
    out_split: uint16 [n_rows, >= 2 k] or None; both are updated in place (rows that no segment covers keep what they held) and returned."""
    n_rows = (out if out is not None else out_split).shape[0]
    for src, first in segments:
        rows = src.shape[0]
        if rows <= 0:
            continue
        for j in range(rows):
            r = first + j
            if r < 0 or r >= n_rows:                          # clipped to 0 .. n_rows - 1
                continue
            row = np.ascontiguousarray(src[j, :k], dtype=np.float32)
            if out is not None:
                out[r, :k] = row
            if out_split is not None:
                out_split[r, :2 * k] = split(row[None])[0]
    return out, out_split
