"""Plain NumPy restatements of what the GEMMs of gims_amd/csrc/linear.hip and linear6.hip read and write -- TEST INFRASTRUCTURE.
The operand layouts are written from the definitions in include/gims_hip.h (hi = bf16_rne(x), lo = bf16_rne(x - hi); SPL32 = [32 hi | 32 lo]
per 32-channel block; SPL3 = [32 a1 | 32 a2 | 32 a3]), the product is float64, the canaries are fixed NaN bit patterns around every output
window, and x3p_instance restates the shape rule by which gims_linear picks a pre-split kernel instance.  tests/test_linear_ref_cpu.py
checks the restatements against torch.bfloat16; tests/test_linear_instances_gpu.py uses them."""
import numpy as np

CANARY_F32 = 0x7FC01234          # quiet NaNs with a payload no kernel computes
CANARY_16 = 0x7FC1
BF16_MAX = float(np.array([0x7F7F0000], dtype=np.uint32).view(np.float32)[0])      # largest finite bf16


def ceil_to(x, m):
    return (x + m - 1) // m * m


# ------------------------------------------------------------------------------------------------ number formats
def bf16_bits(x):
    """float32 array -> uint16 bit patterns of round-to-nearest-even bfloat16 (NaN stays a quiet NaN)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32)
    r = ((u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) >> np.uint32(16)).astype(np.uint16)      # (wraps for NaNs only)
    nan = np.isnan(x)
    if nan.any():
        r = np.where(nan, ((u >> np.uint32(16)) | np.uint32(0x40)).astype(np.uint16), r)
    return r


def bf16_value(bits):
    """uint16 bfloat16 bit patterns -> float32."""
    return (np.asarray(bits).astype(np.uint32) << 16).view(np.float32)


def f16_sat_bits(x):
    """float32 array -> uint16 bit patterns of IEEE half, round to nearest even, saturated at +-65504 (GIMS_LINEAR_OUT_F16)."""
    return np.clip(np.asarray(x, dtype=np.float32), np.float32(-65504.0), np.float32(65504.0)).astype(np.float16).view(np.uint16)


def split2(x):
    """The two-way split of the header: (hi, lo) uint16 bit patterns, hi = bf16(x), lo = bf16(x - hi) with the subtraction in float32."""
    x = np.asarray(x, dtype=np.float32)
    hi = bf16_bits(x)
    with np.errstate(invalid="ignore"):
        lo = bf16_bits(x - bf16_value(hi))
    return hi, lo


def split3(x):
    """The three-way split of GIMS_PREC_BF16X6: a1 = bf16(x), a2 = bf16(x - a1), a3 = bf16(x - a1 - a2), each residual in float32."""
    x = np.asarray(x, dtype=np.float32)
    a1 = bf16_bits(x)
    with np.errstate(invalid="ignore"):
        r1 = x - bf16_value(a1)
        a2 = bf16_bits(r1)
        a3 = bf16_bits(r1 - bf16_value(a2))
    return a1, a2, a3


# Three bf16 planes hold 24 significant bits, but no bit below 2^-133 (the smallest bf16 subnormal; f32 reaches 2^-149): a1 + a2 + a3 == x
# exactly for x == 0 and |x| >= SPL3_EXACT_MIN (whose 24th bit is 2^-133), below that to within half of that last bit.
SPL3_EXACT_MIN = 2.0 ** -110
SPL3_TINY_ERR = 2.0 ** -134


def assert_spl3_sums_back(planes_sum, x):
    """planes_sum: a1 + a2 + a3 in float64, x: the float32 input.  Exact wherever three bf16 planes can hold x, else within half the
    smallest bf16 subnormal."""
    x64 = np.asarray(x, dtype=np.float64)
    holds = (x64 == 0) | (np.abs(x64) >= SPL3_EXACT_MIN)
    assert (planes_sum[holds] == x64[holds]).all(), "SPL3 planes do not sum back to the input"
    assert (np.abs(planes_sum[~holds] - x64[~holds]) <= SPL3_TINY_ERR).all(), "SPL3 planes of a tiny value are off by more than half the smallest bf16 subnormal"


def spl_col(c):
    """Column of channel c's hi value in an SPL32 row; the lo value sits 32 further."""
    return (c >> 5) * 64 + (c & 31)


def spl32(x):
    """float32 [rows, k] (k % 32 == 0) -> uint16 [rows, 2k] in the SPL32 layout."""
    rows, k = x.shape
    hi, lo = split2(x)
    return np.stack([hi.reshape(rows, k // 32, 32), lo.reshape(rows, k // 32, 32)], axis=2).reshape(rows, 2 * k)


def spl3(x):
    """float32 [rows, k] (k % 32 == 0) -> uint16 [rows, 3k] in the SPL3 layout."""
    rows, k = x.shape
    return np.stack([p.reshape(rows, k // 32, 32) for p in split3(x)], axis=2).reshape(rows, 3 * k)


def spl32_written(n, width):
    """Boolean [width]: the columns of an SPL32 output row that a launch with n output channels writes (hi and lo of channels < n)."""
    mask = np.zeros(width, dtype=bool)
    c = np.arange(n)
    mask[spl_col(c)] = True
    mask[spl_col(c) + 32] = True
    return mask


# ------------------------------------------------------------------------------------------------ the product
def linear_ref(a, w, bias=None, residual=None, scale=1.0, relu=False):
    """act(scale * a w^T + bias) + residual in float64, and its error scale |a| |w|^T |scale| + |bias| + |residual|.
    a is [a0 | a1] already concatenated."""
    a64, w64 = np.asarray(a, dtype=np.float64), np.asarray(w, dtype=np.float64)
    ref = a64 @ w64.T * scale
    err_scale = np.abs(a64) @ np.abs(w64).T * abs(scale)
    if bias is not None:
        ref = ref + np.asarray(bias, dtype=np.float64)
        err_scale = err_scale + np.abs(np.asarray(bias, dtype=np.float64))
    if relu:
        ref = np.maximum(ref, 0.0)
    if residual is not None:
        ref = ref + np.asarray(residual, dtype=np.float64)
        err_scale = err_scale + np.abs(np.asarray(residual, dtype=np.float64))
    return ref, err_scale


# ------------------------------------------------------------------------------------------------ canaries
def canary_bits(shape, dtype):
    """A host array of the canary pattern: dtype uint32 (f32 outputs) or uint16 (16-bit outputs)."""
    return np.full(shape, CANARY_F32 if np.dtype(dtype) == np.uint32 else CANARY_16, dtype=dtype)


def assert_pad_intact(bits, m, n, what="", written_cols=None):
    """bits: the whole padded output as unsigned integers [rows >= m, cols >= n].  Everything outside the window [:m, :n] -- or, with
    written_cols (boolean per column), outside those columns of the first m rows -- must still be the canary, bit for bit."""
    canary = CANARY_F32 if bits.dtype == np.uint32 else CANARY_16
    inside = np.zeros(bits.shape, dtype=bool)
    inside[:m, :n] = True if written_cols is None else written_cols[None, :n]
    bad = np.argwhere(~inside & (bits != canary))
    assert len(bad) == 0, f"{what}: {len(bad)} elements outside the {m} x {n} window were written, first at {tuple(int(v) for v in bad[0]) if len(bad) else None} (buffer {bits.shape})"


def is_canary(bits):
    return bits == (CANARY_F32 if bits.dtype == np.uint32 else CANARY_16)


# ------------------------------------------------------------------------------------------------ the instance rule
def x3p_instance(m, n, hi_only=False, guarded=False, cus=256):
    """Which pre-split instance gims_linear launches for an m x n problem (the shape rule of gims_amd/csrc/linear.hip, with none of the
    GIMS_X3P_* overrides set), as the lower-case GIMS_LINEAR_KERNEL_* name that hip.linear_launch_counts() reports.
    Returns (name, tile rows, tile columns)."""
    cdiv = lambda a, b: (a + b - 1) // b       # noqa: E731
    big_blocks = cdiv(m, 256) * cdiv(n, 256)
    tiles128 = cdiv(m, 128) * cdiv(n, 128)
    big = big_blocks >= 192 and (n % 256 == 0 or n > 512)
    if big and hi_only:
        return "x3p_256x128_w8_s3_hi", 256, 128
    if big:
        if guarded and 8 * cdiv(cdiv(m, 256), 8) * cdiv(n, 256) > cus:
            return "x3p_256x256_w8_s2_walk", 256, 256
        return "x3p_256x256_w8_s2", 256, 256
    if n <= 64 and not hi_only:
        return ("x3p_128x32_w4_s2", 128, 32) if n <= 32 else ("x3p_128x64_w4_s2", 128, 64)
    if tiles128 <= 128:
        return ("x3p_64x64_w4_s4_hi", 64, 64) if hi_only else ("x3p_64x64_w4_s3", 64, 64)
    if hi_only:
        return "x3p_128x128_w4_s4_hi", 128, 128
    if tiles128 > 256:
        return "x3p_128x128_w4_s2", 128, 128
    return "x3p_128x128_w8_s2", 128, 128


# the shapes of tests/test_linear_instances_gpu.py: (expected instance, m, n, hi_only).  Every m leaves ONE row in the last row tile; every
# n is a multiple of 4 whose last eight-column lane group is half in range (n % 8 == 4: the `cok && !full` stores of the epilogue)
INSTANCE_TABLE = (
    ("x3p_64x64_w4_s3", 129, 516, False),
    ("x3p_64x64_w4_s4_hi", 129, 516, True),
    ("x3p_128x32_w4_s2", 129, 28, False),
    ("x3p_128x64_w4_s2", 257, 36, False),
    ("x3p_128x128_w8_s2", 3329, 516, False),
    ("x3p_128x128_w4_s2", 6529, 516, False),
    ("x3p_128x128_w4_s4_hi", 3329, 516, True),
    ("x3p_256x256_w8_s2", 16129, 516, False),
    ("x3p_256x128_w8_s3_hi", 16129, 516, True),
)

# the six-pass score GEMM walks 256 x 128 tiles, at most 1024 problems per launch
X6_TM, X6_TN, X6_MAX_PROBLEMS = 256, 128, 1024


def x6_tiles(m, n, upper=False):
    """Tiles of one problem in linear_x6_kernel's list: all of them, or for GIMS_LINEAR_UPPER those not entirely below the diagonal."""
    ntm, ntn = -(-m // X6_TM), -(-n // X6_TN)
    if not upper:
        return ntm * ntn
    return sum(max(ntn - 2 * by, 0) for by in range(ntm))
