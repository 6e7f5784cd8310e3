"""The restatements of tests/linear_ref.py against a second formulation: torch.bfloat16 conversion for the number formats and layouts, exact
reconstruction for SPL3, and the shape table of tests/test_linear_instances_gpu.py against the restated instance rule."""
import numpy as np
import torch

from tests import linear_ref as R


def _values(seed=3, n=4096):
    """Wide-range values plus the cases a rounding routine gets wrong: signed zeros, f32 subnormals, exact bf16 ties (even and odd
    neighbours), values one ulp beside a tie, the largest finite bf16."""
    r = np.random.default_rng(seed)
    x = (r.normal(size=n) * np.exp(r.normal(size=n) * 4)).astype(np.float32)
    x = x[np.abs(x) < R.BF16_MAX]
    u = x[:512].view(np.uint32)
    ties = ((u & 0xFFFF0000) | 0x8000).astype(np.uint32)
    special = np.array([0.0, -0.0, 1e-40, -3e-42, 1.4e-45, -1.4e-45, R.BF16_MAX, -R.BF16_MAX, 1.0, 321.5], dtype=np.float32)
    return np.concatenate([x, ties.view(np.float32), (ties + 1).view(np.float32), (ties - 1).view(np.float32), special])


def _torch_bf16_bits(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def test_bf16_rounding_equals_torch():
    x = _values()
    np.testing.assert_array_equal(R.bf16_bits(x), _torch_bf16_bits(x))
    np.testing.assert_array_equal(R.bf16_value(R.bf16_bits(x)), torch.from_numpy(x).to(torch.bfloat16).float().numpy())
    # ties go to the even neighbour
    assert R.bf16_bits(np.array([0x3F808000], dtype=np.uint32).view(np.float32))[0] == 0x3F80
    assert R.bf16_bits(np.array([0x3F818000], dtype=np.uint32).view(np.float32))[0] == 0x3F82
    nan = R.bf16_value(R.bf16_bits(np.array([np.nan, np.inf, -np.inf], dtype=np.float32)))
    assert np.isnan(nan[0]) and nan[1] == np.inf and nan[2] == -np.inf


def test_half_saturates_and_rounds_like_torch():
    x = np.concatenate([_values(), np.array([65504.0, 65519.9, 65520.0, 1e9, -1e9, 7e4, 2049.0, 2051.0], dtype=np.float32)])
    want = torch.from_numpy(x).clamp(-65504.0, 65504.0).to(torch.float16).view(torch.int16).numpy().view(np.uint16)
    got = R.f16_sat_bits(x)
    np.testing.assert_array_equal(got, want)
    assert np.isfinite(got.view(np.float16)).all()


def test_split2_and_spl32_layout():
    x = _values()[-4064:].reshape(127, 32)
    x = np.concatenate([x, x[::-1] * np.float32(-0.75)], axis=1)    # [127, 64]: two channel blocks
    hi, lo = R.split2(x)
    t = torch.from_numpy(x)
    th = t.to(torch.bfloat16)
    tl = (t - th.float()).to(torch.bfloat16)
    np.testing.assert_array_equal(hi, th.view(torch.int16).numpy().view(np.uint16))
    np.testing.assert_array_equal(lo, tl.view(torch.int16).numpy().view(np.uint16))
    buf = R.spl32(x)
    assert buf.shape == (127, 128)
    for c in (0, 5, 31, 32, 63):
        np.testing.assert_array_equal(buf[:, R.spl_col(c)], hi[:, c])
        np.testing.assert_array_equal(buf[:, R.spl_col(c) + 32], lo[:, c])
    np.testing.assert_array_equal(buf[:, 64:96], hi[:, 32:64])
    np.testing.assert_array_equal(buf[:, 96:128], lo[:, 32:64])
    mask = R.spl32_written(36, 192)
    assert mask.sum() == 72 and mask[:32].all() and mask[32:64].all() and mask[64:68].all() and mask[96:100].all() and not mask[68:96].any() and not mask[100:].any()


def test_spl3_reconstructs_exactly():
    x = _values()[-4064:].reshape(127, 32)
    x = np.concatenate([x, -x[::-1]], axis=1)
    a1, a2, a3 = R.split3(x)
    rec = R.bf16_value(a1).astype(np.float64) + R.bf16_value(a2) + R.bf16_value(a3)
    # 8 + 8 + 8 significant bits: the split is exact, down to what bf16 can hold at all (f32 subnormals have bits below 2^-133)
    R.assert_spl3_sums_back(rec, x)
    tiny = np.abs(x) < R.SPL3_EXACT_MIN
    assert tiny.sum() >= 12 and (~tiny).sum() > 8000
    assert (rec[~tiny] == x[~tiny].astype(np.float64)).all()
    np.testing.assert_array_equal(a1, _torch_bf16_bits(x))
    buf = R.spl3(x)
    assert buf.shape == (127, 192)
    np.testing.assert_array_equal(buf[:, 96:128], a1[:, 32:64])
    np.testing.assert_array_equal(buf[:, 128:160], a2[:, 32:64])
    np.testing.assert_array_equal(buf[:, 160:192], a3[:, 32:64])


def test_linear_ref_equals_a_loop():
    r = np.random.default_rng(1)
    a, w = r.normal(size=(5, 8)).astype(np.float32), r.normal(size=(3, 8)).astype(np.float32)
    bias, res = r.normal(size=3).astype(np.float32), r.normal(size=(5, 3)).astype(np.float32)
    ref, sc = R.linear_ref(a, w, bias, res, scale=-0.5, relu=True)
    for i in range(5):
        for j in range(3):
            dot = sum(float(a[i, k]) * float(w[j, k]) for k in range(8))
            mag = sum(abs(float(a[i, k]) * float(w[j, k])) for k in range(8))
            assert abs(ref[i, j] - (max(-0.5 * dot + float(bias[j]), 0.0) + float(res[i, j]))) < 1e-12
            assert abs(sc[i, j] - (0.5 * mag + abs(float(bias[j])) + abs(float(res[i, j])))) < 1e-12


def test_canary_helpers():
    for dt in (np.uint32, np.uint16):
        b = R.canary_bits((5, 9), dt)
        b[:3, :4] = 7
        R.assert_pad_intact(b, 3, 4)
        for bad in ((3, 0), (0, 4), (4, 8)):
            c = b.copy()
            c[bad] = 0
            try:
                R.assert_pad_intact(c, 3, 4, "probe")
            except AssertionError as e:
                assert "probe" in str(e) and str(bad) in str(e)
            else:
                raise AssertionError(f"a write at {bad} went unnoticed")
    assert np.isnan(np.array([R.CANARY_F32], dtype=np.uint32).view(np.float32)[0]) and np.isnan(R.bf16_value(np.array([R.CANARY_16], dtype=np.uint16))[0])


def test_instance_table_agrees_with_the_rule():
    """Every shape of the GPU module reaches the instance it names, leaves one row in the last row tile of that instance and half a lane
    group (four columns) at the end of its last column tile; the table names nine different instances."""
    assert len({row[0] for row in R.INSTANCE_TABLE}) == len(R.INSTANCE_TABLE) == 9
    for name, m, n, hi_only in R.INSTANCE_TABLE:
        got, tm, tn = R.x3p_instance(m, n, hi_only)
        assert got == name, (m, n, hi_only, got)
        assert m % tm == 1 and n % 4 == 0 and n % 8 == 4, (name, m, n)
        assert name == f"x3p_{tm}x{tn}_" + name.split("_", 2)[2]
    # the shapes of the existing row-independence test and of the walked guarded launch
    assert R.x3p_instance(300, 256)[0] == "x3p_64x64_w4_s3" and R.x3p_instance(8320, 256)[0] == "x3p_128x128_w8_s2"
    assert R.x3p_instance(49153, 256)[0] == "x3p_256x256_w8_s2"
    assert R.x3p_instance(2304 * 16, 768, guarded=True)[0] == "x3p_256x256_w8_s2_walk" and R.x3p_instance(2304 * 16, 768)[0] == "x3p_256x256_w8_s2"
    # the seams of the rule itself: 128 / 129 and 256 / 257 tiles of 128 x 128, 191 / 192 tiles of 256 x 256
    assert R.x3p_instance(128 * 32, 512)[0] == "x3p_64x64_w4_s3" and R.x3p_instance(128 * 32 + 1, 512)[0] == "x3p_128x128_w8_s2"
    assert R.x3p_instance(128 * 64, 512)[0] == "x3p_128x128_w8_s2" and R.x3p_instance(128 * 64 + 1, 512)[0] == "x3p_128x128_w4_s2"
    assert R.x3p_instance(256 * 95 + 1, 512)[0] == "x3p_256x256_w8_s2" and R.x3p_instance(256 * 95, 512)[0] == "x3p_128x128_w4_s2"
    assert R.x3p_instance(16128, 516)[0] == "x3p_128x128_w4_s2" and R.x3p_instance(16129, 512)[0] == "x3p_128x128_w4_s2"


def test_x6_tile_counts():
    assert R.x6_tiles(1, 1) == 1 and R.x6_tiles(257, 129) == 4 and R.x6_tiles(1300, 1300) == 66
    # symmetric product: row by of 256-row tiles keeps the 128-column tiles bx >= 2 by
    assert R.x6_tiles(700, 700, upper=True) == 6 + 4 + 2 and R.x6_tiles(1300, 1300, upper=True) == 11 + 9 + 7 + 5 + 3 + 1


def test_kernel_kind_names_follow_the_header():
    from gims_amd import hip
    assert len(hip.LINEAR_KERNEL_NAMES) == hip.ABI.constants["GIMS_LINEAR_KERNEL_KINDS"] == 17
    for i, name in enumerate(hip.LINEAR_KERNEL_NAMES):
        assert hip.ABI.constants["GIMS_LINEAR_KERNEL_" + name.upper()] == i
    assert hip.LINEAR_KERNEL_NAMES[:5] == ("f32", "bf16x3", "f32_batch", "bf16x3_batch", "x6_batch")
    assert {row[0] for row in R.INSTANCE_TABLE} <= set(hip.LINEAR_KERNEL_NAMES)
