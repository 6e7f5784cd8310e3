"""CPU tests of image-set matching: the ABI constant and the argument checks of GIMS_AUX_ASSEMBLE_ROWS (they run before any HIP call), the
pins a feature must leave alone, the host-side table builder of hip.assemble_rows, and the NumPy restatement (tests/features_ref.py)
against hand-worked bit patterns."""
import numpy as np
import pytest
import torch

import gims_amd
from gims_amd import hip
from tests import features_ref as R


def test_abi_constant_and_pins():
    assert hip.AUX_ASSEMBLE_ROWS == 8 == hip.ABI.constants["GIMS_AUX_ASSEMBLE_ROWS"]
    # the feature adds no export, no struct and no ABI version
    assert len(hip.EXPORTS) == 90 and len(hip.ABI.structs) == 28 and hip.ABI_VERSION == 5 == hip.load().gims_abi_version()
    assert not any("assemble" in name.lower() for name in hip.EXPORTS)
    assert gims_amd.ImageFeatures is gims_amd.gmatcher.ImageFeatures and "ImageFeatures" in gims_amd.__all__


def _run(ptrs, ints):
    """Through hip.run_ops, on the null stream (no device is needed: a refused call makes no HIP call, an empty one none either)."""
    with hip.on_stream(0):
        hip.run_ops(hip.make_ops([hip.op_aux(hip.AUX_ASSEMBLE_ROWS, ptrs, ints)]))


def test_argument_checks_come_before_any_hip_call():
    """Every GIMS_EINVAL case of the header, with a message naming assemble_rows; the pointers are never dereferenced."""
    p = [0x10000, 0x20000, 0x30000]                                # table, out, out_split
    good = [3, 100, 256, 256, 512, 0]                              # n_seg, n_rows, k, ld_out, ld_split, reserved

    def refused(ptrs, ints, word):
        with pytest.raises(hip.GimsHipError, match="assemble_rows") as e:
            _run(ptrs, ints)
        assert word in str(e.value) and f"({hip.GIMS_EINVAL})" in str(e.value), str(e.value)

    refused([None, p[1], p[2]], good, "table is NULL")
    refused([p[0], None, None], good, "both NULL")
    refused(p, [-1] + good[1:], "n_seg = -1")
    refused(p, [3, -5] + good[2:], "n_rows = -5")
    for k in (0, -32, 48, 257):
        refused(p, [3, 100, k, 256, 512, 0], f"k = {k}")
    refused(p, [3, 100, 256, 252, 512, 0], "ld_out = 252")
    refused(p, [3, 100, 256, 256, 448, 0], "ld_split = 448")
    refused([p[0], p[1], None], [3, 100, 256, 252, 0, 0], "ld_out = 252")        # ... and for the one output that is there
    refused([p[0], None, p[2]], [3, 100, 256, 0, 448, 0], "ld_split = 448")
    # the alignment rules of gims_linear's pre-split operands: addresses, then pitches
    refused([p[0], p[1] + 4, p[2]], good, "alignment")
    refused([p[0], p[1], p[2] + 64], good, "alignment")
    refused(p, [3, 100, 256, 258, 512, 0], "alignment")
    refused(p, [3, 100, 256, 256, 544, 0], "alignment")
    refused(p, [3, 100, 256, 256, 1 << 22, 0], "alignment")
    refused([p[0] + 4, p[1], p[2]], good, "table must be 8-byte aligned")
    refused(p, good[:5] + [1], "reserved")
    # i[5] would select a later form of the function, so it is read first: whatever the other words hold, this version does not know the call
    refused([None] * 3, [8, 8, 8, 8, 8, 8], "unknown auxiliary function form")
    # an output that is absent has no pitch to check
    _run([None, p[1], None], [0, 100, 256, 256, 0, 0])
    _run([None, None, p[2]], [0, 100, 256, 0, 512, 0])


def test_empty_calls_are_ok_and_touch_nothing():
    _run([None, 0x20000, 0x30000], [0, 100, 256, 256, 512, 0])                    # n_seg == 0, even with a NULL table
    _run([0x10000, 0x20000, 0x30000], [3, 0, 256, 256, 512, 0])                   # n_rows == 0
    _run([None, 0x20000, None], [0, 0, 128, 128, 0, 0])
    with pytest.raises(hip.GimsHipError, match="both NULL"):                      # the other arguments are still checked
        _run([None, None, None], [0, 0, 256, 256, 512, 0])


def test_table_builder():
    """assemble_table: a repeated source is fine; overlapping destinations, destinations past the output and a non-f32 source are not."""
    a = torch.zeros((7, 256))
    b = torch.zeros((40, 320))[3:8, :256]                                         # pitch 320, first row inside its allocation
    tab = hip.assemble_table([(b, 14), (a, 0), (a, 7)], 19, 256, "cpu")
    assert tab.dtype == np.int64 and tab.shape == (3, 4)
    np.testing.assert_array_equal(tab, [[a.data_ptr(), 256, 7, 0], [a.data_ptr(), 256, 7, 7], [b.data_ptr(), 320, 5, 14]])   # ascending by destination
    assert hip.assemble_table([], 5, 256, "cpu").shape == (0, 4)
    assert hip.assemble_table([(a[:0], 3), (a, 3)], 10, 256, "cpu").tolist()[1] == [a.data_ptr(), 256, 7, 3]                # an empty segment holds nothing
    with pytest.raises(ValueError, match="overlap"):
        hip.assemble_table([(a, 0), (a, 6)], 19, 256, "cpu")
    with pytest.raises(ValueError, match="overlap"):
        hip.assemble_table([(a, 5), (b, 8), (a, 12)], 19, 256, "cpu")
    with pytest.raises(ValueError, match="outside"):
        hip.assemble_table([(a, 13)], 19, 256, "cpu")
    with pytest.raises(ValueError, match="outside"):
        hip.assemble_table([(a, -1)], 19, 256, "cpu")
    with pytest.raises(ValueError, match="float32"):
        hip.assemble_table([(a.double(), 0)], 19, 256, "cpu")
    with pytest.raises(ValueError, match="float32"):
        hip.assemble_table([(a.to(torch.bfloat16), 0)], 19, 256, "cpu")
    with pytest.raises(ValueError, match="unit stride"):
        hip.assemble_table([(torch.zeros((256, 7)).t(), 0)], 19, 256, "cpu")
    with pytest.raises(ValueError, match="unit stride"):
        hip.assemble_table([(a[:, :128], 0)], 19, 256, "cpu")                     # fewer than k channels
    with pytest.raises(ValueError, match="16-byte aligned"):
        hip.assemble_table([(torch.zeros((7, 258))[:, 1:257], 0)], 19, 256, "cpu")
    with pytest.raises(ValueError, match="16-byte aligned"):
        hip.assemble_table([(torch.zeros((7, 258))[:, :256], 0)], 19, 256, "cpu")  # pitch 258
    with pytest.raises(ValueError, match="is on"):
        hip.assemble_table([(a, 0)], 19, 256, "cuda:0")


def test_restatement_against_hand_worked_values():
    """bf16 is the upper half of the float32 pattern after rounding to nearest, ties to even; lo = bf16(x - hi) in float32.
      1.0          3F800000 -> hi 3F80; lo = bf16(0) = 0000
      -0.0         80000000 -> hi 8000; lo = bf16(-0.0 - -0.0 = +0.0) = 0000
      1 + 2^-9     3F804000: the dropped half 4000 is below 8000 -> hi 3F80 (1.0); lo = 2^-9 = 3B00
      1 + 2^-8     3F808000: a tie, 3F80 is even -> hi 3F80; lo = 2^-8 = 3B80
      1 + 3 2^-8   3F818000: a tie, 3F81 is odd -> hi 3F82 (1 + 2^-6); lo = -2^-8 = BB80
      3e38         7F61B1E6: B1E6 is above 8000 -> hi 7F62; x - hi = -(620000 - 61B1E6) = -4E1A units of 2^104 = -1.0011100 0011010b 2^118 ->
                   sign 1, exponent 118 + 127 = F5, mantissa 0011100 (the dropped 0011010 is below half) -> lo FA9C
      1e-40        a denormal, 000116C2: 16C2 is below 8000 -> hi 0001 (2^-133); x - hi = 000016C2 -> lo 0000"""
    x = np.array([1.0, -0.0, 1 + 2.0 ** -9, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 3e38, 1e-40], dtype=np.float32)
    assert x.view(np.uint32).tolist() == [0x3F800000, 0x80000000, 0x3F804000, 0x3F808000, 0x3F818000, 0x7F61B1E6, 0x000116C2]
    hi = R.f2bf(x)
    lo = R.f2bf(x - R.bf2f(hi))
    assert hi.tolist() == [0x3F80, 0x8000, 0x3F80, 0x3F80, 0x3F82, 0x7F62, 0x0001]
    assert lo.tolist() == [0x0000, 0x0000, 0x3B00, 0x3B80, 0xBB80, 0xFA9C, 0x0000]
    # placement: channel c of a row -> hi at 64 (c / 32) + c % 32, lo 32 further
    assert R.spl_col(np.array([0, 31, 32, 63, 64, 255])).tolist() == [0, 31, 64, 95, 128, 479]
    row = np.zeros((1, 64), dtype=np.float32)
    row[0, [0, 33]] = x[[2, 5]]
    s = R.split(row)
    assert s.shape == (1, 128) and s[0, 0] == 0x3F80 and s[0, 32] == 0x3B00 and s[0, 64 + 1] == 0x7F62 and s[0, 96 + 1] == 0xFA9C
    assert np.count_nonzero(s) == 4


def test_restatement_clips_and_skips():
    src = np.arange(5 * 32, dtype=np.float32).reshape(5, 32)
    out = np.full((6, 32), -7.0, dtype=np.float32)
    spl = np.full((6, 64), 0x1234, dtype=np.uint16)
    R.assemble([(src[:2], 0), (src[:0], 2), (src[2:], 4)], 32, out, spl)          # rows 2 and 3: a gap; the last segment overruns by one row
    np.testing.assert_array_equal(out[[0, 1, 4, 5]], src[[0, 1, 2, 3]])
    assert (out[2:4] == -7.0).all() and (spl[2:4] == 0x1234).all()
    np.testing.assert_array_equal(spl[[0, 1, 4, 5]], R.split(src[:4]))
