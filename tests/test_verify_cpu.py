"""The estimator of gims_verify_pairs without a GPU: the NumPy restatement (tests/verify_ref.py) against the oracle's RANSAC where the two
specifications coincide (lo_iters = 0), the guarantees of the local optimisation on every fixture, the degenerate inputs, the ctypes
mirror of gims_verify_set, the argument checks that run before any device call, and the conditions under which tests/test_verify_gpu.py
may compare index sets exactly."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from gims_amd import hip
from oracle import eval_oracle as E
from tests import eval_cases as C
from tests import verify_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = [(K, it) for K in R.KS if K >= 4 for it in R.ITERS]


def _pairs(spec):
    kp0, kp1, m0 = spec[0], spec[1], spec[2]
    valid = m0 > -1
    return kp0[valid], kp1[m0[valid]]


ANCHORS = [("compaction", 1025, 1001), ("compaction", 2049, 500), ("two_model", None, C.TWO_MODEL_ITERS)]


def anchor_spec(kind, n0):
    return (C.compaction_case(n0, "all")[0], C.RANSAC_SEED) if kind == "compaction" else (C.two_model_case()[0], C.two_model_case()[1]["seed"])


@pytest.mark.parametrize("kind,n0,iters", ANCHORS)
def test_lo_iters_0_is_the_oracles_ransac(kind, n0, iters):
    """lo_iters = 0 has the specification of gims_eval_pairs: the same model (bit for bit here: the same NumPy calls) and the same mask."""
    spec, seed = anchor_spec(kind, n0)
    p0, p1 = _pairs(spec)
    Hr, mask = E.ransac_homography(p0, p1, seed=seed, iters=iters, thresh=3.0)
    v = R.verify(p0, p1, seed, iters, 3.0, 0)
    assert v["ok"] == 1 and Hr is not None
    np.testing.assert_array_equal(v["H"], Hr)
    np.testing.assert_array_equal(v["mask"], mask)
    assert v["lo_rounds"] == 0 and v["conditions"]["margin"] >= R.MARGIN


def test_lo_iters_0_on_the_degenerate_batch():
    specs, ks = C.degenerate_batch()
    exp = C.degenerate_expected()
    for name, spec in specs.items():
        p0, p1 = _pairs(spec)
        v = R.verify(p0, p1, C.RANSAC_SEED, 500, 3.0, 0)
        assert v["ok"] == int(exp[name]["record"][10]), name
        assert v["n_inliers"] == int(exp[name]["record"][6]), name
        if v["ok"]:
            np.testing.assert_array_equal(v["H"], exp[name]["Hr"])


@pytest.mark.parametrize("K,iters", FIXTURES)
def test_local_optimisation_never_loses_inliers_and_converges(K, iters):
    for lo in (1, 8):
        v = R.fixture_expected(K, iters, lo)
        assert v["ok"] == 1
        assert v["n_inliers"] >= v["best_hyp_inliers"]
        assert v["lo_rounds"] <= lo and v["lo_rounds"] < 8
        prev = v["best_hyp_inliers"]
        for before, after in v["conditions"]["steps"][:v["lo_rounds"]]:
            assert before == prev and after >= before
            prev = after
        assert prev == v["n_inliers"]
    one, eight = R.fixture_expected(K, iters, 1), R.fixture_expected(K, iters, 8)
    assert one["best_hyp"] == eight["best_hyp"] and one["n_inliers"] <= eight["n_inliers"]


def test_local_optimisation_gains_on_the_large_fixtures():
    """What the feature is for: at 30 % outliers the 4-point model misses inliers that the refits recover."""
    for K in (1025, 2049):
        v = R.fixture_expected(K, 500, 8)
        assert v["n_inliers"] > v["best_hyp_inliers"]


@pytest.mark.parametrize("K,iters", FIXTURES)
def test_fixture_conditions(K, iters):
    """(a) score gap, (b) threshold margins, (c) no round one inlier short -- see verify_ref.fixture_conditions."""
    for lo in (1, 8):
        bad = R.fixture_conditions(K, R.fixture_expected(K, iters, lo)["conditions"], iters)
        assert not bad, (K, iters, lo, bad)


def test_no_exactly_collinear_samples_in_the_fixtures():
    """Every hypothesis of every planted fixture has a model: the only degenerate geometry of the GPU tests is the all-identical set."""
    for K in R.KS:
        if K >= 4:
            scores, _ = R.fixture_stage1(K, R.SEEDS[K])
            assert (scores >= 0).all(), K


def test_no_model():
    for K in (0, 3):
        p0, p1 = R.correspondences(R.planted_spec(K))
        assert len(p0) == K
        v = R.verify(p0, p1, 1, 500, 3.0, 8)
        assert v["ok"] == 0 and v["H"] is None and v["n_inliers"] == 0 and not v["mask"].any() and v["n_valid"] == K
    p0, p1 = R.correspondences(R.planted_spec(64))
    assert R.verify(p0, p1, 1, 0, 3.0, 8)["ok"] == 0                                       # no hypotheses
    same0, same1 = np.repeat(p0[:1], 8, 0), np.repeat(p1[:1], 8, 0)                        # all-identical points: every pivot is an exact zero
    for lo in (0, 8):
        v = R.verify(same0, same1, 1, 64, 3.0, lo)
        assert v["ok"] == 0 and v["n_inliers"] == 0


def test_verify_set_layout_matches_the_header(tmp_path):
    fields = [f[0] for f in hip.VerifySet._fields_]
    body = 'printf("size %zu\\n", sizeof(gims_verify_set));\n' + "".join('printf("%s %%zu\\n", offsetof(gims_verify_set, %s));\n' % (f, f) for f in fields)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gims_hip.h"\nint main(void) {\n' + body + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(hip.VerifySet)
    for f in fields:
        assert int(got[f]) == getattr(hip.VerifySet, f).offset, f
    assert hip.VERIFY_FIELDS == ("n_valid", "ok", "n_inliers", "best_hyp", "best_hyp_inliers", "lo_rounds", "err_corner")


def _fake_sets(n, n0=300, matches=True):
    """Sets whose pointers are never followed: the checks below fail before any device call."""
    arr = (hip.VerifySet * n)()
    for i in range(n):
        arr[i] = hip.VerifySet(0x1000, 0x2000, 0x3000 if matches else None, n0, n0 + (0 if matches else 1), 600, 800, 0, 0, (ctypes.c_float * 9)(),
                               0x4000, 0x5000, 0x6000)
    return arr


def test_arguments_are_checked_before_any_device_call():
    """GIMS_EINVAL (-1) with a message, also on a machine without a GPU (a device call there would come back as GIMS_EHIP)."""
    lib = hip.load()
    arr = _fake_sets(2)
    need = lib.gims_verify_workspace_bytes(arr, 2, 500)
    per_set = 300 * 16 + 256 * ((300 * 4 + 255) // 256) + 256 * ((500 * 4 + 255) // 256) + 256
    assert need >= 2 * per_set and need % 256 == 0
    assert lib.gims_verify_workspace_bytes(arr, 2, 501) >= need
    assert lib.gims_verify_pairs(arr, 2, 3.0, 500, 8, 0, 0x7000, need - 1, None) == hip.GIMS_EINVAL
    assert b"workspace too small" in lib.gims_last_error()
    assert lib.gims_verify_pairs(arr, 2, 3.0, 500, 8, 0, None, need, None) == hip.GIMS_EINVAL
    assert lib.gims_verify_pairs(arr, 2, -1.0, 500, 8, 0, 0x7000, need, None) == hip.GIMS_EINVAL
    assert lib.gims_verify_pairs(arr, 2, float("nan"), 500, 8, 0, 0x7000, need, None) == hip.GIMS_EINVAL
    assert lib.gims_verify_pairs(arr, 2, 3.0, -1, 8, 0, 0x7000, need, None) == hip.GIMS_EINVAL
    assert lib.gims_verify_pairs(arr, 2, 3.0, 500, -1, 0, 0x7000, need, None) == hip.GIMS_EINVAL
    assert lib.gims_verify_workspace_bytes(arr, 0, 500) == 0 and lib.gims_verify_workspace_bytes(None, 2, 500) == 0
    ident = _fake_sets(1, matches=False)                                                   # identity pairing with n0 != n1
    big = lib.gims_verify_workspace_bytes(ident, 1, 500)
    assert lib.gims_verify_pairs(ident, 1, 3.0, 500, 8, 0, 0x7000, big, None) == hip.GIMS_EINVAL and b"identity" in lib.gims_last_error()
    many = _fake_sets(65536, n0=1)                                                         # the sets are the grid's y dimension
    assert lib.gims_verify_pairs(many, 65536, 3.0, 16, 8, 0, 0x7000, 1 << 40, None) == hip.GIMS_EINVAL and b"65535" in lib.gims_last_error()
