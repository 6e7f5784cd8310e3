"""The restatement of the fundamental-matrix estimator (tests/fundamental_ref.py) against independent references, the conditions under
which tests/test_fundamental_gpu.py may compare index sets exactly, and the place of the `model` field in gims_verify_set.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from gims_amd import hip
from oracle import eval_oracle as E
from tests import fundamental_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_up_to_scale_and_sign(A, B):
    """Largest entry of A / ||A|| -+ B / ||B||, whichever sign fits."""
    a, b = A / np.linalg.norm(A), B / np.linalg.norm(B)
    return min(np.abs(a - b).max(), np.abs(a + b).max())


def _svd_8point(p0, p1):
    """Hartley's normalised 8-point algorithm with np.linalg.svd: the independent reference."""
    def norm(p):
        p = p.astype(np.float64)
        c = p.mean(0)
        s = np.sqrt(2.0) / np.sqrt(((p - c) ** 2).sum(1)).mean()
        return (p - c) * s, np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])
    q0, T0 = norm(p0)
    q1, T1 = norm(p1)
    A = np.stack([q1[:, 0] * q0[:, 0], q1[:, 0] * q0[:, 1], q1[:, 0], q1[:, 1] * q0[:, 0], q1[:, 1] * q0[:, 1], q1[:, 1], q0[:, 0], q0[:, 1],
                  np.ones(len(q0))], 1)
    Fn = np.linalg.svd(A)[2][-1].reshape(3, 3)
    U, s, Vt = np.linalg.svd(Fn)
    Fn = U @ np.diag([s[0], s[1], 0.0]) @ Vt
    return T1.T @ Fn @ T0


def test_the_first_four_indices_are_the_homography_sample():
    for seed in (0, 1, 77, 2 ** 63 + 5):
        for hyp in (0, 1, 15, 16, 499, 2 ** 20 - 1):
            for k in (8, 9, 63, 2049):
                s = R.sample8(seed, hyp, k)
                assert len(set(s.tolist())) == 8 and s.min() >= 0 and s.max() < k
                np.testing.assert_array_equal(s[:4], E.ransac_sample(seed, hyp, k))


@pytest.mark.parametrize("config", R.CONFIGS)
def test_noise_free_scenes_recover_the_planted_model(config):
    p0, p1 = R.clean_pairs(config, 64)
    Ft = R.planted_F(config)
    if config == "xtrans":
        assert Ft[2, 2] == 0                                          # no named entry of F can be fixed to 1
    # float32 coordinates of an 800 x 600 image: the entries of the unit-norm F are determined to about 1e-7 relative to the largest
    for lo in R.LO_ITERS:
        v = R.verify(p0, p1, 3, 20, R.THRESH, lo)
        assert v["ok"] == 1 and v["n_inliers"] == 64 and v["mask"].all()
        assert abs(np.linalg.norm(v["F"]) - 1) <= 1e-12
        assert _same_up_to_scale_and_sign(v["F"], Ft) <= 1e-6, (config, lo)
        assert _same_up_to_scale_and_sign(v["F"], _svd_8point(p0, p1)) <= 1e-6, (config, lo)
        assert abs(np.linalg.det(v["F"])) <= 1e-15                    # rank 2 at rounding level (the entries are at most 1)
    # the minimal model of eight clean points is the planted one, too, and so is a refit of all of them
    F8 = R.minimal_model(p0[:8], p1[:8])
    assert _same_up_to_scale_and_sign(F8, Ft) <= 1e-4
    assert _same_up_to_scale_and_sign(R.lo_round(F8, p0, p1, 9.0), _svd_8point(p0, p1)) <= 1e-6      # rank 2 taken in other coordinates


def test_jacobi_against_eigh_and_tiny_off_diagonals():
    r = np.random.default_rng(5)
    for n in (3, 9):
        B = r.standard_normal((40, n))
        S = B.T @ B
        w, U = np.linalg.eigh(S)
        v = R.jacobi(S)
        assert min(np.abs(v - U[:, 0]).max(), np.abs(v + U[:, 0]).max()) <= 1e-12
    # off-diagonal entries far below the diagonal's differences: the angle is formed without a quotient that overflows
    S = np.diag([3.0, 1.0, 2.0])
    S[0, 1] = S[1, 0] = 1e-300
    S[1, 2] = S[2, 1] = 5e-324
    v = R.jacobi(S)
    assert np.isfinite(v).all() and abs(abs(v[1]) - 1) <= 1e-15


def test_degenerate_samples_have_no_model():
    same = np.repeat(np.array([[10.0, 20.0]], dtype=np.float32), 8, 0)
    assert R.minimal_model(same, same) is None
    assert R.verify(same, same, 1, 16)["ok"] == 0
    p0, p1 = R.clean_pairs("general", 7)
    assert R.verify(p0, p1, 1, 16)["ok"] == 0                         # fewer than eight correspondences


@pytest.mark.parametrize("config", R.CONFIGS)
@pytest.mark.parametrize("K", R.KS)
def test_every_fixture_meets_the_margin(K, config):
    """What makes the exact comparison of masks, counts and rounds on the GPU legitimate: no inlier decision of any scored hypothesis or
    of any model of stage 2 lies within MARGIN of the threshold, at every hypothesis count and lo_iters the GPU test uses."""
    if K < 8:
        assert all(R.fixture_expected(K, config, it, lo)["ok"] == 0 for it in R.ITERS for lo in R.LO_ITERS)
        return
    assert (K, config) in R.SEEDS
    assert R.fixture_margin(K, config) >= R.MARGIN
    for it in R.ITERS:
        for lo in R.LO_ITERS:
            v = R.fixture_expected(K, config, it, lo)
            # (a lone contaminated hypothesis may keep fewer than its eight points once it is made rank 2: no count is asserted here)
            assert v["ok"] == 1 and abs(np.linalg.det(v["F"])) <= 1e-15
    # the planted inliers are found: at 500 hypotheses at least 90 % of the correspondences that are no outliers (eight or nine noisy
    # points do not determine the planted model: nothing to find there)
    if K <= 9:
        return
    spec = R.planted_spec(K, config)
    p0, p1 = R.correspondences(spec)
    planted, _ = R.decisions(spec[3] / np.linalg.norm(spec[3]), p0, p1, R.THRESH ** 2)
    assert R.fixture_expected(K, config, 500, 8)["mask"][planted].mean() >= 0.9


def test_summation_order_spread_is_what_the_gpu_test_quotes():
    """The spread of the model under the order of the inlier sums, the figure in the header of tests/test_fundamental_gpu.py."""
    from tests.test_fundamental_gpu import SPREAD
    worst = 0.0
    for K in (63, 257, 2049):
        for config in R.CONFIGS:
            a, b = R.fixture_expected(K, config, 500, 8), R.fixture_expected(K, config, 500, 8, reverse=True)
            assert a["lo_rounds"] == b["lo_rounds"] and (a["mask"] == b["mask"]).all()
            worst = max(worst, float(np.abs(a["F"] - b["F"]).max()))
    assert worst <= SPREAD, worst


def test_model_field_and_constants_match_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gims_hip.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %d %d\\n", sizeof(gims_verify_set), offsetof(gims_verify_set, has_ref), '
                   'offsetof(gims_verify_set, model), offsetof(gims_verify_set, h_ref), GIMS_VERIFY_MODEL_HOMOGRAPHY, '
                   'GIMS_VERIFY_MODEL_FUNDAMENTAL);\nreturn 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = hip.VerifySet
    # `model` sits where `reserved` sat: the second int32 after the four shape fields, 44 bytes in
    assert got[:4] == [ctypes.sizeof(S), S.has_ref.offset, S.model.offset, S.h_ref.offset] == [112, 40, 44, 48]
    assert got[4:] == [hip.VERIFY_MODELS["homography"], hip.VERIFY_MODELS["fundamental"]] == [0, 1]
    assert not hasattr(S, "reserved")
    assert hip.verify_model("fundamental") == hip.verify_model(1) == 1 and hip.verify_model("homography") == hip.verify_model(0) == 0
    for bad in ("essential", 2, True, None):
        with pytest.raises(hip.GimsHipError, match="model"):
            hip.verify_model(bad)
