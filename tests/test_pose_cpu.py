"""The restatement of the calibrated relative-pose model (tests/pose_ref.py) against independent references, the conditions under which
tests/test_pose_gpu.py may compare index sets exactly, and the place of the new model in gims_verify_set.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from gims_amd import hip
from oracle import eval_oracle as E
from tests import pose_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dist(A, B):
    """Largest entry of A / ||A|| -+ B / ||B||, whichever sign fits."""
    a, b = A / np.linalg.norm(A), B / np.linalg.norm(B)
    return min(np.abs(a - b).max(), np.abs(a + b).max())


def _sample(config, n, seed, exact=False):
    """Camera coordinates of a noise-free scene; exact: from the float64 projections, not from their float32 roundings."""
    a, b, on = R.project_pair(config, n, np.random.default_rng(seed)) if exact else R.clean_pairs(config, n, seed)
    K0, K1 = R.cameras(config)[:2]
    q0, q1 = R.normalise(a.astype(np.float64), b.astype(np.float64), R.intr8(K0, K1))
    return q0, q1, on


def test_the_first_four_indices_are_the_homography_sample():
    for seed in (0, 1, 77, 2 ** 63 + 5):
        for hyp in (0, 1, 15, 16, 499, 2 ** 20 - 1):
            for k in (5, 6, 63, 2049):
                s = R.sample5(seed, hyp, k)
                assert len(set(s.tolist())) == 5 and s.min() >= 0 and s.max() < k
                np.testing.assert_array_equal(s[:4], E.ransac_sample(seed, hyp, k))


BOUND = 1e-6       # float64 rounding (2e-16) through a minimal problem: one fixed bound for every scene, planes included


def test_every_root_satisfies_the_constraints_and_an_independent_route_finds_the_same_roots():
    """Every E of every sample of all five scenes, the planar ones included, at ONE fixed bound: unit norm and x1^T E x0 = 0 on its five
    points to 1e-12 (E is a combination of null vectors, whatever the root); det E and 2 E E^T E - tr(E E^T) E to BOUND; one root of every
    sample is the planted E to BOUND (the median sample finds it to 1e-10).  An independent route -- np.linalg.svd's null space,
    np.linalg.solve for the elimination, np.roots -- has to find the planted E as well and, where no root is multiple, the same number
    of real roots (with R = I the planted root itself is a double one, which np.roots splits into a complex pair)."""
    r = np.random.default_rng(11)
    total = 0
    for config in ("general", "forward", "sideways", "plane7of8", "planar"):
        q0, q1, _ = _sample(config, 64, 2, exact=True)
        idx = np.stack([r.permutation(64)[:5] for _ in range(20)])
        Es, nm, _ = R.five_point(q0[idx], q1[idx])
        planted = R.planted_E(config)
        found = []
        for h in range(20):
            assert 1 <= nm[h] <= 10 and nm[h] % 2 == 0, (config, h, nm[h])      # real roots of a real degree-10 polynomial come in pairs
            x0 = np.concatenate([q0[idx[h]], np.ones((5, 1))], 1)
            x1 = np.concatenate([q1[idx[h]], np.ones((5, 1))], 1)
            for m in range(nm[h]):
                Em = Es[h, m].reshape(3, 3)
                res = max(abs(np.linalg.det(Em)), np.abs(2 * Em @ Em.T @ Em - np.trace(Em @ Em.T) * Em).max())
                assert abs(np.linalg.norm(Em) - 1) <= 1e-12
                assert np.abs(np.einsum("ki,ij,kj->k", x1, Em, x0)).max() <= 1e-12
                assert res <= BOUND, (config, h, m, res)
            found.append(min(_dist(Es[h, m].reshape(3, 3), planted) for m in range(nm[h])))
            assert found[-1] <= BOUND, (config, h, found[-1])
            # the independent route
            x, y, u, v = x0[:, 0], x0[:, 1], x1[:, 0], x1[:, 1]
            A = np.stack([u * x, u * y, u, v * x, v * y, v, x, y, np.ones(5)], 1)
            B = np.linalg.svd(A)[2][5:][None]
            M = R.constraints(B)[0]
            red = np.linalg.solve(M[:, :10], M[:, 10:])
            Bz = R.zmatrix(np.concatenate([np.zeros((6, 10)), red[4:10]], 1)[None])
            roots = np.roots(R.zdet(Bz)[0][::-1])
            real = np.sort(roots[np.abs(roots.imag) <= 1e-9 * (1 + np.abs(roots))].real)
            if config != "sideways":
                assert len(real) == nm[h], (config, h, len(real), nm[h])
                Ei, _ = R.models_at(Bz, B, np.concatenate([real, np.zeros(10 - len(real))])[None], np.array([len(real)]))
                assert min(_dist(Ei[0, k].reshape(3, 3), planted) for k in range(len(real))) <= 1e-2      # (that route is not pivoted)
            total += nm[h]
        assert np.median(found) <= 1e-10, (config, np.median(found))
    assert total >= 200


def test_the_hidden_variable_is_pivoted():
    """Why the order of the basis is chosen per sample: with the first order alone, samples of the plane scenes lose the planted E by
    1e-4 and more; the order with the largest smallest pivot does not."""
    r = np.random.default_rng(11)
    for config in ("plane7of8", "planar"):
        q0, q1, _ = _sample(config, 64, 2, exact=True)
        idx = np.stack([r.permutation(64)[:5] for _ in range(20)])
        x, y, u, v = q0[idx][:, :, 0], q0[idx][:, :, 1], q1[idx][:, :, 0], q1[idx][:, :, 1]
        B, _ = R.null5x9(np.stack([u * x, u * y, u, v * x, v * y, v, x, y, np.ones_like(x)], 2))
        R6, _, quality = R.eliminate10(R.constraints(B))
        Bp, R6p, _ = R.pivoted_elimination(B)
        worst = []
        for basis, rows in ((B, R6), (Bp, R6p)):
            Bz = R.zmatrix(rows)
            roots, count, _, _ = R.real_roots(R.zdet(Bz))
            Es, valid = R.models_at(Bz, basis, roots, count)
            worst.append(max(min([_dist(Es[h, m].reshape(3, 3), R.planted_E(config)) for m in range(10) if valid[h, m]] or [1.0]) for h in range(20)))
        assert worst[0] > 1e-5 and worst[1] <= BOUND, (config, worst)
        assert (R.eliminate10(R.constraints(Bp))[2] >= quality).all()


# the restatement's errors against the planted pose on noise-free float32 points, in degrees (rotation, translation), lo_iters 0 and 8:
# the figures quoted in tests/test_pose_gpu.py and DESIGN.md 4.13
CLEAN = {"general": (8.6e-6, 4.9e-5), "forward": (1.4e-5, 1.2e-4), "sideways": (3.2e-5, 5.1e-5), "plane7of8": (2.9e-5, 3.5e-4)}


@pytest.mark.parametrize("config", R.CONFIGS)
def test_planted_scenes_recover_the_planted_pose(config):
    a, b, on = R.clean_pairs(config, 64)
    intr = R.intr8(*R.cameras(config)[:2])
    worst_r = worst_t = 0.0
    for lo in R.LO_ITERS:
        v = R.verify(a, b, intr, 3, 20, R.THRESH, lo)
        assert v["ok"] == 1 and v["n_inliers"] == 64 and v["n_front"] == 64 and abs(np.linalg.norm(v["E"]) - 1) <= 1e-12
        assert abs(np.linalg.det(v["R"]) - 1) <= 1e-12 and abs(np.linalg.norm(v["t"]) - 1) <= 1e-12
        assert _dist(v["E"], R.planted_E(config)) <= 1e-5              # float32 pixels (5e-8 of the focal length) through a minimal sample
        err_r, err_t = R.pose_errors(R.T_0to1(config), v["R"], v["t"])
        worst_r, worst_t = max(worst_r, err_r), max(worst_t, err_t)
    print(config, "rotation", worst_r, "translation", worst_t)
    assert worst_r <= CLEAN[config][0] and worst_t <= CLEAN[config][1]
    from tests.test_pose_gpu import CLEAN_WORST
    assert max(worst_r, worst_t) <= CLEAN_WORST == max(max(c) for c in CLEAN.values())
    if config == "plane7of8":
        # why this model exists: the 8-point system of the points on the plane has a three-dimensional null space
        q0, q1, _ = _sample(config, 64, 1)
        x, y, u, v = q0[on, 0], q0[on, 1], q1[on, 0], q1[on, 1]
        s = np.linalg.svd(np.stack([u * x, u * y, u, v * x, v * y, v, x, y, np.ones(on.sum())], 1), compute_uv=False)
        assert on.sum() == 56 and s[5] > 1e-3 * s[0] and s[6] <= 1e-6 * s[0]
        # and a minimal sample with four of its five points on the plane still determines the pose
        idx = np.concatenate([np.nonzero(on)[0][:4], np.nonzero(~on)[0][:1]])
        Es, nm, _ = R.five_point(q0[idx][None], q1[idx][None])
        assert min(_dist(Es[0, m].reshape(3, 3), R.planted_E(config)) for m in range(nm[0])) <= 1e-5


def test_a_purely_planar_scene_returns_one_of_its_two_essential_matrices():
    """Every point on one plane: H = R + t n^T / d fits all of them, and so do two essential matrices: the planted one and its twin
    [t']x R' from the other decomposition of H.  Only that is asserted; no pose error."""
    a, b, on = R.clean_pairs("planar", 64)
    assert on.all()
    K0, K1, Rm, t = R.cameras("planar")
    intr = R.intr8(K0, K1)
    n, d = np.array([-0.3, 0.2, 1.0]), 8.0
    H = Rm + np.outer(t, n) / d
    U, s, Vt = np.linalg.svd(H)
    H = H / s[1]
    # the two decompositions of a plane-induced homography (Faugeras): from the eigenvectors of H^T H
    w, V = np.linalg.eigh(H.T @ H)
    v1, v2, v3 = V[:, 2], V[:, 1], V[:, 0]
    if np.linalg.det(np.stack([v1, v2, v3], 1)) < 0:
        v3 = -v3
    s1, s3 = w[2], w[0]
    c1, c3 = np.sqrt((1 - s3) / (s1 - s3)), np.sqrt((s1 - 1) / (s1 - s3))
    cands = []
    for sg in (1.0, -1.0):
        uu = c1 * v1 + sg * c3 * v3
        Uo = np.stack([v2, uu, np.cross(v2, uu)], 1)
        Wo = np.stack([H @ v2, H @ uu, np.cross(H @ v2, H @ uu)], 1)
        Rc = Wo @ Uo.T
        nc = np.cross(v2, uu)
        tc = (H - Rc) @ nc
        tx = np.array([[0, -tc[2], tc[1]], [tc[2], 0, -tc[0]], [-tc[1], tc[0], 0]])
        cands.append(tx @ Rc)
    assert min(_dist(c, R.planted_E("planar")) for c in cands) <= 1e-9
    for lo in R.LO_ITERS:
        v = R.verify(a, b, intr, 3, 20, R.THRESH, lo)
        assert v["ok"] == 1 and v["n_inliers"] == 64 and v["mask"].all()
        assert min(_dist(v["E"], c) for c in cands) <= 1e-4, [_dist(v["E"], c) for c in cands]


def test_degenerate_samples_have_no_model():
    intr = R.intr8(*R.cameras("general")[:2])
    same = np.repeat(np.array([[10.0, 20.0]], dtype=np.float32), 8, 0)
    assert R.verify(same, same, intr, 1, 16)["ok"] == 0
    a, b, _ = R.clean_pairs("general", 4)
    assert R.verify(a, b, intr, 1, 16)["ok"] == 0                      # fewer than five correspondences
    a, b, _ = R.clean_pairs("general", 9)
    assert R.verify(a, b, intr, 1, 0)["ok"] == 0                       # no hypotheses


@pytest.mark.parametrize("config", R.CONFIGS)
@pytest.mark.parametrize("K", R.KS)
def test_every_fixture_meets_the_conditions_of_an_exact_comparison(K, config):
    """What makes the exact comparison of hypotheses, roots, masks, counts, rounds and votes on the GPU legitimate, at every hypothesis
    count and lo_iters the GPU test uses: R.fixture_problems lists every violated condition (margins of all inlier decisions, score and
    vote gaps, depth margins, root stability of the hypotheses within 2 of the best)."""
    if K < 5:
        assert all(R.fixture_expected(K, config, it, lo)["ok"] == 0 for it in R.ITERS for lo in R.LO_ITERS)
        return
    assert (K, config) in R.SEEDS
    assert R.fixture_problems(K, config) == []
    for it in R.ITERS:
        for lo in R.LO_ITERS:
            v = R.fixture_expected(K, config, it, lo)
            assert v["ok"] == 1 and abs(np.linalg.det(v["R"]) - 1) <= 1e-12 and v["n_front"] <= v["n_inliers"]
    if K <= 6:
        return
    # the planted pose is found from 0.5 px of noise and 30 % outliers at 500 hypotheses: degrees, not a twisted pair
    v = R.fixture_expected(K, config, 500, 8)
    err_r, err_t = R.pose_errors(R.T_0to1(config), v["R"], v["t"])
    assert err_r <= 2.0 and v["n_front"] >= 0.9 * v["n_inliers"], (err_r, err_t)        # (a chance inlier may lie behind a camera)


def test_model_constant_layout_and_names(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gims_hip.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %d\\n", sizeof(gims_verify_set), offsetof(gims_verify_set, has_ref), '
                   'offsetof(gims_verify_set, model), offsetof(gims_verify_set, h_ref), GIMS_VERIFY_MODEL_POSE);\nreturn 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = hip.VerifySet
    assert got[:4] == [ctypes.sizeof(S), S.has_ref.offset, S.model.offset, S.h_ref.offset] == [112, 40, 44, 48]
    assert got[4] == hip.VERIFY_MODELS["pose"] == 3 and hip.verify_model("pose") == hip.verify_model(3) == 3
    assert hip.VERIFY_POSE_FLOATS == 24
    for bad in ("essential", 2, True, None, "Pose", 4):                # 2 stays refused: no model is derived from the 8-point F
        with pytest.raises(hip.GimsHipError, match="model"):
            hip.verify_model(bad)


def test_pose_error_and_epipolar_error_are_the_reference_formulas():
    """verify.pose_error / epipolar_error on the CPU (they are batched torch, no kernel) against the formulas of the reference's
    compute_pose_error / compute_epipolar_error written out in NumPy float64."""
    import torch
    from gims_amd import epipolar_error, pose_error, pose_summary
    r = np.random.default_rng(3)
    T = R.T_0to1("general")
    Rm, t = R._rot(0.05, -0.08, 0.02), np.array([0.69, 0.18, 0.28])
    et, er = pose_error(T, Rm, t)
    cos_r = np.clip((np.trace(Rm.T @ T[:3, :3]) - 1) / 2, -1, 1)
    cos_t = np.clip(t @ T[:3, 3] / (np.linalg.norm(t) * np.linalg.norm(T[:3, 3])), -1, 1)
    want_t = np.rad2deg(np.arccos(cos_t))
    assert abs(er.item() - np.rad2deg(np.arccos(cos_r))) <= 1e-6 and abs(et.item() - min(want_t, 180 - want_t)) <= 1e-6
    assert pose_error(T, Rm, -t)[0].item() == pytest.approx(et.item(), abs=1e-12)          # the sign ambiguity of E
    # near zero, where arccos of a rounded cosine stops resolving: 1e-7 degrees of rotation are still seen
    tiny = R._rot(0.0, 0.0, np.deg2rad(1e-7))
    assert pose_error(T, T[:3, :3] @ tiny, T[:3, 3])[1].item() == pytest.approx(1e-7, rel=1e-6)
    et2, er2 = pose_error(torch.from_numpy(np.stack([T, T])), np.stack([Rm, T[:3, :3]]), np.stack([t, T[:3, 3]]))
    assert et2.shape == (2,) and er2[1].item() <= 1e-12 and et2[0].item() == et.item()
    K0, K1 = R.cameras("general")[:2]
    a, b, _ = R.project_pair("general", 30, r)
    b = b + r.standard_normal(b.shape)
    d = epipolar_error(a, b, T, K0, K1).numpy()
    x0 = np.concatenate([(a - K0[:2, 2]) / [K0[0, 0], K0[1, 1]], np.ones((30, 1))], 1)
    x1 = np.concatenate([(b - K1[:2, 2]) / [K1[0, 0], K1[1, 1]], np.ones((30, 1))], 1)
    tv = T[:3, 3]
    Em = np.array([[0, -tv[2], tv[1]], [tv[2], 0, -tv[0]], [-tv[1], tv[0], 0]]) @ T[:3, :3]
    Ep0, Etp1 = x0 @ Em.T, x1 @ Em
    want = np.sum(x1 * Ep0, -1) ** 2 * (1 / (Ep0[:, 0] ** 2 + Ep0[:, 1] ** 2) + 1 / (Etp1[:, 0] ** 2 + Etp1[:, 1] ** 2))
    np.testing.assert_allclose(d, want, rtol=1e-12)
    assert epipolar_error(a, R.project_pair("general", 30, np.random.default_rng(3))[1], T, K0, K1).max().item() <= 1e-20
    s = pose_summary([1.0, (2.0, 0.5), None, float("nan")], thresholds=(5, 10, 20))
    assert s["n_pairs"] == 4 and s["n_posed"] == 2 and s["auc"] == [100.0 * v for v in __import__("gims_amd").evalh.pose_auc([1.0, 2.0, np.inf, np.inf], (5, 10, 20))]


def _fake_set(model, h, has_ref=0, n0=300):
    """A set whose pointers are never dereferenced: the argument checks run before any device call."""
    return hip.VerifySet(0x1000, 0x2000, 0x3000, n0, n0, 600, 800, has_ref, model, (ctypes.c_float * 9)(*h), 0x4000, 0x5000, 0x6000)


def test_pose_arguments_are_checked_before_any_device_call():
    """The GIMS_EINVAL cases of the pose model, also on a machine without a GPU (a device call there would come back as another code), and
    the workspace of a pose set: that of another set plus the best model of every workgroup of hypotheses."""
    lib = hip.load()
    good = [600.0, 610.0, 393.0, 304.0, 590.0, 605.0, 405.0, 297.0, 0.0]
    big = 1 << 40

    def call(model, h, has_ref=0, n0=300):
        arr = (hip.VerifySet * 1)(_fake_set(model, h, has_ref, n0))
        return lib.gims_verify_pairs(arr, 1, 1.0, 500, 8, 0, 0x7000, big, None)

    for which in (0, 1, 4, 5):                                         # the four focal lengths
        for bad in (0.0, -600.0, float("nan"), float("inf")):
            h = list(good)
            h[which] = bad
            assert call(3, h) == hip.GIMS_EINVAL and b"pose" in lib.gims_last_error(), (which, bad)
    for which in (2, 3, 6, 7):                                         # the principal points
        h = list(good)
        h[which] = float("nan")
        assert call(3, h) == hip.GIMS_EINVAL and b"pose" in lib.gims_last_error()
    assert call(3, good[:8] + [1.0]) == hip.GIMS_EINVAL and b"h_ref[8]" in lib.gims_last_error()
    assert call(3, good, has_ref=1) == hip.GIMS_EINVAL and b"has_ref" in lib.gims_last_error()
    assert call(2, good) == hip.GIMS_EINVAL and b"model = 2" in lib.gims_last_error()      # 2 stays refused
    assert call(4, good) == hip.GIMS_EINVAL
    # sizing: the pose set takes 18 more int32 per 16 hypotheses (and two for alignment), the other models what they took
    one = lambda model, iters: lib.gims_verify_workspace_bytes((hip.VerifySet * 1)(_fake_set(model, good if model == 3 else [0.0] * 9)), 1, iters)
    assert one(0, 500) == one(1, 500)
    extra = lambda iters: 256 * ((4 * (iters + 2 + 18 * ((iters + 15) // 16)) + 255) // 256) - 256 * ((4 * iters + 255) // 256)
    for iters in (1, 16, 17, 500, 3000):
        assert one(3, iters) - one(0, iters) == extra(iters), iters
    arr = (hip.VerifySet * 1)(_fake_set(3, good))
    assert lib.gims_verify_pairs(arr, 1, 1.0, 500, 8, 0, 0x7000, one(3, 500) - 1, None) == hip.GIMS_EINVAL
    assert b"workspace too small" in lib.gims_last_error()
