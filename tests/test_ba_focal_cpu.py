"""CPU tests of bundle adjustment with focal groups: the ABI constant and the pins it must leave alone, the new argument
checks of GIMS_AUX_BUNDLE_ADJUST_FOCAL (they run before any HIP call), the layout of its buffer, the new ValueErrors of
gims_amd.bundle_adjust(refine_focal=...), the NumPy restatement (tests/ba_focal_ref.py) checked on its own, and the conditions on the
fixtures that tests/test_ba_focal_gpu.py compares with the device.

The restatement on its own.  Without a group it gives the bytes of tests/ba_pcg_ref.py.  Fu, Fv equal central differences in s to 1e-6
relative, the bar tests/test_ba_cpu.py uses for the other Jacobians.  The matrix-free S v, b and M_g against a dense Schur complement of
the full damped normal equations with the group columns included differ, relative to the largest entry of what is compared, by at most
  S v  1.3e-13      b  3.8e-13      M_g  1.1e-15
as measured here (the dense route inverts the whole point block at once); SV_BAR, B_BAR and MG_BAR are 16 x these.

Recovery and TOL_FOCAL.  The noise-free scenes of tests/test_ba_cpu.py with 5 and 17 cameras (float32 pixels), the starting focal 5 % too
long for a shared group and +-3 .. 5 % per image; 30 rounds.  Every case is solved forward and in reverse (tests/ba_focal_ref.py says what
is reversed): the largest difference of a word of xyz, R, t, fx, fy, a cost of the history (each divided by max(1, |word|)) or of a
focal_scale is SPREAD_FOCAL = 2.6e-7 (17 cameras, per image: with a lens per image and exact data the cost is flat along focal against
depth, and the two orders end at different places on that floor; 2.0e-9 for 5 cameras per image, 2.3e-13 and below for a shared group).
TOL_FOCAL = 16 x SPREAD_FOCAL = 4.2e-6 is the bound on |focal_scale x planted factor - 1| (measured: 1.3e-6 at worst, 3.1e-7 and 2.5e-8
for the shared groups) and the bar of every comparison with the device, where equality to the bit is what is expected.  On the same
scenes function 14's restatement, with K held wrong, ends at a cost at least 10 x higher (measured: 1.4e8 x and more): the reprojection
floor that no pose and point refinement removes.

Margins (test_fixture_margins): LEAD, DEPTH, PIVOT, CG_STOP, PQ and M_PIVOT are those of tests/test_ba_pcg_cpu.py; MG_PIVOT = 1e-9: every
M_g relative to its A*_g; F1 = 1e-3: every candidate's 1 + ds is that far from 0.  A fixture that failed a margin got another seed or
another cap, not another margin: none had to."""
import functools

import numpy as np
import pytest
import torch

import gims_amd
from gims_amd import hip
from tests import ba_focal_ref as F
from tests import ba_pcg_ref as P
from tests import ba_ref as B
from tests.test_ba_cpu import DEPTH, LEAD, PIVOT, _Points, noise_free, relative_difference
from tests.test_ba_pcg_cpu import CG_STOP, M_PIVOT, PQ, _bits
from tests.test_ba_pcg_cpu import scene as pcg_scene
from tests.test_resect_cpu import _host_tracks

SV_BAR, B_BAR, MG_BAR = 2.1e-12, 6.1e-12, 1.9e-14              # 16 x the measured differences; test_the_matrix_free_system_equals_the_dense_one keeps them honest
TOL_FOCAL = 4.2e-6                                             # 16 x SPREAD_FOCAL, rounded up to two digits; test_recovery_and_tol_focal keeps it honest
MG_PIVOT, F1 = 1e-9, 1e-3


def wrong_focal(sc, factors):
    """The scene with fx, fy of image k multiplied by factors[k] (a scalar: every image)."""
    cams = sc["cams"].copy()
    cams[:, 0], cams[:, 1] = cams[:, 0] * factors, cams[:, 1] * factors
    return dict(sc, cams=cams)


def per_image_factors(n):
    """+-3 .. 5 %, alternating in sign."""
    k = np.arange(n)
    return 1.0 + np.where(k % 2 == 0, 1.0, -1.0) * (0.03 + 0.005 * (k * 7 % 5))


@functools.lru_cache(maxsize=None)
def fixture(name):
    """-> (scene, group [n_images])."""
    if name in ("shared5", "badcam", "behind", "rejtake"):
        sc = wrong_focal(pcg_scene("c5" if name == "shared5" else name), 1.05)
        return sc, np.zeros(len(sc["mode"]), np.int32)
    if name == "two5":
        return wrong_focal(pcg_scene("c5"), np.array([1.05, 1.05, 0.96, 0.96, 0.96])), np.array([0, 0, 1, 1, 1], np.int32)
    if name.startswith("per"):
        n = int(name[3:])
        return wrong_focal(pcg_scene(f"c{n}"), per_image_factors(n)), np.arange(n, dtype=np.int32)
    if name == "none5":                                                       # no group at all: function 14
        return wrong_focal(pcg_scene("c5"), 1.05), np.full(5, -1, np.int32)
    if name == "fixed5":                                                      # the two fixed cameras only
        return wrong_focal(pcg_scene("c5"), np.array([1.05, 1.05, 1.0, 1.0, 1.0])), np.array([0, 0, -1, -1, -1], np.int32)
    if name == "absent":                                                      # group 0 has no posed image (held); the absent image's id is out of range and ignored;
        sc = pcg_scene("poison")                                              # group 1 holds every posed image, the held camera among them
        f = np.where(sc["mode"] != 0, 1.04, 1.0)
        return wrong_focal(sc, f), np.array([1, 1, 1, 1, 1, 1000, 1], np.int32)
    if name == "few":                                                         # the only group has three observations: held
        return pcg_scene("poison"), np.array([-1, -1, -1, -1, -1, -1, 0], np.int32)
    if name == "nfree0":                                                      # both cameras fixed: the lens and the points move
        return wrong_focal(pcg_scene("two"), 1.05), np.zeros(2, np.int32)
    if name.startswith("g"):                                                  # n images in one group: 300 tracks of 8 observations
        n = int(name[1:])
        sc = B.planted_scene(300 + n, [8] * 300, n, noise=0.5, fixed=(0, n - 1), pert_cam=0.005, pert_pt=0.005)
        return wrong_focal(sc, 1.05), np.zeros(n, np.int32)
    if name.startswith("d"):                                                  # 259 images, a group of its own for each of the first n
        n = int(name[1:])
        sc = B.planted_scene(559, [8] * 300, 259, noise=0.5, fixed=(0, 258), pert_cam=0.005, pert_pt=0.005)
        f = np.ones(259)
        f[:n] = per_image_factors(n)
        return wrong_focal(sc, f), np.where(np.arange(259) < n, np.arange(259), -1).astype(np.int32)
    if name.startswith("L"):                                                  # the fixed images 0 and 1 have lists of exactly n observations
        return wrong_focal(pcg_scene(name), 1.05), np.zeros(4, np.int32)
    if name == "mirror":                                                      # the fixed camera 1 rolled by 180 degrees: its own focal group wants 1 + ds = -1
        sc = pcg_scene("c5")
        cams, D = sc["cams"].copy(), np.diag([-1.0, -1.0, 1.0])
        cams[1, 4:13], cams[1, 13:16] = (D @ cams[1, 4:13].reshape(3, 3)).reshape(9), D @ cams[1, 13:16]
        return dict(sc, cams=cams), np.array([-1, 0, -1, -1, -1], np.int32)
    raise KeyError(name)


# every fixture the GPU test compares with the restatement: (fixture, iters, huber, lambda0, cg_iters, cg_tol)
CASES = ([("shared5", 10, 0.0, 1e-4, 128, 1e-6), ("shared5", 0, 0.0, 1e-4, 128, 1e-6), ("shared5", 1, 0.0, 1e-4, 128, 1e-6), ("shared5", 10, 1.5, 1e-4, 128, 1e-6),
          ("shared5", 10, 0.0, 1e-4, 1, 1e-6), ("shared5", 10, 1.5, 1e-4, 2, 0.0), ("two5", 10, 0.0, 1e-4, 128, 1e-6)]
         + [(f"per{n}", 10, 0.0, 1e-4, 128, 1e-6) for n in (3, 5, 17)]
         + [("fixed5", 10, 0.0, 1e-4, 128, 1e-6), ("absent", 10, 0.0, 1e-4, 128, 1e-6), ("absent", 10, 1.5, 1e-4, 128, 1e-6), ("few", 10, 0.0, 1e-4, 128, 1e-6),
            ("nfree0", 10, 0.0, 1e-4, 128, 1e-6)]
         + [(f"g{n}", 2, 0.0, 1e-4, 128, 1e-6) for n in (63, 64, 65, 255, 256, 257)] + [(f"d{n}", 2, 0.0, 1e-4, 128, 1e-6) for n in (255, 256, 257)]
         + [(f"L{n}", 3, 0.0, 1e-4, 128, 1e-6) for n in (63, 64, 65)]
         + [("rejtake", 14, 0.0, 1e-4, 128, 1e-6), ("mirror", 10, 0.0, 1e-4, 128, 1e-6), ("mirror", 8, 0.0, 1e-6, 128, 1e-6), ("badcam", 10, 0.0, 1e-4, 128, 1e-6),
            ("behind", 10, 0.0, 1e-4, 128, 1e-6)])


@functools.lru_cache(maxsize=None)
def reference(name, iters, huber, lambda0, cg_iters, cg_tol, order="forward"):
    """The restatement on a fixture, computed once and shared (do not write to it)."""
    sc, group = fixture(name)
    return F.run(sc, group, iters=iters, huber=huber, lambda0=lambda0, cg_iters=cg_iters, cg_tol=cg_tol, order=order)


def focal_difference(a, b, sc):
    """relative_difference of tests/test_ba_cpu.py, and likewise the words fx, fy of the posed cameras and focal_scale."""
    posed = sc["mode"] != 0
    worst = relative_difference(a, b, sc)
    for x, y in ((a["cams"][posed][:, :2], b["cams"][posed][:, :2]), (a["focal_scale"], b["focal_scale"])):
        if y.size:
            worst = max(worst, float((np.abs(x - y) / np.maximum(1.0, np.abs(y))).max()))
    return worst


# ------------------------------------------------------------------------------------------------ pins, argument checks, layout
def test_abi_constant_and_pins():
    assert hip.AUX_BUNDLE_ADJUST_FOCAL == 16 == hip.ABI.constants["GIMS_AUX_BUNDLE_ADJUST_FOCAL"]
    assert hip.AUX_BUNDLE_ADJUST_PCG == 14 and hip.AUX_BUNDLE_ADJUST == 13
    used = [v for k, v in hip.ABI.constants.items() if k.startswith("GIMS_AUX_")]
    assert 12 not in used and 15 not in used and 99 not in used and -1 not in used
    # the feature adds a constant and a table entry: no export, no struct and no ABI version
    assert len(hip.EXPORTS) == 90 and len(hip.ABI.structs) == 28 and hip.ABI_VERSION == 5 == hip.load().gims_abi_version()
    assert not any("bundle" in name.lower() or "ba_" in name.lower() or "focal" in name.lower() for name in hip.EXPORTS)
    assert hip.BA_TABLE_WORDS == 8


def _run(ptrs, ints, floats=(0.0, 1e-4), fn=None):
    """Through hip.run_ops, on the null stream (no device is needed: a refused call makes no HIP call)."""
    with hip.on_stream(0):
        hip.run_ops(hip.make_ops([hip.op_aux(hip.AUX_BUNDLE_ADJUST_FOCAL if fn is None else fn, ptrs, ints, floats)]))


def test_argument_checks_come_before_any_hip_call():
    """Every new GIMS_EINVAL case of the header, with a message naming bundle_adjust, and what function 14 refuses; no device pointer is
    ever dereferenced.  Every call here is refused.  The group is checked last, so a call refused for its group has passed all the others."""
    group = np.array([0, 0, 1, -1, 7], np.int32)                              # (image 4 is absent: its id is not looked at)
    store = np.zeros(10, np.int64)
    store[:8] = [0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 64, _bits(1e-6), group.ctypes.data]
    mode = np.array([1, 1, 2, 2, 0], np.int32)
    p = [store.ctypes.data, 0x60000, 0x70000, 0x80000, mode.ctypes.data, 0x90000]      # table (host), kpts, xyz, cams, mode (host), out
    good = [100, 400, 5, 900, 10, 0]                                          # T, n_obs, n_images, N, iters, the form word

    def refused(ptrs, ints, word, floats=(0.0, 1e-4)):
        with pytest.raises(hip.GimsHipError, match="bundle_adjust") as e:
            _run(ptrs, ints, floats)
        assert word in str(e.value) and f"({hip.GIMS_EINVAL})" in str(e.value), str(e.value)

    def with_table(**kw):
        tab = store.copy()
        for k, v in kw.items():
            tab[int(k[1:])] = v
        return tab

    # the group: an id outside -1 .. n_images - 1, NULL, misaligned
    for k, bad in ((0, 5), (2, -2), (3, 1 << 20), (1, -(1 << 31))):
        wrong = group.copy()
        wrong[k] = bad
        tab = with_table(w7=wrong.ctypes.data)
        refused([tab.ctypes.data] + p[1:], good, f"image {k}: group = {bad} is out of range")
    tab = with_table(w7=0)
    refused([tab.ctypes.data] + p[1:], good, "group (table word 7) is NULL while n_images = 5")
    tab = with_table(w7=group.ctypes.data + 2)
    refused([tab.ctypes.data] + p[1:], good, "group (table word 7) must be 4-byte aligned")
    # what function 14 refuses, this function refuses: the words of the iteration, the shared checks, the form word (read first)
    for bad in (0, 257):
        tab = with_table(w5=bad)
        refused([tab.ctypes.data] + p[1:], good, f"cg_iters = {bad}")
    tab = with_table(w6=_bits(1.0))
    refused([tab.ctypes.data] + p[1:], good, "cg_tol")
    many = np.full(65538, 2, np.int32)
    many[0] = 1
    refused(p[:4] + [many.ctypes.data, p[5]], [100, 400, 65538, 900, 10, 0], "65537 free cameras")
    refused(p, [-1] + good[1:], "T = -1")
    refused(p, good[:4] + [256, 0], "iters = 256")
    refused(p, good, "huber", floats=(-1.0, 1e-4))
    refused(p, good, "lambda0", floats=(0.0, 0.0))
    refused(p[:5] + [None], good, "output buffer is NULL")
    refused([None] + p[1:], good, "table is NULL")
    refused(p[:4] + [None, p[5]], good, "NULL while n_images = 5")
    wrong = mode.copy()
    wrong[2] = 3
    refused(p[:4] + [wrong.ctypes.data, p[5]], good, "image 2: mode = 3")
    refused(p, good[:5] + [1], "reserved")
    refused([None] * 6, [10, 10, 10, 10, 10, 10], "unknown auxiliary function form")
    # functions 13 and 14 are as they were: word 7 stays reserved there; 12, 15, 99 and -1 are unknown
    with pytest.raises(hip.GimsHipError, match="word 7 is reserved"):
        _run(p, good, fn=hip.AUX_BUNDLE_ADJUST_PCG)
    with pytest.raises(hip.GimsHipError, match="reserved and must be 0"):
        _run(p, good, fn=hip.AUX_BUNDLE_ADJUST)
    for fn in (12, 15, 99, -1):
        with pytest.raises(hip.GimsHipError, match=f"unknown auxiliary function {fn}"):
            _run(p, good, fn=fn)
    # the table and the op
    tab = hip.ba_table(0x10000, 0x20000, None, 0x40000, 0x50000, cg_iters=64, cg_tol=1e-6, group=group)
    assert tab.tolist() == [0x10000, 0x20000, 0, 0x40000, 0x50000, 64, _bits(1e-6), group.ctypes.data]
    assert hip.ba_table(0x10000, 0x20000, None, 0x40000, 0x50000, cg_iters=64, cg_tol=1e-6)[7] == 0
    for bad in (group.astype(np.int64), list(group), group[::2]):
        with pytest.raises(ValueError, match="bundle_adjust: group"):
            hip.ba_table(0x10000, 0x20000, None, 0x40000, 0x50000, group=bad)
    op = hip.op_bundle_adjust_focal(store[:8].copy(), p[1], p[2], p[3], mode, p[5], 100, 400, 900)
    assert op.u.aux.fn == 16 and list(op.u.aux.i) == [100, 400, 5, 900, 20, 0]
    assert hip.ba_focal_groups(mode, group) == 2 and hip.ba_focal_groups(mode, np.full(5, -1)) == 0 and hip.ba_focal_groups(np.zeros(0), np.zeros(0)) == 0
    with pytest.raises(ValueError, match="solver='pcg'"):
        hip.bundle_adjust(*([None] * 8), np.zeros(0, np.int32), group=np.zeros(0, np.int32))


def test_out_layout():
    """Against the restatement of the formula of the header, region by region."""
    al = lambda x: (x + 255) & ~255      # noqa: E731
    order = ["xyz", "cams", "obs_error", "cam_obs", "history", "taken", "counters", "cg_used", "cg_res", "focal_scale", "group_obs"]
    for T, n_obs, n_images, iters, n_free, n_groups in ((0, 0, 0, 0, 0, 0), (0, 0, 3, 5, 1, 1), (0, 0, 65538, 2, 65536, 65536), (0, 0, 65538, 0, 0, 65536), (1, 2, 2, 1, 0, 1),
                                                        (257, 900, 17, 10, 15, 17), (300, 2400, 259, 2, 257, 256), (9462, 40000, 50, 20, 48, 0)):
        o = hip.ba_focal_out_layout(T, n_obs, n_images, iters, n_free, n_groups)
        assert o == F.out_layout(T, n_obs, n_images, iters, n_free, n_groups)
        sizes = [24 * T, 144 * n_images, 4 * n_obs, 4 * n_images, 16 * (iters + 1), iters, 32, 4 * iters, 8 * iters, 8 * n_groups, 4 * n_groups]
        assert o["xyz"] == 0 and all(o[k] % 256 == 0 for k in order) and o["bytes"] % 256 == 0 and o["scratch"] == o["outputs"]
        for a, b, size in zip(order, order[1:] + ["outputs"], sizes):
            assert o[b] - o[a] == al(size), (a, b)                            # back to back: nothing overlaps, nothing is wasted
        pcg = hip.ba_pcg_out_layout(T, n_obs, n_images, iters, n_free)
        assert all(o[k] == pcg[k] for k in order[:9]) and o["focal_scale"] == pcg["outputs"]      # function 14's regions lie at function 14's offsets
        if n_groups == 0:
            assert o["outputs"] == pcg["outputs"]
    # linear in n_groups
    big, small = (hip.ba_focal_out_layout(0, 0, 0, 0, 0, g)["bytes"] for g in (65536, 32768))
    assert abs(big - 2 * small) <= 16 * 256 and big < 8 << 20


# ------------------------------------------------------------------------------------------------ the Python layer
def test_value_errors_before_the_device_is_touched():
    tr, pts = _host_tracks(), _Points(1, 2)
    images = [torch.zeros(3, 2), torch.zeros(2, 2)]
    K = np.tile(np.diag([500.0, 500.0, 1.0]), (2, 1, 1))
    Rm, t = np.tile(np.eye(3), (2, 1, 1)), np.zeros((2, 3))

    def refused(word, cameras=(K, Rm, t), **kw):
        with pytest.raises(ValueError, match="bundle_adjust") as e:
            gims_amd.bundle_adjust(pts, tr, images, cameras, **kw)
        assert word in str(e.value), str(e.value)

    refused("solver='pcg'", refine_focal="shared")                              # the default solver is 'dense': the message points to the way out
    refused("solver='pcg'", refine_focal=[0, 0], solver="dense")
    refused("refine_focal must be", refine_focal="all", solver="pcg")
    refused("refine_focal must be", refine_focal=3, solver="pcg")
    refused("3 group ids for 2 images", refine_focal=[0, 0, 0], solver="pcg")  # a wrong length
    for bad in (0.0, "0", None, True, 1.5):
        refused("a group id must be an integer", refine_focal=[0, bad], solver="pcg")
    refused("refine_focal[1] = -2", refine_focal=[0, -2], solver="pcg")         # an id below -1
    K2 = K.copy()
    K2[1, 1, 1] = 480.0
    refused("one scale cannot serve them", cameras=(K2, Rm, t), refine_focal="shared", solver="pcg")
    refused("one scale cannot serve them", cameras=(K2, Rm, t), refine_focal=[4, 4], solver="pcg")
    # everything is right: the tracks are host tensors, which is the last thing checked
    for ok in ("shared", "per_image", [0, 0], [-1, 5], np.array([3, -1]), (7, 7)):
        refused("on the GPU", refine_focal=ok, solver="pcg")
    refused("on the GPU", cameras=(K2, Rm, t), refine_focal="per_image", solver="pcg")      # different ratios in different groups are fine
    refused("on the GPU", cameras=(K2, Rm, t), refine_focal=[0, -1], solver="pcg")
    # the dense ids
    from gims_amd.bundle import _focal_groups
    posed = np.array([True, False, True, True])
    K4 = np.tile(K[:1], (4, 1, 1))
    assert _focal_groups("x", "shared", "pcg", posed, K4).tolist() == [0, -1, 0, 0]
    assert _focal_groups("x", "per_image", "pcg", posed, K4).tolist() == [0, -1, 1, 2]
    assert _focal_groups("x", [9, 9, -1, 4], "pcg", posed, K4).tolist() == [0, -1, -1, 1]      # an absent image's id is dropped, the others made dense
    assert _focal_groups("x", None, "dense", posed, K4) is None


# ------------------------------------------------------------------------------------------------ the restatement on its own
def test_without_a_group_the_restatement_is_function_14s():
    for name, huber in (("c5", 0.0), ("c17", 1.5), ("poison", 0.0), ("two", 0.0), ("T0", 0.0)):
        sc = pcg_scene(name)
        a, b = P.run(sc, iters=6, huber=huber), F.run(sc, np.full(len(sc["mode"]), -1), iters=6, huber=huber)
        for k in ("xyz", "cams", "history", "taken", "cg_used", "cg_res", "obs_error", "cam_obs"):
            assert np.array_equal(a[k], b[k], equal_nan=True), (name, k)
        assert a["stats"] == b["stats"] and b["focal_scale"].shape == (0,)
    # a held group changes nothing either
    sc, group = fixture("few")
    a, b = P.run(sc, iters=6), F.run(sc, group, iters=6)
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("xyz", "cams", "history", "taken", "cg_used", "cg_res", "obs_error"))
    assert b["focal_scale"].tolist() == [1.0] and b["group_obs"].tolist() == [3]


def test_focal_jacobian_equals_central_differences():
    worst = 0.0
    for name, huber in (("shared5", 0.0), ("per5", 0.0), ("absent", 0.0)):
        (sc, group), rounds = fixture(name), []
        F.run(sc, group, iters=1, huber=huber, cg_iters=1, rounds_out=rounds)
        rd = rounds[0]
        h = 1e-6
        for g in np.flatnonzero(~rd["gheld"]):
            mine = np.flatnonzero(rd["ogrp"] == g)
            imgs = np.flatnonzero(np.where(sc["mode"] != 0, group, -1) == g)

            def f(ds):
                C = rd["C"].copy()
                C[imgs, 0], C[imgs, 1] = C[imgs, 0] * (1 + ds), C[imgs, 1] * (1 + ds)
                ru, rv, _ = B.observe(C, rd["X"][rd["ot"]], rd["ok"], rd["uv"], jac=False)
                return np.stack([ru, rv], axis=1)

            num, ana = (f(h) - f(-h)) / (2 * h), np.stack([rd["Fu"], rd["Fv"]], axis=1)
            worst = max(worst, np.abs(num[mine] - ana[mine]).max() / np.abs(ana[mine]).max())
            other = np.setdiff1d(np.arange(len(ana)), mine)
            assert len(mine) and (len(other) == 0 or np.abs(num[other]).max() == 0)
    print(f"Fu, Fv against central differences in s: {worst:.3g} relative")
    assert worst < 1e-6


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _dense_reduced(rd, T):
    """The Schur complement over the points of the full damped normal equations, group columns included -> (S, b, M_g), the unknowns
    [6 per slot | 1 per group]; M_g = A* - sum_o G_o V*^-1 G_o^T by dense inverses."""
    n_slots, n_groups = len(rd["held"]), len(rd["gheld"])
    nc = 6 * n_slots + n_groups
    J, r = np.zeros((2 * len(rd["ot"]), nc + 3 * T)), np.zeros(2 * len(rd["ot"]))
    for j in range(len(rd["ot"])):
        if rd["oslot"][j] >= 0:
            J[2 * j, 6 * rd["oslot"][j]:6 * rd["oslot"][j] + 6], J[2 * j + 1, 6 * rd["oslot"][j]:6 * rd["oslot"][j] + 6] = rd["Ju"][j], rd["Jv"][j]
        if rd["ogrp"][j] >= 0:
            J[2 * j, 6 * n_slots + rd["ogrp"][j]], J[2 * j + 1, 6 * n_slots + rd["ogrp"][j]] = rd["Fu"][j], rd["Fv"][j]
        J[2 * j, nc + 3 * rd["ot"][j]:nc + 3 * rd["ot"][j] + 3], J[2 * j + 1, nc + 3 * rd["ot"][j]:nc + 3 * rd["ot"][j] + 3] = rd["Pu"][j], rd["Pv"][j]
        r[2 * j], r[2 * j + 1] = rd["ru"][j], rd["rv"][j]
    H, g = J.T @ J, J.T @ r
    still = np.concatenate([np.repeat(rd["held"], 6), rd["gheld"]])          # held: an identity entry, a zero right-hand side
    used = np.flatnonzero(np.diag(H)[nc:] > 0) + nc
    H = H + rd["lam"] * np.diag(np.maximum(np.diag(H), 1e-6))
    Hpp_inv = np.linalg.inv(H[np.ix_(used, used)])
    S = H[:nc, :nc] - H[:nc, used] @ Hpp_inv @ H[used, :nc]
    b = -g[:nc] + H[:nc, used] @ Hpp_inv @ g[used]
    S[still], S[:, still], b[still] = 0.0, 0.0, 0.0
    S[still, still] = 1.0
    Mg = np.ones(n_groups)
    for gi in np.flatnonzero(~rd["gheld"]):
        mine = np.flatnonzero(rd["ogrp"] == gi)
        Mg[gi] = H[6 * n_slots + gi, 6 * n_slots + gi]
        for j in mine:
            Gj = rd["Fu"][j] * rd["Pu"][j] + rd["Fv"][j] * rd["Pv"][j]
            t = rd["ot"][j]
            Mg[gi] -= Gj @ np.linalg.inv(H[nc + 3 * t:nc + 3 * t + 3, nc + 3 * t:nc + 3 * t + 3]) @ Gj
    return S, b, Mg


def test_the_matrix_free_system_equals_the_dense_one():
    worst = dict(sv=0.0, b=0.0, mg=0.0)
    rng = np.random.default_rng(4)
    for name, huber in (("shared5", 0.0), ("shared5", 1.5), ("two5", 0.0), ("per5", 0.0), ("fixed5", 0.0), ("absent", 0.0), ("nfree0", 0.0), ("per17", 0.0)):
        (sc, group), rounds = fixture(name), []
        F.run(sc, group, iters=1, huber=huber, cg_iters=1, rounds_out=rounds)
        rd = rounds[0]
        n_slots, n_groups = len(rd["held"]), len(rd["gheld"])
        S, b, Mg = _dense_reduced(rd, len(sc["xyz"]))
        worst["b"] = max(worst["b"], _rel(np.concatenate([rd["b"].reshape(-1), rd["bg"]]), b))
        worst["mg"] = max(worst["mg"], _rel(rd["Mg"], Mg))
        assert (rd["Mg"] > 0).all()
        for _ in range(3):
            vs, vg = rng.standard_normal((n_slots, 6)), rng.standard_normal(n_groups)
            vs[rd["held"]], vg[rd["gheld"]] = 0.0, 0.0
            qs, qg = rd["Sp"](vs, vg)
            want = S @ np.concatenate([vs.reshape(-1), vg])
            worst["sv"] = max(worst["sv"], _rel(np.concatenate([qs.reshape(-1), qg]), want))
    print({k: f"{v:.4g}" for k, v in worst.items()}, "bars", SV_BAR, B_BAR, MG_BAR)
    for k, bar in (("sv", SV_BAR), ("b", B_BAR), ("mg", MG_BAR)):
        assert 0.8 * bar <= 16 * worst[k] <= bar, (k, worst[k], bar)


RECOVERY = [(5, 64, "shared"), (17, 257, "shared"), (5, 64, "per_image"), (17, 257, "per_image")]


def test_recovery_and_tol_focal():
    """The planted focal comes back to within TOL_FOCAL, function 14 with the wrong K cannot follow, and TOL_FOCAL is 16 x the measured spread."""
    spread, worst = 0.0, 0.0
    for n_cams, T, kind in RECOVERY:
        factors = np.full(n_cams, 1.05) if kind == "shared" else per_image_factors(n_cams)
        sc = wrong_focal(noise_free(n_cams, T), factors)
        group = np.zeros(n_cams, np.int32) if kind == "shared" else np.arange(n_cams, dtype=np.int32)
        fwd, rev = (F.run(sc, group, iters=30, order=order) for order in ("forward", "reverse"))
        assert fwd["stats"] == rev["stats"] and (fwd["taken"] == rev["taken"]).all() and (fwd["cg_used"] == rev["cg_used"]).all() and fwd["stats"]["status"] == 0
        s = focal_difference(fwd, rev, sc)
        got = float(np.abs(fwd["focal_scale"] * (factors[0] if kind == "shared" else factors) - 1.0).max())
        fixed_k = P.run(sc, iters=30)
        ratio = fixed_k["history"][-1, 0] / fwd["history"][-1, 0]
        print(f"{n_cams} cameras, {kind}: focal_scale x planted - 1 = {got:.3g}; spread {s:.3g}; cost {fwd['history'][0, 0]:.4g} -> {fwd['history'][-1, 0]:.3g}, "
              f"function 14 with the wrong K ends at {fixed_k['history'][-1, 0]:.4g} ({ratio:.3g} x); rounds taken {fwd['stats']['rounds_taken']}, cg_used {fwd['cg_used'].max()}")
        assert ratio >= 10.0
        assert np.abs(fwd["cams"][:, :2] - sc["cams"][:, :2] * fwd["focal_scale"][group][:, None]).max() <= 1e-9 * 700      # fx, fy moved by the scale
        assert (fwd["cams"][:, 2:4] == sc["cams"][:, 2:4]).all() and fwd["group_obs"].sum() == (fwd["stats"]["n_active_obs"] if kind == "shared" else fwd["cam_obs"].sum())
        spread, worst = max(spread, s), max(worst, got)
    print(f"SPREAD_FOCAL = {spread:.4g}, 16 x SPREAD_FOCAL = {16 * spread:.4g}, TOL_FOCAL = {TOL_FOCAL:.4g}; worst distance to the planted ratio {worst:.4g}")
    assert 0.8 * TOL_FOCAL <= 16 * spread <= TOL_FOCAL
    assert worst <= TOL_FOCAL


def test_edge_cases_of_the_restatement():
    few = reference("few", 10, 0.0, 1e-4, 128, 1e-6)
    assert few["focal_scale"].tolist() == [1.0] and few["group_obs"].tolist() == [3]
    ab = reference("absent", 10, 0.0, 1e-4, 128, 1e-6)
    sc, _ = fixture("absent")
    assert ab["group_obs"][0] == 0 and ab["focal_scale"][0] == 1.0 and ab["group_obs"][1] == ab["stats"]["n_active_obs"] and abs(ab["focal_scale"][1] * 1.04 - 1) < 1e-2
    assert ab["cams"][6, 0] != sc["cams"][6, 0] and (ab["cams"][6, 2:] == sc["cams"][6, 2:]).all()      # the held camera's lens moves with its group, its pose stays
    assert np.array_equal(ab["cams"][5], sc["cams"][5], equal_nan=True)
    nf = reference("nfree0", 10, 0.0, 1e-4, 128, 1e-6)
    assert nf["stats"]["n_free"] == 0 and nf["stats"]["rounds_taken"] >= 2 and (nf["cg_used"][nf["taken"] == 1] == 1).all() and abs(nf["focal_scale"][0] * 1.05 - 1) < 0.02
    fx = reference("fixed5", 10, 0.0, 1e-4, 128, 1e-6)
    sc5, _ = fixture("fixed5")
    assert (fx["cams"][2:, :4] == sc5["cams"][2:, :4]).all() and (fx["cams"][:2, 4:] == sc5["cams"][:2, 4:]).all() and abs(fx["focal_scale"][0] * 1.05 - 1) < 3e-2
    rt = reference("rejtake", 14, 0.0, 1e-4, 128, 1e-6)["taken"].tolist()
    assert any(a == 0 and b == 1 for a, b in zip(rt, rt[1:])), rt               # a refused round followed by a taken one
    mi = reference("mirror", 10, 0.0, 1e-4, 128, 1e-6)
    first = int(np.argmax(mi["taken"]))
    assert first >= 1 and (1.0 + mi["ds"][:first, 0] <= 0).all() and 1.0 + mi["ds"][first, 0] > 0, (mi["taken"], mi["ds"][:, 0])      # refused for 1 + ds <= 0, then taken
    idle = reference("mirror", 8, 0.0, 1e-6, 128, 1e-6)
    assert idle["taken"].sum() == 0 and (1.0 + idle["ds"][:5, 0] <= 0).all() and (idle["cg_used"][:5] > 0).all() and (idle["cg_used"][5:] == 0).all()      # five refusals, then idle
    assert idle["focal_scale"].tolist() == [1.0]
    for name, bit in (("badcam", B.BAD_CAMERA), ("behind", B.BAD_START)):
        out = reference(name, 10, 0.0, 1e-4, 128, 1e-6)
        assert out["stats"]["status"] == bit and (out["focal_scale"] == 1).all() and (out["cg_used"] == 0).all()
    for n in (3, 5, 17):
        out = reference(f"per{n}", 10, 0.0, 1e-4, 128, 1e-6)
        assert len(out["focal_scale"]) == n and (out["focal_scale"] != 1).all() and out["stats"]["rounds_taken"] >= 3 and out["history"][-1, 0] < 0.1 * out["history"][0, 0]
    capped = reference("shared5", 10, 0.0, 1e-4, 1, 1e-6)
    assert set(capped["cg_used"].tolist()) <= {0, 1} and capped["cg_used"][0] == 1 and capped["cg_res"][0] > 1e-6      # the cap is hit
    assert reference("shared5", 0, 0.0, 1e-4, 128, 1e-6)["focal_scale"].tolist() == [1.0]
    for n in (255, 256, 257):
        assert len(reference(f"d{n}", 2, 0.0, 1e-4, 128, 1e-6)["focal_scale"]) == n
    for n in (63, 64, 65):
        assert reference(f"L{n}", 3, 0.0, 1e-4, 128, 1e-6)["cam_obs"].tolist() == [n] * 4


@pytest.mark.parametrize("name,iters,huber,lambda0,cg_iters,cg_tol", CASES)
def test_fixture_margins(name, iters, huber, lambda0, cg_iters, cg_tol):
    """What makes an exact comparison of taken, cg_used, the counters and cam_obs with the device fair: no decision of the restatement is close."""
    mg = reference(name, iters, huber, lambda0, cg_iters, cg_tol)["margins"]
    print(name, iters, huber, lambda0, cg_iters, cg_tol, {k: f"{v:.3g}" for k, v in mg.items()})
    assert mg["lead"] > LEAD and mg["depth"] > DEPTH and mg["det"] > PIVOT, mg
    assert mg["cg_stop"] > CG_STOP and mg["pq"] > PQ and mg["m_pivot"] > M_PIVOT, mg
    assert mg["mg_pivot"] > MG_PIVOT and mg["f1"] > F1, mg
