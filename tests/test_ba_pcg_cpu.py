"""CPU tests of the conjugate-gradient form of bundle adjustment: the ABI constant and the pins it must leave alone, the
argument checks of GIMS_AUX_BUNDLE_ADJUST_PCG (they run before any HIP call), the layout of its buffer, the new ValueErrors of
gims_amd.bundle_adjust, the NumPy restatement (tests/ba_pcg_ref.py) checked on its own and against the dense restatement
(tests/ba_ref.py), and the conditions on the fixtures that tests/test_ba_pcg_gpu.py compares with the device.

The restatement on its own.  On the round records of ba_ref.adjust(rounds_out=...), whose S and b are formed densely, the matrix-free
product S p, the right-hand side b and -- on scenes where no image sees a track twice -- the preconditioner blocks M against the diagonal
blocks of S differ, relative to the largest entry of what is compared, by at most
  S p  1.8e-15      b  6.7e-16      M  5.7e-16
as measured here (the two restatements take the same sums in other orders); SP_BAR, B_BAR and M_BAR are 16 x these.

TOL_PCG_VS_DENSE.  With cg_tol = 1e-12 and cg_iters = 128 the iteration is run to the end; on the fixtures of DENSE_CASES `taken` equals the
dense restatement's, and the largest difference of a word of the final xyz, R, t or of a cost of the history, divided by max(1, |word|),
is VS_DENSE = 1.5e-14 (on 'c17' with huber = 1.5; 5.1e-15 and below without).  TOL_PCG_VS_DENSE = 16 x that = 2.4e-13.

TOL_PCG.  Every fixture of CASES is solved forward and in reverse (tests/ba_pcg_ref.py says what is reversed); the largest such difference
is SPREAD_PCG = 6.2e-14 (on 'rejtake', a start far from the minimum; 1.2e-14 and below on the others), TOL_PCG = 16 x SPREAD_PCG = 1.0e-12.
The numbers recorded below are asserted to be the measured ones.

Margins (test_fixture_margins).  LEAD, DEPTH and PIVOT (the det of a point) are those of tests/test_ba_cpu.py.  CG_STOP = 1e-6: every stop
comparison rho' <= cg_tol^2 rho_0 is that far (relative to the larger side) from equality, so cg_used can be compared exactly; PQ = 1e-9:
every p . q relative to the sum of the magnitudes of its products; M_PIVOT = 1e-9: every pivot of every M_s relative to its diagonal entry;
cg_used is the same in the two orders.  A fixture that failed a margin got another seed or another iteration cap, not another margin."""
import functools

import numpy as np
import pytest
import torch

import gims_amd
from gims_amd import hip
from tests import ba_pcg_ref as P
from tests import ba_ref as B
from tests.test_ba_cpu import DEPTH, LEAD, PIVOT, _Points, relative_difference
from tests.test_ba_cpu import scene as dense_scene
from tests.test_resect_cpu import _host_tracks

SP_BAR, B_BAR, M_BAR = 3.0e-14, 1.1e-14, 9.3e-15               # 16 x the measured differences; test_the_matrix_free_system_equals_the_dense_one keeps them honest
TOL_PCG_VS_DENSE = 2.4e-13                                    # 16 x VS_DENSE, rounded up to two digits
TOL_PCG = 1.0e-12                                             # 16 x SPREAD_PCG, rounded up to two digits
TOL_CG_RES = 4.5e-11                                             # 16 x the same spread of cg_res (a ratio, at most about 1: the absolute difference)
CG_STOP, PQ, M_PIVOT = 1e-6, 1e-9, 1e-9
FREE_SEEDS = {63: 200, 64: 200, 65: 200, 129: 200, 257: 208}            # 300 tracks of 8 observations: the first seed from 200 that leaves no free camera held


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "f1":                                                          # one free camera between two fixed ones
        return B.planted_scene(41, [3] * 300, 3, noise=0.5, fixed=(0, 2), pert_cam=0.005, pert_pt=0.005)
    if name == "f128":
        return dense_scene("cap")
    if name.startswith("f"):                                                  # n free and 2 fixed images, 300 points of 8 observations, no camera held
        n = int(name[1:])
        return B.planted_scene(FREE_SEEDS[n], [8] * 300, n + 2, noise=0.5, fixed=(0, n + 1), pert_cam=0.005, pert_pt=0.005)
    if name.startswith("L"):                                                  # four images, every track seen by all four: lists of exactly n observations
        return B.planted_scene(60 + int(name[1:]), [4] * int(name[1:]), 4, noise=0.5, pert_cam=0.01, pert_pt=0.01)
    return dense_scene(name)


# every fixture the GPU test compares with the restatement: (scene, iters, huber, lambda0, cg_iters, cg_tol)
CASES = ([(f"f{n}", 2, 0.0, 1e-4, 128, 1e-6) for n in (1, 63, 64, 65, 128, 129, 257)] + [("f129", 2, 0.0, 1e-4, 64, 1e-6)]
         + [(f"L{n}", 3, 0.0, 1e-4, 128, 1e-6) for n in (63, 64, 65, 129)]
         + [("c17", 10, 0.0, 1e-4, 128, 1e-6), ("c17", 10, 1.5, 1e-4, 128, 1e-6), ("c17", 10, 0.0, 1e-4, 1, 1e-6), ("c17", 10, 0.0, 1e-4, 2, 0.0), ("c17", 10, 0.0, 1e-4, 24, 0.0),
            ("c5", 0, 0.0, 1e-4, 128, 1e-6), ("c5", 1, 0.0, 1e-4, 128, 1e-6), ("c5", 10, 0.0, 1e-4, 128, 1e-6), ("c5", 10, 1.5, 1e-4, 2, 0.0), ("c3", 10, 0.0, 1e-4, 128, 1e-6),
            ("two", 10, 0.0, 1e-4, 128, 1e-6)]
         + [(f"T{T}", 10, 0.0, 1e-4, 128, 1e-6) for T in (0, 1, 257)]
         + [("poison", 10, 0.0, 1e-4, 128, 1e-6), ("poison", 10, 1.5, 1e-4, 128, 1e-6), ("badcam", 10, 0.0, 1e-4, 128, 1e-6), ("behind", 10, 0.0, 1e-4, 128, 1e-6),
            ("atmin", 8, 0.0, 1e-4, 128, 1e-6), ("rejtake", 14, 0.0, 1e-4, 128, 1e-6)])
# the fixtures on which the two forms are compared: run to the end
DENSE_CASES = [(name, iters, huber, 1e-4, 128, 1e-12) for name, iters, huber in (("c3", 10, 0.0), ("c5", 10, 0.0), ("c5", 10, 1.5), ("c17", 10, 0.0), ("c17", 10, 1.5),
                                                                                  ("poison", 10, 0.0), ("f128", 2, 0.0))]


@functools.lru_cache(maxsize=None)
def reference(name, iters, huber, lambda0, cg_iters, cg_tol, order="forward"):
    """The restatement on a fixture, computed once and shared (do not write to it)."""
    return P.run(scene(name), iters=iters, huber=huber, lambda0=lambda0, cg_iters=cg_iters, cg_tol=cg_tol, order=order)


@functools.lru_cache(maxsize=None)
def dense_reference(name, iters, huber, lambda0):
    return B.run(scene(name), iters=iters, huber=huber, lambda0=lambda0)


# ------------------------------------------------------------------------------------------------ pins, argument checks, layout
def test_abi_constant_and_pins():
    assert hip.AUX_BUNDLE_ADJUST_PCG == 14 == hip.ABI.constants["GIMS_AUX_BUNDLE_ADJUST_PCG"] and hip.AUX_BUNDLE_ADJUST == 13
    assert 12 not in [v for k, v in hip.ABI.constants.items() if k.startswith("GIMS_AUX_")]
    # the feature adds a constant and a table entry: no export, no struct and no ABI version
    assert len(hip.EXPORTS) == 90 and len(hip.ABI.structs) == 28 and hip.ABI_VERSION == 5 == hip.load().gims_abi_version()
    assert not any("bundle" in name.lower() or "ba_" in name.lower() or "pcg" in name.lower() for name in hip.EXPORTS)
    assert hip.BA_PCG_MAX_FREE_CAMERAS == 65536 == P.MAX_FREE and hip.BA_PCG_MAX_CG_ITERS == 256 == P.MAX_CG_ITERS and hip.BA_MAX_FREE_CAMERAS == 128
    assert hip.BA_TABLE_WORDS == 8


def _run(ptrs, ints, floats=(0.0, 1e-4), fn=None):
    """Through hip.run_ops, on the null stream (no device is needed: a refused call makes no HIP call)."""
    with hip.on_stream(0):
        hip.run_ops(hip.make_ops([hip.op_aux(hip.AUX_BUNDLE_ADJUST_PCG if fn is None else fn, ptrs, ints, floats)]))


def _bits(x):
    return int(np.array([x], np.float64).view(np.int64)[0])


def test_argument_checks_come_before_any_hip_call():
    """Every GIMS_EINVAL case of the header, with a message naming bundle_adjust; no device pointer is ever dereferenced.  Every call
    here is refused: the words of this form are checked behind the checks the two forms share, so a call with cg_iters = 0 that is refused
    for its cg_iters has passed all the others, the count of the free cameras among them."""
    store = np.zeros(10, np.int64)                                            # the table, with room to misalign it
    store[:7] = [0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 64, _bits(1e-6)]
    mode = np.array([1, 1, 2, 2, 0], np.int32)
    p = [store.ctypes.data, 0x60000, 0x70000, 0x80000, mode.ctypes.data, 0x90000]      # table (host), kpts, xyz, cams, mode (host), out
    good = [100, 400, 5, 900, 10, 0]                                          # T, n_obs, n_images, N, iters, the form word

    def refused(ptrs, ints, word, floats=(0.0, 1e-4)):
        with pytest.raises(hip.GimsHipError, match="bundle_adjust") as e:
            _run(ptrs, ints, floats)
        assert word in str(e.value) and f"({hip.GIMS_EINVAL})" in str(e.value), str(e.value)

    def ints(**kw):
        return [kw.get(k, v) for k, v in zip(["T", "n_obs", "n_images", "N", "iters", "form"], good)]

    def with_table(**kw):
        tab = store.copy()
        for k, v in kw.items():
            tab[int(k[1:])] = v
        return tab

    # the words of this form (every other argument is good: these calls got as far as the last checks)
    for bad in (0, 257, -1):
        tab = with_table(w5=bad)
        refused([tab.ctypes.data] + p[1:], good, f"cg_iters = {bad}")
    for bad in (-1.0, 1.0, float("nan"), float("inf"), 1.5):
        tab = with_table(w6=_bits(bad))
        refused([tab.ctypes.data] + p[1:], good, "cg_tol")
    tab = with_table(w7=1)
    refused([tab.ctypes.data] + p[1:], good, "word 7 is reserved")
    # the count of the free cameras: 65537 are refused; 129 and 65536 pass it and are refused for the cg_iters = 0 behind it
    zero_iters = with_table(w5=0)
    for n_free, word in ((129, "cg_iters = 0"), (65536, "cg_iters = 0"), (65537, "65537 free cameras")):
        many = np.full(n_free + 1, 2, np.int32)
        many[0] = 1
        refused([zero_iters.ctypes.data] + p[1:4] + [many.ctypes.data, p[5]], ints(n_images=n_free + 1), word)
    # what the dense form refuses, this form refuses
    for name in ("T", "n_obs", "N"):
        refused(p, ints(**{name: -1}), f"{name} = -1")
        refused(p, ints(**{name: (1 << 30) + 1}), "2^30")
    refused(p, ints(n_images=-1), "n_images = -1")
    refused(p, ints(n_images=(1 << 24) + 1), "2^24")
    for bad in (-1, 256):
        refused(p, ints(iters=bad), f"iters = {bad}")
    for bad in (-1.0, float("nan"), float("inf")):
        refused(p, good, "huber", floats=(bad, 1e-4))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused(p, good, "lambda0", floats=(0.0, bad))
    refused(p[:5] + [None], good, "output buffer is NULL")
    refused(p[:5] + [None], ints(T=0), "output buffer is NULL")
    refused([None] + p[1:], good, "table is NULL")
    refused(p[:5] + [p[5] + 8], good, "16-byte aligned")
    refused([p[0] + 4] + p[1:], good, "8-byte aligned")
    for k in (2, 3):
        refused(p[:k] + [p[k] + 4] + p[k + 1:], good, "8-byte aligned")
    for k in (1, 4):
        refused(p[:k] + [p[k] + 2] + p[k + 1:], good, "4-byte aligned")
    for k in (0, 1, 2):
        tab = with_table(**{f"w{k}": store[k] + 2})
        refused([tab.ctypes.data] + p[1:], good, "4-byte aligned")
    for k in range(5):
        tab = with_table(**{f"w{k}": 0})
        refused([tab.ctypes.data] + p[1:], good, "NULL while T = 100")
    for k in (1, 2):
        refused(p[:k] + [None] + p[k + 1:], good, "NULL while T = 100")
    for k in (3, 4):
        refused(p[:k] + [None] + p[k + 1:], good, "NULL while n_images = 5")
    for bad in (3, -1):
        wrong = mode.copy()
        wrong[2] = bad
        refused(p[:4] + [wrong.ctypes.data, p[5]], good, f"image 2: mode = {bad}")
    refused(p, ints(form=1), "reserved")
    refused([None] * 6, [10, 10, 10, 10, 10, 10], "unknown auxiliary function form")
    refused([None] * 6, [-5, -5, -5, -5, -5, 7], "unknown auxiliary function form", floats=(float("nan"), float("nan")))
    # the dense form is as it was: its three words stay reserved, its cap stays 128; 12 and 15 are unknown
    with pytest.raises(hip.GimsHipError, match="reserved and must be 0"):
        _run(p, good, fn=hip.AUX_BUNDLE_ADJUST)
    many = np.full(130, 2, np.int32)
    many[0] = 1
    with pytest.raises(hip.GimsHipError, match="129 free cameras, at most GIMS_BA_MAX_FREE_CAMERAS = 128"):
        _run([with_table(w5=0, w6=0).ctypes.data] + p[1:4] + [many.ctypes.data, p[5]], ints(n_images=130), fn=hip.AUX_BUNDLE_ADJUST)
    for fn in (12, 15, 99, -1):
        with pytest.raises(hip.GimsHipError, match=f"unknown auxiliary function {fn}"):
            _run(p, good, fn=fn)
    # the table
    tab = hip.ba_table(0x10000, 0x20000, None, 0x40000, 0x50000)
    assert tab.dtype == np.int64 and tab.tolist() == [0x10000, 0x20000, 0, 0x40000, 0x50000, 0, 0, 0]      # the defaults keep the dense table
    tab = hip.ba_table(0x10000, 0x20000, None, 0x40000, 0x50000, cg_iters=64, cg_tol=1e-6)
    assert tab.tolist() == [0x10000, 0x20000, 0, 0x40000, 0x50000, 64, _bits(1e-6), 0] and tab[6:7].view(np.float64)[0] == 1e-6
    op = hip.op_bundle_adjust_pcg(store[:8].copy(), p[1], p[2], p[3], mode, p[5], 100, 400, 900)
    assert op.u.aux.fn == 14 and list(op.u.aux.i) == [100, 400, 5, 900, 20, 0]
    with pytest.raises(ValueError, match="bundle_adjust: table"):
        hip.op_bundle_adjust_pcg(store[:5], p[1], p[2], p[3], mode, p[5], 100, 400, 900)
    with pytest.raises(ValueError, match="bundle_adjust: mode"):
        hip.op_bundle_adjust_pcg(store[:8].copy(), p[1], p[2], p[3], list(mode), p[5], 100, 400, 900)


def test_out_layout():
    """Against a restatement of the formula of the header, region by region."""
    al = lambda x: (x + 255) & ~255      # noqa: E731
    order = ["xyz", "cams", "obs_error", "cam_obs", "history", "taken", "counters", "cg_used", "cg_res"]
    for T, n_obs, n_images, iters, n_free in ((0, 0, 0, 0, 0), (0, 0, 3, 5, 1), (1, 2, 2, 1, 0), (257, 900, 17, 10, 15), (300, 2400, 131, 2, 129), (9462, 40000, 50, 20, 48),
                                              (70000, 600000, 65538, 255, 65536)):
        o = hip.ba_pcg_out_layout(T, n_obs, n_images, iters, n_free)
        assert o == P.out_layout(T, n_obs, n_images, iters, n_free)
        sizes = [24 * T, 144 * n_images, 4 * n_obs, 4 * n_images, 16 * (iters + 1), iters, 32, 4 * iters, 8 * iters]
        assert o["xyz"] == 0 and all(o[k] % 256 == 0 for k in order) and o["bytes"] % 256 == 0
        for a, b, size in zip(order, order[1:] + ["outputs"], sizes):
            assert o[b] - o[a] == al(size), (a, b)                            # back to back: nothing overlaps, nothing is wasted
        dense = hip.ba_out_layout(T, n_obs, n_images, iters, min(n_free, 128))
        assert all(o[k] == dense[k] for k in order[:7]) and o["cg_used"] == dense["outputs"]      # the seven regions lie where the dense form has them
        assert o["scratch"] == o["outputs"] and o["bytes"] - o["scratch"] == (
            256 + al(4 * n_images) + 3 * al(4 * n_free) + al(4 * n_free + 4) + al(24 * T) + al(144 * n_images) + al(T) + al(n_obs) + 4 * al(4 * n_obs) + al(72 * T)
            + al(400 * n_obs) + al(8 * T) + al(24 * T) + al(336 * n_free) + 5 * al(48 * n_free))
    # linear: no n x n region (the dense form at 65536 cameras would need 1.2 TB)
    o = hip.ba_pcg_out_layout(0, 0, 65538, 0, 65536)
    assert o["bytes"] < 64 << 20
    big, small = hip.ba_pcg_out_layout(0, 0, 0, 0, 65536)["bytes"], hip.ba_pcg_out_layout(0, 0, 0, 0, 32768)["bytes"]
    assert abs(big - 2 * small) <= 16 * 256


# ------------------------------------------------------------------------------------------------ the Python layer
def test_value_errors_before_the_device_is_touched():
    tr, pts = _host_tracks(), _Points(1, 2)
    images = [torch.zeros(3, 2), torch.zeros(2, 2)]
    K = np.tile(np.diag([500.0, 500.0, 1.0]), (2, 1, 1))
    Rm, t = np.tile(np.eye(3), (2, 1, 1)), np.zeros((2, 3))

    def refused(word, tracks=tr, images=images, cameras=(K, Rm, t), **kw):
        with pytest.raises(ValueError, match="bundle_adjust") as e:
            gims_amd.bundle_adjust(pts, tracks, images, cameras, **kw)
        assert word in str(e.value), str(e.value)

    for solver in ("cg", "PCG", None, 14):
        refused("solver must be", solver=solver)
    for solver in ("dense", "pcg"):                                              # the two are checked whichever solver is named
        for kw in (dict(cg_iters=0), dict(cg_iters=257), dict(cg_iters=1.5), dict(cg_iters=True), dict(cg_tol=-1.0), dict(cg_tol=1.0), dict(cg_tol=float("nan")),
                   dict(cg_tol="1e-6"), dict(cg_tol=True)):
            refused(next(iter(kw)), solver=solver, **kw)
        refused("on the GPU", solver=solver, cg_iters=1, cg_tol=0.0)            # everything is right: the tracks are host tensors
        refused("iters must be", solver=solver, iters=256)
    # 131 posed images, two fixed by default: 129 free cameras are refused by the dense form and pass the count of 'pcg'
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)      # noqa: E731

    def many(n):
        big = gims_amd.Tracks(torch.zeros(n, dtype=torch.int32), i32(0, 2), i32(0, 1), i32(0, 0), torch.zeros(1, dtype=torch.uint8),
                              dict(n_tracks=1, n_obs=2, n_conflicting=0, n_edges=1, n_bad=0, status=0), list(range(0, n + 1)))
        return dict(tracks=big, images=[torch.zeros(1, 2)] * n, cameras=(np.tile(K[:1], (n, 1, 1)), np.tile(Rm[:1], (n, 1, 1)), np.zeros((n, 3))))

    refused("129 free cameras, at most 128", **many(131))
    refused("solver='pcg'", **many(131))                                         # the message points to the way out
    refused("on the GPU", solver="pcg", **many(131))
    with pytest.raises(ValueError, match="solver must be"):
        hip.bundle_adjust(*([None] * 8), np.zeros(0, np.int32), solver="cg")


# ------------------------------------------------------------------------------------------------ the restatement on its own
def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def test_the_matrix_free_system_equals_the_dense_one():
    """S p, b and M of ba_pcg_ref against the S and b that ba_ref forms densely, at the first round of five fixtures."""
    worst = dict(sp=0.0, b=0.0, m=0.0)
    rng = np.random.default_rng(3)
    for name, huber, no_repeats in (("c5", 0.0, True), ("c5", 1.5, True), ("poison", 0.0, False), ("c17", 0.0, False), ("f128", 0.0, True)):
        sc, dense, free = scene(name), [], []
        B.run(sc, iters=1, huber=huber, rounds_out=dense)
        P.run(sc, iters=1, huber=huber, cg_iters=1, rounds_out=free)
        rd, pr = dense[0], free[0]
        n_slots = len(pr["held"])
        assert (rd["held"] == pr["held"]).all() and rd["lam"] == pr["lam"]
        worst["b"] = max(worst["b"], _rel(pr["b"].reshape(-1), rd["b"]))
        for _ in range(3):
            v = rng.standard_normal((n_slots, 6))
            v[pr["held"]] = 0.0
            want = (rd["S"] @ v.reshape(-1)).reshape(n_slots, 6)
            want[pr["held"]] = 0.0
            worst["sp"] = max(worst["sp"], _rel(pr["Sp"](v), want))
        blocks = np.stack([rd["S"][6 * s:6 * s + 6, 6 * s:6 * s + 6] for s in range(n_slots)])
        assert (pr["M"] == pr["M"].transpose(0, 2, 1)).all()
        if no_repeats:                                                          # no image sees a track twice: M is the diagonal block of S
            worst["m"] = max(worst["m"], _rel(pr["M"], blocks))
        else:                                                                   # a repeat adds cross terms to S that M leaves out: M - S_ss is positive semi-definite
            assert min(np.linalg.eigvalsh(pr["M"][s] - blocks[s]).min() / np.abs(blocks[s]).max() for s in range(n_slots)) > -1e-12
        assert all(np.linalg.eigvalsh(pr["M"][s]).min() > 0 for s in range(n_slots))
    print({k: f"{v:.4g}" for k, v in worst.items()}, "bars", SP_BAR, B_BAR, M_BAR)
    for k, bar in (("sp", SP_BAR), ("b", B_BAR), ("m", M_BAR)):
        assert 0.8 * bar <= 16 * worst[k] <= bar, (k, worst[k], bar)


def test_edge_cases_of_the_restatement():
    c5 = reference("c5", 10, 0.0, 1e-4, 128, 1e-6)
    assert (c5["cg_used"][c5["taken"] == 1] > 0).all() and (c5["cg_used"] <= 18).all()       # 18 unknowns: conjugate gradients end by then
    assert ((c5["cg_res"] <= 1e-6) | (c5["cg_used"] == 18)).all()
    capped = reference("c17", 10, 0.0, 1e-4, 2, 0.0)
    assert set(capped["cg_used"].tolist()) <= {0, 2} and capped["cg_used"][0] == 2 and (capped["cg_res"][capped["cg_used"] == 2] > 1e-6).all()      # the cap is hit
    early = reference("c17", 10, 0.0, 1e-4, 128, 1e-6)
    assert 0 < early["cg_used"].max() < 128 and (early["cg_res"] <= 1e-6).all()               # an early stop: the tail does nothing
    for name in ("two", "T0", "T1", "badcam", "behind"):                                       # no moving camera, or nothing computed: no iteration
        out = reference(name, 10, 0.0, 1e-4, 128, 1e-6)
        assert (out["cg_used"] == 0).all() and (out["cg_res"] == 0).all(), name
    assert reference("T1", 10, 0.0, 1e-4, 128, 1e-6)["stats"]["n_held"] == 3                  # every free camera held
    atmin = reference("atmin", 8, 0.0, 1e-4, 128, 1e-6)
    assert atmin["taken"].sum() == 0 and (atmin["cg_used"][:5] > 0).all() and (atmin["cg_used"][5:] == 0).all()      # five rounds not taken, then nothing
    for n in (1, 63, 64, 65, 128, 129, 257):
        st = reference(f"f{n}", 2, 0.0, 1e-4, 128, 1e-6)["stats"]
        assert st["n_free"] == n and st["n_held"] == 0 and st["rounds_taken"] == 2, (n, st)
    for n in (63, 64, 65, 129):
        out = reference(f"L{n}", 3, 0.0, 1e-4, 128, 1e-6)
        assert out["cam_obs"].tolist() == [n] * 4 and out["stats"]["n_free"] == 2 and out["stats"]["rounds_taken"] >= 2
    assert reference("c5", 0, 0.0, 1e-4, 128, 1e-6)["cg_used"].shape == (0,)


# ------------------------------------------------------------------------------------------------ the two forms, the bars, the margins
def test_agreement_with_the_dense_form():
    worst = 0.0
    for name, iters, huber, lambda0, cg_iters, cg_tol in DENSE_CASES:
        got, want = reference(name, iters, huber, lambda0, cg_iters, cg_tol), dense_reference(name, iters, huber, lambda0)
        assert (got["taken"] == want["taken"]).all() and got["stats"] == want["stats"] and (got["history"][:, 1] == want["history"][:, 1]).all(), name
        d = relative_difference(got, want, scene(name))
        print(name, iters, huber, f"differs from the dense form by {d:.3g}; cg_used {got['cg_used'].tolist()}")
        worst = max(worst, d)
    print(f"VS_DENSE = {worst:.4g}, 16 x = {16 * worst:.4g}, TOL_PCG_VS_DENSE = {TOL_PCG_VS_DENSE:.4g}")
    assert 0.8 * TOL_PCG_VS_DENSE <= 16 * worst <= TOL_PCG_VS_DENSE


def test_tol_pcg_is_the_measured_one():
    spread, res = 0.0, 0.0
    for case in CASES:
        fwd, rev = reference(*case), reference(*case, "reverse")
        assert fwd["stats"] == rev["stats"] and (fwd["taken"] == rev["taken"]).all() and (fwd["history"][:, 1] == rev["history"][:, 1]).all(), case
        assert (fwd["cg_used"] == rev["cg_used"]).all(), case
        s = relative_difference(fwd, rev, scene(case[0]))
        assert ((fwd["cg_res"] == 0) == (rev["cg_res"] == 0)).all(), case
        rs = float(np.abs(fwd["cg_res"] - rev["cg_res"]).max()) if len(fwd["cg_res"]) else 0.0      # (cg_res is a ratio: the difference is not divided again)
        print(*case, f"spread {s:.3g}, of cg_res {rs:.3g}")
        spread, res = max(spread, s), max(res, rs)
    print(f"SPREAD_PCG = {spread:.4g}, 16 x SPREAD_PCG = {16 * spread:.4g}, TOL_PCG = {TOL_PCG:.4g}; of cg_res {res:.4g}, 16 x = {16 * res:.4g}, TOL_CG_RES = {TOL_CG_RES:.4g}")
    assert 0.8 * TOL_PCG <= 16 * spread <= TOL_PCG and 0.8 * TOL_CG_RES <= 16 * res <= TOL_CG_RES


@pytest.mark.parametrize("name,iters,huber,lambda0,cg_iters,cg_tol", CASES + DENSE_CASES)
def test_fixture_margins(name, iters, huber, lambda0, cg_iters, cg_tol):
    """What makes an exact comparison of taken, cg_used, the counters and cam_obs with the device fair: no decision of the restatement is close."""
    mg = reference(name, iters, huber, lambda0, cg_iters, cg_tol)["margins"]
    print(name, iters, huber, lambda0, cg_iters, cg_tol, {k: f"{v:.3g}" for k, v in mg.items()})
    assert mg["lead"] > LEAD and mg["depth"] > DEPTH and mg["det"] > PIVOT, mg
    assert mg["cg_stop"] > CG_STOP and mg["pq"] > PQ and mg["m_pivot"] > M_PIVOT, mg
