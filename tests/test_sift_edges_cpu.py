"""The cases of tests/sift_cases.py are fit for purpose: conditions on the inputs, checked with the NumPy restatement (tests/sift_ref.py)
alone.  tests/test_sift_edges_gpu.py runs the same cases on the device and allows as many unmatched keypoints as these conditions allow
fragile ones, so the cap here is what keeps that test sharp.

A keypoint is fragile when the smallest relative slack of the decisions that admitted it (``margin``) is below 1e-3: an ulp in a
transcendental can then flip it.  Measured over 30 draws of ``blocks`` at the sizes below: 3.0 % fragile overall, 4.1 % for the worst
image.  The cap is twice that, 8 %; a case with fewer than 25 keypoints has none (one of 24 is already 4 %).  The seeds of sift_cases are
chosen so that this holds; a size that misses it gets another seed, never a wider cap.

Measured (2026-10-21), keypoints / fragile: 6x200 2/0, 9x33 4/0, 31x33 18/0, 32x32 22/0, 64x64 102/4, 33x65 52/0, 63x129 227/4,
65x127 236/6, 16x513 120/3, 12x16384 2079/77, 16384x12 2013/75, 128x257 961/47; colour noise 33x65 2/0, 65x127 37/0, 128x257 103/4;
gray noise 6x200 4/0; blocks8 40/1, checker8 194/0.  The slowest case, 16384x12, takes 1.2 s."""
import numpy as np
import pytest

from gims_amd import hip
from tests import sift_cases as SC
from tests import sift_ref as R
from tests import test_sift_cpu as T0

FRAGILE = 1e-3
CAP = 0.08
SMALL = 25

NAMES = [n for n, _ in SC.CASES]
IMG = dict(SC.CASES)


def _det(name):
    return SC.reference(name, IMG[name])[2]


def test_case_list_covers_the_sizes_and_kinds():
    sizes = {im.shape[:2] for n, im in SC.CASES if n.startswith("blocks_")}
    want = {(2, 2), (2, 300), (2, 16384), (3, 200), (5, 64), (6, 200), (8, 32), (9, 33), (31, 33), (32, 32), (64, 64), (33, 65), (63, 129),
            (65, 127), (16, 513), (12, 16384), (16384, 12), (128, 257)}
    assert want <= sizes
    colour = {im.shape[:2] for n, im in SC.CASES if n.startswith("noise3_") and im.ndim == 3 and im.shape[2] == 3}
    assert {(33, 65), (65, 127), (128, 257)} <= colour
    assert IMG["const_gray_40x56"].shape == (40, 56) and IMG["const_gray_40x56"].min() == IMG["const_gray_40x56"].max() > 0
    assert IMG["zero_bgr_40x56"].shape == (40, 56, 3) and not IMG["zero_bgr_40x56"].any()
    assert len(set(NAMES)) == len(NAMES) and all(im.dtype == np.uint8 for im in IMG.values())
    # a block of 4 spans all of 2 or 3 rows: the thin sizes also come as noise, whose rows differ, so that a fold of the row index counts
    for h, w in ((2, 2), (2, 300), (2, 16384), (3, 200), (5, 64), (6, 200)):
        assert (IMG[f"blocks_{h}x{w}"][0] == IMG[f"blocks_{h}x{w}"][min(h, 4) - 1]).all()
        thin = IMG[f"noise_{h}x{w}"]
        assert thin.shape == (h, w) and all((thin[r] != thin[r + 1]).any() for r in range(h - 1))
    # the builders are seeded: the same call gives the same bytes
    assert np.array_equal(SC.blocks(9, 33, 5), IMG["blocks_9x33"]) and np.array_equal(SC.noise(33, 65, 2, 3), IMG["noise3_33x65"])
    # the colour cases and batches really have three different channels somewhere
    assert (IMG["noise3_33x65"][..., 0] != IMG["noise3_33x65"][..., 2]).any()
    mc = SC.mixed_batch(True)
    assert mc.shape == (4, 40, 56, 3) and (mc[0][..., 0] != mc[0][..., 2]).any() and SC.mixed_batch().shape == (4, 40, 56)
    assert SC.batch_gray().shape == (3, 33, 65) and SC.batch_colour().shape == (3, 63, 129, 3)


@pytest.mark.parametrize("name", NAMES)
def test_fragile_share_is_under_the_cap(name):
    k = _det(name)
    n, fragile = len(k["size"]), int((k["margin"] < FRAGILE).sum())
    print(name, "keypoints", n, "fragile", fragile)
    assert fragile == 0 if n < SMALL else fragile <= CAP * n, (n, fragile)


@pytest.mark.parametrize("name", ["blocks8", "checker8"])
def test_fragile_share_of_the_tie_images(name):
    img = dict(SC.tie_images())[name]
    k = SC.reference(name, img)[2]
    n, fragile = len(k["size"]), int((k["margin"] < FRAGILE).sum())
    print(name, "keypoints", n, "fragile", fragile)
    assert n >= SMALL and fragile <= CAP * n
    # the doubled image has plateaus: some DoG sample of a searched layer equals a neighbour exactly, so >= and <= decide
    dp = SC.reference(name, img)[1]
    assert any((lv[i][5:-5, 5:-6] == lv[i][5:-5, 6:-5]).any() for lv in dp[:2] for i in (1, 2, 3))


def test_reach_octaves():
    seen = set()
    for name in NAMES:
        seen |= set((_det(name)["octave"] & 255).tolist())
    assert {255, 0, 1, 2} <= seen, seen          # pyramid octaves 0, 1, 2, 3 (firstOctave = -1)
    big = set((_det("blocks_128x257")["octave"] & 255).tolist())
    assert {255, 0, 1, 2} <= big, big


def test_reach_counts():
    assert len(_det("blocks_12x16384")["size"]) >= 2000
    assert len(_det("blocks_16384x12")["size"]) >= 2000
    assert len(_det("blocks_128x257")["size"]) >= 900
    for name in SC.EMPTY:
        k = _det(name)
        assert len(k["size"]) == 0 and k["pt"].shape == (0, 2), name
    assert set(SC.EMPTY) >= {"blocks_2x2", "blocks_2x300", "blocks_2x16384", "blocks_3x200", "blocks_5x64", "const_gray_40x56", "zero_bgr_40x56"}


def test_reach_more_than_one_orientation_at_a_position():
    multi = {}
    for name in NAMES:
        k = _det(name)
        if len(k["size"]):
            _, cnt = np.unique(np.column_stack([k["pt"], k["size"]]), axis=0, return_counts=True)
            multi[name] = int((cnt > 1).sum())
    assert sum(multi.values()) > 0
    assert multi["blocks_6x200"] > 0              # also on the level 12 rows high, where most of the orientation window is out of range


def test_reach_duplicates_for_the_final_pass_to_remove(monkeypatch):
    """Two candidates of a plateau refine to the same keypoint: the restatement's removeDuplicatedSorted must have something to drop,
    or the device's duplicate removal would go untested."""
    seen = []
    lexsort = np.lexsort
    monkeypatch.setattr(np, "lexsort", lambda keys: (seen.append(len(keys[0])), lexsort(keys))[1])
    k = R.detect(IMG["blocks_128x257"])
    assert seen and seen[-1] > len(k["size"]), (seen, len(k["size"]))


def test_mixed_batch_counts():
    for colour in (False, True):
        n = [len(SC.reference(f"mixed{int(colour)}_{i}", im)[2]["size"]) for i, im in enumerate(SC.mixed_batch(colour))]
        assert n[0] >= SMALL and n[2] >= SMALL and n[1] == 0 and n[3] == 0, n


@pytest.mark.parametrize("name", NAMES)
def test_layout_equals_restatement_at_every_case_size(name):
    T0.test_layout_equals_restatement(*IMG[name].shape[:2])


@pytest.mark.parametrize("h,w", [(1, 50), (50, 1), (16385, 8), (8, 16385)])
def test_layout_refuses(h, w):
    with pytest.raises(hip.GimsHipError):
        hip.sift_layout(h, w)


def test_restatement_is_quick_enough():
    """The restatement took at most 1.7 s per case where the cases were chosen (the 16384-pixel ones); twice that and a little is allowed
    for a slower machine.  A case that needs more does not belong in a suite that every later change runs."""
    secs = {name: SC.reference(name, IMG[name])[3] for name in NAMES}
    worst = max(secs, key=secs.get)
    print("slowest", worst, round(secs[worst], 2), "s; total", round(sum(secs.values()), 2), "s")
    assert secs[worst] <= 4.0, (worst, secs[worst])
