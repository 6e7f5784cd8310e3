"""gims_train_labels (csrc/eval.hip) through homography.training_labels at ties, one-point images, sizes around the 1024-row chunks of its
row compaction, all-match and no-match pairs, in one ragged batch: rows equal to tests/warp_ref.label_rows (the CPU oracle of
torch_find_matches) exactly.  The inputs are tests/eval_cases.label_batch()."""
import numpy as np
import pytest
import torch

from gims_amd import homography as HG
from tests import eval_cases as C
from tests import warp_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


@pytest.fixture(scope="module")
def batch():
    k0, k1, hs, names = C.label_batch()
    dev = ([torch.from_numpy(a).to(DEV) for a in k0], [torch.from_numpy(b).to(DEV) for b in k1], torch.from_numpy(np.stack(hs)).to(DEV))
    return k0, k1, hs, names, dev


def _matches(rows):
    return int((rows[:, 1:] >= 0).all(1).sum())


@pytest.mark.parametrize("n_iters", [1, 3, 6])
def test_label_rows_equal_oracle_in_a_ragged_batch(batch, n_iters):
    k0, k1, hs, names, (d0, d1, dh) = batch
    got = HG.training_labels(d0, d1, dh, 3, n_iters).cpu().numpy()
    want = R.label_rows(k0, k1, hs, 3, n_iters)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert len(got) == sum(len(a) + len(b) for a, b in zip(k0, k1)) - _matches(got)
    per = {n: got[got[:, 0] == k] for k, n in enumerate(names)}
    assert _matches(per["identity"]) == len(k0[names.index("identity")]) == len(per["identity"])          # everything matches
    assert _matches(per["far"]) == 0                                                                        # nothing does
    if n_iters > 1:
        for n in names:
            if n.startswith("lattice"):          # ties leave work for later iterations (CPU test): the rows of more iterations differ
                k = names.index(n)
                one = R.label_rows(k0[k:k + 1], k1[k:k + 1], hs[k:k + 1], 3, 1)
                assert _matches(per[n]) > _matches(one)
    # the batch is the concatenation of single-pair calls with the pair index rewritten
    singles = []
    for k in range(len(k0)):
        r = HG.training_labels(d0[k:k + 1], d1[k:k + 1], dh[k:k + 1], 3, n_iters).cpu().numpy()
        assert (r[:, 0] == 0).all()
        r[:, 0] = k
        singles.append(r)
    assert np.array_equal(got, np.concatenate(singles))


def test_zero_iterations_give_misses_only(batch):
    k0, k1, hs, names, (d0, d1, dh) = batch
    got = HG.training_labels(d0, d1, dh, 3, 0).cpu().numpy()
    assert len(got) == sum(len(a) + len(b) for a, b in zip(k0, k1)) and _matches(got) == 0
    want = []
    for k, (a, b) in enumerate(zip(k0, k1)):
        want.append(np.stack([np.full(len(a), k), np.arange(len(a)), np.full(len(a), -1)], 1))
        want.append(np.stack([np.full(len(b), k), np.full(len(b), -1), np.arange(len(b))], 1))
    assert np.array_equal(got, np.concatenate(want))
    assert np.array_equal(got, R.label_rows(k0, k1, hs, 3, 0))
