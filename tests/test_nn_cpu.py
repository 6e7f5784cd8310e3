"""Descriptor baselines (NNDR / MNN), the parts that need no GPU: the float64 restatement (tests/nn_ref.py) against the reference's own
outputs on every nn_* fixture (tests/golden/nn_*.npz, tools/gen_golden_nn.py), the ctypes mirror of gims_nn_pair, the argument checks of
gims_nn_match (they come back before any HIP call) and the ValueError of baselines.mnn."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from gims_amd import baselines, hip
from tests import nn_ref
from tests.helpers import golden_names, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [name for name, _ in nn_ref.FIXTURES]


@functools.lru_cache(maxsize=None)
def solved(name, mutual):
    g = load_golden(name)
    recipe = nn_ref.recipe_from_npz(g)
    a, b = nn_ref.build_fixture(recipe)
    return recipe, a, b, nn_ref.solve(a, b, recipe["threshold"], mutual)


def test_every_fixture_has_its_golden_and_its_recipe():
    assert sorted(golden_names("nn_")) == sorted(NAMES)
    for name, recipe in nn_ref.FIXTURES:
        stored = nn_ref.recipe_from_npz(load_golden(name))
        assert stored == nn_ref.recipe_from_npz(nn_ref.recipe_arrays(recipe)), name
        g = load_golden(name)
        want = nn_ref.EXPECTED_MATCHES[name]
        assert g["nndr/ratios"].size == want[0] and (want[1] is None or g["mnn/ratios"].size == want[1])
    g = load_golden("nn_n1024_s1002_d12_t60_k64")          # exactly one match: the reference's squeeze() leaves 0-dim indices
    assert g["nndr/match_indices"].shape == () and g["nndr/good_matches"].shape == () and g["nndr/ratios"].shape == (1,)
    assert g["mnn/match_indices"].shape == () and g["mnn/ratios"].shape == (1,)


@pytest.mark.parametrize("method", ["nndr", "mnn"])
@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_reference(name, method):
    """Match sets and good_matches equal, ratios within 1e-5 (measured reference-against-float64 gap: 1.8e-6); rows may be left out only by
    the rule of nn_ref.excluded_rows, and at most 1 % of a fixture's rows."""
    mutual = method == "mnn"
    recipe, a, b, ref = solved(name, mutual)
    g = load_golden(name)
    excl = nn_ref.excluded_rows(ref, recipe["threshold"], mutual)
    n_ex, err = nn_ref.compare_with_golden(name, a.shape[1], ref["nn1"], ref["ratio"], ref["match"], excl, g[f"{method}/match_indices"],
                                           g[f"{method}/good_matches"], g[f"{method}/ratios"], 1e-5)
    print(f"{name} {method}: {int(ref['match'].sum())} matches, {n_ex} rows excluded, largest ratio difference {err:.2e}")


def test_restatement_preselection_equals_brute_force():
    """two_nearest evaluates only preselected columns in the fixed order; against all columns it must give the same answer (with duplicates)."""
    a, b = nn_ref.build_fixture(dict(kind="pair", n=96, seed=11, noise=0.1, threshold=0.8, twins=0))
    a, b = np.ascontiguousarray(a.T), np.ascontiguousarray(b.T)
    b[7] = b[3]
    b[50] = b[3]
    a[5] = b[3]
    fast, full = nn_ref.two_nearest(a, b), nn_ref.two_nearest(a, b, everything=True)
    for x, y in zip(fast, full):
        np.testing.assert_array_equal(x, y)
    assert fast[0][5] == 3 and fast[1][5] == 7 and fast[2][5] == 0.0


def test_pair_struct_layout_matches_header(tmp_path):
    fields = [f for f, _ in hip.NnPair._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gims_hip.h"\nint main(void) {\nprintf("%zu\\n", sizeof(gims_nn_pair));\n'
                   + "".join('printf("%%zu\\n", offsetof(gims_nn_pair, %s));\n' % f for f in fields) + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(hip.NnPair)] + [getattr(hip.NnPair, f).offset for f in fields]
    assert got[0] == 152 and hip.NnPair.debug.offset == 144
    assert "gims_nn_match" in hip.EXPORTS and "gims_nn_workspace_bytes" in hip.EXPORTS
    assert hip.load().gims_abi_version() == hip.ABI_VERSION == 5


def _fake_pair(n0=300, n1=200, d=256, mutual=0, **kw):
    """Never dereferenced: the checks under test return before any HIP call."""
    p = hip.NnPair(0x10000, 0x20000, d, d, n0, n1, d, mutual, 0.8, 0, *([0x30000] * 8), 0x40000, 0x50000, 0x60000, None)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _call(pairs, flags=0, work=0x100000, work_bytes=None):
    lib = hip.load()
    arr = (hip.NnPair * len(pairs))(*pairs)
    need = int(lib.gims_nn_workspace_bytes(arr, len(pairs), flags))
    rc = lib.gims_nn_match(arr, len(pairs), flags, work, need if work_bytes is None else work_bytes, None)
    return rc, (lib.gims_last_error() or b"").decode(), need


@pytest.mark.parametrize("pair, text", [
    (dict(d=100), "multiple of 32"), (dict(d=1024), "multiple of 32"), (dict(n1=1), "n1 >= 2"), (dict(n0=0), "n0 >= 1"),
    (dict(n0=32769), "32768"), (dict(n1=40000), "32768"), (dict(n0=1, mutual=1), "mutual"), (dict(a=None), "null pointer"),
    (dict(ratio=None), "null pointer"), (dict(info=None), "null pointer"), (dict(mutual=1, matches1=None), "matches1"),
    (dict(lda=128), "pitch"), (dict(ldb=258), "pitch"), (dict(b=0x20004), "aligned")])
def test_bad_arguments_are_refused_before_any_device_call(pair, text):
    rc, msg, need = _call([_fake_pair(), _fake_pair(**pair)])
    assert rc == hip.GIMS_EINVAL and need == 0
    assert "gims_nn_match: pair 1" in msg and text in msg, msg


def test_bad_calls_are_refused_before_any_device_call():
    ok = [_fake_pair(), _fake_pair(mutual=1)]
    lib = hip.load()
    arr = (hip.NnPair * 2)(*ok)
    need = int(lib.gims_nn_workspace_bytes(arr, 2, 0))
    assert need > 0 and int(lib.gims_nn_workspace_bytes(arr, 2, hip.NN_EXHAUSTIVE)) > 0
    assert int(lib.gims_nn_workspace_bytes(arr, 2, 6)) == 0 and int(lib.gims_nn_workspace_bytes(None, 2, 0)) == 0
    rc, msg, _ = _call(ok, work_bytes=need - 1)
    assert rc == hip.GIMS_EINVAL and "workspace too small" in msg
    rc, msg, _ = _call(ok, work=None)
    assert rc == hip.GIMS_EINVAL and "workspace" in msg
    rc, msg, _ = _call(ok, flags=2)
    assert rc == hip.GIMS_EINVAL and "flag" in msg
    assert lib.gims_nn_match(None, 1, 0, 0x100000, 1 << 20, None) == hip.GIMS_EINVAL
    assert lib.gims_nn_match(arr, 0, 0, 0x100000, 1 << 20, None) == hip.GIMS_EINVAL


def test_python_interface_refuses_what_the_reference_cannot_index():
    one, many = np.zeros((256, 1), np.float32), np.zeros((256, 5), np.float32)
    with pytest.raises(ValueError, match="first set needs at least 2"):
        baselines.mnn(one, many)
    with pytest.raises(ValueError, match="second-nearest"):
        baselines.nndr(many, one)
    with pytest.raises(ValueError, match="method"):
        baselines.nn_match_pairs([dict(descriptors0=many[None], descriptors1=many[None])], method="flann")
    import gims_amd
    assert gims_amd.nndr is baselines.nndr and gims_amd.mnn is baselines.mnn and gims_amd.nn_match_pairs is baselines.nn_match_pairs
