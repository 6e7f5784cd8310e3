"""The sweep fixtures (tests/golden/sweep_*, tools/gen_golden_sweep.py: one pair under a grid of graph parameters, by the reference)
against the CPU oracle, before a GPU sees them; and the host-side pieces of the per-image graph parameters: the ctypes mirror of
gims_agc_params, the refusals match_pairs keeps by default."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest
import torch

from gims_amd import GMatcher, hip, synth
from oracle import gims_oracle as O
from tests.helpers import golden_names, load_golden, pair_to_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = {"sinkhorn_iterations": 20, "match_threshold": 0.02}        # the model settings of the reference's parameter_search.py
STORED = {"sweep_n1024sparse_s2001": 30, "sweep_n512_s7001": 48}      # settings per pair: 4 x 4 x {7, 10} minus two exact ties; 4 x 4 x {0, 7, 10}


def sweep_fixture(prefix):
    """All radius files of one pair -> (pair, [(radius, percentile, min_size)], {setting: dict with 'out/*' or 'error_type' / 'error_text'}, ties)."""
    names = golden_names(prefix + "_")
    assert len(names) == 4, names
    settings, per, ties, pair = [], {}, [], None
    for name in sorted(names, key=lambda nm: int(nm.rsplit("_r", 1)[1])):
        g = load_golden(name)
        n, seed, cw, ch, radius, iters = (int(v) for v in g["meta"])
        assert iters == CONFIG["sinkhorn_iterations"] and float(g["match_threshold"]) == CONFIG["match_threshold"]
        if pair is None:
            pair = synth.make_pair(n, seed, canvas=(cw, ch) if cw else None)
        ties += [tuple(int(v) for v in t) for t in g["ties"]]
        for r, t, m in g["settings"].tolist():
            assert r == radius
            key = f"r{r}t{t}m{m}/"
            per[(r, t, m)] = {k[len(key):]: v for k, v in g.items() if k.startswith(key)}
            settings.append((r, t, m))
    return pair, settings, per, ties


def test_fixture_counts():
    """A regenerated fixture cannot quietly shrink: 30 and 48 stored settings, four of them recorded as the reference's ValueError, and
    the only grid settings left out are the two exact ties of the reference's OT matrix the generator's rule finds."""
    for prefix, count in STORED.items():
        _, settings, per, ties = sweep_fixture(prefix)
        assert len(settings) == len(set(settings)) == count
        errors = [s for s in settings if "error_type" in per[s]]
        if prefix.startswith("sweep_n1024sparse"):
            assert sorted(ties) == [(22, 10, 7), (22, 10, 10)]
            assert sorted(errors) == [(10, 0, 10), (10, 2, 10), (10, 5, 10), (10, 10, 10)]
            assert sorted(set(settings) | set(ties)) == sorted((r, t, m) for r in (10, 15, 22, 30) for t in (0, 2, 5, 10) for m in (7, 10))
        else:
            assert not ties and not errors
            assert sorted(settings) == sorted((r, t, m) for r in (10, 15, 22, 30) for t in (0, 2, 5, 10) for m in (0, 7, 10))
        for s in settings:
            if s not in errors:
                assert min(per[s]["out/gap0"].min(), per[s]["out/gap1"].min()) > 0


@pytest.mark.parametrize("prefix", list(STORED))
def test_oracle_reproduces_every_stored_setting(prefix, synth_sd):
    """Kept ids and match indices equal, scores within 1e-4, the same exception where the reference raised."""
    pair, settings, per, _ = sweep_fixture(prefix)
    worst = 0.0
    for r, t, m in settings:
        g = per[(r, t, m)]
        data = pair_to_data(pair, r, t, m)
        if "error_type" in g:
            with pytest.raises(ValueError) as ei:
                O.gmatcher_forward(synth_sd, data, CONFIG)
            assert type(ei.value).__name__ == str(g["error_type"]) and str(ei.value) == str(g["error_text"])
            continue
        out = O.gmatcher_forward(synth_sd, data, CONFIG)
        for s in ("0", "1"):
            np.testing.assert_array_equal(np.asarray(data[f"kept_kpts{s}_indices"][0]), g["out/kept" + s], err_msg=str((r, t, m)))
            np.testing.assert_array_equal(out["matches" + s][0].numpy(), g["out/matches" + s], err_msg=str((r, t, m)))
            err = float(np.abs(out["matching_scores" + s][0].numpy() - g["out/matching_scores" + s]).max())
            assert err < 1e-4, ((r, t, m), err)
            worst = max(worst, err)
    print(f"{prefix}: {len(settings)} settings, largest score difference {worst:.2e}")


def test_params_struct_layout_matches_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gims_hip.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu\\n", sizeof(gims_agc_params), offsetof(gims_agc_params, radius), '
                   'offsetof(gims_agc_params, percentile), offsetof(gims_agc_params, min_size), offsetof(gims_agc_params, reserved));\nreturn 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    P = hip.AgcParams
    assert got == [ctypes.sizeof(P), P.radius.offset, P.percentile.offset, P.min_size.offset, P.reserved.offset] == [24, 0, 8, 16, 20]
    assert "gims_agc_build" in hip.EXPORTS and hip.load().gims_abi_version() == 5
    with pytest.raises(ValueError, match="parameter triples"):
        hip.agc_build_each([object(), object()], [(15, 2, 7)], None)


def _fake_data(**kw):
    """What match_pairs looks at before any device work: the device and the batch size of keypoints0."""
    return dict(keypoints0=types.SimpleNamespace(device=torch.device("cuda"), shape=(1, 8, 2)), **kw)


def test_match_pairs_still_refuses_mixed_settings_by_default():
    m = GMatcher({}).eval()
    with pytest.raises(ValueError, match="radius / percentile / min_size"):
        m.match_pairs([_fake_data(radius=15, percentile=2, min_size=7), _fake_data(radius=25, percentile=7, min_size=8)])
    with pytest.raises(ValueError, match="radius / percentile / min_size"):
        m.match_pairs([_fake_data(radius=15, percentile=2, min_size=7), _fake_data(radius=15, percentile=2, min_size=8)], per_pair_graph=False)
    with pytest.raises(ValueError, match="delaunay"):
        m.match_pairs([_fake_data(delaunay=True), _fake_data()])
    with pytest.raises(TypeError):
        m.match_pairs([_fake_data()], True)                       # keyword-only


def test_graph_setting_defaults():
    assert GMatcher._graph_setting({}) == (25, 7, 8, False)
    assert GMatcher._graph_setting({"radius": 10, "delaunay": 1}) == (10, 7, 8, True)
    assert GMatcher._graph_setting((15, 2, 7)) == (15, 2, 7, False)


def test_parameter_sweep_tool_writes_the_reference_row_format():
    """tools/parameter_sweep.py: the reference tool's ranges (inclusive) and its record.txt row [r, t, m, correct, total, time], with
    total = len(matches0) = the kept keypoints of image 0, and [r, t, m, 0, 0, time] for a setting that kept nothing."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("parameter_sweep", os.path.join(ROOT, "tools", "parameter_sweep.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.parse_args([])
    grid = [(r, t, m) for r in tool.str_to_range(a.r_range) for t in tool.str_to_range(a.t_range) for m in tool.str_to_range(a.m_range)]
    assert len(grid) == 2541 and grid[0] == (10, 0, 0) and grid[-1] == (30, 10, 10) and a.max_keypoints == -1
    recs = [dict(radius=15, percentile=2, min_size=7, kept0=307, kept1=305, error=None),
            dict(radius=10, percentile=0, min_size=10, kept0=0, kept1=0, error="ValueError: need at least one array to concatenate")]
    assert tool.records_to_lines(recs, [251.0, 0], 0.5) == ["[15, 2, 7, 251, 307, 0.5]", "[10, 0, 10, 0, 0, 0.5]"]
