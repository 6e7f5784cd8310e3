"""The plain benchmark run (`bench.py --gpus 1 --steps K --warmup W`, no --full) as a fresh child process: exactly K timed steps, the
headline keys and nothing it did not measure, no bench_extra.json, and with --dump-outputs the outputs of the last timed step -- the same
arrays from two runs of the same arguments (the inputs are seeded)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--kpts", "256", "--pairs", "2", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_bench_plain_run_times_its_steps_and_dumps_its_outputs(tmp_path):
    extra = os.path.join(ROOT, "bench_extra.json")
    before = os.path.getmtime(extra) if os.path.exists(extra) else None
    res = _plain_run(tmp_path / "a")
    assert res["steps"] == 3 and res["warmup"] == 1 and res["n_gpus"] == 1 and res["unit"] == "pairs/s" and res["higher_is_better"] is True
    assert res["metric"] == "image-pairs/sec at 2x256 keypoints" and "MFMA attention" in res["dtype"]
    assert res["value"] > 0 and abs(res["value"] * res["ms_per_step"] - 1e3 * 2) < 1e-2 * 2e3        # value = pairs / step time
    for k in ("roofline", "cpu_baseline", "also", "stage_ms_per_step", "extra", "parity_pair0"):
        assert k not in res, k
    assert (os.path.getmtime(extra) if os.path.exists(extra) else None) == before
    names = sorted(f[:-4] for f in os.listdir(tmp_path / "a"))
    assert "stats" in names and {f"pair000{p}_{k}{s}" for p in "01" for k in ("matches", "matching_scores", "kept") for s in "01"} <= set(names)
    a = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in names}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    m0 = a["pair0000_matches0"]
    assert m0.shape == a["pair0000_matching_scores0"].shape and (m0 >= 0).sum() > 128
    assert sorted(a["stats"][:, 0].tolist()) == [0.0, 1.0]

    _plain_run(tmp_path / "b")
    assert sorted(f[:-4] for f in os.listdir(tmp_path / "b")) == names
    for n in names:
        b = np.load(tmp_path / "b" / (n + ".npy"))
        if "matches" in n or "kept" in n or "rows" in n:
            np.testing.assert_array_equal(b, a[n], err_msg=n)
        else:
            np.testing.assert_allclose(b, a[n], rtol=0, atol=1e-5, err_msg=n)
