"""D-GIMS (delaunay=True) checks that need no GPU: the dgims_* fixtures against the exact Delaunay checker, the predicate header
(gims_amd/csrc/delaunay_pred.h) compiled for the host against exact integer arithmetic, the C ABI symbols, and scratch-free kernels."""
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from gims_amd import hip
from tests import dgims_helpers as H
from tests.helpers import golden_names, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gims_amd", "csrc")


# ---------------------------------------------------------------- fixtures
@pytest.mark.parametrize("name", golden_names("dgims_tri_"))
def test_triangulation_fixture_is_delaunay(name):
    g = load_golden(name)
    n, seed = (int(v) for v in g["meta"])
    xy = H.fixture_points(str(g["kind"]), n, seed)
    assert xy.astype(np.float64).sum() == g["xy_sum"], "the input generator drifted from the fixture"
    rep = H.lowest_id_map(xy)
    st = H.check_delaunay(xy, rep[g["edges"].astype(np.int64)])
    if str(g["kind"]) == "sift":
        assert st["n_distinct"] < n                     # the duplicate fixture has duplicates


def test_readme_pair_fixture_is_delaunay():
    from gims_amd import synth
    g = load_golden("dgims_tripair_n15382_14870_s4003")
    n0, n1, c, seed = (int(v) for v in g["meta"])
    pair = synth.make_pair_unbalanced(n0, n1, c, seed)
    for s in ("0", "1"):
        xy = pair["keypoints" + s][0]
        assert xy.astype(np.float64).sum() == g["xy_sum" + s]
        H.check_delaunay(xy, g["edges" + s])


@pytest.mark.parametrize("name", golden_names("dgims_e2e_"))
def test_end_to_end_fixture_graphs_are_delaunay(name):
    g = load_golden(name)
    pair = H.e2e_pair(g["meta"])
    for s in ("0", "1"):
        xy = pair["keypoints" + s][0]
        np.testing.assert_array_equal(g["out/kept" + s], np.arange(len(xy)))
        H.check_delaunay(xy, np.stack([g["out/dgl_src" + s], g["out/dgl_dst" + s]], axis=1))


def test_checker_rejects_a_non_delaunay_triangulation():
    xy = np.asarray([[0, 0], [4, 0], [4, 1], [0, 1.5]], dtype=np.float32)     # 0-2 is the Delaunay diagonal, 1-3 is not
    H.check_delaunay(xy, [[0, 1], [1, 2], [2, 3], [3, 0], [0, 2]])
    with pytest.raises(AssertionError):
        H.check_delaunay(xy, [[0, 1], [1, 2], [2, 3], [3, 0], [1, 3]])


# ---------------------------------------------------------------- predicates on the host
DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include "delaunay_pred.h"
using namespace dpred;
int main(void) {
  char buf[4096];
  while (fgets(buf, sizeof buf, stdin)) {
    double v[8]; int id[4]; char* p = buf;
    for (int i = 0; i < 8; ++i) v[i] = strtod(p, &p);
    for (int i = 0; i < 4; ++i) id[i] = (int)strtol(p, &p, 10);
    printf("%d %d %d %d %d %d %d %d\n", orient_filter(v[0], v[1], v[2], v[3], v[4], v[5]), orient_exact(v[0], v[1], v[2], v[3], v[4], v[5]),
           incircle_filter(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]), incircle_exact(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]),
           incircle_sos<true>(v[0], v[1], id[0], v[2], v[3], id[1], v[4], v[5], id[2], v[6], v[7], id[3]),
           incircle_sos<false>(v[0], v[1], id[0], v[2], v[3], id[1], v[4], v[5], id[2], v[6], v[7], id[3]),
           dist_cmp_filter(v[0], v[1], v[2], v[3], v[4], v[5]), dist_cmp_exact(v[0], v[1], v[2], v[3], v[4], v[5]));
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def pred_exe(tmp_path_factory):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    d = tmp_path_factory.mktemp("pred")
    src, exe = d / "pred.cpp", d / "pred"
    src.write_text(DRIVER)
    subprocess.run(["gcc", "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", CSRC, str(src), "-o", str(exe), "-lm"], check=True)
    return str(exe)


def run_pred(exe, quads, ids=None):
    quads = np.asarray(quads, dtype=np.float32).reshape(-1, 8)
    ids = np.tile(np.arange(4), (len(quads), 1)) if ids is None else np.asarray(ids).reshape(-1, 4)
    lines = "".join(" ".join(float(x).hex() for x in q) + " " + " ".join(str(int(i)) for i in d) + "\n" for q, d in zip(quads, ids))
    out = subprocess.run([exe], input=lines, capture_output=True, text=True, check=True).stdout
    return np.asarray([[int(t) for t in line.split()] for line in out.splitlines()], dtype=np.int64)


def sgn(v):
    return (v > 0) - (v < 0)


def exact_signs(q, ids):
    """Python-integer orient(a,b,c), incircle(a,b,c,d), the tie rule of delaunay_pred.h, |a-b|^2 vs |a-c|^2 (p = a)."""
    P = H.exact_ints(np.asarray(q, dtype=np.float32).reshape(4, 2))
    (ax, ay), (bx, by), (cx, cy), (dx, dy) = P.tolist()
    o = sgn(H.orient_int(ax, ay, bx, by, cx, cy))
    ic = sgn(H.incircle_int(ax, ay, bx, by, cx, cy, dx, dy))
    sos = ic
    if ic == 0:
        cof = [sgn(H.orient_int(bx, by, cx, cy, dx, dy)), -sgn(H.orient_int(ax, ay, cx, cy, dx, dy)),
               sgn(H.orient_int(ax, ay, bx, by, dx, dy)), -sgn(H.orient_int(ax, ay, bx, by, cx, cy))]
        sos = next((cof[k] for k in np.argsort(ids) if cof[k] != 0), 0)
    dc = sgn((bx - ax) ** 2 + (by - ay) ** 2 - (cx - ax) ** 2 - (cy - ay) ** 2)
    return o, ic, sos, dc


def adversarial_quads(rng):
    f32 = np.float32
    quads = []
    # near-cocircular: four float32-rounded points of one circle, at several centres and scales
    for scale, off in ((1.0, 0.0), (1e3, 5e2), (1e-3, 1.0), (7.0, 4096.0), (1e6, -3e6)):
        for _ in range(150):
            t = rng.uniform(0, 2 * np.pi, 4)
            quads.append(np.stack([off + scale * np.cos(t), off + scale * np.sin(t)], axis=1).ravel())
    # points one ulp off a line through a, b
    for _ in range(400):
        a, b = rng.uniform(-1e3, 1e3, 2).astype(f32), rng.uniform(-1e3, 1e3, 2).astype(f32)
        c = (a + f32(rng.uniform()) * (b - a)).astype(f32)
        c[rng.integers(2)] = np.nextafter(c[rng.integers(2)], f32(np.inf) if rng.integers(2) else f32(-np.inf))
        d = (a + f32(rng.uniform()) * (b - a)).astype(f32)
        quads.append(np.concatenate([a, b, c, d]))
    # widely different magnitudes
    mags = np.asarray([1e-38, 1e-30, 2.0 ** -120, 1e-6, 1.0, 3.0, 1e6, 1e20, 1e30, 2e38], dtype=np.float64)
    for _ in range(400):
        quads.append(rng.choice(mags, 8) * rng.choice([-1.0, 1.0], 8) * rng.uniform(1, 1.5, 8))
    return np.asarray(quads, dtype=np.float32)


def tie_quads():
    """Exactly cocircular quadruples (no three collinear): unit squares, Pythagorean circles, scaled and shifted by powers of two."""
    base = [[(0, 0), (1, 0), (1, 1), (0, 1)], [(5, 0), (3, 4), (0, 5), (-4, -3)], [(5, 0), (-3, 4), (0, -5), (4, 3)],
            [(25, 0), (7, 24), (-15, 20), (-24, -7)], [(0, 0), (2, 0), (2, 3), (0, 3)]]
    out = []
    for q in base:
        for k in (-20, 0, 12):
            for off in (0.0, 1000.0, 0.5):
                v = np.asarray(q, dtype=np.float64) * 2.0 ** k + off
                if (v.astype(np.float32) == v).all():            # representable: still exactly cocircular
                    out.append(v.ravel())
    return np.asarray(out, dtype=np.float32)


def test_predicates_match_exact_arithmetic(pred_exe):
    rng = np.random.default_rng(11)
    quads = np.concatenate([adversarial_quads(rng), tie_quads()])
    ids = np.stack([rng.permutation(4) * 3 + rng.integers(0, 3) for _ in range(len(quads))])
    got = run_pred(pred_exe, quads, ids)
    und = 0
    for q, d, (of, oe, icf, ice, sos, sosf, dcf, dce) in zip(quads, ids, got):
        o, ic, s, dc = exact_signs(q, d)
        assert oe == o and ice == ic and dce == dc, (q.tolist(), (oe, ice, dce), (o, ic, dc))
        assert of in (o, 2) and icf in (ic, 2) and dcf in (dc, 2), (q.tolist(), (of, icf, dcf))
        assert sos == s and sosf in (s, 2), (q.tolist(), d.tolist(), sos, sosf, s)
        und += icf == 2
    assert und > 100, "the adversarial inputs should defeat the float64 filter often"
    assert (got[:, 0] == 2).sum() > 5, "the off-the-line inputs should defeat the orientation filter"


def test_tie_rule_is_consistent_under_every_permutation(pred_exe):
    rng = np.random.default_rng(5)
    ties = tie_quads()
    for q in ties:
        pts = q.reshape(4, 2)
        ids = rng.permutation(100)[:4]
        perms = list(itertools.permutations(range(4)))
        quads = np.stack([pts[list(p)].ravel() for p in perms])
        got = run_pred(pred_exe, quads, np.stack([ids[list(p)] for p in perms]))
        assert (got[:, 3] == 0).all(), "tie inputs must be exactly cocircular"
        parity = np.asarray([1 if sum(p[i] > p[j] for i in range(4) for j in range(i + 1, 4)) % 2 == 0 else -1 for p in perms])
        s0 = got[0, 4]
        assert s0 in (-1, 1)
        np.testing.assert_array_equal(got[:, 4], parity * s0)
        if (pts == np.round(pts)).all() and np.ptp(pts, axis=0).max() <= 4096:
            assert (got[:, 5] == got[:, 4]).all(), "small-integer ties are decided by the filter tier"
        # the lowest id, queried against the CCW circle of the other three, counts as outside
        k = int(np.argmin(ids))
        others = [j for j in range(4) if j != k]
        if H.orient_int(*H.exact_ints(pts[others]).ravel().tolist()) < 0:
            others = others[::-1]
        r = run_pred(pred_exe, pts[others + [k]].ravel()[None], ids[others + [k]][None])
        assert r[0, 4] == -1


# ---------------------------------------------------------------- ABI and build
def test_delaunay_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gims_hip.h")).read()
    for name in ("gims_delaunay_build", "gims_delaunay_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, hdr)
        assert name in hip.EXPORTS
    assert "#define GIMS_DT_INFO_DEGENERATE 4" in hdr and "#define GIMS_DT_INFO_ASYMMETRIC 8" in hdr
    assert (hip.DT_INFO_DEGENERATE, hip.DT_INFO_ASYMMETRIC) == (4, 8)
    from gims_amd import build as B
    assert "delaunay.hip" in B.SOURCES


def test_delaunay_kernels_use_no_scratch():
    """The grid, star and CSR kernels of delaunay.hip compile to `ScratchSize: 0` for gfx950; only the exact fallback kernel may use scratch."""
    import tempfile
    from gims_amd import build as B
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [hipcc, *B.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(B.CSRC, "delaunay.hip"), "-o", os.path.join(tmp, "x.o")]
        out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True).stdout
    cur, scratch = None, {}
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            scratch[cur] = int(m.group(1))
    for name in ("dt_grid_kernel", "dt_star_kernelILb0", "dt_star_kernelILb1", "dt_scan_kernel", "dt_check_kernel", "dt_info_kernel"):
        hits = {k: v for k, v in scratch.items() if name in k}
        assert hits, f"no kernel named like {name} in the compiler remarks"
        assert all(v == 0 for v in hits.values()), f"scratch in {hits}"
    assert any("dt_fallback_kernel" in k for k in scratch)
