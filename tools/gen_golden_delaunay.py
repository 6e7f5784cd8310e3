#!/usr/bin/env python3
"""Generate the D-GIMS golden vectors (tests/golden/dgims_*.npz) BY RUNNING THE REFERENCE ITSELF.

Runs only in the build container (needs /root/reference, scipy and networkx).  The reference is imported unmodified, with the stubs of
tools/_ref_stubs (see tools/gen_golden.py).

  * triangulation goldens: models.agc.build_graph_from_keypoints_Delaunay (scipy's Qhull) on the inputs, its undirected edge list stored;
  * end-to-end goldens: the unmodified reference GMatcher.forward with models.gmatcher.build_optimize_graph_with_cosine_similarity
    replaced by the reference's Delaunay builder plus kept = list(range(N)) -- the contract of delaunay=True (the reference's own
    delaunay branch never binds kept_kpts{0,1}_indices, gmatcher.py:223-231 vs 250-251).  For inputs with exact duplicate coordinates
    the builder first relabels every edge endpoint to the lowest id of its duplicate group (Qhull keeps an insertion-order-dependent
    member of the group);
  * self-check: every stored triangulation is verified to be truly Delaunay in exact integer arithmetic (tests/dgims_helpers.py); a
    fixture on which Qhull's floating-point result is not is refused.

Inputs are stored as seeds (tests/dgims_helpers.py regenerates them from gims_amd.synth) plus a checksum.

    python tools/gen_golden_delaunay.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import gen_golden as GG  # noqa: E402  (puts the reference and the stubs on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from models import agc as RA  # noqa: E402  (the reference)
from models import gmatcher as RG  # noqa: E402  (the reference)
from gims_amd import synth  # noqa: E402
from tests import dgims_helpers as H  # noqa: E402

torch.set_grad_enabled(False)


def ref_edges(xy):
    """Undirected edge list of the reference's Delaunay graph of one image (keypoints only matter)."""
    kp = torch.from_numpy(np.asarray(xy, dtype=np.float32)[None])
    n = kp.shape[1]
    with GG.quiet():
        g = RA.build_graph_from_keypoints_Delaunay(kp, torch.zeros((1, 1, n)), torch.zeros((1, n)))[0]
    src, dst = g.edges()
    return H.canon_edges(np.stack([src.numpy(), dst.numpy()], axis=1))


def checked(xy, edges):
    rep = H.lowest_id_map(xy)
    st = H.check_delaunay(xy, H.canon_edges(rep[edges]))
    return st


class DelaunayBuilder:
    """Stands in for models.gmatcher.build_optimize_graph_with_cosine_similarity: the reference's Delaunay graphs (duplicate endpoints
    relabelled to the lowest id of their group), every keypoint kept."""

    def __init__(self):
        self.orig = RA.build_graph_Delaunay

    def relabelled(self, keypoints, descriptors, scores):
        import networkx as nx
        out = []
        for b, g in enumerate(self.orig(keypoints, descriptors, scores)):
            rep = H.lowest_id_map(keypoints[b].cpu().numpy())
            h = nx.Graph()
            h.add_nodes_from(g.nodes(data=True))
            h.add_edges_from((int(rep[u]), int(rep[v])) for u, v in g.edges if rep[u] != rep[v])
            out.append(h)
        return out

    def __call__(self, keypoints, descriptors, scores, radius, percentile, min_size, device, image=None, show=False):
        RA.build_graph_Delaunay = self.relabelled
        try:
            graphs = RA.build_graph_from_keypoints_Delaunay(keypoints, descriptors, scores, device=device)
        finally:
            RA.build_graph_Delaunay = self.orig
        return graphs, [list(range(keypoints.shape[1])) for _ in range(keypoints.shape[0])]


def save(name, **arrs):
    GG.save(name, **arrs)


def main():
    # ---- triangulations -------------------------------------------------------------------------------------
    for kind, n, seed in (("uniform", 64, 4000), ("uniform", 1024, 4001), ("uniform", 4096, 4002), ("cluster", 4096, 4005),
                          ("sift", 4096, 4006), ("uniform", 32768, 4004)):
        xy = H.fixture_points(kind, n, seed)
        e = ref_edges(xy)
        st = checked(xy, e)
        print(kind, n, st)
        save(f"dgims_tri_{kind}_n{n}_s{seed}", edges=e.astype(np.int32), meta=np.asarray([n, seed], dtype=np.int64),
             kind=np.asarray(kind), xy_sum=np.float64(xy.astype(np.float64).sum()))
    # README-size unbalanced pair (both images)
    pair = synth.make_pair_unbalanced(15382, 14870, 12000, 4003)
    arrs = {"meta": np.asarray([15382, 14870, 12000, 4003], dtype=np.int64)}
    for s in ("0", "1"):
        xy = pair["keypoints" + s][0]
        e = ref_edges(xy)
        print("readme", s, checked(xy, e))
        arrs["edges" + s] = e.astype(np.int32)
        arrs["xy_sum" + s] = np.float64(xy.astype(np.float64).sum())
    save("dgims_tripair_n15382_14870_s4003", **arrs)

    # ---- end to end -----------------------------------------------------------------------------------------
    builder = DelaunayBuilder()
    orig = RG.build_optimize_graph_with_cosine_similarity
    RG.build_optimize_graph_with_cosine_similarity = builder
    try:
        models = {}
        for n, seed, wseed, iters, thr, dup in ((256, 5000, 123, 100, 0.2, False), (1024, 5001, 123, 100, 0.2, False),
                                                (256, 5002, 123, 20, 0.02, True), (1024, 5003, 7, 20, 0.02, False),
                                                ((1500, 900), 5004, 123, 100, 0.2, False)):
            cfg = {} if iters == 100 else {"sinkhorn_iterations": 20, "match_threshold": 0.02}
            if (wseed, iters) not in models:
                models[(wseed, iters)] = GG.ref_model(synth.make_state_dict(wseed), cfg)
            meta = np.asarray([seed, wseed, iters, int(dup)] + list(n if isinstance(n, tuple) else (n, n)), dtype=np.int64)
            pair = H.e2e_pair(meta)
            tag = f"n{n[0]}_{n[1]}" if isinstance(n, tuple) else f"n{n}"
            tag += "dup" if dup else ""
            for s in ("0", "1"):
                xy = pair["keypoints" + s][0]
                checked(xy, ref_edges(xy))
            r = GG.run_reference(models[(wseed, iters)], pair, 15, 2, 7)
            arrs = {"out/" + k: v for k, v in r.items()}
            arrs["meta"] = meta
            arrs["match_threshold"] = np.float64(thr)
            save(f"dgims_e2e_{tag}_s{seed}_w{wseed}_i{iters}", **arrs)
    finally:
        RG.build_optimize_graph_with_cosine_similarity = orig


if __name__ == "__main__":
    main()
