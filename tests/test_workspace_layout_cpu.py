"""Scratch workspaces, the parts that need no GPU.  Every batched entry point sizes and carves its workspace with one layout routine
(csrc/common.h: WsLayout); this file pins what the size queries return and checks that a workspace one byte short is refused before any
device call.

EXPECTED was recorded from a build of the commit BEFORE the layout routines were shared (its library loaded through hip.load(path) and run
through queries() below), never from the code under test: a layout edit that changes a size has to change a literal here on purpose.
The Sinkhorn rows are taken with GIMS_OT_RESIDENT=0 (read per call), which makes them independent of whether a device is present."""
import ctypes as C
import os

import numpy as np
import pytest

from gims_amd import hip

SHAPES = [(1, 1), (63, 65), (64, 64), (257, 4097), (700, 650)]          # element counts on and around a 256-byte boundary, ragged
GRAPH_N = [2, 63, 64, 65, 257, 700]
NN_SHAPES = [(2, 2), (63, 65), (64, 64), (257, 4097), (700, 650)]       # n1 >= 2 always, n0 >= 2 for the mutual test

EXPECTED = {
    "eval/0": 97280, "eval/1": 98560, "eval/64": 98560, "eval/3000": 157440,
    "labels": 109312,
    "sinkhorn/all": 2983936, "sinkhorn/each": [2048, 8704, 7680, 3232768, 698624],
    "sinkhorn_backward": 16875264,
    "agc/window": 4770048, "agc/robust": 5917696,
    "delaunay": 64768,
    "nn/plain": 866560, "nn/mutual": 3059712, "nn/exhaustive": 81664, "nn/mutual+exhaustive": 184832,
}


class _env:
    def __init__(self, **kv):
        self.kv, self.old = kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def fake_ot(shapes):
    """Fake non-null pointers everywhere (never dereferenced on the host); scores 16-byte aligned, ld a multiple of 4."""
    return (hip.OtProblem * len(shapes))(*[hip.OtProblem(0x10000, (m + 3) // 4 * 4, n, m, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000) for n, m in shapes])


def fake_eval(shapes):
    return (hip.EvalPair * len(shapes))(*[hip.EvalPair(0x10000, 0x20000, 0x30000, 0x40000, n0, n1, 480, 640, (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1),
                                                       0x50000, 0x60000, 0x70000, 0x80000) for n0, n1 in shapes])


def fake_labels(shapes):
    return (hip.LabelPair * len(shapes))(*[hip.LabelPair(0x10000, 0x20000, n0, n1) for n0, n1 in shapes])


def fake_images(ns, d=256):
    return (hip.AgcImage * len(ns))(*[hip.AgcImage(0x10000, 0x20000, d, n, d, 0x30000, 0x40000, 0x50000, 64 * n + 100, 0x60000) for n in ns])


def fake_nn(shapes, mutual, d=64):
    """mutual: one value for every pair, or one per pair."""
    mutual = list(mutual) if isinstance(mutual, (list, tuple)) else [mutual] * len(shapes)
    return (hip.NnPair * len(shapes))(*[hip.NnPair(0x10000, 0x20000, d, d, n0, n1, d, int(mu), 0.8, 0, *([0x30000] * 8), None, 0x50000, 0x60000, None)
                                        for (n0, n1), mu in zip(shapes, mutual)])


def queries(lib):
    """Every size query of the library over the ragged lists above."""
    k = len(SHAPES)
    out = {f"eval/{it}": int(lib.gims_eval_workspace_bytes(fake_eval(SHAPES), k, it)) for it in (0, 1, 64, 3000)}
    out["labels"] = int(lib.gims_train_labels_workspace_bytes(fake_labels(SHAPES), k))
    with _env(GIMS_OT_RESIDENT="0"):
        out["sinkhorn/all"] = int(lib.gims_sinkhorn_workspace_bytes(fake_ot(SHAPES), k))
        out["sinkhorn/each"] = [int(lib.gims_sinkhorn_workspace_bytes(fake_ot([s]), 1)) for s in SHAPES]
    out["sinkhorn_backward"] = int(lib.gims_sinkhorn_backward_workspace_bytes(fake_ot(SHAPES), k))
    with _env(GIMS_AGC_ROBUST="0"):
        out["agc/window"] = int(lib.gims_agc_workspace_bytes(fake_images(GRAPH_N), len(GRAPH_N), 0))
        out["agc/robust"] = int(lib.gims_agc_workspace_bytes(fake_images(GRAPH_N), len(GRAPH_N), hip.AGC_ROBUST))
    out["delaunay"] = int(lib.gims_delaunay_workspace_bytes(fake_images(GRAPH_N), len(GRAPH_N)))
    for name, mutual, flags in (("plain", 0, 0), ("mutual", 1, 0), ("exhaustive", 0, hip.NN_EXHAUSTIVE), ("mutual+exhaustive", 1, hip.NN_EXHAUSTIVE)):
        out[f"nn/{name}"] = int(lib.gims_nn_workspace_bytes(fake_nn(NN_SHAPES, mutual), len(NN_SHAPES), flags))
    return out


def test_size_queries_return_what_they_returned_before_the_layouts_were_shared():
    got = queries(hip.load())
    assert sorted(got) == sorted(EXPECTED)
    for key in EXPECTED:
        assert got[key] == EXPECTED[key], (key, got[key], EXPECTED[key])


WORK = 0x100000          # fake, 256-byte aligned, never dereferenced: the refusal comes before any device call


def _short_eval(lib, short):
    arr = fake_eval(SHAPES)
    need = int(lib.gims_eval_workspace_bytes(arr, len(SHAPES), 65))
    return need, lib.gims_eval_pairs(arr, len(SHAPES), 3.0, 3, 3.0, 65, 1, WORK, need - short, None)


def _short_labels(lib, short):
    arr = fake_labels(SHAPES)
    need = int(lib.gims_train_labels_workspace_bytes(arr, len(SHAPES)))
    return need, lib.gims_train_labels(arr, len(SHAPES), 0x70000, 3.0, 3, 0x80000, 0x90000, WORK, need - short, None)


def _short_match(lib, short):
    arr = fake_ot(SHAPES)
    need = int(lib.gims_sinkhorn_workspace_bytes(arr, len(SHAPES)))
    return need, lib.gims_sinkhorn_match(arr, len(SHAPES), 1.0, 10, 0.2, WORK, need - short, 0, None)


def _short_history(lib, short):
    arr = fake_ot(SHAPES)
    hist = (C.c_void_p * len(SHAPES))(*[0x70000] * len(SHAPES))
    need = int(lib.gims_sinkhorn_workspace_bytes(arr, len(SHAPES)))
    return need, lib.gims_sinkhorn_history(arr, len(SHAPES), 1.0, 3, hist, WORK, need - short, None)


def _short_backward(lib, short):
    arr = fake_ot(SHAPES)
    hist, dz = (C.c_void_p * len(SHAPES))(*[0x70000] * len(SHAPES)), (C.c_void_p * len(SHAPES))(*[0x80000] * len(SHAPES))
    need = int(lib.gims_sinkhorn_backward_workspace_bytes(arr, len(SHAPES)))
    return need, lib.gims_sinkhorn_backward(arr, len(SHAPES), 1.0, 3, hist, dz, 0x90000, WORK, need - short, None)


def _short_agc(lib, short):
    arr = fake_images(GRAPH_N)
    params = (hip.AgcParams * len(GRAPH_N))(*[hip.AgcParams(15.0, 2.0, 7, 0)] * len(GRAPH_N))
    need = int(lib.gims_agc_workspace_bytes(arr, len(GRAPH_N), 0))
    return need, lib.gims_agc_build(arr, len(GRAPH_N), params, len(GRAPH_N), 0, WORK, need - short, None)


def _short_delaunay(lib, short):
    arr = fake_images(GRAPH_N)
    need = int(lib.gims_delaunay_workspace_bytes(arr, len(GRAPH_N)))
    return need, lib.gims_delaunay_build(arr, len(GRAPH_N), WORK, need - short, None)


@pytest.mark.parametrize("call, name", [
    (_short_eval, "gims_eval_pairs"), (_short_labels, "gims_train_labels"), (_short_match, "gims_sinkhorn_match"),
    (_short_history, "gims_sinkhorn_history"), (_short_backward, "gims_sinkhorn_backward"), (_short_agc, "gims_agc_build"),
    (_short_delaunay, "gims_delaunay_build")])
def test_a_workspace_one_byte_short_is_refused_before_any_device_call(call, name):
    """The message carries both byte counts."""
    lib = hip.load()
    with _env(GIMS_OT_RESIDENT="0", GIMS_AGC_ROBUST="0"):
        need, rc = call(lib, 1)
    msg = (lib.gims_last_error() or b"").decode()
    assert need > 0 and rc == hip.GIMS_EINVAL
    assert name in msg and "workspace too small" in msg, msg
    assert str(need) in msg and str(need - 1) in msg, msg


# ------------------------------------------------------------------------------------------------ the auxiliary functions of gims_run_ops
# Their buffers are laid out by the library's own routines too, reported by gims_aux_layout; the hip functions below name the regions.  The
# sizes sit on and around a 256-byte boundary of every element size (1, 4, 8, 24 ... bytes), plus the empty case.
TRI_SIZES = [(0, 0), (1, 2), (32, 64), (33, 65), (64, 256), (65, 257), (257, 1300), (300, 2400)]                     # (T, n_obs)
RESECT_SIZES = [((), 0), ((2,), 1), ((100, 156), 64), ((100, 157), 65), ((4,) * 64, 1), ((4,) * 65, 3), ((700, 0, 650), 1024)]      # (n_k per entry, iters)
BA_SIZES = [(0, 0, 0, 0, 0), (1, 2, 2, 1, 1), (32, 64, 3, 2, 2), (33, 65, 3, 2, 3), (257, 1300, 7, 20, 5), (300, 2400, 130, 2, 128)]
BA_PCG_SIZES = BA_SIZES + [(300, 2400, 130, 2, 65536)]                                                             # (T, n_obs, n_images, iters, n_free)
BA_FOCAL_SIZES = ([(0, 0, 0, 0, 0, 0), (1, 2, 2, 1, 1, 1), (32, 64, 3, 2, 2, 32), (257, 1300, 7, 20, 5, 64), (300, 2400, 130, 2, 128, 65)]
                  + [s + (g,) for s in ((33, 65, 3, 2, 3), (300, 2400, 130, 2, 65536)) for g in (0, 1, 3, 33, 65536)])      # ... and n_groups
NMS_SIZES = [(0, 1), (1, 1), (16, 1), (17, 2), (64, 1), (65, 3), (256, 1), (257, 4), (700, 5)]                      # (n, n_images)
TRACKS_N = [0, 1, 63, 64, 65, 2047, 2048, 4097, 70000, 3000000]             # the last one has "huge" components above N / 1024 nodes
PAIRS_SIZES = [((0, 0), 32), ((1, 2), 32), ((32, 32), 64), ((33, 31, 64), 96), ((128, 128), 128), ((100, 0, 257, 64, 31), 256), ((512,) * 9, 512)]      # (m_i, D)
GUIDED_SIZES = [[(1, 1, False)], [(2, 2, True)], [(63, 65, False), (64, 64, True)], [(257, 4097, True), (700, 650, False)]]      # (n0, n1, mutual) per pair


def _resect_cams(n_k):
    rec = np.zeros((len(n_k), hip.RESECT_CAMERA_WORDS))
    rec[:, 5] = n_k
    return rec


def aux_layouts():
    """Everything the nine layout and size functions of gims_amd.hip return over the lists above."""
    out = {f"triangulate/{s}": hip.triangulate_out_layout(*s) for s in TRI_SIZES}
    out.update({f"resect/{s}": hip.resect_out_layout(_resect_cams(s[0]), s[1]) for s in RESECT_SIZES})
    out.update({f"ba/{s}": hip.ba_out_layout(*s) for s in BA_SIZES})
    out.update({f"ba_pcg/{s}": hip.ba_pcg_out_layout(*s) for s in BA_PCG_SIZES})
    out.update({f"ba_focal/{s}": hip.ba_focal_out_layout(*s) for s in BA_FOCAL_SIZES})
    out.update({f"nms/{s}": hip.diou_nms_workspace_bytes(*s) for s in NMS_SIZES})
    out.update({f"tracks/{n}": hip.tracks_work_bytes(3, 4, n) for n in TRACKS_N})
    out.update({f"pairs/{s}": hip.pairs_work_bytes(list(s[0]), s[1]) for s in PAIRS_SIZES})
    for flags in (0, hip.NN_EXHAUSTIVE):
        out.update({f"guided/{flags}/{s}": hip.guided_layout(s, flags) for s in GUIDED_SIZES})
    return out


# Recorded from the commit BEFORE gims_aux_layout existed, whose Python functions summed the header's formulas by hand (aux_layouts() run on
# that commit's gims_amd/hip.py), never from the code under test.
AUX_EXPECTED = {
    'triangulate/(0, 0)': {'xyz': 0, 'max_angle': 0, 'rms_error': 0, 'n_inliers': 0, 'obs_error': 0, 'status': 0, 'obs_inlier': 0, 'counters': 0, 'outputs': 256, 'scratch': 256, 'bytes': 512},
    'triangulate/(1, 2)': {'xyz': 0, 'max_angle': 256, 'rms_error': 512, 'n_inliers': 768, 'obs_error': 1024, 'status': 1280, 'obs_inlier': 1536, 'counters': 1792, 'outputs': 2048, 'scratch': 2048, 'bytes': 2816},
    'triangulate/(32, 64)': {'xyz': 0, 'max_angle': 768, 'rms_error': 1024, 'n_inliers': 1280, 'obs_error': 1536, 'status': 1792, 'obs_inlier': 2048, 'counters': 2304, 'outputs': 2560, 'scratch': 2560, 'bytes': 3328},
    'triangulate/(33, 65)': {'xyz': 0, 'max_angle': 1024, 'rms_error': 1280, 'n_inliers': 1536, 'obs_error': 1792, 'status': 2304, 'obs_inlier': 2560, 'counters': 2816, 'outputs': 3072, 'scratch': 3072, 'bytes': 3840},
    'triangulate/(64, 256)': {'xyz': 0, 'max_angle': 1536, 'rms_error': 1792, 'n_inliers': 2048, 'obs_error': 2304, 'status': 3328, 'obs_inlier': 3584, 'counters': 3840, 'outputs': 4096, 'scratch': 4096, 'bytes': 4864},
    'triangulate/(65, 257)': {'xyz': 0, 'max_angle': 1792, 'rms_error': 2304, 'n_inliers': 2816, 'obs_error': 3328, 'status': 4608, 'obs_inlier': 4864, 'counters': 5376, 'outputs': 5632, 'scratch': 5632, 'bytes': 6912},
    'triangulate/(257, 1300)': {'xyz': 0, 'max_angle': 6400, 'rms_error': 7680, 'n_inliers': 8960, 'obs_error': 10240, 'status': 15616, 'obs_inlier': 16128, 'counters': 17664, 'outputs': 17920, 'scratch': 17920, 'bytes': 20736},
    'triangulate/(300, 2400)': {'xyz': 0, 'max_angle': 7424, 'rms_error': 8704, 'n_inliers': 9984, 'obs_error': 11264, 'status': 20992, 'obs_inlier': 21504, 'counters': 24064, 'outputs': 24320, 'scratch': 24320, 'bytes': 27136},
    'resect/((), 0)': {'pose': 0, 'n_corr': 0, 'ok': 0, 'n_inliers': 0, 'best_hyp': 0, 'best_hyp_inliers': 0, 'lo_rounds': 0, 'rms_error': 0, 'kp_inlier': 0, 'kp_error': 0, 'counters': 0, 'outputs': 256, 'scratch': 256, 'bytes': 256, 'slots': [0]},
    'resect/((2,), 1)': {'pose': 0, 'n_corr': 256, 'ok': 512, 'n_inliers': 768, 'best_hyp': 1024, 'best_hyp_inliers': 1280, 'lo_rounds': 1536, 'rms_error': 1792, 'kp_inlier': 2048, 'kp_error': 2304, 'counters': 2560, 'outputs': 2816, 'scratch': 2816, 'bytes': 3584, 'slots': [0, 2]},
    'resect/((100, 156), 64)': {'pose': 0, 'n_corr': 256, 'ok': 512, 'n_inliers': 768, 'best_hyp': 1024, 'best_hyp_inliers': 1280, 'lo_rounds': 1536, 'rms_error': 1792, 'kp_inlier': 2048, 'kp_error': 2304, 'counters': 3328, 'outputs': 3584, 'scratch': 3584, 'bytes': 16640, 'slots': [0, 100, 256]},
    'resect/((100, 157), 65)': {'pose': 0, 'n_corr': 256, 'ok': 512, 'n_inliers': 768, 'best_hyp': 1024, 'best_hyp_inliers': 1280, 'lo_rounds': 1536, 'rms_error': 1792, 'kp_inlier': 2048, 'kp_error': 2560, 'counters': 3840, 'outputs': 4096, 'scratch': 4096, 'bytes': 17664, 'slots': [0, 100, 257]},
    'resect/((4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4), 1)': {'pose': 0, 'n_corr': 6144, 'ok': 6400, 'n_inliers': 6656, 'best_hyp': 6912, 'best_hyp_inliers': 7168, 'lo_rounds': 7424, 'rms_error': 7680, 'kp_inlier': 7936, 'kp_error': 8192, 'counters': 9216, 'outputs': 9472, 'scratch': 9472, 'bytes': 25600, 'slots': [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52, 56, 60, 64, 68, 72, 76, 80, 84, 88, 92, 96, 100, 104, 108, 112, 116, 120, 124, 128, 132, 136, 140, 144, 148, 152, 156, 160, 164, 168, 172, 176, 180, 184, 188, 192, 196, 200, 204, 208, 212, 216, 220, 224, 228, 232, 236, 240, 244, 248, 252, 256]},
    'resect/((4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4), 3)': {'pose': 0, 'n_corr': 6400, 'ok': 6912, 'n_inliers': 7424, 'best_hyp': 7936, 'best_hyp_inliers': 8448, 'lo_rounds': 8960, 'rms_error': 9472, 'kp_inlier': 9984, 'kp_error': 10496, 'counters': 11776, 'outputs': 12032, 'scratch': 12032, 'bytes': 29440, 'slots': [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52, 56, 60, 64, 68, 72, 76, 80, 84, 88, 92, 96, 100, 104, 108, 112, 116, 120, 124, 128, 132, 136, 140, 144, 148, 152, 156, 160, 164, 168, 172, 176, 180, 184, 188, 192, 196, 200, 204, 208, 212, 216, 220, 224, 228, 232, 236, 240, 244, 248, 252, 256, 260]},
    'resect/((700, 0, 650), 1024)': {'pose': 0, 'n_corr': 512, 'ok': 768, 'n_inliers': 1024, 'best_hyp': 1280, 'best_hyp_inliers': 1536, 'lo_rounds': 1792, 'rms_error': 2048, 'kp_inlier': 2304, 'kp_error': 3840, 'counters': 9472, 'outputs': 9728, 'scratch': 9728, 'bytes': 87296, 'slots': [0, 700, 700, 1350]},
    'ba/(0, 0, 0, 0, 0)': {'xyz': 0, 'cams': 0, 'obs_error': 0, 'cam_obs': 0, 'history': 0, 'taken': 256, 'counters': 256, 'outputs': 512, 'scratch': 512, 'bytes': 1024},
    'ba/(1, 2, 2, 1, 1)': {'xyz': 0, 'cams': 256, 'obs_error': 768, 'cam_obs': 1024, 'history': 1280, 'taken': 1536, 'counters': 1792, 'outputs': 2048, 'scratch': 2048, 'bytes': 8192},
    'ba/(32, 64, 3, 2, 2)': {'xyz': 0, 'cams': 768, 'obs_error': 1280, 'cam_obs': 1536, 'history': 1792, 'taken': 2048, 'counters': 2304, 'outputs': 2560, 'scratch': 2560, 'bytes': 36608},
    'ba/(33, 65, 3, 2, 3)': {'xyz': 0, 'cams': 1024, 'obs_error': 1536, 'cam_obs': 2048, 'history': 2304, 'taken': 2560, 'counters': 2816, 'outputs': 3072, 'scratch': 3072, 'bytes': 41216},
    'ba/(257, 1300, 7, 20, 5)': {'xyz': 0, 'cams': 6400, 'obs_error': 7424, 'cam_obs': 12800, 'history': 13056, 'taken': 13568, 'counters': 13824, 'outputs': 14080, 'scratch': 14080, 'bytes': 600576},
    'ba/(300, 2400, 130, 2, 128)': {'xyz': 0, 'cams': 7424, 'obs_error': 26368, 'cam_obs': 36096, 'history': 36864, 'taken': 37120, 'counters': 37376, 'outputs': 37632, 'scratch': 37632, 'bytes': 5827584},
    'ba_pcg/(0, 0, 0, 0, 0)': {'xyz': 0, 'cams': 0, 'obs_error': 0, 'cam_obs': 0, 'history': 0, 'taken': 256, 'counters': 256, 'cg_used': 512, 'cg_res': 512, 'outputs': 512, 'scratch': 512, 'bytes': 1024},
    'ba_pcg/(1, 2, 2, 1, 1)': {'xyz': 0, 'cams': 256, 'obs_error': 768, 'cam_obs': 1024, 'history': 1280, 'taken': 1536, 'counters': 1792, 'cg_used': 2048, 'cg_res': 2304, 'outputs': 2560, 'scratch': 2560, 'bytes': 9984},
    'ba_pcg/(32, 64, 3, 2, 2)': {'xyz': 0, 'cams': 768, 'obs_error': 1280, 'cam_obs': 1536, 'history': 1792, 'taken': 2048, 'counters': 2304, 'cg_used': 2560, 'cg_res': 2816, 'outputs': 3072, 'scratch': 3072, 'bytes': 38400},
    'ba_pcg/(33, 65, 3, 2, 3)': {'xyz': 0, 'cams': 1024, 'obs_error': 1536, 'cam_obs': 2048, 'history': 2304, 'taken': 2560, 'counters': 2816, 'cg_used': 3072, 'cg_res': 3328, 'outputs': 3584, 'scratch': 3584, 'bytes': 41728},
    'ba_pcg/(257, 1300, 7, 20, 5)': {'xyz': 0, 'cams': 6400, 'obs_error': 7424, 'cam_obs': 12800, 'history': 13056, 'taken': 13568, 'counters': 13824, 'cg_used': 14080, 'cg_res': 14336, 'outputs': 14592, 'scratch': 14592, 'bytes': 597760},
    'ba_pcg/(300, 2400, 130, 2, 128)': {'xyz': 0, 'cams': 7424, 'obs_error': 26368, 'cam_obs': 36096, 'history': 36864, 'taken': 37120, 'counters': 37376, 'cg_used': 37632, 'cg_res': 37888, 'outputs': 38144, 'scratch': 38144, 'bytes': 1175296},
    'ba_pcg/(300, 2400, 130, 2, 65536)': {'xyz': 0, 'cams': 7424, 'obs_error': 26368, 'cam_obs': 36096, 'history': 36864, 'taken': 37120, 'counters': 37376, 'cg_used': 37632, 'cg_res': 37888, 'outputs': 38144, 'scratch': 38144, 'bytes': 39896832},
    'ba_focal/(0, 0, 0, 0, 0, 0)': {'xyz': 0, 'cams': 0, 'obs_error': 0, 'cam_obs': 0, 'history': 0, 'taken': 256, 'counters': 256, 'cg_used': 512, 'cg_res': 512, 'focal_scale': 512, 'group_obs': 512, 'outputs': 512, 'scratch': 512, 'bytes': 1280},
    'ba_focal/(1, 2, 2, 1, 1, 1)': {'xyz': 0, 'cams': 256, 'obs_error': 768, 'cam_obs': 1024, 'history': 1280, 'taken': 1536, 'counters': 1792, 'cg_used': 2048, 'cg_res': 2304, 'focal_scale': 2560, 'group_obs': 2816, 'outputs': 3072, 'scratch': 3072, 'bytes': 14592},
    'ba_focal/(32, 64, 3, 2, 2, 32)': {'xyz': 0, 'cams': 768, 'obs_error': 1280, 'cam_obs': 1536, 'history': 1792, 'taken': 2048, 'counters': 2304, 'cg_used': 2560, 'cg_res': 2816, 'focal_scale': 3072, 'group_obs': 3328, 'outputs': 3584, 'scratch': 3584, 'bytes': 47104},
    'ba_focal/(257, 1300, 7, 20, 5, 64)': {'xyz': 0, 'cams': 6400, 'obs_error': 7424, 'cam_obs': 12800, 'history': 13056, 'taken': 13568, 'counters': 13824, 'cg_used': 14080, 'cg_res': 14336, 'focal_scale': 14592, 'group_obs': 15104, 'outputs': 15360, 'scratch': 15360, 'bytes': 688128},
    'ba_focal/(300, 2400, 130, 2, 128, 65)': {'xyz': 0, 'cams': 7424, 'obs_error': 26368, 'cam_obs': 36096, 'history': 36864, 'taken': 37120, 'counters': 37376, 'cg_used': 37632, 'cg_res': 37888, 'focal_scale': 38144, 'group_obs': 38912, 'outputs': 39424, 'scratch': 39424, 'bytes': 1352704},
    'ba_focal/(33, 65, 3, 2, 3, 0)': {'xyz': 0, 'cams': 1024, 'obs_error': 1536, 'cam_obs': 2048, 'history': 2304, 'taken': 2560, 'counters': 2816, 'cg_used': 3072, 'cg_res': 3328, 'focal_scale': 3584, 'group_obs': 3584, 'outputs': 3584, 'scratch': 3584, 'bytes': 47872},
    'ba_focal/(33, 65, 3, 2, 3, 1)': {'xyz': 0, 'cams': 1024, 'obs_error': 1536, 'cam_obs': 2048, 'history': 2304, 'taken': 2560, 'counters': 2816, 'cg_used': 3072, 'cg_res': 3328, 'focal_scale': 3584, 'group_obs': 3840, 'outputs': 4096, 'scratch': 4096, 'bytes': 50432},
    'ba_focal/(33, 65, 3, 2, 3, 3)': {'xyz': 0, 'cams': 1024, 'obs_error': 1536, 'cam_obs': 2048, 'history': 2304, 'taken': 2560, 'counters': 2816, 'cg_used': 3072, 'cg_res': 3328, 'focal_scale': 3584, 'group_obs': 3840, 'outputs': 4096, 'scratch': 4096, 'bytes': 50432},
    'ba_focal/(33, 65, 3, 2, 3, 33)': {'xyz': 0, 'cams': 1024, 'obs_error': 1536, 'cam_obs': 2048, 'history': 2304, 'taken': 2560, 'counters': 2816, 'cg_used': 3072, 'cg_res': 3328, 'focal_scale': 3584, 'group_obs': 4096, 'outputs': 4352, 'scratch': 4352, 'bytes': 52736},
    'ba_focal/(33, 65, 3, 2, 3, 65536)': {'xyz': 0, 'cams': 1024, 'obs_error': 1536, 'cam_obs': 2048, 'history': 2304, 'taken': 2560, 'counters': 2816, 'cg_used': 3072, 'cg_res': 3328, 'focal_scale': 3584, 'group_obs': 527872, 'outputs': 790016, 'scratch': 790016, 'bytes': 5552896},
    'ba_focal/(300, 2400, 130, 2, 65536, 0)': {'xyz': 0, 'cams': 7424, 'obs_error': 26368, 'cam_obs': 36096, 'history': 36864, 'taken': 37120, 'counters': 37376, 'cg_used': 37632, 'cg_res': 37888, 'focal_scale': 38144, 'group_obs': 38144, 'outputs': 38144, 'scratch': 38144, 'bytes': 42420992},
    'ba_focal/(300, 2400, 130, 2, 65536, 1)': {'xyz': 0, 'cams': 7424, 'obs_error': 26368, 'cam_obs': 36096, 'history': 36864, 'taken': 37120, 'counters': 37376, 'cg_used': 37632, 'cg_res': 37888, 'focal_scale': 38144, 'group_obs': 38400, 'outputs': 38656, 'scratch': 38656, 'bytes': 42423552},
    'ba_focal/(300, 2400, 130, 2, 65536, 3)': {'xyz': 0, 'cams': 7424, 'obs_error': 26368, 'cam_obs': 36096, 'history': 36864, 'taken': 37120, 'counters': 37376, 'cg_used': 37632, 'cg_res': 37888, 'focal_scale': 38144, 'group_obs': 38400, 'outputs': 38656, 'scratch': 38656, 'bytes': 42423552},
    'ba_focal/(300, 2400, 130, 2, 65536, 33)': {'xyz': 0, 'cams': 7424, 'obs_error': 26368, 'cam_obs': 36096, 'history': 36864, 'taken': 37120, 'counters': 37376, 'cg_used': 37632, 'cg_res': 37888, 'focal_scale': 38144, 'group_obs': 38656, 'outputs': 38912, 'scratch': 38912, 'bytes': 42425856},
    'ba_focal/(300, 2400, 130, 2, 65536, 65536)': {'xyz': 0, 'cams': 7424, 'obs_error': 26368, 'cam_obs': 36096, 'history': 36864, 'taken': 37120, 'counters': 37376, 'cg_used': 37632, 'cg_res': 37888, 'focal_scale': 38144, 'group_obs': 562432, 'outputs': 824576, 'scratch': 824576, 'bytes': 47926016},
    'nms/(0, 1)': 256,
    'nms/(1, 1)': 2048,
    'nms/(16, 1)': 2048,
    'nms/(17, 2)': 2816,
    'nms/(64, 1)': 3840,
    'nms/(65, 3)': 5888,
    'nms/(256, 1)': 13824,
    'nms/(257, 4)': 16384,
    'nms/(700, 5)': 38656,
    'tracks/0': 768,
    'tracks/1': 3840,
    'tracks/63': 3840,
    'tracks/64': 3840,
    'tracks/65': 6912,
    'tracks/2047': 99072,
    'tracks/2048': 99072,
    'tracks/4097': 200448,
    'tracks/70000': 3371008,
    'tracks/3000000': 150006784,
    'pairs/((0, 0), 32)': 6144,
    'pairs/((1, 2), 32)': 6144,
    'pairs/((32, 32), 64)': 10240,
    'pairs/((33, 31, 64), 96)': 35328,
    'pairs/((128, 128), 128)': 35328,
    'pairs/((100, 0, 257, 64, 31), 256)': 134912,
    'pairs/((512, 512, 512, 512, 512, 512, 512, 512, 512), 512)': 2380288,
    'guided/0/[(1, 1, False)]': {'bytes': 4608, 'csplit': [1], 'items': 1},
    'guided/0/[(2, 2, True)]': {'bytes': 6656, 'csplit': [1, 1], 'items': 2},
    'guided/0/[(63, 65, False), (64, 64, True)]': {'bytes': 44800, 'csplit': [1, 1, 1], 'items': 3},
    'guided/0/[(257, 4097, True), (700, 650, False)]': {'bytes': 2981120, 'csplit': [7, 3, 6], 'items': 156},
    'guided/1/[(1, 1, False)]': {'bytes': 3840, 'csplit': [1], 'items': 1},
    'guided/1/[(2, 2, True)]': {'bytes': 5120, 'csplit': [1, 1], 'items': 2},
    'guided/1/[(63, 65, False), (64, 64, True)]': {'bytes': 17152, 'csplit': [1, 1, 1], 'items': 3},
    'guided/1/[(257, 4097, True), (700, 650, False)]': {'bytes': 346624, 'csplit': [7, 3, 6], 'items': 156},
}


def test_aux_layouts_are_what_the_hand_summed_formulas_returned():
    got = aux_layouts()
    assert sorted(got) == sorted(AUX_EXPECTED)
    for key in AUX_EXPECTED:
        assert got[key] == AUX_EXPECTED[key], (key, got[key], AUX_EXPECTED[key])


def _guided_sizes(pairs, flags=0):
    return [flags, len(pairs)] + [int(v) for p in pairs for v in p]


def query_cases():
    """(fn, sizes as gims_aux_layout takes them) over the lists above."""
    cases = [(hip.AUX_TRIANGULATE_TRACKS, list(s)) for s in TRI_SIZES]
    cases += [(hip.AUX_RESECT_IMAGES, [len(n_k), sum(n_k), iters]) for n_k, iters in RESECT_SIZES]
    cases += [(hip.AUX_BUNDLE_ADJUST, list(s)) for s in BA_SIZES] + [(hip.AUX_BUNDLE_ADJUST_PCG, list(s)) for s in BA_PCG_SIZES]
    cases += [(hip.AUX_BUNDLE_ADJUST_FOCAL, list(s)) for s in BA_FOCAL_SIZES]
    cases += [(hip.AUX_DIOU_NMS, list(s)) for s in NMS_SIZES] + [(hip.AUX_BUILD_TRACKS, [n]) for n in TRACKS_N]
    cases += [(hip.AUX_SELECT_PAIRS, [d, len(ms), *ms]) for ms, d in PAIRS_SIZES]
    cases += [(hip.AUX_GUIDED_MATCH, _guided_sizes(s, flags)) for s in GUIDED_SIZES for flags in (0, hip.NN_EXHAUSTIVE)]
    return cases


def _query(fn, sizes, capacity=None):
    """gims_aux_layout itself -> (rc, offsets or None, n_regions, n_outputs, bytes); capacity None: the counts-only form (NULL, 0)."""
    lib = hip.load()
    arr = (C.c_int64 * max(len(sizes), 1))(*sizes)
    nr, no, nb = C.c_int32(-1), C.c_int32(-1), C.c_size_t(0)
    offs = None if capacity is None else (C.c_int64 * max(capacity, 1))()
    rc = lib.gims_aux_layout(fn, arr, len(sizes), offs, capacity or 0, C.byref(nr), C.byref(no), C.byref(nb))
    return rc, (None if offs is None else list(offs[:max(nr.value, 0)])), nr.value, no.value, nb.value


def test_aux_layout_offsets_ascend_on_256_bytes_and_end_at_bytes():
    has_outputs = set(hip._AUX_REGIONS)
    for fn, sizes in query_cases():
        rc, _, n_regions, n_outputs, total = _query(fn, sizes)
        assert rc == hip.GIMS_OK and n_regions > 0, (fn, sizes, hip.load().gims_last_error())
        assert (_query(fn, sizes, n_regions)[0], *_query(fn, sizes, n_regions)[2:]) == (hip.GIMS_OK, n_regions, n_outputs, total)      # the two forms agree
        offsets = _query(fn, sizes, n_regions)[1]
        assert offsets[0] == 0 and all(o % 256 == 0 for o in offsets) and offsets == sorted(offsets) and total % 256 == 0 and total >= offsets[-1]
        assert 0 <= n_outputs <= n_regions and (n_outputs > 0) == (fn in has_outputs), (fn, n_outputs)
        assert hip._aux_layout(fn, sizes) == (offsets, n_outputs, total)
    # bytes = the last offset + the last extent, where the last take's size is known: n_list int32 [2], rowoff int32 [N], n_huge int32 [1]
    for fn, sizes, last in ((hip.AUX_TRIANGULATE_TRACKS, [257, 1300], 256), (hip.AUX_SELECT_PAIRS, [96, 3, 33, 31, 64], 256), (hip.AUX_BUILD_TRACKS, [4097], 256),
                            (hip.AUX_SELECT_PAIRS, [32, 65, *[1] * 65], 512), (hip.AUX_RESECT_IMAGES, [3, 10, 100], 1280), (hip.AUX_BUNDLE_ADJUST, [1, 2, 2, 1, 33], 1792)):
        _, offsets, n_regions, _, total = _query(fn, sizes, 64)
        assert total == offsets[-1] + last, (fn, sizes, total, offsets[-1])


# (fn, good sizes, index of a size with an upper bound, a value above it)
AUX_BOUNDS = [(hip.AUX_TRIANGULATE_TRACKS, [5, 9], 0, 2 ** 30 + 1), (hip.AUX_RESECT_IMAGES, [2, 9, 4], 0, 2 ** 24 + 1), (hip.AUX_RESECT_IMAGES, [2, 9, 4], 2, 65536),
              (hip.AUX_BUNDLE_ADJUST, [5, 9, 3, 2, 2], 4, 129), (hip.AUX_BUNDLE_ADJUST_PCG, [5, 9, 3, 2, 2], 4, 65537),
              (hip.AUX_BUNDLE_ADJUST_FOCAL, [5, 9, 3, 2, 2, 1], 3, 256), (hip.AUX_DIOU_NMS, [5, 2], 0, 2 ** 29 + 1), (hip.AUX_BUILD_TRACKS, [5], 0, 2 ** 30 + 1),
              (hip.AUX_SELECT_PAIRS, [64, 2, 5, 6], 0, 1056), (hip.AUX_SELECT_PAIRS, [64, 2, 5, 6], 3, 4097), (hip.AUX_GUIDED_MATCH, [0, 1, 5, 6, 1], 2, 32769)]


def _refused(fn, sizes, capacity=None):
    rc, _, _, _, _ = _query(fn, sizes, capacity)
    msg = (hip.load().gims_last_error() or b"").decode()
    assert rc == hip.GIMS_EINVAL and "gims_aux_layout" in msg, (fn, sizes, rc, msg)
    return msg


@pytest.mark.parametrize("fn, sizes, k, above", AUX_BOUNDS)
def test_aux_layout_refuses_sizes_the_op_refuses(fn, sizes, k, above):
    assert _query(fn, sizes)[0] == hip.GIMS_OK
    _refused(fn, sizes + [0])                                   # a wrong n_sizes
    _refused(fn, sizes[:-1])
    _refused(fn, sizes[:-1] + [-1])                             # a negative size (the last one: n_obs, iters, n_free, n_groups, n_images, N, m, mutual)
    assert str(above) in _refused(fn, sizes[:k] + [above] + sizes[k + 1:])
    n_regions = _query(fn, sizes)[2]
    assert str(n_regions) in _refused(fn, sizes, n_regions - 1)      # a capacity one too small


@pytest.mark.parametrize("fn", [hip.AUX_SIFT_DESCRIBE, hip.AUX_ASSEMBLE_ROWS, 12, 15, 99, -1])
def test_aux_layout_refuses_functions_without_such_a_buffer(fn):
    assert str(fn) in _refused(fn, [1, 1])


@pytest.mark.parametrize("name, dtype, shape", [("xyz", None, (11, 3)), ("cams", "float32", None), ("taken", None, (0,)), ("counters", None, (65,))])
def test_a_region_table_that_drifts_from_the_layout_routine_raises(monkeypatch, name, dtype, shape):
    """The Python tables name and type the output regions; the extents are the library's.  One perturbed entry is an exception where the
    buffer would be sized, naming the region and both byte counts."""
    import torch
    sizes = (5, 9, 3, 2, 2)
    good = hip._ba_regions(*sizes)
    assert hip.ba_out_layout(*sizes)["bytes"] > 0
    bad = tuple((n, getattr(torch, dtype) if dtype and n == name else dt, shape if shape and n == name else sh) for n, dt, sh in good)
    monkeypatch.setitem(hip._AUX_REGIONS, hip.AUX_BUNDLE_ADJUST, lambda *s: bad)
    with pytest.raises(hip.GimsHipError, match=rf"region {name}: \d+ bytes in the library's layout, \d+ for"):
        hip.ba_out_layout(*sizes)
    monkeypatch.setitem(hip._AUX_REGIONS, hip.AUX_BUNDLE_ADJUST, lambda *s: good[:-1])
    with pytest.raises(hip.GimsHipError, match="7 output regions"):
        hip.ba_views(None, *sizes)
