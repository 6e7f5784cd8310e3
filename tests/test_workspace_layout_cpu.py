"""Scratch workspaces, the parts that need no GPU.  Every batched entry point sizes and carves its workspace with one layout routine
(csrc/common.h: WsLayout); this file pins what the size queries return and checks that a workspace one byte short is refused before any
device call.

EXPECTED was recorded from a build of the commit BEFORE the layout routines were shared (its library loaded through hip.load(path) and run
through queries() below), never from the code under test: a layout edit that changes a size has to change a literal here on purpose.
The Sinkhorn rows are taken with GIMS_OT_RESIDENT=0 (read per call), which makes them independent of whether a device is present."""
import ctypes as C
import os

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
