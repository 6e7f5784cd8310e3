"""CPU-only tests: the C-ABI library loads and exports every symbol include/gims_hip.h declares, the host
mirror keeps the reference's interface (state-dict names, config keys, checkpoint layouts, error behaviour).
No compute call is made here (there is no GPU in the build container)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from gims_amd import GMatcher, Matching, hip, synth
from gims_amd.attention_tiers import AttentionTiers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "gims_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gims_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 20
    assert declared == set(hip.EXPORTS), declared ^ set(hip.EXPORTS)
    assert len(hip.EXPORTS) == 90 and len(hip.ABI.structs) == 28          # at this commit: a parser that drops a declaration fails here
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    assert hip.load().gims_abi_version() == hip.ABI_VERSION == 5


def test_library_defines_no_entry_point_the_header_does_not_declare():
    """The unmangled dynamic symbols of the library that start with gims_ are exactly the header's prototypes: an entry point left behind
    without a declaration (a forwarder, an old spelling) fails here."""
    import subprocess
    nm = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], check=True, capture_output=True, text=True).stdout
    defined = {line.split()[-1] for line in nm.splitlines() if line.split() and line.split()[-1].startswith("gims_")}
    assert defined == set(hip.ABI.signatures), defined ^ set(hip.ABI.signatures)


def _gcc(tmp_path, code, run=True):
    """Compile C code that includes the header (gcc, LP64); run=True: link, run it and return its "key value" output lines as a dict."""
    import subprocess
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gims_hip.h"\n' + code)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)] + ([] if run else ["-c"]), check=True)
    if run:
        return dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())


def _layout(c_name, cls, path="", base=0):
    """{C expression: value} of the offset and the size of every field of a ctypes class; the members of a union by their member path."""
    out = {}
    for f, t in cls._fields_:
        d = getattr(cls, f)
        out[f"offsetof({c_name}, {path}{f})"] = base + d.offset
        out[f"sizeof((({c_name}*)0)->{path}{f})"] = d.size
        if issubclass(t, ctypes.Union):
            out.update(_layout(c_name, t, f"{path}{f}.", base + d.offset))
    return out


def _check_layouts(tmp_path, structs):
    """sizeof of every struct in {C name: ctypes class}, and offset and size of every field, against a gcc-compiled program."""
    want = {}
    for c_name, cls in structs.items():
        want[f"sizeof({c_name})"] = ctypes.sizeof(cls)
        want.update(_layout(c_name, cls))
    got = _gcc(tmp_path, "int main(void) {\n" + "".join('printf("%s %%zu\\n", (size_t)%s);\n' % (e, e) for e in want) + "return 0; }\n")
    assert {e: int(v) for e, v in got.items()} == want
    return want


def test_struct_layouts_match_header(tmp_path):
    """Size of every struct the binding derives from include/gims_hip.h, and offset and size of every field, against what a C compiler
    makes of the header (gcc, LP64)."""
    want = _check_layouts(tmp_path, hip.ABI.structs)
    assert "offsetof(gims_op, u.aux)" in want and "sizeof(((gims_sift_info*)0)->kernel)" in want


def test_optimizer_table_layouts_match_header(tmp_path):
    """The SGD / EMA table structs against the header (same harness), and the NumPy dtypes the optimizers build their tables with
    against those structs."""
    _check_layouts(tmp_path, {c: hip.ABI.structs[c] for c in ("gims_sgd_tensor", "gims_sgd_group", "gims_ema_tensor", "gims_adam_tensor")})
    for py, dt in ((hip.AdamTensor, hip.ADAM_TENSOR_DTYPE), (hip.SgdTensor, hip.SGD_TENSOR_DTYPE), (hip.EmaTensor, hip.EMA_TENSOR_DTYPE)):
        d = np.dtype(dt)
        assert d.itemsize == ctypes.sizeof(py) and list(d.names) == [f[0] for f in py._fields_]
        assert [d.fields[n][1] for n in d.names] == [getattr(py, n).offset for n in d.names]
    assert ctypes.sizeof(hip.SgdTensor) == 40 and ctypes.sizeof(hip.SgdGroup) == 40 and ctypes.sizeof(hip.EmaTensor) == 24
    assert hip.load().gims_abi_version() == 5


def test_prototypes_and_scalar_types_match_the_compiler(tmp_path):
    """Every prototype the binding read from the header, rebuilt from the parsed type text, is the type gcc gives the function; every C
    scalar has the size and the signedness of the ctypes type it is mapped to."""
    from gims_amd import _abi
    assert set(hip.ABI.c_types) == set(hip.ABI.signatures) == set(hip.EXPORTS)
    code = ""
    for name, (ret, args) in hip.ABI.c_types.items():
        assert len(args) == len(hip.ABI.signatures[name][1])
        code += '_Static_assert(__builtin_types_compatible_p(__typeof__(&%s), %s (*)(%s)), "%s");\n' % (name, ret, ", ".join(args) or "void", name)
    for c, py in _abi.SCALARS.items():
        code += '_Static_assert(sizeof(%s) == %d, "sizeof(%s)");\n' % (c, ctypes.sizeof(py), c)
        code += '_Static_assert(((%s)-1 < 0) == %d, "signedness of %s");\n' % (c, py(-1).value < 0, c)
    _gcc(tmp_path, code, run=False)


def test_constants_equal_the_header():
    """Every `#define GIMS_X <integer>` of the header that the binding has a name for (hip.X, or hip.GIMS_X for the error codes)."""
    checked = 0
    for name, value in hip.ABI.constants.items():
        for py in (name, name[len("GIMS_"):]):
            if hasattr(hip, py) and name != "GIMS_ATTN_KERNEL_KINDS":
                assert getattr(hip, py) == value and isinstance(getattr(hip, py), int), name
                checked += 1
    assert checked >= 41                                                     # the names the binding had when the mirrors were hand-written, minus the removed gather-mode flag of gims_linear
    assert len(hip.ATTN_KERNEL_KINDS) == hip.ABI.constants["GIMS_ATTN_KERNEL_KINDS"] == 6


def test_header_parser_rejects_what_it_cannot_read():
    """An unknown type, a missing ';': the parser raises and names the text, never skips."""
    from gims_amd import _abi
    good = "#define GIMS_N 4\ntypedef struct gims_t { int32_t a, b[GIMS_N + 1]; const float* p; } gims_t;\nint gims_f(const gims_t* t, void* stream);\n"
    abi = _abi.parse_text(good)
    assert ctypes.sizeof(abi.structs["gims_t"]) == 32 and abi.signatures["gims_f"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p])
    for bad, named in (("int gims_g(wchar_t x);\n", "wchar_t"), ("int gims_g(const wchar_t* x);\n", "wchar_t"), ("int gims_g(int32_t a)\nint gims_h(void);\n", "gims_g(int32_t a)"),
                       ("typedef struct gims_u { unsigned long a; } gims_u;\n", "unsigned long a"), ("typedef struct gims_u { int32_t a; int32_t b } gims_u;\n", "int32_t b"),
                       ("typedef struct gims_u { int32_t a; } gims_u\n", "typedef struct gims_u"), ("#define GIMS_S \"text\"\n", "text"),
                       ("int gims_g(int32_t);\n", "gims_g")):
        with pytest.raises(hip.GimsHipError, match="line [34]: .*" + re.escape(named)):
            _abi.parse_text(good + bad)
    with pytest.raises(hip.GimsHipError, match="nowhere.h"):
        _abi.parse("/nowhere.h")


def test_pyramid_layout_equals_the_reference_schedule(golden_dir):
    """gims_pyramid_layout (host arithmetic only): number of levels and every level's size, against what the reference's
    buildGaussianPyramid produced for the same image sizes (tests/golden/patch_pyramid_calls.npz, tools/gen_golden_patches.py)."""
    import numpy as np
    g = np.load(os.path.join(golden_dir, "patch_pyramid_calls.npz"))
    for (h, w) in g["shapes"]:
        levels, _, _ = hip.pyramid_layout(int(h), int(w), 3)
        assert len(levels) == int(g[f"{h}x{w}/n_levels"])
        assert [[L.h, L.w] for L in levels] == g[f"{h}x{w}/level_shapes"].tolist()


def test_missing_library_fails_loudly(tmp_path):
    with pytest.raises(hip.GimsHipError):
        hip.load(str(tmp_path / "nope.so"))


def test_state_dict_names_and_checkpoint_layouts(tmp_path, synth_sd):
    m = GMatcher({})
    names = list(m.state_dict().keys())
    assert len(names) == 348 and "bin_score" in names
    assert "gnn.layers.17.attn.proj.2.weight" in names and "kenc.encoder.12.bias" in names
    assert "gnn_encoder.layers.0.fc_neigh.weight" in names and "gnn.layers.0.mlp.1.running_var" in names
    assert set(names) == set(synth_sd.keys())
    sd_t = {k: torch.from_numpy(np.asarray(v)) for k, v in synth_sd.items()}
    for layout in ("raw", "model", "ema", "module."):
        blob = {"raw": sd_t, "model": {"model": sd_t, "ema": None}, "ema": {"ema": sd_t, "model": {}},
                "module.": {"module." + k: v for k, v in sd_t.items()}}[layout]
        p = tmp_path / f"{layout}.pt"
        torch.save(blob, p)
        mm = GMatcher({"weights_path": str(p)})
        assert torch.equal(mm.state_dict()["final_proj.weight"], sd_t["final_proj.weight"])
    # older-DGL SAGEConv bias layout
    old = dict(synth.make_state_dict(123, sage_bias_layout="bias"))
    assert "gnn_encoder.layers.0.bias" in old
    mm = GMatcher({})
    mm.load_state_dict(old)
    assert torch.equal(mm.state_dict()["gnn_encoder.layers.1.fc_self.bias"], torch.from_numpy(old["gnn_encoder.layers.1.bias"]))


def test_default_config_keys_match_reference():
    for k, v in {"descriptor_dim": 256, "weights_path": None, "keypoint_encoder": [32, 64, 128, 256],
                 "transformer_layers": ["self", "cross"] * 9, "sinkhorn_iterations": 100, "match_threshold": 0.2,
                 "use_layernorm": False, "input_dim": 256, "num_heads": 4}.items():
        assert GMatcher.default_config[k] == v


def test_no_cpu_fallback_and_matching_shell():
    m = Matching({})
    pair = synth.make_pair(64, 1000)
    data = {k: torch.from_numpy(v) for k, v in pair.items() if k != "gt_perm"}
    with pytest.raises(hip.GimsHipError):
        m(data)
    with pytest.raises(NotImplementedError):
        m({"image0": pair["image0"], "image1": pair["image1"]})


def test_matching_front_end_hook_is_called_like_sift_forward():
    """Without keypoints, Matching calls its front end once per image with the reference's argument dict
    (models/matching.py:17-24) and feeds the stacked lists to GMatcher (which then refuses CPU tensors: no fallback)."""
    pair = synth.make_pair(64, 1000)
    calls = []

    def fake_front_end(d, device):
        calls.append((d["image"].shape, d["max_keypoints"], d["carhynet"], device))
        s = "0" if len(calls) == 1 else "1"
        return {"keypoints": [torch.from_numpy(pair["keypoints" + s][0])], "scores": [torch.from_numpy(pair["scores" + s][0])],
                "descriptors": [torch.from_numpy(pair["descriptors" + s][0])]}

    m = Matching({"front_end": fake_front_end, "max_keypoints": 77})
    with pytest.raises(hip.GimsHipError):
        m({"image0": pair["image0"], "image1": pair["image1"], "carhynet": "net", "device": "cpu"})
    assert calls == [(pair["image0"].shape, 77, "net", "cpu"), (pair["image1"].shape, 77, "net", "cpu")]
    assert "front_end" not in m.gmodel.config
    with pytest.raises(TypeError):
        Matching({"front_end": 3})


def test_product_code_never_imports_the_oracle():
    for root, _, files in os.walk(os.path.join(ROOT, "gims_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(root, f)).read()
                assert "oracle" not in src.replace("no oracle", ""), f


def test_pose_auc_and_summarize_equal_reference():
    """gims_amd.evalh.pose_auc against the reference's pose_auc outputs (tests/golden/eval_metrics.npz)."""
    from gims_amd import evalh
    from tests.helpers import load_golden
    g = load_golden("eval_metrics")
    for i in range(4):
        np.testing.assert_allclose(evalh.pose_auc(g[f"errors{i}"], [5, 10, 25]), g[f"auc{i}"], rtol=0, atol=1e-12)
    rec = np.zeros((3, 16))
    rec[:, 0] = [100, 5, 50]          # n_valid: the second pair has too few matches
    rec[:, 9] = rec[:, 10] = 1
    rec[:, 4], rec[:, 5], rec[:, 7], rec[:, 8] = [0.5, 0.1, 1.0], [0.25, 0.1, 0.75], [2.0, 1.0, 30.0], [1.0, 1.0, 3.0]
    s = evalh.summarize(rec)
    assert s["n_pairs"] == 2 and s["precision"] == 75.0 and s["recall"] == 50.0
    np.testing.assert_allclose(s["auc_ransac"], [100 * a for a in evalh.pose_auc([1.0, 3.0])], atol=1e-12)


def test_training_front_end_pads_to_max_keypoints():
    """sift_forward's is_train branch (utils/common.py:866-880): random extra size-1 keypoints up to max_keypoints, drawn with the
    reference's sequence of np.random calls."""
    from gims_amd import frontend
    kps = [frontend.PaddedKeyPoint(3.0, 4.0)]
    np.random.seed(5)
    out = frontend.pad_training_keypoints(kps, 6, (480, 640, 3))
    np.random.seed(5)
    c = np.random.random((5, 2)) * 640
    c[:, 1] = np.random.random(5) * 480
    assert len(out) == 6 and out[0] is kps[0]
    assert [k.pt for k in out[1:]] == [(float(x), float(y)) for x, y in c]
    assert all(k.size == 1.0 and k.octave == 0 and k.response == 0.0 for k in out[1:])
    assert frontend.pad_training_keypoints(kps * 7, 6, (480, 640, 3)) == kps * 7          # nothing to add
    kp4, octv, resp = frontend.keypoint_arrays(out)
    assert kp4.shape == (6, 4) and octv.tolist() == [0] * 6


def test_training_entry_points_validate_arguments_without_a_gpu():
    """Argument checks of the training-step ABI run before any HIP call: bad arguments come back as GIMS_EINVAL (-1) with a message,
    also on a machine without a GPU."""
    import ctypes as C
    lib = hip.load()
    g = hip.Gemm()                                        # all null
    assert lib.gims_gemm_f32(C.byref(g), None) == -1 and b"gims_gemm_f32" in lib.gims_last_error()
    assert lib.gims_gemm_f32(None, None) == -1
    sg = hip.Segments()
    sg.n = 0
    assert lib.gims_batchnorm_workspace_floats(C.byref(sg), 32) == 0
    assert lib.gims_batchnorm_train_forward(None, 0, 32, C.byref(sg), None, None, 1e-5, 0.1, None, None, None, None, 0, 1, None, None) == -1
    assert lib.gims_softmax_rows(None, 0, 4, 4, 1, 0, None) == -1
    assert lib.gims_colsum(None, 0, 4, 4, 0.0, None, None, None) == -1
    assert lib.gims_colsum_workspace_floats(1000, 512) == 64 + 8 * 512
    assert lib.gims_layernorm_backward(None, 0, None, 0, 4, 1, None, None, 1e-6, 1, None, 0, None, None, None) == -1
    assert lib.gims_head_pack(None, None, None, None, None, None, 256, 4, 0, None) == -1
    assert lib.gims_permute3(None, None, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, None) == -1
    assert lib.gims_sinkhorn_history_floats(10, 12, 5) == 6 * 24


def test_agc_build_takes_one_parameter_triple_or_one_per_image():
    """gims_agc_build refuses an n_params that is neither 1 nor n_images, and a null h_params, with GIMS_EINVAL and a message that names
    n_params -- before any HIP call (fake pointers, never dereferenced)."""
    import ctypes as C
    lib = hip.load()
    images = (hip.AgcImage * 5)(*[hip.AgcImage(0x10000, 0x20000, 256, n, 256, 0x30000, 0x40000, 0x50000, 64 * n, 0x60000) for n in (100, 200, 300, 400, 500)])
    params = (hip.AgcParams * 6)(*[hip.AgcParams(15.0, 2.0, 7, 0)] * 6)
    need = lib.gims_agc_workspace_bytes(images, 5, hip.AGC_ROBUST)
    for h_params, n_params in ((params, 0), (params, 2), (params, 6), (None, 5), (None, 1)):
        assert lib.gims_agc_build(images, 5, h_params, n_params, 0, 0x100000, need, None) == hip.GIMS_EINVAL
        assert b"gims_agc_build" in lib.gims_last_error() and b"n_params" in lib.gims_last_error()


def test_adam_table_layout_and_cpu_refusal():
    """gims_adam_tensor / gims_adam_group as the binding lays them out (include/gims_hip.h), and the optimizer's refusal to step CPU
    parameters (there is no CPU path)."""
    import ctypes as C
    import numpy as np
    import pytest
    import torch
    from gims_amd import hip
    from gims_amd.optim import Adam
    assert C.sizeof(hip.AdamTensor) == 48 == np.dtype(hip.ADAM_TENSOR_DTYPE).itemsize
    assert [f[0] for f in hip.AdamTensor._fields_] == list(np.dtype(hip.ADAM_TENSOR_DTYPE).names)
    assert C.sizeof(hip.AdamGroup) == 48
    p = [torch.nn.Parameter(torch.zeros(4))]
    with pytest.raises(NotImplementedError):
        Adam(p, amsgrad=True)
    with pytest.raises(ValueError):
        Adam(p, lr=-1.0)
    o = Adam(p, lr=1e-3, weight_decay=1e-4)
    assert o.param_groups[0]['betas'] == (0.9, 0.999) and o.param_groups[0]['weight_decay'] == 1e-4
    o.add_param_group({'params': [torch.nn.Parameter(torch.zeros(2))], 'weight_decay': 0.5})       # train.py:56
    assert len(o.param_groups) == 2 and o.param_groups[1]['lr'] == 1e-3
    p[0].grad = torch.ones(4)
    with pytest.raises(RuntimeError):
        o.step()


def test_hot_kernels_use_no_scratch():
    """Round 3 found the staging registers of several attention kernels living in scratch (a global-memory round trip per key tile; the split-bf16
    kernel went 1.26 -> 0.73 ms per launch once K and V took the LDS-DMA path instead).  This pins the invariant: the kernels of the hot path that are
    meant to be scratch-free compile to `ScratchSize: 0` for gfx950 (hipcc cross-compiles here; the remark comes from the register allocator)."""
    import os
    import re
    import shutil
    import subprocess
    import tempfile
    from gims_amd import build as B
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        import pytest
        pytest.skip("no hipcc")
    must_be_clean = {"attention.hip": ["attention8_bf16_kernel", "attention_bf16_kernel", "attention_x3_kernel", "attention_split_kernelILi2"],
                     "linear6.hip": ["linear_x6_kernel"], "linear.hip": ["linear_x3p_kernel"],
                     "carhynet.hip": ["ch_conv_block_kernel", "ch_sandglass_kernelILi32"]}
    with tempfile.TemporaryDirectory() as tmp:
        for src, names in must_be_clean.items():
            cmd = [hipcc, *B.FLAGS, *B.EXTRA.get(src, []), "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(B.CSRC, src), "-o", os.path.join(tmp, "x.o")]
            out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True).stdout
            cur, scratch = None, {}
            for line in out.splitlines():
                m = re.search(r"Function Name: (\S+)", line)
                if m:
                    cur = m.group(1)
                m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
                if m and cur:
                    scratch[cur] = int(m.group(1))
            for n in names:
                hits = {k: v for k, v in scratch.items() if n in k}
                assert hits, f"{src}: no kernel named like {n} in the compiler remarks"
                assert all(v == 0 for v in hits.values()), f"{src}: scratch in a hot kernel: {hits}"


def test_auto_attention_routes_on_the_tail_and_the_range():
    """The decision rule of 'auto' on hand-made statistics (no GPU work: the folding of a read-back into per-layer modes):
    a head with 5 % one-hot rows among diffuse ones has a small MEAN row maximum (0.05) but a tail fraction of 0.05 -> half;
    operands beyond `attention_f16_range` -> split-bf16; layers only move up."""
    L, H = len(GMatcher.default_config['transformer_layers']), 4
    t = AttentionTiers(L, H, 7, dict(GMatcher.default_config))

    def feed(mean, tail, rng):
        raw = np.zeros((L, H + 1, 4), dtype=np.int64)
        raw[:, :H, 1] = 1000
        raw[:, :H, 0] = np.round(np.asarray(mean) * 1000 * 2 ** 24).astype(np.int64)
        raw[:, :H, 3] = np.round(np.asarray(tail) * 1000).astype(np.int64)
        raw[:, H, :3] = np.asarray(rng, dtype=np.float32).view(np.uint32).astype(np.int64)
        t.fold(raw)
        return t.report()["modes"]

    mean, tail, rng = np.full((L, H), 0.01), np.zeros((L, H)), np.full((L, 3), 20.0)
    mean[1, 2] = 0.3                     # plainly peaked head
    mean[2, 0], tail[2, 0] = 0.05, 0.05  # small mean, fat tail
    mean[3, 1], rng[3, 1] = 0.5, 5.0e4   # peaked AND out of half's range
    rng[4, 0] = 5.0e4                    # wide operands but diffuse: bf16 has the range
    modes = feed(mean, tail, rng)
    assert modes[:5] == ["bf16", "f16", "f16", "bf16x3", "bf16"] and set(modes[5:]) == {"bf16"}
    mean2 = np.full((L, H), 0.01)        # a later, calmer measurement never moves a layer down ...
    assert feed(mean2, np.zeros((L, H)), np.full((L, 3), 20.0)) == modes
    rng3 = np.full((L, 3), 20.0); rng3[1, 2] = 4.0e4      # ... and a half layer whose operands grow goes up
    mean3 = mean2.copy(); mean3[1, 2] = 0.3
    modes3 = feed(mean3, np.zeros((L, H)), rng3)
    assert modes3[1] == "bf16x3" and t.report()["switched"] == [1]
    # the device's record of a redo (stat[H][3], set by a guarded attention launch that fired) is counted per layer
    raw = np.zeros((L, H + 1, 4), dtype=np.int64)
    raw[5, H, 3] = 1
    t.fold(raw)
    assert t.report()["redone"].tolist() == [0] * 5 + [1] + [0] * (L - 6)
    # round 6: ONE sharply peaked row inside a diffuse bf16 layer (the head's largest row maximum reaches attention_auto_rowmax = 0.5 while mean
    # and tail stay under their thresholds) is recorded as `rare` and makes forward() repeat the batch with the device-side guards -- the layer is
    # NOT moved up; the same maximum on a layer that is not on the bf16 tier means nothing
    raw = np.zeros((L, H + 1, 4), dtype=np.int64)
    raw[:, :H, 1] = 1000
    raw[:, :H, 0] = int(0.01 * 1000 * 2 ** 24)
    raw[:, H, :3] = np.asarray(np.full(3, 20.0), dtype=np.float32).view(np.uint32).astype(np.int64)
    raw[7, 3, 2] = int(0.97 * 2 ** 24)      # layer 7 (bf16 tier): a row at 0.97
    raw[1, 0, 2] = int(0.99 * 2 ** 24)      # layer 1 (split-bf16 by now): irrelevant
    before = t.report()["modes"]
    t.begin()
    assert t.fold(raw) == 0
    assert t.rare_last is True       # (speaks of the read-backs folded in since begin())
    rep = t.report()
    assert rep["modes"] == before and rep["rare"].tolist() == [0] * 7 + [1] + [0] * (L - 8)
    raw[7, 3, 2] = int(0.3 * 2 ** 24)
    t.begin()
    t.fold(raw)
    assert t.rare_last is False and t.report()["rare"].sum() == 1
    # ... but a layer that does it on attention_auto_rare_batches (3) batches is no outlier: it moves to the half tier (cheaper than a redo per batch)
    raw[7, 3, 2] = int(0.9 * 2 ** 24)
    for k in (2, 3):
        t.begin()
        moved = t.fold(raw)
        assert t.report()["rare"][7] == k and moved == (1 if k == 3 else 0)
    assert t.report()["modes"][7] == "f16" and t.report()["modes"][8] == "bf16"


def test_auto_attention_counts_an_outlier_batch_once():
    """forward() repeats a batch with an outlier row and reads that batch's statistic a second time: the repeat's read-back does not add to
    `rare` (attention_auto_rare_batches counts BATCHES, as match_pairs does), and `rare_last` -- forward()'s reason to repeat -- is False after
    any call that consumed no read-back (an unmeasured batch, attention_monitor_period > 1) instead of keeping an earlier batch's verdict."""
    L, H = len(GMatcher.default_config['transformer_layers']), 4
    t = AttentionTiers(L, H, 7, dict(GMatcher.default_config))
    t.mode, t.calibrated = [0] * L, True

    raw = np.zeros((L, H + 1, 4), dtype=np.int64)
    raw[:, :H, 1] = 1000
    raw[:, :H, 0] = int(0.01 * 1000 * 2 ** 24)
    raw[:, H, :3] = np.asarray(np.full(3, 20.0), dtype=np.float32).view(np.uint32).astype(np.int64)
    raw[7, 3, 2] = int(0.97 * 2 ** 24)

    def feed(**kw):          # one consume call that finds one read-back
        t.begin()
        return t.fold(raw.copy(), **kw)

    for batch in (1, 2):                                   # two outlier batches through forward(): attempt 0, then the repeat
        assert feed() == 0 and t.rare_last is True and t.rare[7] == batch
        assert feed(repeat=True) == 0 and t.rare[7] == batch and t.rare_last is True      # the repeat still sees the row (its guards answer it)
        assert t.mode[7] == 0
    t.begin()                                              # nothing pending: an unmeasured batch
    assert t.rare_last is False
    assert feed() == 1 and t.rare[7] == 3 and t.mode[7] == 1                                # the third BATCH moves the layer up
    t.begin()
    assert t.rare_last is False


def test_attention_stats_consume_folds_its_own_generation_only():
    """GMatcher._attention_stats_consume hands a lane's finished read-back to the tier table when the batch ran on that table's generation of
    the weights, drops it when it did not (weights replaced in between), and empties the slot either way."""
    m = GMatcher({}).eval()
    L, H = m.n_layers, 4
    t = m._tiers = AttentionTiers(L, H, 7, m.config)
    t.mode, t.calibrated = [0] * L, True

    class Ev:
        def synchronize(self):
            pass

    raw = np.zeros((L, H + 1, 4), dtype=np.int64)
    raw[:, :H, 1] = 1000
    raw[:, :H, 0] = int(0.01 * 1000 * 2 ** 24)
    raw[:, H, :3] = np.asarray(np.full(3, 20.0), dtype=np.float32).view(np.uint32).astype(np.int64)
    raw[2, 1, 0] = int(0.3 * 1000 * 2 ** 24)       # layer 2: a peaked head (-> half)
    raw[7, 3, 2] = int(0.97 * 2 ** 24)             # layer 7: one outlier row
    slot = [torch.from_numpy(raw.copy()), Ev(), 6]      # a batch of the previous weights
    m.__dict__["_attn_pending"] = {0: slot}
    assert m._attention_stats_consume(0) == 0 and slot[1] is None
    assert t.mode == [0] * L and t.rare.tolist() == [0] * L and t.rare_last is False and not t.peak.any()
    slot[1], slot[2] = Ev(), 7
    assert m._attention_stats_consume(1) == 0 and slot[1] is not None       # another lane's consume leaves it pending
    assert m._attention_stats_consume(0) == 1 and slot[1] is None
    assert t.mode == [0, 0, 1] + [0] * (L - 3) and t.rare[7] == 1 and t.rare_last is True and t.switched == [2]
    assert m._attention_stats_consume(0) == 0 and t.rare_last is False and t.rare[7] == 1       # the slot is empty: nothing is folded twice
    assert m.attention_report()["modes"][2] == "f16"


def test_attention_tiers_constructor_creates_every_field():
    """A fresh table reports every key GMatcher.attention_report() documents, in the shapes they keep (`rare` used to appear with the first fold)."""
    L, H = len(GMatcher.default_config['transformer_layers']), 4
    rep = AttentionTiers(L, H, 1, dict(GMatcher.default_config)).report()
    assert set(rep) == {"modes", "calibrated", "peak", "peak_max", "tail", "range", "switched", "redone", "rare", "threshold", "tail_threshold"}
    assert rep["modes"] == ["bf16x3"] * L and rep["calibrated"] is False and rep["switched"] == []
    assert rep["peak"].shape == rep["peak_max"].shape == rep["tail"].shape == (L, H) and rep["range"].shape == (L, 3)
    assert rep["rare"].shape == rep["redone"].shape == (L,) and rep["rare"].dtype == rep["redone"].dtype == np.int64
    assert not rep["rare"].any() and not rep["redone"].any()
    assert (rep["threshold"], rep["tail_threshold"]) == (0.08, 0.02)
    assert GMatcher({}).attention_report() is None


def test_train_backward_precision_takes_the_documented_values():
    """config['train_backward_precision']: 'bf16x3' (default), 'bf16x6', 'f32' -- the GEMMs of the reverse pass run in three or six bf16 passes
    ('f32' is the six-pass, f32-class form), the attention reverse is asked for exact-f32 products by name under 'f32' only; anything else raises."""
    from gims_amd import trainstep
    assert trainstep._backward_precision({}) == hip.PREC_BF16X3
    assert trainstep._backward_precision({"train_backward_precision": "bf16x3"}) == hip.PREC_BF16X3
    assert trainstep._backward_precision({"train_backward_precision": "bf16x6"}) == hip.PREC_BF16X6
    assert trainstep._backward_precision({"train_backward_precision": "f32"}) == hip.PREC_BF16X6
    assert trainstep._attention_backward_kwargs({"train_backward_precision": "f32"}) == {"precision": hip.PREC_F32}
    for v in ("bf16x3", "bf16x6"):
        assert trainstep._attention_backward_kwargs({"train_backward_precision": v}) == {}
    assert trainstep._attention_backward_kwargs({}) == {}
    for bad in ("fp32", "F32", "bf16", "", None, 0, "bf16x9"):
        with pytest.raises(ValueError, match="train_backward_precision"):
            trainstep._backward_precision({"train_backward_precision": bad})
    assert GMatcher.default_config["train_backward_precision"] == "bf16x3"


def test_graph_build_flag_words_decide_the_repeat():
    """info[7] of a graph build (include/gims_hip.h): bit 1 = the predicted percentile window was missed -- every output of that image is void,
    its overflow bit too, so the repeat with the robust flow comes before any capacity growth; bit 0 alone = grow the edge buffers; a robust
    build that reports a miss is an error (it predicts nothing)."""
    import numpy as np
    import pytest
    from gims_amd import GMatcher, hip
    R = GMatcher._agc_retry
    assert R(np.array([0, 0, 0]), False) is None
    assert R(np.array([0, 1, 0]), False) == "grow"
    assert R(np.array([0, 2, 0]), False) == "robust"
    assert R(np.array([1, 3, 0]), False) == "robust"          # a missed image may also claim an overflow: void
    assert R(np.array([1, 0, 0]), True) == "grow"
    with pytest.raises(hip.GimsHipError):
        R(np.array([0, 2]), True)


def test_bench_line_is_compact_and_parses_from_the_stored_tail():
    """The driver keeps the last 8000 characters of stdout and parses the last line: bench.py's line must stay under 4 KB
    whatever the full record holds (round 4 lost its measurement to a 24-KB line), also with 8 ranks and every extra block."""
    import json
    import bench
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    full = json.load(open(os.path.join(root, "profiles", "r04_bench_default.json")))        # a real 24-KB record
    assert len(json.dumps(full)) > 20000
    full["n_gpus"], full["world_size_seen"] = 8, 8
    full["ranks"] = [{"rank": r, "device": r, "device_name": "AMD Instinct MI355X", "backend": "nccl", "pid": 1000 + r} for r in range(8)]
    full["also"]["readme_boat_15k"] = dict(full["also"]["2x4096_eval_setting"], agc_ms_per_image=3.21)
    line = bench.compact_line(full)
    assert "\n" not in line and len(line) < bench.LINE_LIMIT <= 4096
    stdout = "x" * 20000 + "\n" + line + "\n"
    got = json.loads(stdout[-8000:].strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline", "cross_attention", "world_size_seen", "ranks"):
        assert k in got, k
    assert set(got["roofline"]) >= {"bound", "achieved", "peak", "unit", "frac", "traffic", "kernel"}
    assert set(got["cpu_baseline"]) >= {"value", "unit", "cores", "kind", "sample"}
    assert got["config"]["workload"] and got["also"]["2x1024"]["value"] > 0
    assert abs(got["value"] - full["value"]) / full["value"] < 1e-3
    # a record that is still too long sheds its optional parts instead of the contract's keys
    full["config"]["workload"] = "w" * 3000
    line = bench.compact_line(full)
    assert len(line) < bench.LINE_LIMIT and "roofline" in json.loads(line) and "cpu_baseline" in json.loads(line)


def test_bench_ranks_keep_to_disjoint_core_slices():
    """bench.py N > 1: every rank restricts itself to its own slice of the inherited CPU set before it touches the GPU (the step is host-bound within
    ~1 % of the GPU time: N interpreters must not share cores).  Equal contiguous shares, disjoint, inside the inherited set, whatever that set
    looks like (a cgroup may hand out a sparse one); too few cores -> the affinity is left alone."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    for cores, world in ((range(256), 8), (range(0, 128, 2), 4), ([3, 4, 5, 9, 10, 11, 12, 40], 2), (range(96), 8)):
        cores = list(cores)
        parts = [bench.rank_affinity(cores, r, world) for r in range(world)]
        assert all(p is not None and len(p) == len(cores) // world for p in parts)
        flat = [c for p in parts for c in p]
        assert len(set(flat)) == len(flat) and set(flat) <= set(cores)
        assert all(p == sorted(p) for p in parts)
    assert bench.rank_affinity(range(8), 3, 8) is None and bench.rank_affinity(range(15), 0, 8) is None
    assert bench.rank_affinity(range(64), 9, 8) == list(range(8, 16))          # (a global rank used as local rank wraps instead of running off the set)


def test_launch_tables_and_their_size_limit(monkeypatch):
    """GMatcher._replays: the gims_run_ops tables are the default at every size; `launch_replay_rows` > 0 restricts them to calls of at
    most that many keypoint rows (larger batches then launch one by one).  enable_timing(stepwise=True) and GIMS_NO_REPLAY / GIMS_REPLAY
    override."""
    monkeypatch.delenv("GIMS_NO_REPLAY", raising=False)
    monkeypatch.delenv("GIMS_REPLAY", raising=False)
    m = GMatcher({}).eval()
    assert m.config['launch_replay_rows'] == 0
    for part in ("encoder", "layers"):
        assert m._replays(part, 2 * 4096) and m._replays(part, 8 * 2 * 4096) and m._replays(part, 1 << 22)
    m = GMatcher({"launch_replay_rows": 16384}).eval()
    for part in ("encoder", "layers"):
        assert m._replays(part, 2 * 4096) and m._replays(part, 16384) and not m._replays(part, 16385) and not m._replays(part, 8 * 2 * 4096)
    monkeypatch.setenv("GIMS_REPLAY", "1")
    assert m._replays("layers", 65536) and m._replays("encoder", 65536)
    monkeypatch.setenv("GIMS_NO_REPLAY", "1")
    assert not m._replays("layers", 1024) and not m._replays("encoder", 1024)
    monkeypatch.setenv("GIMS_NO_REPLAY", "2")
    assert m._replays("layers", 65536) and not m._replays("encoder", 1024)
    monkeypatch.setenv("GIMS_NO_REPLAY", "3")
    assert not m._replays("layers", 1024) and m._replays("encoder", 65536)
    monkeypatch.delenv("GIMS_NO_REPLAY")
    monkeypatch.delenv("GIMS_REPLAY")
    m._stepwise = True
    assert not m._replays("layers", 1024)


def test_bench_event_sampling_schedule():
    """bench.py records its HIP events on every 5th timed step, mid-stride (bracketing every launch of every step costs 2 % of the step)."""
    import bench
    assert bench.event_steps(20, 5) == (5, [2, 7, 12, 17])
    assert bench.event_steps(5, 5) == (5, [2]) and bench.event_steps(3, 5) == (3, [1]) and bench.event_steps(1, 5) == (1, [0])
    assert bench.event_steps(20, 1) == (1, list(range(20))) and bench.event_steps(7, 0) == (1, list(range(7)))


def test_bench_plain_run_is_the_default_and_full_is_opt_in():
    """`bench.py --gpus 1 --steps K --warmup W` is the plain run: one workload, no extra blocks; --full and --dump-outputs are opt-in."""
    import bench
    a = bench.parser().parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    a = bench.parser().parse_args(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"


def test_bench_plain_line_carries_the_headline_and_nothing_it_did_not_measure():
    """A plain run's record has no roofline, stage times, CPU baseline or extra blocks and writes no bench_extra.json: its line must not claim them."""
    import json
    import bench
    res = {"metric": "image-pairs/sec at 2x4096 keypoints", "value": 550.0, "unit": "pairs/s", "n_gpus": 1, "steps": 20, "warmup": 3,
           "ms_per_step": 14.5, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "data": "synthetic",
           "dtype": "bf16 MFMA attention and Q/K/V projection + ...", "dtype_short": "bf16 MFMA attention + bf16x3 MFMA linears + f32 Sinkhorn",
           "config": {"workload": "8 pairs/step/GPU of 2x4096", "keypoints": 4096}, "world_size_seen": 1, "stats_rows_gathered": 8}
    got = json.loads(bench.compact_line(res, extra=None))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config"):
        assert k in got, k
    assert got["dtype"] == res["dtype_short"] and got["ms_per_step"] == 14.5
    for k in ("roofline", "cross_attention", "cpu_baseline", "stage_ms_per_step", "host_step_ms", "attention_layers", "also", "extra"):
        assert k not in got, k


def _fake_outs(pair_ids, n):
    g = torch.Generator().manual_seed(5)
    outs, datas = [], []
    for pid in pair_ids:
        o, d = {}, {}
        for s in "01":
            o[f"keypoints{s}"] = torch.rand(1, n, 2, generator=g)
            o[f"descriptors{s}"] = torch.rand(1, 256, n, generator=g)
            o[f"mdesc{s}"] = torch.rand(n, 256, generator=g)
            o[f"matches{s}"] = torch.randint(-1, n, (1, n), generator=g)
            o[f"matching_scores{s}"] = torch.rand(1, n, generator=g)
            d[f"kept_kpts{s}_indices"] = [torch.arange(n, dtype=torch.int64)]
        outs.append(o)
        datas.append(d)
    return outs, datas


def test_bench_dump_outputs_is_complete_seeded_and_bounded(tmp_path):
    """--dump-outputs: float32 / float64 .npy files of what match_pairs returned; the descriptor sample depends on the pair id only, so two runs
    (two builds) write the same names and rows; the total stays within the limit (whole pairs are left out, in order, beyond it)."""
    import bench
    outs, datas = _fake_outs([0, 1, 2], 700)
    stats = torch.rand(3, 5)
    names = bench.dump_outputs(str(tmp_path / "a"), [0, 1, 2], outs, datas, stats)
    assert "stats" in names and "pair0002_mdesc1_sample" in names and "pair0000_matches0" in names
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(n + ".npy" for n in names)
    arrs = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert arrs["pair0001_mdesc0_sample"].shape == (bench.DUMP_ROWS, 256)
    rows = arrs["pair0001_sample_rows0"].astype(np.int64)
    np.testing.assert_array_equal(arrs["pair0001_mdesc0_sample"], outs[1]["mdesc0"].numpy()[rows])
    np.testing.assert_array_equal(arrs["pair0001_descriptors0_sample"], outs[1]["descriptors0"][0].numpy()[:, rows].T)
    np.testing.assert_array_equal(arrs["pair0002_matches1"], outs[2]["matches1"][0].numpy().astype(np.float64))
    again = bench.dump_outputs(str(tmp_path / "b"), [0, 1, 2], outs, datas, stats)
    assert again == names
    np.testing.assert_array_equal(np.load(tmp_path / "b" / "pair0001_sample_rows0.npy"), arrs["pair0001_sample_rows0"])
    assert sum(a.nbytes for a in arrs.values()) <= bench.DUMP_LIMIT
    per_pair = sum(a.nbytes for n, a in arrs.items() if n.startswith("pair0000_"))
    few = bench.dump_outputs(str(tmp_path / "c"), [0, 1, 2], outs, datas, None, limit=2 * per_pair + 1)
    assert {n.split("_")[0] for n in few} == {"pair0000", "pair0001"}
    assert sum(os.path.getsize(tmp_path / "c" / f) for f in os.listdir(tmp_path / "c")) < 2 * per_pair + 1 + 128 * len(few)
