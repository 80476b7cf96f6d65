"""Host tests (no GPU) of the power-of-two stream scale of precision "f16x3": the host arithmetic that picks a scale, the
homogeneous blow-up fixture the GPU tests run on (checked here on the CPU oracle), the C ABI of revision 11 and the Python
surface (make_model(stream_scale=), state_dict, the packed-stream cache key)."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import pytest
import torch

from helpers import load_golden, mlp_params, scene_for
from oracle import pnr_oracle as O
from pixelnerf_amd import _lib, ops

FP16_MAX = 65504.0


def blow_up(p, A):
    """The homogeneous blow-up: lin_in, every lin_z and every block bias times A, lin_out.weight divided by A.  ReLU is
    positively homogeneous, so in exact arithmetic the hidden stream is A times the base network's and the outputs are the
    base network's -- rgb stays in its ordinary, unsaturated range."""
    q = {k: v.clone() for k, v in p.items()}
    for k in q:
        if k.startswith(("lin_in.", "lin_z.")) or (k.startswith("blocks.") and k.endswith(".bias")):
            q[k] = q[k] * A
    q["lin_out.weight"] = q["lin_out.weight"] / A
    return q


def test_stream_scale_for():
    f = ops.stream_scale_for
    assert f(0.0) == 0 and f(1.0) == 0 and f(16384.0) == 0
    assert f(math.nextafter(16384.0, math.inf)) == 1 and f(32768.0) == 1 and f(32769.0) == 2
    prev = 0
    for a in sorted(m * 2.0 ** e for e in range(-4, 44) for m in (1.0, 1.3, 1.999)):
        s = f(a)  # monotone, and the smallest scale that brings the value to <= 16384
        assert s >= prev
        assert a * 2.0 ** -s <= 16384.0 and (s == 0 or a * 2.0 ** -(s - 1) > 16384.0)
        prev = s
    for k in range(0, 29):
        assert f(FP16_MAX * 2.0 ** k) == k + 2
    for bad in (float("inf"), float("nan"), -1.0):
        with pytest.raises(ValueError):
            f(bad)
    with pytest.raises(ValueError, match="limit is 30"):
        f(16384.0 * 2.0 ** 31)


@pytest.mark.parametrize("name", ["sn64", "mv_mini"])
def test_blow_up_fixture_leaves_the_outputs_alone_and_the_fp16_range_far_behind(name):
    A = 48000.0
    g = load_golden("stages")
    scene, _ = scene_for(name, 2)
    xyz, vd = torch.from_numpy(g[f"{name}_xyz"]), torch.from_numpy(g[f"{name}_viewdirs"])
    base = mlp_params(11)
    with torch.no_grad():
        o0, h0 = O.pixelnerf_forward(scene, base, xyz, vd, return_hidden=True)
        o1, h1 = O.pixelnerf_forward(scene, blow_up(base, A), xyz, vd, return_hidden=True)
    e_rgb = float((o1[..., :3] - o0[..., :3]).abs().max())
    e_s = float(((o1[..., 3] - o0[..., 3]).abs() / o0[..., 3].clamp(min=1.0)).max())
    print(f"blow-up A={A:g} [{name}]: |x| max {float(h0.abs().max()):.1f} -> {float(h1.abs().max()):.3e}, fp32 oracle blown up vs base: "
          f"rgb {e_rgb:.2e}, sigma rel {e_s:.2e}")
    assert e_rgb <= 2e-6
    assert float(h1.abs().max()) > 4 * FP16_MAX


def test_abi_revision_11_declares_and_exports_the_probe_and_the_scale_field(repo_root, tmp_path):
    src = open(os.path.join(repo_root, "include", "pixelnerf_hip.h")).read()
    assert int(re.search(r"#define\s+PNR_ABI_VERSION\s+(\d+)", src).group(1)) == 11 == _lib.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+pnr_range_probe\s*\(\s*float\s*\*", code)
    assert re.search(r"int32_t\s+stream_scale_log2\s*;", code)
    assert "pnr_range_probe" in _lib.PROTOTYPES
    _lib.build_library()
    lib = _lib.load()
    assert lib.pnr_abi_version() == 11 and hasattr(lib, "pnr_range_probe")
    assert lib.pnr_range_probe(None) == 0  # disarming needs no device
    # the struct as gcc lays the header out against the ctypes mirror
    assert [f for f, _ in _lib.PnrMlpWeights._fields_][-2:] == ["combine_max", "stream_scale_log2"]
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pixelnerf_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(PnrMlpWeights));']
    for fname, _ in _lib.PnrMlpWeights._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(PnrMlpWeights, {fname}));')
    lines += ['  return 0;', '}']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(repo_root, "include"), str(c), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(_lib.PnrMlpWeights)
    for fname, _ in _lib.PnrMlpWeights._fields_:
        assert int(got[fname]) == getattr(_lib.PnrMlpWeights, fname).offset, fname


def test_entries_without_a_scaled_form_refuse_the_field_on_the_host():
    """the f16 / bf16 pack entries and the training entries that take the weight struct: PNR_E_INVALID before any HIP call"""
    _lib.build_library()
    lib = _lib.load()
    w = _lib.PnrMlpWeights()
    w.stream_scale_log2 = 3
    ref = ctypes.byref(w)
    for prec in (_lib.PREC_F16, _lib.PREC_BF16):
        assert lib.pnr_pack_mlp(ref, prec, 64, None) == -1 and b"stream scale" in lib.pnr_last_error()
        assert lib.pnr_pack_mlp_folded(ref, prec, 64, None) == -1 and b"stream scale" in lib.pnr_last_error()
        assert lib.pnr_pack_mlp_bwd(ref, prec, 64, None) == -1 and b"stream scale" in lib.pnr_last_error()
    sv = _lib.PnrSplitSaved()
    assert lib.pnr_mlp_backward_split(ref, ctypes.byref(sv), 64, 10, 1, None, 64, None, 64, 64, 1 << 40, None) == -1
    assert b"stream scale" in lib.pnr_last_error()
    fs = _lib.PnrF32Saved()
    assert lib.pnr_mlp_backward_f32(ref, ctypes.byref(fs), 64, 10, 1, None, 64, None, 0, None, 64, 1 << 40, None) == -1
    assert b"stream scale" in lib.pnr_last_error()
    sc = _lib.PnrScene()
    sc.SB = 1
    assert lib.pnr_eval_ray_samples_f32_train(ctypes.byref(sc), ref, 64, 64, 4, 4, 8, 64, ctypes.byref(fs), 0, None) == -1
    assert b"stream scale" in lib.pnr_last_error()
    for bad in (-1, 31):
        w.stream_scale_log2 = bad
        assert lib.pnr_pack_mlp_split(ref, 64, None) == -1 and b"[0, 30]" in lib.pnr_last_error()


def _model(**kw):
    from pixelnerf_amd.model import make_model
    from pixelnerf_amd.util.conf import default_model_conf
    return make_model(default_model_conf(), **kw)


def test_make_model_takes_a_stream_scale_and_keeps_it_out_of_the_state_dict():
    base = _model()
    assert base.stream_scale == (0, 0) and base.stream_scale_resolved()
    keys = set(base.state_dict())
    for value, want in ((0, (0, 0)), (6, (6, 6)), (30, (30, 30)), ("auto", "auto")):
        net = _model(precision="f16x3", stream_scale=value)
        assert net.stream_scale == want
        assert set(net.state_dict()) == keys and not any("scale" in k for k in keys)
        net.load_state_dict(base.state_dict())  # the reference's checkpoints keep loading unchanged
        assert net.stream_scale == want
    assert not _model(stream_scale="auto").stream_scale_resolved()
    for bad in (-1, 31, 100):
        with pytest.raises(ValueError):
            _model(stream_scale=bad)
    for bad in (1.5, True, None):
        with pytest.raises(TypeError):
            _model(stream_scale=bad)
    with pytest.raises(ValueError):
        _model(stream_scale="automatic")
    net = _model()
    net.stream_scale = (3, 5)  # settable, per network
    assert (net.mlp_coarse.stream_scale, net.mlp_fine.stream_scale) == (3, 5) and net.stream_scale == (3, 5)
    net.stream_scale = "auto"
    assert net.stream_scale == "auto" and (net.mlp_coarse.stream_scale, net.mlp_fine.stream_scale) == (0, 0)
    with pytest.raises(ValueError):
        net.stream_scale = (1, 2, 3)
    net.mlp_fine = None
    net.stream_scale = 4
    assert net.stream_scale == (4, 4)


def test_the_scale_is_part_of_the_packed_cache_key():
    from pixelnerf_amd.model.resnetfc import ResnetFC
    key = ResnetFC._packed_key
    assert key("f16x3", True, 0) == ("f16x3", True)  # an unscaled stream keeps the key it always had
    assert len({key("f16x3", True, 0), key("f16x3", True, 4), key("f16x3", True, 8)}) == 3
    mlp = _model().mlp_coarse
    seen = []
    mlp._cached = lambda k, prec, build, training_pass=False: seen.append((k, training_pass)) or k
    mlp.packed("f16x3", folded=True)
    mlp.stream_scale = 5
    mlp.packed("f16x3", folded=True)
    mlp.packed("f16", folded=True)  # the 16-bit kernels have no scale: their stream does not follow it
    assert [k for k, _ in seen] == [("f16x3", True), ("f16x3", True, 5), ("f16", True)]
    with pytest.raises(NotImplementedError, match="stream scale"):
        mlp.packed("f16x3", folded=True, training_pass=True)
    mlp.stream_scale = 31
    with pytest.raises(ValueError):
        mlp.packed("f16x3", folded=True)


def test_parallel_wrappers_refuse_an_unresolved_automatic_scale():
    """sharded = unsharded bit for bit needs the same scale on every rank / device: an integer passes, "auto" must be resolved"""
    from pixelnerf_amd.render.nerf import _check_scale_resolved
    net = _model(stream_scale="auto")
    with pytest.raises(RuntimeError, match="calibrate_stream_scale"):
        _check_scale_resolved(net, "bind_parallel")
    net.stream_scale = 6
    _check_scale_resolved(net, "bind_parallel")
