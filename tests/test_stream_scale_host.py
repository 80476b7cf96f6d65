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


def test_abi_revision_12_declares_the_launch_struct_and_the_scale_field(repo_root, tmp_path):
    src = open(os.path.join(repo_root, "include", "pixelnerf_hip.h")).read()
    assert int(re.search(r"#define\s+PNR_ABI_VERSION\s+(\d+)", src).group(1)) == 12 == _lib.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"int32_t\s+stream_scale_log2\s*;", code)
    assert re.search(r"typedef\s+struct\s+PnrSplitAux\s*\{[^}]*\}\s*PnrSplitAux\s*;", code)
    _lib.build_library()
    lib = _lib.load()
    assert lib.pnr_abi_version() == 12
    # guard, probe and scale are arguments of the launch (PnrSplitAux): the entries that armed them per host thread are gone
    for gone in ("pnr_saturation_guard", "pnr_range_probe"):
        assert gone not in code and gone not in _lib.PROTOTYPES and not hasattr(lib, gone)
    # the structs as gcc lays the header out against the ctypes mirrors
    assert [f for f, _ in _lib.PnrMlpWeights._fields_][-2:] == ["combine_max", "stream_scale_log2"]
    assert [f for f, _ in _lib.PnrSplitAux._fields_] == ["stream_scale_log2", "sat_flag", "range_probe"]
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    structs = {"PnrMlpWeights": _lib.PnrMlpWeights, "PnrSplitAux": _lib.PnrSplitAux}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pixelnerf_hip.h"', 'int main(void) {']
    for name, cls in structs.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{name}.{fname} %zu\\n", offsetof({name}, {fname}));')
    lines += ['  return 0;', '}']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(repo_root, "include"), str(c), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for name, cls in structs.items():
        assert int(got[name]) == ctypes.sizeof(cls), name
        for fname, _ in cls._fields_:
            assert int(got[f"{name}.{fname}"]) == getattr(cls, fname).offset, f"{name}.{fname}"


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


def _split_aux_calls(lib, sc, sv):
    """every entry that takes a PnrSplitAux, with well-formed sizes and dummy (never dereferenced) device addresses:
    name -> (call(aux_pointer), is a render entry)"""
    render_tail = (64, 4, 4, 8, 16, 4, 0.01, 0, 0)  # rays, R, rays_per_obj, Kc, Kf, Kfd, depth_std, white_bkgd, lindisp
    outs = (64, 64, 64, 64, 64, 64, 64)             # rgb_c .. weights_f, workspace
    return {
        "pnr_eval_ray_samples_split": (lambda a: lib.pnr_eval_ray_samples_split(sc, 64, 64, 64, 64, 4, 4, 8, 64, a, None), False),
        "pnr_eval_points_split": (lambda a: lib.pnr_eval_points_split(sc, 64, 64, 64, 64, 4, 64, a, None), False),
        "pnr_eval_ray_samples_split_train": (lambda a: lib.pnr_eval_ray_samples_split_train(sc, 64, 64, 64, 64, 4, 4, 8, 64, sv, a, None), False),
        "pnr_render_forward_folded": (lambda a, p=_lib.PREC_F16X3, f=None: lib.pnr_render_forward_folded(
            sc, 64, 64, 64, 64, p, *render_tail, 64, 64, 64, 64, *outs, a, f, None), True),
        "pnr_render_forward_seeded": (lambda a, p=_lib.PREC_F16X3, f=None: lib.pnr_render_forward_seeded(
            sc, 64, 64, 64, 64, p, *render_tail, 7, 0, 0, *outs, a, f, None), True),
        "pnr_render_views": (lambda a, p=_lib.PREC_F16X3, f=None: lib.pnr_render_views(
            sc, 64, 64, 64, 64, p, 64, 1, 2, 2, 1.0, 1.0, 1.0, 1.0, 0.5, 2.0, 8, 16, 4, 0.01, 0, 0, None, None, None, None, 7,
            *outs, a, f, None), True),
    }


def test_entries_refuse_a_bad_launch_struct_on_the_host():
    """PnrSplitAux is checked before any HIP call: a scale outside [0, 30] (every entry, coarse and fine struct), any scale on the
    training entry, and a struct with a field set at a 16-bit precision (render entries) are PNR_E_INVALID, the message names the
    field.  (On a machine without a GPU a HIP call would fail with PNR_E_HIP = -2 instead.)"""
    _lib.build_library()
    lib = _lib.load()
    scene = _lib.PnrScene()
    scene.latent_nhwc, scene.poses, scene.focal, scene.c = 64, 64, 64, 64
    scene.SB, scene.NS, scene.Hl, scene.Wl, scene.n_focal, scene.n_c = 1, 1, 8, 8, 1, 1
    saved = _lib.PnrSplitSaved()
    calls = _split_aux_calls(lib, ctypes.byref(scene), ctypes.byref(saved))
    assert sorted(calls) == sorted(n for n, (_, args) in _lib.PROTOTYPES.items() if _lib._AUX in args)
    for name, (call, render) in calls.items():
        for bad in (-1, 31):
            aux = _lib.PnrSplitAux(stream_scale_log2=bad)
            assert call(ctypes.byref(aux)) == -1, name
            assert b"stream_scale_log2" in lib.pnr_last_error() and b"[0, 30]" in lib.pnr_last_error(), name
            if render:
                assert call(None, f=ctypes.byref(aux)) == -1, name
                assert b"stream_scale_log2" in lib.pnr_last_error(), name
        if render:
            for prec in (_lib.PREC_F16, _lib.PREC_BF16):
                for field in ("stream_scale_log2", "sat_flag", "range_probe"):
                    aux = _lib.PnrSplitAux(**{field: 64 if field != "stream_scale_log2" else 3})
                    for kw in (dict(a=ctypes.byref(aux)), dict(a=None, f=ctypes.byref(aux))):
                        assert call(p=prec, **kw) == -1, (name, prec, field)
                        assert field.encode() in lib.pnr_last_error() and b"PNR_PREC_F16X3" in lib.pnr_last_error(), (name, prec, field)
    aux = _lib.PnrSplitAux(stream_scale_log2=3)
    assert calls["pnr_eval_ray_samples_split_train"][0](ctypes.byref(aux)) == -1
    assert b"stream scale" in lib.pnr_last_error() and b"stream_scale_log2" in lib.pnr_last_error()


def test_the_library_keeps_no_launch_state(repo_root):
    """what a launch does is a function of its arguments: the only thread-local of the library is the errno-style message behind
    pnr_last_error, and nothing is guarded by a mutex (a text check, kept to these two words)"""
    csrc = os.path.join(repo_root, "pixel-nerf_amd", "csrc")
    hits = []
    for fn in sorted(os.listdir(csrc)):
        if fn.endswith((".hip", ".h")):
            for line in open(os.path.join(csrc, fn)):
                if "thread_local" in line or "std::mutex" in line:
                    hits.append((fn, line.strip()))
    assert hits == [("pnr_api.hip", 'static thread_local char g_err[512] = "";')]


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
