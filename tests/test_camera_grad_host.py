"""CPU tests of the camera-gradient feature: the reference fixture's layout, the new C entries (declared, exported, bound),
and the argument checks of the new ops, which run before any device work."""
import os
import re

import pytest
import torch

from helpers import load_golden
from pixelnerf_amd import _lib, ops

NEW_ENTRIES = ("pnr_camera_backward", "pnr_camera_backward_workspace_bytes", "pnr_composite_backward_far",
               "pnr_gen_rays_backward", "pnr_sample_bounds_backward")
SCENARIOS = {"train_64_32": (4, 32, 4), "srn_mini_64_128": (1, 64, 2), "dtu_mini_64_128": (1, 64, 3),
             "mv_mini_lindisp": (2, 32, 4)}  # name: (objects, rays per object, source views SB*NS)


def test_fixture_keys_and_shapes():
    g = load_golden("camera_gradients")
    for name, (SB, B, NV) in SCENARIOS.items():
        assert g[f"{name}_grad_rays"].shape == (SB * B, 8)
        assert g[f"{name}_grad_c2w"].shape == g[f"{name}_c2w"].shape == (NV, 4, 4)
        assert g[f"{name}_grad_focal"].shape == g[f"{name}_focal"].shape == (1, 2)
        assert g[f"{name}_grad_c"].shape == g[f"{name}_c"].shape == (1, 2)
        assert g[f"{name}_gt"].shape == (SB, B, 3)
        assert float(abs(g[f"{name}_grad_c2w"]).sum()) > 0
    assert g["gen_rays_pose"].shape == g["gen_rays_grad_pose"].shape == (1, 4, 4)
    assert g["gen_rays_gt"].shape == (1, 64, 3)


def test_new_entries_are_declared_exported_and_bound(repo_root):
    _lib.build_library()
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(repo_root, "include", "pixelnerf_hip.h")).read(), flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES, name
    assert lib.pnr_camera_backward_workspace_bytes(0, 8, 1, 1) == 0


class _Scene:
    NS, SB = 1, 1


def test_camera_backward_argument_checks():
    R, K = 4, 8
    ok = dict(rays=torch.zeros(R, 8), z=torch.zeros(R, K), d_in42=torch.zeros(R * K, 42), d_zlat=torch.zeros(R * K, 512))
    for key, bad in (("rays", torch.zeros(R, 7)), ("rays", torch.zeros(R, 8, dtype=torch.float64)), ("z", torch.zeros(R + 1, K)),
                     ("d_in42", torch.zeros(R * K, 64)), ("d_zlat", torch.zeros(R * K, 512, dtype=torch.float16))):
        args = dict(ok, **{key: bad})
        with pytest.raises(ValueError, match=key):
            ops.camera_backward(_Scene(), args["rays"], args["z"], args["d_in42"], args["d_zlat"])
    with pytest.raises(ValueError, match="ranks"):
        ops.camera_backward(_Scene(), *ok.values(), ranks=torch.zeros(R, 2, dtype=torch.int64))


def test_gen_rays_backward_argument_checks():
    with pytest.raises(ValueError, match="d_rays"):
        ops.gen_rays_backward(torch.zeros(1, 4, 5, 8), 4, 4, 3.0)
    with pytest.raises(ValueError, match="d_rays"):
        ops.gen_rays_backward(torch.zeros(1, 4, 4, 8, dtype=torch.float64), 4, 4, 3.0)
