"""Host tests (no GPU) of the cameras-to-images entry: argument checks that happen before any device work, and the wrappers
that do not implement it."""
import pytest
import torch

from pixelnerf_amd import _lib
from pixelnerf_amd.render import NeRFRenderer
from pixelnerf_amd.render.nerf import _MultiDeviceRenderWrapper, _RenderWrapper


class _Model(torch.nn.Module):
    def forward(self, xyz, coarse=True, viewdirs=None):
        return torch.zeros(*xyz.shape[:-1], 4)


def test_render_views_checks_its_arguments_and_has_no_cpu_path():
    rend = NeRFRenderer(n_coarse=4, n_fine=0).eval()
    par = rend.bind_parallel(_Model(), None, simple_output=True)
    assert isinstance(par, _RenderWrapper)
    poses = torch.eye(4).expand(1, 2, 4, 4)
    with pytest.raises(ValueError, match="poses_c2w"):
        par.render_views(torch.eye(4), 6, 5, 10.0, 0.5, 2.0)
    with pytest.raises(ValueError, match="views_per_call"):
        par.render_views(poses, 6, 5, 10.0, 0.5, 2.0, views_per_call=0)
    with pytest.raises(_lib.PixelNerfHipError):  # host tensors: rays are built, every renderer stage is a HIP kernel
        par.render_views(poses, 6, 5, 10.0, 0.5, 2.0)


def test_sharding_wrappers_name_forward():
    from pixelnerf_amd.dist import ShardedRenderWrapper
    rend = NeRFRenderer(n_coarse=4, n_fine=0).eval()
    multi = _MultiDeviceRenderWrapper(_Model(), rend, True, [0, 1])
    sharded = ShardedRenderWrapper.__new__(ShardedRenderWrapper)
    for w in (multi, sharded):
        with pytest.raises(NotImplementedError, match="forward"):
            w.render_views(torch.eye(4).expand(1, 1, 4, 4), 6, 5, 10.0, 0.5, 2.0)
