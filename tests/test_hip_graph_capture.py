"""
GPU test (-m gpu): the training step of BASELINE config 5's shape inside a HIP graph (torch.cuda.CUDAGraph).

Every launch of the differentiable path -- the TRAIN forward, compositing, both backward chains, the weight-gradient launch, the
latent scatter with its segment pre-pass -- must be capturable: no allocation, no host synchronisation and no per-stream state
inside the library (the scatter's workspace comes from the caller since C ABI rev 7, the multi-view kernels' view-sum scratch since
rev 10: a scratch keyed by stream was not found on the capture stream and failed the capture).  The replayed graph must produce the
bits of the eager step: parameter gradients are fixed-order reductions, the grid gradient comes out of the LDS-slab scatter
(pnr_scatter.hip).
"""
import os
import subprocess
import sys

import pytest
import torch

from helpers import golden_setup, mlp_params

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("precision,name", [("f16x3", "train_64_32"), ("f16", "train_64_32"), ("f16x3", "srn_mini_64_128")])
def test_training_step_is_capturable_and_replays_the_eager_bits(precision, name):
    """train_64_32: 4 objects x 32 rays, one source view.  srn_mini_64_128: two source views -- the multi-view kernels' view-sum
    scratch is the scene's and the backward dumps' (torch tensors), nothing the library keeps per stream."""
    dev = torch.device("cuda:0")
    net, step = _train_net(dev, name, precision)
    eager = [t.clone() for t in step()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()  # warm-up on a side stream, as torch's capture recipe asks (allocator pools, lazy initialisations)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # captures on a stream of its own: nothing in the library may be keyed by the stream
        static = step()  # the graph's static outputs: loss, parameter gradients, latent gradient
    names = ["loss"] + [n for n, _ in net.mlp_coarse.named_parameters()] + [n for n, _ in net.mlp_fine.named_parameters()] + ["latent"]
    for _ in range(2):
        for t in static:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        bad = [(n, float((a - b).abs().max())) for n, a, b in zip(names, static, eager) if not torch.equal(a, b)]
        assert not bad, bad
    assert float(static[-1].abs().max()) > 0


@pytest.mark.parametrize("name", ["sn64_64_128", "dtu_mini_64_128"])
def test_render_call_is_capturable_and_replays_the_eager_bits(name):
    """inference: NeRFRenderer.forward (in-kernel draws off: explicit noise) captured once, replayed; single- and three-view scenes"""
    from test_api_gpu import build_net
    from pixelnerf_amd.render import NeRFRenderer
    dev = torch.device("cuda:0")
    g, scene, meta, mc, mf, rays, noise = golden_setup(name)
    net = build_net(dev, scene)
    rend = NeRFRenderer(n_coarse=int(g["n_coarse"]), n_fine=int(g["n_fine"]), n_fine_depth=int(g["n_fine_depth"]),
                        white_bkgd=bool(g["white_bkgd"]), lindisp=bool(g["lindisp"]), depth_std=float(g["depth_std"])).to(dev).eval()
    r = rays.to(dev)
    nz = {k: v.to(dev) for k, v in noise.items()}
    with torch.no_grad():
        eager = rend(net, r, want_weights=True, _noise=nz)
        e_rgb, e_w = eager.fine.rgb.clone(), eager.fine.weights.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            rend(net, r, want_weights=True, _noise=nz)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = rend(net, r, want_weights=True, _noise=nz)
        s_rgb, s_w = out.fine.rgb, out.fine.weights
        for _ in range(2):
            s_rgb.zero_(); s_w.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(s_rgb, e_rgb) and torch.equal(s_w, e_w)


def _train_net(dev, name, precision):
    """the training setup of test_training_step_is_capturable_and_replays_the_eager_bits -> (step(), outputs)"""
    from pixelnerf_amd.model import make_model
    from pixelnerf_amd.render import NeRFRenderer
    from pixelnerf_amd.util.conf import default_model_conf
    g, scene, meta, mc, mf, rays, noise = golden_setup(name)
    net = make_model(default_model_conf(), precision=precision).to(dev).train()
    net.mlp_coarse.load_state_dict(mlp_params(11))
    net.mlp_fine.load_state_dict(mlp_params(12))
    lat = scene["latent"].to(dev).clone().requires_grad_(True)
    net.encoder.latent = lat
    ls = torch.tensor([float(lat.shape[-1]), float(lat.shape[-2])], device=dev)
    net.encoder.latent_scaling = ls / (ls - 1) * 2.0
    net.poses, net.image_shape = scene["poses"].to(dev), scene["image_shape"].to(dev)
    net.focal, net.c = scene["focal"].to(dev), scene["c"].to(dev)
    net.num_objs, net.num_views_per_obj = scene["SB"], scene["NS"]
    rend = NeRFRenderer(n_coarse=int(g["n_coarse"]), n_fine=int(g["n_fine"]), n_fine_depth=int(g["n_fine_depth"]),
                        white_bkgd=bool(g["white_bkgd"]), lindisp=bool(g["lindisp"]), depth_std=float(g["depth_std"])).to(dev).train()
    params = list(net.mlp_coarse.parameters()) + list(net.mlp_fine.parameters())
    r, nz = rays.to(dev), {k: v.to(dev) for k, v in noise.items()}
    gt = torch.rand(r.shape[0], r.shape[1], 3, device=dev)
    loss_out = torch.zeros((), device=dev)

    def step():
        out = rend(net, r, want_weights=True, _noise=nz)
        loss = ((out.coarse.rgb - gt) ** 2).mean() + ((out.fine.rgb - gt) ** 2).mean()
        for p in params:
            p.grad = None
        lat.grad = None
        loss.backward()
        loss_out.copy_(loss.detach())
        return [loss_out] + [p.grad for p in params] + [lat.grad]

    return net, step


def _capture_first_child():
    """child of test_multiview_capture_before_any_eager_multiview_call: single-view warm-up only, then a multi-view render and
    multi-view training steps are CAPTURED before any multi-view launch ran eagerly; replays must give the eager bits computed after"""
    from test_api_gpu import build_net
    from pixelnerf_amd.render import NeRFRenderer
    dev = torch.device("cuda:0")
    net1, step1 = _train_net(dev, "train_64_32", "f16x3")  # one source view: library, allocator and torch warmed up
    step1()
    torch.cuda.synchronize()
    g, scene, meta, mc, mf, rays, noise = golden_setup("srn_mini_64_128")
    assert scene["NS"] > 1
    net = build_net(dev, scene)
    net.scene()  # (the scene struct is built from host-side shapes: not inside a capture; no kernel of the network runs)
    rend = NeRFRenderer(n_coarse=int(g["n_coarse"]), n_fine=int(g["n_fine"]), n_fine_depth=int(g["n_fine_depth"]),
                        white_bkgd=bool(g["white_bkgd"]), lindisp=bool(g["lindisp"]), depth_std=float(g["depth_std"])).to(dev).eval()
    r, nz = rays.to(dev), {k: v.to(dev) for k, v in noise.items()}
    with torch.no_grad():
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = rend(net, r, want_weights=True, _noise=nz)
        graph.replay()
        torch.cuda.synchronize()
        eager = rend(net, r, want_weights=True, _noise=nz)
        assert torch.equal(out.fine.rgb, eager.fine.rgb) and torch.equal(out.fine.weights, eager.fine.weights), "render"
    for precision in ("f16x3", "f16"):
        net, step = _train_net(dev, "srn_mini_64_128", precision)
        net.scene()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static = step()
        graph.replay()  # the first step fills the packed-weight caches: captured, they hold data only once the graph has run
        torch.cuda.synchronize()
        eager = [t.clone() for t in step()]
        torch.cuda.synchronize()
        for t in static:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        bad = [i for i, (a, b) in enumerate(zip(static, eager)) if not torch.equal(a, b)]
        assert not bad, (precision, bad)
    print("CAPTURE_FIRST_OK")


def test_multiview_capture_before_any_eager_multiview_call():
    """the view-sum scratch comes with the scene / the backward dumps: a multi-view render and training step capture in a process
    whose library never ran a multi-view launch eagerly (the library-owned scratch of ABI rev 9 had nothing to lend there).  A
    fresh child process, under a time limit: a timeout or a signal ends the test without starting anything else on the GPU."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([here, os.path.dirname(here), os.environ.get("PYTHONPATH", "")]))
    res = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0 and "CAPTURE_FIRST_OK" in res.stdout, (res.returncode, res.stdout[-2000:], res.stderr[-4000:])


if __name__ == "__main__":
    _capture_first_child()
