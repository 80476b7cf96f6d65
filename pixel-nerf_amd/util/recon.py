"""
Mesh reconstruction tools: src/util/recon.py on the device.

The reference evaluates sigma on a grid chunk by chunk, gathers it on the host and calls PyMCubes.  Here the grid points come from
pnr_gen_grid_points, every chunk goes through `occu_net(xyz[None], coarse=, viewdirs=)` (the fused HIP network for a PixelNeRFNet),
the sigma column is gathered into one device grid, and pnr_marching_cubes_count / pnr_marching_cubes_emit extract an indexed mesh
on the device (semantics: include/pixelnerf_hip.h).  Deviations from the reference, all deliberate:
  * points are passed as (1, N, 3): the reference passes (N, 3) to a forward that unpacks `SB, B, _ = xyz.shape` (recon.py:57,64);
  * the fake view direction of a grid point at the exact origin is (0,0,0), not 0/0 = NaN (recon.py:54);
  * a non-finite density raises ValueError instead of reaching the mesher;
  * the case table, vertex order and triangle order are this library's own (one vertex per crossed grid edge, shared by its cells).
    Triangles are wound so that their normal points from inside (sigma > isosurface) to outside; whether PyMCubes winds the same
    way could not be checked when this was written -- flip a column of `triangles` if a consumer expects the opposite.
"""
import warnings

import numpy as np
import torch


def density_grid(occu_net, c1, c2, reso, coarse=True, sigma_idx=3, eval_batch_size=100000, device=None, what="density_grid"):
    """
    The density of an encoded object on the grid of src/util/recon.py:43-66, on the device: what marching_cubes meshes and what
    util.occupancy.OccupancyGrid.from_model turns into an occupancy bitfield.  The points come from ops.gen_grid_points (with the
    reference's fake view directions, and its warning, when the network uses view directions), every chunk of eval_batch_size
    points goes through `occu_net(xyz (1,N,3), coarse=, viewdirs=)`; runs under torch.no_grad() in eval mode, the network's
    train / eval flag is restored.
    :param coarse which network: True / False, or a tuple of them -> the element-wise MAXIMUM over those passes
    :return (sigmas (prod reso,) float32 on the device -- `.view(*reso)` is the grid, x the slowest axis --, reso as a list of ints)
    """
    from .. import ops
    use_viewdirs = bool(getattr(occu_net, "use_viewdirs", False))
    if use_viewdirs:
        warnings.warn("Running marching cubes with fake view dirs (pointing to origin), output may be invalid")
    if int(getattr(occu_net, "num_objs", 1) or 1) > 1:
        raise ValueError(f"{what}: the network encoded {int(occu_net.num_objs)} objects; encode one object")
    reso = [int(r) for r in reso]
    if len(reso) != 3 or len(c1) != 3 or len(c2) != 3:
        raise ValueError(f"{what}: c1, c2, reso must have 3 entries each")
    if device is None:
        device = next(occu_net.parameters()).device
    device = torch.device(device)
    passes = tuple(coarse) if isinstance(coarse, (tuple, list)) else (coarse,)
    total = reso[0] * reso[1] * reso[2]
    is_train = bool(getattr(occu_net, "training", False))
    if hasattr(occu_net, "eval"):
        occu_net.eval()
    try:
        with torch.no_grad():
            sigmas = torch.empty((total,), dtype=torch.float32, device=device)
            for first in range(0, total, int(eval_batch_size)):
                count = min(int(eval_batch_size), total - first)
                pnts, vd = ops.gen_grid_points(c1, c2, reso, first, count, device=device, viewdirs=use_viewdirs)
                for n, which in enumerate(passes):
                    outputs = occu_net(pnts[None], coarse=which, viewdirs=vd[None] if use_viewdirs else None)
                    sigma = outputs.reshape(count, -1)[:, sigma_idx]
                    sigmas[first:first + count] = sigma if n == 0 else torch.maximum(sigmas[first:first + count], sigma)
    finally:
        if is_train:
            occu_net.train()
    return sigmas, reso


def marching_cubes(
    occu_net,
    c1=[-1, -1, -1],
    c2=[1, 1, 1],
    reso=[128, 128, 128],
    isosurface=50.0,
    sigma_idx=3,
    eval_batch_size=100000,
    coarse=True,
    device=None,
    align_to_grid=False,
    as_tensors=False,
):
    """
    Run marching cubes on network (src/util/recon.py:12-78), on the device.
    WARNING: does not make much sense with viewdirs in current form, since sigma depends on viewdirs.
    :param occu_net main NeRF type network: any model(xyz (1,N,3), coarse=, viewdirs=) -> (1,N,C) callable that encoded ONE object
    :param c1 corner 1 of marching cube bounds x,y,z
    :param c2 corner 2 of marching cube bounds x,y,z (all > c1)
    :param reso resolutions of marching cubes x,y,z (>= 2 each)
    :param isosurface sigma-isosurface of marching cubes
    :param sigma_idx index of 'sigma' value in last dimension of occu_net's output
    :param eval_batch_size batch size for evaluation
    :param coarse whether to use coarse NeRF for evaluation
    :param device optionally, device to put points for evaluation. By default uses device of occu_net's first parameter.
    :param align_to_grid the reference scales grid indices by (c2 - c1) / reso (recon.py:74) although the points it evaluated
    are (c2 - c1) / (reso - 1) apart, which shrinks the mesh towards c1 by a factor (reso - 1) / reso.  False keeps that; True
    uses the true spacing, so that a vertex lies where its density was sampled.
    :param as_tensors return device tensors (vertices float32, triangles int32) instead of numpy arrays
    :return vertices (V,3) float64, triangles (T,3) int32 (numpy, like the reference)
    """
    from .. import ops
    sigmas, reso = density_grid(occu_net, c1, c2, reso, coarse=coarse, sigma_idx=sigma_idx, eval_batch_size=eval_batch_size,
                                device=device, what="marching_cubes")
    lo, hi = np.array(c1, dtype=np.float64), np.array(c2, dtype=np.float64)
    scale = (hi - lo) / (np.array(reso) - 1 if align_to_grid else np.array(reso))
    vertices, triangles = ops.marching_cubes(sigmas.view(*reso), float(isosurface), c1=lo, scale=scale)
    if as_tensors:
        return vertices, triangles
    return vertices.cpu().numpy().astype(np.float64), triangles.cpu().numpy()


def save_obj(vertices, triangles, path, vert_rgb=None):
    """
    Save OBJ file, optionally with vertex colors (src/util/recon.py:81-106: `v %.4f ...` lines, then 1-based `f %d %d %d`
    lines).  One format operation per block of lines instead of a Python loop per vertex.
    :param vertices (N, 3)
    :param triangles (N, 3)
    :param vert_rgb (N, 3) rgb
    """
    to_np = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)  # noqa: E731
    v = to_np(vertices).reshape(-1, 3)
    line = "v %.4f %.4f %.4f\n"
    if vert_rgb is not None:
        v = np.concatenate((v, to_np(vert_rgb).reshape(-1, 3)), axis=1)
        line = "v %.4f %.4f %.4f %.4f %.4f %.4f\n"
    f = to_np(triangles).reshape(-1, 3).astype(np.int64) + 1
    with open(path, "w") as file:
        file.write((line * v.shape[0]) % tuple(v.reshape(-1).tolist()))
        file.write(("f %d %d %d\n" * f.shape[0]) % tuple(f.reshape(-1).tolist()))
