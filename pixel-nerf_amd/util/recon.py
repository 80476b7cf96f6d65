"""
Mesh reconstruction tools: src/util/recon.py on the device.

The reference evaluates sigma on a grid chunk by chunk, gathers it on the host and calls PyMCubes.  Here the grid points come from
pnr_gen_grid_points, every chunk goes through `occu_net(xyz[None], coarse=, viewdirs=)` (the fused HIP network for a PixelNeRFNet),
the sigma column is gathered into one device grid, and pnr_marching_cubes_count / pnr_marching_cubes_emit extract an indexed mesh
on the device (semantics: include/pixelnerf_hip.h).  Beyond the reference: remove_floaters drops the stray blobs of a grid
(connected components, pnr_grid_components), vertex_normals / vertex_colors give the attributes save_obj / save_ply can write, and
extract_mesh chains all of it.  Deviations from the reference, all deliberate:
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


def remove_floaters(field, isosurface, keep_largest=None, min_voxels=None):
    """
    Drop the stray blobs of a density grid: the connected components (ops.grid_components: voxels > isosurface, joined along the
    grid edges -- exactly the voxels marching cubes joins without a surface between them) that are too small.  A component is
    KEPT iff it has at least min_voxels voxels AND is among the keep_largest biggest; ties in size go to the component whose
    smallest linear voxel index is smaller (a stable sort on an integer key: the choice is the same on every run).  Every voxel of a
    dropped component is set to `isosurface`, which is outside under the mesher's `>` rule; all other values, non-finite ones
    included, are left as they are.  The labelling is HIP, the selection and the `where` are torch.
    :param field (nx,ny,nz) float32 grid on the device (density_grid(...)[0].view(*reso))
    :param keep_largest None or an int >= 1; :param min_voxels None or an int >= 1
    :return (filtered field, info) -- info: host ints n_components, n_kept, voxels_inside, voxels_dropped (one host
    synchronisation).  With both arguments None: (field itself, None) and nothing is launched.
    """
    keep_largest, min_voxels = _check_floater_args("remove_floaters", keep_largest, min_voxels)
    if keep_largest is None and min_voxels is None:
        return field, None
    from .. import ops
    labels, sizes, counts = ops.grid_components(field, float(isosurface))
    floor = 1 if min_voxels is None else min_voxels
    if keep_largest is None:
        keep_root = sizes >= floor
    else:
        order = torch.sort(-sizes.to(torch.int64), stable=True).indices[:keep_largest]  # biggest first, ties: smaller index first
        keep_root = torch.zeros_like(sizes, dtype=torch.bool)
        keep_root[order] = sizes[order] >= floor  # (fewer components than keep_largest: the rest of `order` has size 0)
    inside = labels >= 0
    dropped = inside & ~keep_root[labels.clamp(min=0).long()]
    filtered = torch.where(dropped, torch.full((), float(isosurface), dtype=field.dtype, device=field.device), field)
    n_in, n_comp, n_kept, n_drop = torch.cat((counts.long(), keep_root.sum()[None], dropped.sum()[None])).tolist()
    return filtered, {"n_components": n_comp, "n_kept": n_kept, "voxels_inside": n_in, "voxels_dropped": n_drop}


def _check_floater_args(what, keep_largest, min_voxels):
    out = []
    for name, v in (("keep_largest", keep_largest), ("min_voxels", min_voxels)):
        if v is not None and (isinstance(v, bool) or int(v) != v or int(v) < 1):
            raise ValueError(f"{what}: {name} must be None or an integer >= 1, got {v!r}")
        out.append(None if v is None else int(v))
    return out


def vertex_normals(field, vertices, c1, scale):
    """
    Unit normals at the vertices of a mesh cut from `field` (ops.grid_normals / pnr_grid_normals): minus the normalised gradient
    of the grid -- central differences, blended trilinearly at the vertex, per axis in world units -- so they point from inside
    (high sigma) to outside, the side the triangles of marching_cubes face; (0,0,0) where the gradient vanishes.
    :param field (nx,ny,nz) float32 on the device; :param vertices (V,3) float32, world coordinates
    :param c1, scale what the mesh was extracted with: vertex = index * scale + c1
    :return (V,3) float32 on the device
    """
    from .. import ops
    return ops.grid_normals(field, vertices, c1, scale)


_VIEWDIR_MODES = ("origin", "normal")


def _check_viewdirs(what, viewdirs):
    if isinstance(viewdirs, str) and viewdirs not in _VIEWDIR_MODES:
        raise ValueError(f"{what}: viewdirs must be 'origin', 'normal' or a (V,3) tensor, got {viewdirs!r}")


def origin_viewdirs(points):
    """the reference's fake view direction -p / |p| (src/util/recon.py:54) for arbitrary points; (0,0,0) at the origin"""
    nrm = torch.linalg.norm(points, dim=-1, keepdim=True)
    return torch.where(nrm > 0, -points / nrm, torch.zeros_like(points))


def vertex_colors(net, vertices, viewdirs="origin", normals=None, coarse=True, eval_batch_size=100000):
    """
    Colours at mesh vertices: the rgb of `net(xyz (1,N,3), coarse=, viewdirs=)` at the vertices, chunk by chunk, under
    torch.no_grad() in eval mode with the network's train / eval flag restored (as density_grid).
    :param viewdirs "origin": the reference's fake direction -p/|p| (recon.py:54), with density_grid's warning for a network that
    uses view directions; "normal": -normal, the camera looks straight at the surface (needs `normals`); or a (V,3) tensor.  A
    network that takes no view directions gets none.
    :param eval_batch_size the chunk length, rounded DOWN to an even number (at least 2): at precision "f16x3" a point's last bits
    depend on whether its place in the launch is even or odd (profiles/occupancy_notes.md), so with even chunks a vertex's colour
    does not depend on eval_batch_size.
    :return (V,3) float32 on the vertices' device
    """
    _check_viewdirs("vertex_colors", viewdirs)
    if isinstance(viewdirs, str) and viewdirs == "normal" and normals is None:
        raise ValueError("vertex_colors: viewdirs='normal' needs the normals")
    if not torch.is_tensor(vertices) or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError("vertex_colors: vertices must be a (V,3) tensor")
    use_viewdirs = bool(getattr(net, "use_viewdirs", False))
    vd = None
    if use_viewdirs:
        if isinstance(viewdirs, str) and viewdirs == "origin":
            warnings.warn("Running marching cubes with fake view dirs (pointing to origin), output may be invalid")
            vd = origin_viewdirs(vertices)
        elif isinstance(viewdirs, str):
            vd = -normals
        else:
            vd = viewdirs
        if not torch.is_tensor(vd) or tuple(vd.shape) != tuple(vertices.shape):
            raise ValueError(f"vertex_colors: the view directions must be a {tuple(vertices.shape)} tensor")
        vd = vd.to(device=vertices.device, dtype=vertices.dtype).contiguous()
    V = vertices.shape[0]
    chunk = max(2, int(eval_batch_size) // 2 * 2)
    colors = torch.empty((V, 3), dtype=torch.float32, device=vertices.device)
    is_train = bool(getattr(net, "training", False))
    if hasattr(net, "eval"):
        net.eval()
    try:
        with torch.no_grad():
            for first in range(0, V, chunk):
                sl = slice(first, min(first + chunk, V))
                out = net(vertices[sl][None], coarse=coarse, viewdirs=vd[sl][None] if use_viewdirs else None)
                colors[sl] = out.reshape(sl.stop - sl.start, -1)[:, :3]
    finally:
        if is_train:
            net.train()
    return colors


def extract_mesh(
    net,
    c1=[-1, -1, -1],
    c2=[1, 1, 1],
    reso=[128, 128, 128],
    isosurface=50.0,
    sigma_idx=3,
    eval_batch_size=100000,
    coarse=True,
    device=None,
    align_to_grid=False,
    keep_largest=None,
    min_voxels=None,
    normals=True,
    colors=True,
    viewdirs="origin",
):
    """
    A finished mesh of an encoded object, on the device: density_grid -> remove_floaters -> ops.marching_cubes -> vertex normals ->
    vertex colours.  c1 .. align_to_grid as marching_cubes (which this leaves unchanged); keep_largest / min_voxels as
    remove_floaters (both None: the grid is meshed as it is); viewdirs as vertex_colors; eval_batch_size is rounded down to an
    even number for the density grid too, so the mesh does not depend on it.  The normals are taken from the FILTERED
    field: a dropped voxel is adjacent only to outside voxels and to dropped ones, so the values around a kept surface are the
    unfiltered ones.
    :return DotMap(vertices (V,3) float32, triangles (T,3) int32, normals (V,3) float32 | None, colors (V,3) float32 | None,
    info: remove_floaters' dict | None), tensors on the device
    """
    from .. import ops
    from .dotmap import DotMap
    _check_viewdirs("extract_mesh", viewdirs)
    _check_floater_args("extract_mesh", keep_largest, min_voxels)
    eval_batch_size = max(2, int(eval_batch_size) // 2 * 2)  # even chunks: the result does not depend on it (vertex_colors)
    sigmas, reso = density_grid(net, c1, c2, reso, coarse=coarse, sigma_idx=sigma_idx, eval_batch_size=eval_batch_size,
                                device=device, what="extract_mesh")
    field, info = remove_floaters(sigmas.view(*reso), float(isosurface), keep_largest=keep_largest, min_voxels=min_voxels)
    lo, hi = np.array(c1, dtype=np.float64), np.array(c2, dtype=np.float64)
    scale = (hi - lo) / (np.array(reso) - 1 if align_to_grid else np.array(reso))
    vertices, triangles = ops.marching_cubes(field, float(isosurface), c1=lo, scale=scale)
    by_normal = isinstance(viewdirs, str) and viewdirs == "normal"
    nrm = vertex_normals(field, vertices, lo, scale) if normals or (colors and by_normal) else None
    rgb = None
    if colors:
        rgb = vertex_colors(net, vertices, viewdirs=viewdirs, normals=nrm, coarse=coarse, eval_batch_size=eval_batch_size)
    return DotMap(vertices=vertices, triangles=triangles, normals=nrm if normals else None, colors=rgb, info=info)


def save_obj(vertices, triangles, path, vert_rgb=None, vert_normals=None):
    """
    Save OBJ file, optionally with vertex colors (src/util/recon.py:81-106: `v %.4f ...` lines, then 1-based `f %d %d %d`
    lines).  One format operation per block of lines instead of a Python loop per vertex.
    :param vertices (N, 3)
    :param triangles (N, 3)
    :param vert_rgb (N, 3) rgb
    :param vert_normals (N, 3): `vn %.4f %.4f %.4f` lines after the `v` lines, and the faces as `f a//a b//b c//c`.  Without
    them the file is what the reference writes.
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
        if vert_normals is None:
            file.write(("f %d %d %d\n" * f.shape[0]) % tuple(f.reshape(-1).tolist()))
        else:
            vn = to_np(vert_normals).reshape(-1, 3)
            if vn.shape[0] != v.shape[0]:
                raise ValueError(f"save_obj: {vn.shape[0]} normals for {v.shape[0]} vertices")
            file.write(("vn %.4f %.4f %.4f\n" * vn.shape[0]) % tuple(vn.reshape(-1).tolist()))
            file.write(("f %d//%d %d//%d %d//%d\n" * f.shape[0]) % tuple(np.repeat(f.reshape(-1), 2).tolist()))


def save_ply(path, vertices, triangles, vert_rgb=None, vert_normals=None):
    """
    Save a binary little-endian PLY (numpy only): per vertex x y z float32, then nx ny nz float32 with normals, then red green
    blue uchar with colours (rgb in [0,1], rounded to 0..255); per face the list `uchar 3` + three int32 vertex indices.
    :param vertices (N, 3); :param triangles (M, 3); :param vert_rgb (N, 3) rgb in [0,1]; :param vert_normals (N, 3)
    """
    to_np = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)  # noqa: E731
    v = to_np(vertices).reshape(-1, 3)
    fields, props = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")], ["property float x", "property float y", "property float z"]
    if vert_normals is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        props += ["property float nx", "property float ny", "property float nz"]
    if vert_rgb is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        props += ["property uchar red", "property uchar green", "property uchar blue"]
    rows = np.empty(v.shape[0], dtype=np.dtype(fields))
    for a, name in enumerate("xyz"):
        rows[name] = v[:, a]
    if vert_normals is not None:
        vn = to_np(vert_normals).reshape(-1, 3)
        if vn.shape[0] != v.shape[0]:
            raise ValueError(f"save_ply: {vn.shape[0]} normals for {v.shape[0]} vertices")
        for a, name in enumerate(("nx", "ny", "nz")):
            rows[name] = vn[:, a]
    if vert_rgb is not None:
        rgb = to_np(vert_rgb).reshape(-1, 3)
        if rgb.shape[0] != v.shape[0]:
            raise ValueError(f"save_ply: {rgb.shape[0]} colours for {v.shape[0]} vertices")
        u8 = np.clip(np.rint(np.nan_to_num(rgb.astype(np.float64)) * 255.0), 0, 255).astype(np.uint8)
        for a, name in enumerate(("red", "green", "blue")):
            rows[name] = u8[:, a]
    t = to_np(triangles).reshape(-1, 3)
    faces = np.empty(t.shape[0], dtype=np.dtype([("n", "u1"), ("idx", "<i4", (3,))]))
    faces["n"] = 3
    faces["idx"] = t
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}"] + props + [
        f"element face {t.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as file:
        file.write(("\n".join(header) + "\n").encode("ascii"))
        file.write(rows.tobytes())
        file.write(faces.tobytes())
