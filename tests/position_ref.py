"""Test helper (not a test): the geometry chain sample -> world point -> rotated point -> positional code / view direction /
projection / bilinear lookup in plain torch at any dtype, its gradients by torch autograd, and the seeded inputs, edge mask, error
and bar that tests/test_position_ref_host.py and tests/test_hip_position_stage.py share.  No GPU, no package import.

What is differentiated (the forward of oracle/pnr_oracle.py: pixelnerf_forward up to the MLP input):
    x = o + z d,  xr = R x,  xc = xr + t                                          (nerf.py:185, models.py:161-165)
    in42 = [xr, sin(f_k xr), sin(f_k xr + fp32(pi/2)), R d],  f_k = 1.5 * 2^k     (code.py:37-41, models.py:188-196)
    uv = -xc[:2] / xc[2] * focal + c,  zlat = border-clamped bilinear lookup      (models.py:206-215, encoder.py:96-109)
    L = sum in42 . g_in + sum zlat . g_z
Rows are ordered as the kernels take them: view * P + point, point = ray * K + k, rays object-major.

The bilinear derivative jumps at cell edges and at the border clip.  edge_mask() marks every row whose fp64 grid coordinate lies
within 1e-3 texel of such a jump (or within 1e-3 of a source camera's plane) and make_inputs() zeroes those rows of g_z: the lookup
term of such a sample is then zero whichever cell is differentiated, and every other term is smooth.  point_grad and grid_coords
disagree by a few ulp of a coordinate <= 200, i.e. <= 1e-4 texel, so 1e-3 leaves a decade.
"""
import collections
import functools
import math

import torch

import composite_bwd_ref as CR
from oracle import pnr_oracle as O
from testdata import synthetic

BAR_FLOOR, BAR_CAP, BAR_FACTOR = 2e-6, 2e-4, 10.0
EPS = 1e-3

# name, scene, rays per object, K, focal / c as (SB,2) rows with distinct values, (Hl, Wl) of a replacement grid or None, seed
Case = collections.namedtuple("Case", "name scene per_obj K rows grid seed")
CASES = [
    Case("train_23x89", "train", 23, 89, False, None, 1),       # 2047 samples per object: one CAM_CHUNK, K > 64
    Case("train_32x64", "train", 32, 64, False, None, 2),       # 2048: an exactly full chunk
    Case("train_3x683", "train", 3, 683, False, None, 25),       # 2049: a one-sample ragged second chunk
    Case("mv_mini_24x96", "mv_mini", 24, 96, False, None, 4),   # two chunks, two views, two objects
    Case("dtu_mini_64x24", "dtu_mini", 64, 24, False, None, 5),  # 15 x 20 grid, fx != fy, off-centre c
    Case("train_mv3_33x65", "train_mv3", 33, 65, False, None, 6),  # NS * P = 12870: no multiple of the 4 waves per block
    Case("mv_mini_5x1", "mv_mini", 5, 1, False, None, 7),       # K = 1
    Case("mv_mini_24x96_rows", "mv_mini", 24, 96, True, None, 8),  # n_focal, n_c > 1
]
CASE_IDS = [c.name for c in CASES]
# the latent scatter alone: a 72 x 80 grid (the tiled form; the global-atomic form with PIXELNERF_SCATTER_TILED=0)
GRID_CASE = Case("mv_mini_72x80", "mv_mini", 24, 20, False, (72, 80), 9)
CHILD_CASE = Case("plane_mini_72x80", "plane_mini", 23, 9, False, (72, 80), 13)  # SB = 1, NS = 2, P = 207: no multiple of the run of 16
TINY_CASE = Case("srn_mini_3x5", "srn_mini", 3, 5, False, None, 11)         # finite differences
TENSORS = ("z", "rays", "poses", "focal", "c", "latent")


# ------------------------------------------------------------------------------------------------ forward chain
def _latent_scaling(Wl, Hl):
    ls = torch.tensor([Wl, Hl], dtype=torch.float32)
    return ls / (ls - 1) * 2.0  # encoder.py:161-163, the fp32 values


def geometry(rays, z, poses, focal, c, latent_hw, image_shape, NS, dtype):
    """-> dict of (NS, SB, N, .) tensors at `dtype`: xr (rotated point), vd (rotated direction), xc, and the UNCLAMPED grid position
    ix, iy.  z is (R, K), or (NS, R, K) with a depth of its own per view (the per-view dL/dz)."""
    Hl, Wl = latent_hw
    rays, poses, focal, c = (t.to(dtype) for t in (rays, poses, focal, c))
    zv = z.to(dtype)
    R = rays.shape[0]
    SB = poses.shape[0] // NS
    if zv.dim() == 2:
        zv = zv.unsqueeze(0).expand(NS, -1, -1)
    K = zv.shape[-1]
    N = (R // SB) * K
    o, d = rays[:, :3], rays[:, 3:6]
    # the oracle's own operations in its own layout (row obj * NS + view), so that the float32 chain rounds as it does
    to_nv = lambda t: t.reshape(NS, SB, N, 3).permute(1, 0, 2, 3).reshape(SB * NS, N, 3)
    x = to_nv(o[None, :, None, :] + zv[..., None] * d[None, :, None, :])                       # nerf.py:185, models.py:161
    dd = to_nv(d[None, :, None, :].expand(NS, R, K, 3))
    xr = torch.matmul(poses[:, None, :3, :3], x.unsqueeze(-1))[..., 0]                         # models.py:162-164
    vd = torch.matmul(poses[:, None, :3, :3], dd.unsqueeze(-1))[..., 0]                        # models.py:188-193
    xc = xr + poses[:, None, :3, 3]                                                            # models.py:165
    uv = -xc[..., :2] / xc[..., 2:]                                                            # models.py:206
    uv = uv * O.repeat_interleave(focal.unsqueeze(1), NS if focal.shape[0] > 1 else 1)         # (1 | SB, 2) rows
    uv = uv + O.repeat_interleave(c.unsqueeze(1), NS if c.shape[0] > 1 else 1)
    to_views = lambda t: t.reshape(SB, NS, N, -1).permute(1, 0, 2, 3)
    xr, vd, xc, uv = (to_views(t) for t in (xr, vd, xc, uv))
    scale = _latent_scaling(Wl, Hl).to(dtype) / image_shape.to(torch.float32).to(dtype)        # encoder.py:98
    g = uv * scale - 1.0
    ix = ((g[..., 0] + 1) / 2) * (Wl - 1)
    iy = ((g[..., 1] + 1) / 2) * (Hl - 1)
    return dict(xr=xr, vd=vd, xc=xc, ix=ix, iy=iy)


def positional_code(x):
    """code.py:37-41 on (N, 3) at x's dtype; the phase constant is fp32(pi / 2) cast up"""
    freqs = torch.repeat_interleave(1.5 * 2.0 ** torch.arange(0, 6), 2).view(1, -1, 1).to(x.dtype)
    phases = torch.zeros(12)
    phases[1::2] = math.pi * 0.5
    phases = phases.view(1, -1, 1).to(x.dtype)
    embed = torch.sin(torch.addcmul(phases, x.unsqueeze(1).repeat(1, 12, 1), freqs))
    return torch.cat((x, embed.view(x.shape[0], -1)), dim=-1)


def lookup(latent, ix, iy, NS):
    """index_latent's border-clamped bilinear lookup with the oracle's NaN -> texel 0 rule.  latent (SB*NS, C, Hl, Wl);
    ix, iy (NS, SB, N) unclamped -> (NS, SB, N, C)"""
    NV, C, Hl, Wl = latent.shape
    SB = NV // NS
    ix, iy = torch.clamp(ix, 0, Wl - 1), torch.clamp(iy, 0, Hl - 1)
    ix = torch.where(torch.isnan(ix), torch.zeros_like(ix), ix)
    iy = torch.where(torch.isnan(iy), torch.zeros_like(iy), iy)
    ix0, iy0 = torch.floor(ix), torch.floor(iy)
    ix1, iy1 = ix0 + 1, iy0 + 1
    cl = latent.reshape(SB, NS, C, Hl * Wl).permute(1, 0, 3, 2)  # (NS, SB, Hl*Wl, C)

    def corner(iyc, ixc, w):
        inb = (ixc <= Wl - 1) & (iyc <= Hl - 1)
        flat = (iyc.clamp(0, Hl - 1) * Wl + ixc.clamp(0, Wl - 1)).long()
        vals = torch.gather(cl, 2, flat.unsqueeze(-1).expand(-1, -1, -1, C))
        return vals * (w * inb.to(w.dtype)).unsqueeze(-1)

    out = corner(iy0, ix0, (ix1 - ix) * (iy1 - iy))
    out = out + corner(iy0, ix1, (ix - ix0) * (iy1 - iy))
    out = out + corner(iy1, ix0, (ix1 - ix) * (iy - iy0))
    return out + corner(iy1, ix1, (ix - ix0) * (iy - iy0))


def chain(rays, z, poses, focal, c, latent, image_shape, NS, dtype):
    """-> (in42 (NS*P, 42), zlat (NS*P, 512)) at `dtype`"""
    latent = latent.to(dtype)
    g = geometry(rays, z, poses, focal, c, latent.shape[-2:], image_shape, NS, dtype)
    in42 = torch.cat((positional_code(g["xr"].reshape(-1, 3)), g["vd"].reshape(-1, 3)), dim=-1)
    return in42, lookup(latent, g["ix"], g["iy"], NS).reshape(-1, latent.shape[1])


def edge_mask(ix, iy, Wl, Hl, eps=EPS, xc2=None):
    """rows whose lookup derivative may jump: a coordinate within eps of an integer while within eps of [0, size - 1] (cell edges
    and both ends of the border clip), or a point within 1e-3 of the source camera's plane.  fp64 unclamped coordinates."""
    def near_edge(v, last):
        return ((v - torch.round(v)).abs() < eps) & (v > -eps) & (v < last + eps)
    m = near_edge(ix, Wl - 1) | near_edge(iy, Hl - 1)
    if xc2 is not None:
        m = m | (xc2.abs() < 1e-3)
    return m


# ------------------------------------------------------------------------------------------------ inputs
def with_samples(base, z, gen, z_views=None):
    """`base` (the scene and rays of a case) with the sample positions z (R, K) and fresh upstream gradients drawn from `gen`;
    the masked rows of g_z are zeroed.  z_views (NS, R, K): the depths the mask and the reference take per view, where they are
    not z (hostile_inputs)."""
    inp = dict(base)
    NS, R, K = inp["NS"], inp["R"], z.shape[1]
    rows = NS * R * K
    g_in = torch.randn(rows, 42, generator=gen)
    g_z = torch.randn(rows, 512, generator=gen)
    Hl, Wl = inp["latent"].shape[-2:]
    geo = geometry(inp["rays"], z if z_views is None else z_views, inp["poses"], inp["focal"], inp["c"], (Hl, Wl),
                   inp["image_shape"], NS, torch.float64)
    ix, iy, xc2 = geo["ix"].reshape(-1), geo["iy"].reshape(-1), geo["xc"][..., 2].reshape(-1)
    mask = edge_mask(ix, iy, Wl, Hl, EPS, xc2)
    g_z[mask] = 0.0
    off_x, off_y = (ix <= 0) | (ix >= Wl - 1), (iy <= 0) | (iy >= Hl - 1)
    stats = dict(rows=rows, masked=float(mask.double().mean()), off_x=float(off_x.double().mean()),
                 off_y=float(off_y.double().mean()), one_axis=int((off_x ^ off_y).sum()))
    inp.update(z=z.contiguous(), K=K, g_in=g_in, g_z=g_z, mask=mask, stats=stats)
    return inp


def _build(case):
    """everything in fp32 from seeded generators"""
    scene, meta = synthetic.make_scene(case.scene, seed=2)
    scene = dict(scene)
    gen = torch.Generator().manual_seed(1000 + case.seed)
    SB, NS = scene["SB"], scene["NS"]
    if case.grid is not None:
        scene["latent"] = torch.randn(SB * NS, 512, case.grid[0], case.grid[1], generator=gen) * 0.5
    if case.rows:  # distinct intrinsics per object
        k = torch.arange(SB, dtype=torch.float32)[:, None]
        scene["focal"] = (scene["focal"] * (1.0 + 0.07 * k * torch.tensor([[1.0, -0.6]]))).contiguous()
        scene["c"] = (scene["c"] + k * torch.tensor([[1.75, -2.5]])).contiguous()
    rays = synthetic.target_rays(meta, n_rays=case.per_obj, seed=7 + case.seed).reshape(-1, 8).contiguous()
    R = rays.shape[0]
    base = dict(case=case, rays=rays, poses=scene["poses"], focal=scene["focal"], c=scene["c"], latent=scene["latent"],
                image_shape=scene["image_shape"], NS=NS, SB=SB, R=R, gen=gen)
    return with_samples(base, O.sample_coarse(rays, torch.rand(R, case.K, generator=gen), case.K, False), gen)


@functools.lru_cache(maxsize=None)
def make_inputs(case):
    """the seeded fp32 inputs of one case (shared: treat as read-only)"""
    return _build(case)


HOSTILE_CASE = Case("mv_mini_hostile", "mv_mini", 5, 7, False, None, 15)
DEPTH_CASE = Case("mv_mini_depth", "mv_mini", 24, 32, False, None, 14)  # 32 coarse samples; the fine set is merged by the test


def hostile_inputs():
    """HOSTILE_CASE with three records that both kernels have to drop, -> (inputs, z_views, dropped rows):
      * sample (ray 0, k = 3) lies exactly on the plane of source camera (object 0, view 0): that pose is [I | 0], the ray starts at
        (0.3, 0.2, -1) along (0, 0, 1) and z = 1, so xc2 = 0 with or without contraction;
      * one row of g_in holds +inf -- in a column c < 3 of a row where d_k R_ck has one sign for k = 0, 1, 2, so that the infinity
        reaches dL/dz as an infinity instead of cancelling into a NaN;
      * one row of g_in holds NaN.
    inputs["g_in"] / ["g_z"] are what the kernels get; `dropped` lists the three rows, whose contributions the reference removes
    (reference_without); z_views moves the plane sample of view 0 to z = 1.1 for the reference, where its zeroed row is finite."""
    base = dict(make_inputs(HOSTILE_CASE))
    gen = torch.Generator().manual_seed(77)
    poses, rays, z = base["poses"].clone(), base["rays"].clone(), base["z"].clone()
    poses[0] = torch.eye(4)[:3]
    rays[0] = torch.tensor([0.3, 0.2, -1.0, 0.0, 0.0, 1.0, 0.5, 4.0])
    z[0] = torch.tensor([0.55, 0.7, 0.9, 1.0, 1.6, 2.5, 3.9])
    base.update(poses=poses, rays=rays)
    NS, R, K = base["NS"], base["R"], z.shape[1]
    z_views = z.unsqueeze(0).repeat(NS, 1, 1)
    z_views[0, 0, 3] = 1.1
    inp = with_samples(base, z, gen, z_views=z_views)
    P = R * K
    d, rot = rays[:, 3:6], poses[:, :, :3]
    row_inf = None
    for v, r, col in ((v, r, col) for v in range(NS) for r in range(1, R) for col in range(3)):
        prod = d[r] * rot[(r // (R // base["SB"])) * NS + v, col]
        if row_inf is None and (bool((prod > 1e-3).all()) or bool((prod < -1e-3).all())):
            row_inf, col_inf = v * P + r * K + 2, col
    assert row_inf is not None
    row_plane, row_nan = 0 * P + 0 * K + 3, 0 * P + (R - 1) * K + 5
    inp["g_in"][row_inf, col_inf] = float("inf")
    inp["g_in"][row_nan, 17] = float("nan")
    return inp, z_views, [row_plane, row_inf, row_nan]


def reference_without(inp, z_views, dropped, dtype):
    """the gradients with the contributions of the `dropped` rows removed"""
    g_in, g_z = inp["g_in"].clone(), inp["g_z"].clone()
    g_in[dropped] = 0.0
    g_z[dropped] = 0.0
    return gradients(inp, dtype, z_views=z_views, g_in=g_in, g_z=g_z)


# ------------------------------------------------------------------------------------------------ gradients
def loss(inp, dtype, rays=None, z=None, poses=None, focal=None, c=None, latent=None, g_in=None, g_z=None):
    """L = sum in42 . g_in + sum zlat . g_z at `dtype`; every named argument replaces the input of that name"""
    pick = lambda v, k: inp[k] if v is None else v
    in42, zlat = chain(pick(rays, "rays"), pick(z, "z"), pick(poses, "poses"), pick(focal, "focal"), pick(c, "c"),
                       pick(latent, "latent"), inp["image_shape"], inp["NS"], dtype)
    return (in42 * pick(g_in, "g_in").to(dtype)).sum(), (zlat * pick(g_z, "g_z").to(dtype)).sum()


def gradients(inp, dtype, z_views=None, g_in=None, g_z=None, halves=False):
    """torch autograd of L at `dtype` -> dict: z_views (NS, R, K) the per-view dL/dz, z (R, K) their sum, rays (R, 6), poses
    (SB*NS, 3, 4), focal, c, latent (SB*NS, 512, Hl, Wl).  z_views: depths used in place of inp["z"], per view (the dropped-record
    test moves one sample of one view off a camera plane).  halves: -> (through g_in alone, through g_z alone) instead."""
    NS = inp["NS"]
    leaf = lambda t: t.detach().clone().to(dtype).requires_grad_(True)
    zv = leaf(inp["z"].unsqueeze(0).repeat(NS, 1, 1) if z_views is None else z_views)
    rays = leaf(inp["rays"])
    leaves = dict(z_views=zv, rays=rays, poses=leaf(inp["poses"]), focal=leaf(inp["focal"]), c=leaf(inp["c"]),
                  latent=leaf(inp["latent"]))
    l_in, l_z = loss(inp, dtype, rays=rays, z=zv, poses=leaves["poses"], focal=leaves["focal"], c=leaves["c"],
                     latent=leaves["latent"], g_in=g_in, g_z=g_z)

    def grads(L):
        g = torch.autograd.grad(L, list(leaves.values()), retain_graph=True, allow_unused=True)
        out = {k: (torch.zeros_like(leaves[k]) if v is None else v) for k, v in zip(leaves, g)}
        out["rays"] = out["rays"][:, :6].clone()
        out["z"] = out["z_views"].sum(0)
        return out
    if halves:
        return grads(l_in), grads(l_z)
    return grads(l_in + l_z)


def recover_u(rays, z, lindisp, dtype=torch.float64):
    """the jitter u1 that O.sample_coarse maps onto z (R, K), so that the sampling maps restated for test_sample_bounds_backward_*
    (composite_bwd_ref.coarse_map_ref) are differentiated at exactly these samples"""
    rays, z = rays.to(dtype), z.to(dtype)
    near, far = rays[:, 6:7], rays[:, 7:8]
    s = (1 / z - 1 / near) / (1 / far - 1 / near) if lindisp else (z - near) / (far - near)
    K = z.shape[1]
    return (s - torch.linspace(0, 1 - 1.0 / K, K)[None].to(dtype)) * K


def near_far(inp, dz, lindisp, dtype, d_far=None, depth=None):
    """(R, 2): dL/d near, dL/d far of dz (R, K) = dL/dz through z = near (1 - s) + far s (lindisp: 1/z linear in s), plus d_far (R).
    depth = (ranks, n4, depth_c, depth_std): the depth samples z = clamp(depth_c + n4 std) (nerf.py:157-160) reach near / far
    only where the clamp is active, whole (include/pixelnerf_hip.h: pnr_camera_backward) -- the unclamped ones belong to the
    coarse depth."""
    dz = dz.detach().to(dtype).clone()
    extra = torch.zeros(inp["R"], 2, dtype=dtype)
    if depth is not None:
        ranks, n4, depth_c, depth_std = depth
        state = clamp_state(inp["rays"], n4, depth_c, depth_std)
        dzd = torch.gather(dz, 1, ranks.long())
        extra[:, 0] = (dzd * (state < 0)).sum(1)
        extra[:, 1] = (dzd * (state > 0)).sum(1)
        dz.scatter_(1, ranks.long(), 0.0)
    u = recover_u(inp["rays"], inp["z"], lindisp)
    _, d_rays = CR.coarse_map_ref(inp["rays"], u, dz, inp["K"], lindisp, dtype)
    out = d_rays[:, 6:8] + extra
    if d_far is not None:
        out[:, 1] += d_far.to(dtype)
    return out


def clamp_state(rays, n4, depth_c, depth_std):
    """(R, Kfd) int: -1 clamped at near (zraw <= near), +1 at far (zraw >= far), 0 live; fp64"""
    zraw = depth_c.double()[:, None] + n4.double() * float(depth_std)
    near, far = rays[:, 6:7].double(), rays[:, 7:8].double()
    return (zraw >= far).to(torch.int64) - (zraw <= near).to(torch.int64)


def depth_contrib(inp, dz_views, dz_comp, depth):
    """include/pixelnerf_hip.h: pnr_depth_sample_backward.  contrib[v][r][j] = [near < depth_c[r] + n4[r][j] std < far] *
    (dz_views[v][r][ranks[r][j]] + (dz_comp[r][ranks[r][j]] for v = 0)) -> (NS, R, Kfd)"""
    ranks, n4, depth_c, depth_std = depth
    idx = ranks.long()[None].expand(dz_views.shape[0], -1, -1)
    val = torch.gather(dz_views, 2, idx).clone()
    if dz_comp is not None:
        val[0] += torch.gather(dz_comp.to(val.dtype), 1, ranks.long())
    live = clamp_state(inp["rays"], n4, depth_c, depth_std) == 0
    return val * live[None].to(val.dtype)


# ------------------------------------------------------------------------------------------------ error and bar
def error(got, ref64):
    """max|got - ref| / max|ref|"""
    den = float(ref64.abs().max())
    dif = float((got.double() - ref64).abs().max())
    return dif / den if den > 0 else dif


def errors(got, ref64):
    """per tensor name, for the names both dicts hold"""
    return {k: error(got[k], ref64[k]) for k in ref64 if k in got}


def bar_from(err32):
    """10 x the error of torch's fp32 autograd through the same chain on the same inputs, floor 2e-6, cap 2e-4"""
    return min(max(BAR_FACTOR * err32, BAR_FLOOR), BAR_CAP)


@functools.lru_cache(maxsize=None)
def reference(case):
    """-> (inputs, fp64 gradients, torch-fp32 gradients) of one case, computed once"""
    inp = make_inputs(case)
    return inp, gradients(inp, torch.float64), gradients(inp, torch.float32)
