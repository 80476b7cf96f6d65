"""
CPU tests of tests/position_ref.py, the fp64 reference that tests/test_hip_position_stage.py holds the position and camera gradient
kernels to: the forward chain against the oracle's own functions, the fp64 autograd gradients against central differences, and the
conditions every case of the GPU list has to meet so that no GPU test can hide a failure behind them (few masked rows, finite
references, a torch-fp32 error far below the cap of the bar, the border clip exercised in both axes and in one axis alone).
"""
import pytest
import torch

import position_ref as PR
from oracle import pnr_oracle as O

ALL_CASES = PR.CASES + [PR.GRID_CASE, PR.CHILD_CASE]


@pytest.mark.parametrize("case", [PR.TINY_CASE, PR.CASES[4], PR.CASES[7]], ids=lambda c: c.name)
def test_chain_matches_oracle_forward(case):
    """chain at float32 == O.positional_encoding / O.index_latent on the same points, rows view * P + point"""
    inp = PR.make_inputs(case)
    NS, SB = inp["NS"], inp["SB"]
    in42, zlat = PR.chain(inp["rays"], inp["z"], inp["poses"], inp["focal"], inp["c"], inp["latent"], inp["image_shape"], NS,
                          torch.float32)
    r, z = inp["rays"], inp["z"]
    B = (inp["R"] // SB) * inp["K"]
    xyz = (r[:, None, :3] + z.unsqueeze(2) * r[:, None, 3:6]).reshape(SB, B, 3)
    vd = r[:, None, 3:6].expand(-1, inp["K"], -1).reshape(SB, B, 3)
    poses = inp["poses"]
    xyz_rot = torch.matmul(poses[:, None, :3, :3], O.repeat_interleave(xyz, NS).unsqueeze(-1))[..., 0]
    xyz_cam = xyz_rot + poses[:, None, :3, 3]
    code = O.positional_encoding(xyz_rot.reshape(-1, 3))
    vdr = torch.matmul(poses[:, None, :3, :3], O.repeat_interleave(vd, NS).unsqueeze(-1)).reshape(-1, 3)
    uv = -xyz_cam[:, :, :2] / xyz_cam[:, :, 2:]
    focal, c = inp["focal"], inp["c"]
    uv = uv * O.repeat_interleave(focal.unsqueeze(1), NS if focal.shape[0] > 1 else 1)
    uv = uv + O.repeat_interleave(c.unsqueeze(1), NS if c.shape[0] > 1 else 1)
    lat = O.index_latent(inp["latent"], uv, inp["image_shape"]).transpose(1, 2)  # (SB*NS, B, 512), row obj * NS + view
    to_kernel_rows = lambda t: t.reshape(SB, NS, B, -1).permute(1, 0, 2, 3).reshape(NS * SB * B, -1)
    ref42 = to_kernel_rows(torch.cat((code, vdr), dim=1))
    e42, ez = float((in42 - ref42).abs().max()), float((zlat - to_kernel_rows(lat)).abs().max())
    print(f"{case.name}: chain fp32 vs oracle: in42 {e42:.2e} zlat {ez:.2e}")
    assert e42 <= 1e-6 and ez <= 1e-6


def test_fp64_gradients_match_central_differences():
    """R = 3, K = 5, NS = 2: every entry of d_z, d_rays[:, :6], d_poses, d_focal, d_c and 48 seeded entries of d_latent against
    central differences of L in fp64, step 1e-6, to 1e-6 of the tensor's largest entry"""
    inp = PR.make_inputs(PR.TINY_CASE)
    f64 = torch.float64
    ref = PR.gradients(inp, f64)
    gen = torch.Generator().manual_seed(3)
    h = 1e-6
    for name in PR.TENSORS:
        base = inp[name].double()
        want = ref[name]
        n = base.numel()
        cols = 6 if name == "rays" else None
        if name == "latent":
            picks = torch.randint(0, n, (48,), generator=gen).tolist()
        elif name == "rays":
            picks = [r * 8 + j for r in range(base.shape[0]) for j in range(6)]
        else:
            picks = list(range(n))
        worst = 0.0
        for i in picks:
            vals = []
            for sgn in (1.0, -1.0):
                t = base.clone()
                t.view(-1)[i] += sgn * h
                vals.append(float(sum(PR.loss(inp, f64, **{name: t}))))
            fd = (vals[0] - vals[1]) / (2 * h)
            w = want.reshape(-1, cols)[i // 8, i % 8] if cols else want.reshape(-1)[i]
            worst = max(worst, abs(fd - float(w)))
        rel = worst / float(want.abs().max())
        print(f"finite differences {name}: {rel:.2e} of max|grad| over {len(picks)} entries")
        assert rel <= 1e-6, (name, rel)


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.name)
def test_case_conditions(case):
    inp, ref64, ref32 = PR.reference(case)
    st = inp["stats"]
    err32 = PR.errors(ref32, ref64)
    lind = {ld: PR.error(PR.near_far(inp, ref32["z"], ld, torch.float32), PR.near_far(inp, ref64["z"], ld, torch.float64))
            for ld in (False, True)}
    print(f"{case.name}: rows {st['rows']} masked {100 * st['masked']:.2f} % off-image x {100 * st['off_x']:.0f} % y "
          f"{100 * st['off_y']:.0f} % one axis only {st['one_axis']}; torch-fp32 " +
          " ".join(f"{k} {v:.1e}" for k, v in err32.items()) + f" near/far {lind[False]:.1e} lindisp {lind[True]:.1e}")
    assert st["masked"] <= 0.01
    assert all(bool(torch.isfinite(t).all()) for t in ref64.values())
    assert all(e <= 2e-5 for e in err32.values()), err32
    assert all(e <= 2e-5 for e in lind.values()), lind
    assert st["off_x"] >= 0.10 and st["off_y"] >= 0.10
    assert st["one_axis"] >= 1
    assert not bool(inp["g_z"][inp["mask"]].any())


def test_hostile_inputs_leave_a_finite_reference():
    """the dropped-record inputs: three distinct rows, the plane sample at xc2 == 0 exactly in the kernels' view 0, and a finite fp64
    reference once their contributions are removed"""
    inp, z_views, dropped = PR.hostile_inputs()
    assert len(set(dropped)) == 3 and inp["stats"]["masked"] <= 0.01
    geo = PR.geometry(inp["rays"], inp["z"], inp["poses"], inp["focal"], inp["c"], inp["latent"].shape[-2:], inp["image_shape"],
                      inp["NS"], torch.float32)
    assert float(geo["xc"][0, 0, 3, 2]) == 0.0
    assert torch.isinf(inp["g_in"][dropped[1]]).sum() == 1 and torch.isnan(inp["g_in"][dropped[2]]).sum() == 1
    ref64 = PR.reference_without(inp, z_views, dropped, torch.float64)
    err32 = PR.errors(PR.reference_without(inp, z_views, dropped, torch.float32), ref64)
    print("hostile inputs: torch-fp32 " + " ".join(f"{k} {v:.1e}" for k, v in err32.items()))
    assert all(bool(torch.isfinite(t).all()) for t in ref64.values())
    assert all(e <= 2e-5 for e in err32.values()), err32
