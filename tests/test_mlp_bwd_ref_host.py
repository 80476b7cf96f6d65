"""
Host tests (no GPU) of tests/mlp_bwd_ref.py, the fp64 reference that tests/test_hip_mlp_backward_stage.py holds the fp32-class
MLP backward stage to.

  * the reference is PINNED: with the gates of its own forward it is float64 autograd through oracle.pnr_oracle.resnetfc_forward
    (the oracle's [object][view][point] rows, permuted), NS = 1, 2, 3, all 32 outputs, 1e-12 relative;
  * the committed bars BITE: three subtly wrong backwards miss the loosest committed bar by >= 10x on their worst output, while a
    plain float32 torch run of the same gated chain stays inside the tightest one.
"""
from unittest import mock

import numpy as np
import pytest
import torch

import mlp_bwd_ref as R
from helpers import mlp_params, scene_for
from oracle import pnr_oracle as O

B = 111  # points per object: no multiple of anything


def network_input(scene_name, seed=13):
    """-> (zx (SB*NS*B, 512 + 42) float32 in the oracle's [object][view][point] rows -- what models.py:227 hands to the MLP, SB, NS)"""
    scene, _ = scene_for(scene_name)
    SB = scene["SB"]
    gen = torch.Generator().manual_seed(seed)
    xyz = (torch.rand(SB, B, 3, generator=gen) - 0.5) * 1.6
    vd = torch.nn.functional.normalize(torch.randn(SB, B, 3, generator=gen), dim=-1)
    seen = {}
    inner = O.resnetfc_forward

    def grab(p, zx, dims, **kw):
        seen["zx"] = zx
        return inner(p, zx, dims, **kw)

    with mock.patch.object(O, "resnetfc_forward", grab), torch.no_grad():
        O.pixelnerf_forward(scene, mlp_params(11), xyz, vd)
    return seen["zx"], SB, scene["NS"]


def library_rows(SB, NS):
    """index of the oracle row (o*NS + v)*B + p at the library's row v*(SB*B) + o*B + p"""
    v, o, p = np.meshgrid(np.arange(NS), np.arange(SB), np.arange(B), indexing="ij")
    return torch.from_numpy(((o * NS + v) * B + p).reshape(-1))


def g_out_for(P, seed=5):
    return 1e-3 * torch.randn(P, 4, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("scene_name", ["train", "mv_mini", "train_mv3"])  # NS = 1, 2, 3
def test_reference_is_autograd_through_the_oracle(scene_name):
    zx, SB, NS = network_input(scene_name)
    P = SB * B
    g_out = g_out_for(P)
    # the oracle, float64, its own rows and its own relu
    p = {k: v.double().requires_grad_(True) for k, v in mlp_params(11).items()}
    zx64 = zx.double().requires_grad_(True)
    out = O.resnetfc_forward(p, zx64, (NS, B)).reshape(-1, 4)  # (SB, B, 4): [object][point], the library's point order
    assert out.shape == (P, 4)
    (out * g_out).sum().backward()
    rows = library_rows(SB, NS)
    want = {k: p[k].grad for k in R.PARAM_KEYS}
    want["d_zlat"], want["d_in"] = zx64.grad[rows, :512], zx64.grad[rows, 512:]
    # the reference, library rows, gates of its own forward
    in42, zlat = zx[rows, 512:], zx[rows, :512]
    gates = R.own_gates(mlp_params(11), in42, zlat, NS)
    ref = R.StageRef(mlp_params(11), in42, zlat, gates, NS)
    assert float((ref.out.detach() - out.detach()).abs().max()) <= 1e-12 * float(out.detach().abs().max())
    got = ref.backward(g_out)
    assert set(got) == set(R.OUTPUT_KEYS) and got["d_zlat"].shape == (NS * P, 512) and got["d_in"].shape == (NS * P, 42)
    for k in R.OUTPUT_KEYS:
        assert float(want[k].norm()) > 0, k
        assert R.rel_l2(got[k], want[k]) <= 1e-12, (k, R.rel_l2(got[k], want[k]))
    assert R.row_metric(got["d_zlat"], want["d_zlat"]) <= 1e-12 and R.row_metric(got["d_in"], want["d_in"]) <= 1e-12


def test_mask_decode_inverts_the_documented_layout():
    """decode_relu_masks against the word layout of pnr_device.h written out bit by bit (P = 70: one full tile and a ragged one)"""
    P, NS = 70, 2
    rs = np.random.RandomState(3)
    gates = rs.rand(R.N_GATES, NS, P, 512) > 0.5
    ntiles = 2
    words = np.zeros((R.N_GATES, NS, ntiles, 512), dtype=np.uint64)
    for tile in range(ntiles):
        for t in range(512):
            wv, lane = t >> 6, t & 63
            for it in range(2):
                for jt in range(2):
                    pt = tile * 64 + 32 * jt + (lane & 31)
                    if pt >= P:
                        continue
                    for r in range(16):
                        feat = 64 * wv + 32 * it + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
                        words[:, :, tile, t] |= gates[:, :, pt, feat].astype(np.uint64) << np.uint64((it * 2 + jt) * 16 + r)
    got = R.decode_relu_masks(torch.from_numpy(words.view(np.int64)).view(torch.uint8).reshape(-1), P, NS)
    assert got.shape == gates.shape and (got == gates).all()


@pytest.fixture(scope="module")
def mv_mini_stage():
    zx, SB, NS = network_input("mv_mini")
    rows = library_rows(SB, NS)
    in42, zlat = zx[rows, 512:], zx[rows, :512]
    params = mlp_params(11)
    gates = R.own_gates(params, in42, zlat, NS)
    g_out = g_out_for(SB * B)
    ref = R.StageRef(params, in42, zlat, gates, NS).backward(g_out)
    return params, in42, zlat, gates, NS, g_out, ref


def f16_head(t):
    return t.half().float()


def degraded(kind, params, gates):
    params, gates = dict(params), [g.clone() for g in gates]
    if kind == "every weight = its f16 head":  # every w_tail . x_head product dropped
        params = {k: (f16_head(v) if k.endswith("weight") else v) for k, v in params.items()}
    elif kind == "blocks.1.fc_0.weight = its f16 head":  # one layer reads the wrong tail stream
        params["blocks.1.fc_0.weight"] = f16_head(params["blocks.1.fc_0.weight"])
    elif kind == "one relu mask bit":  # of 1.9 M: gate of net[1], row 0, feature 0
        assert sum(g.numel() for g in gates) == 6 * 444 * 512 + 5 * 222 * 512
        gates[3][0, 0] = 1.0 - gates[3][0, 0]
    else:
        raise KeyError(kind)
    return params, gates


DEGRADATIONS = ["every weight = its f16 head", "blocks.1.fc_0.weight = its f16 head", "one relu mask bit"]


@pytest.mark.parametrize("kind", DEGRADATIONS)
def test_the_bar_bites(mv_mini_stage, kind):
    """mv_mini, 2 objects x 2 views x 111 points, mlp_params(11), g_out = 1e-3 randn; worst of the 32 outputs (relative L2, and
    the row metric of d_zlat / d_in) against the float64 reference.  Measured:

      every weight reduced to its f16 head (every w_tail . x_head product dropped)   4.4e-4 (blocks.4.fc_0.weight); d_zlat 3.9e-4, d_in 4.1e-4
      blocks.1.fc_0.weight alone reduced to its head (one layer's tail stream wrong)  1.9e-4 (blocks.1.fc_1.weight); d_zlat 7.8e-5, d_in 9.3e-5
      one relu mask bit of 1.9 M flipped (net[1], row 0, feature 0)                   1.4e-3 (row metric of d_in);   d_zlat 1.1e-4, d_in 1.4e-4
      plain float32 torch, same gated chain (test_plain_fp32_passes_the_bar)          4.3e-7 (row metric of d_in);   d_zlat 3.8e-7, d_in 4.0e-7

    against committed bars of 3e-6 (exact) and 1e-5 (both split forms): 19x, 44x and 139x the loosest.

    Each must miss the loosest committed bar by at least 10x."""
    params, in42, zlat, gates, NS, g_out, ref = mv_mini_stage
    p, g = degraded(kind, params, gates)
    errs = R.stage_errors(R.StageRef(p, in42, zlat, g, NS).backward(g_out), ref)
    k, e = R.worst(errs)
    print(f"{kind}: worst {e:.2e} ({k}), d_zlat {errs['d_zlat']:.2e}, d_in {errs['d_in']:.2e}")
    assert e >= 10 * max(R.BARS.values()), (kind, k, e)


def test_plain_fp32_passes_the_bar(mv_mini_stage):
    """the same gated chain in float32 torch -- what a correct fp32 implementation looks like -- is inside the tightest bar"""
    params, in42, zlat, gates, NS, g_out, ref = mv_mini_stage
    errs = R.stage_errors(R.StageRef(params, in42, zlat, gates, NS, dtype=torch.float32).backward(g_out), ref)
    k, e = R.worst(errs)
    print(f"plain fp32: worst {e:.2e} ({k}), d_zlat {errs['d_zlat']:.2e}, d_in {errs['d_in']:.2e}")
    assert e <= min(R.BARS.values()), (k, e)
