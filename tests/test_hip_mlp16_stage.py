"""
GPU tests (-m gpu) of the 16-bit training chain at its own resolution: the training forward eval_kernel<.., TRAIN>
(pnr_eval_ray_samples_train: 14 operand dumps, 11 layers of relu masks) and the data-gradient chain bwd_kernel (pnr_mlp_backward:
g_fc1[5], g_fc0[5], g_x0, d_zlat, d_in), precision "f16" and "bf16", against tests/mlp16_ref.py: every dump recomputed in
float64 from the kernel's OWN earlier dumps and held to a derived per-element bound (its derivation is in that module;
tests/test_mlp16_ref_host.py shows what the bounds reject).  Nothing is excluded: every row, feature and dump is compared.

Per test: one training forward, one backward per g_out (0.02 randn; a hostile one: all-zero rows, 1e4 between rows, the last
valid row the largest, the scale picked by ops.grad_scale on the device).  Also exact:
  * a mask bit is set if and only if the dumped element is non-zero (11 layers, every view); no relu'd dump holds a negative zero
  * the pooled mask layers are written for view 0 only; the lin_in operand's padding columns are zero
  * g_fc1[2] is bit-identical across views
  * every buffer is filled with NaN (masks: 0xA5) before the launch and has one guard row behind its last row: afterwards every
    row below `rows` is written and the guard row is untouched -- dump_image's rows_left on the ragged last tile.
The shapes are test_hip_mlp_backward_stage.CASES; the measured figures are in profiles/mlp16_stage_notes.md.
"""
import pytest
import torch

import mlp16_ref as M
from helpers import scene_for
from mlp_bwd_ref import N_GATES, PER_VIEW_GATES, gates_from_masks
from test_hip_mlp_backward_stage import CASES, network
from testdata import synthetic

pytestmark = pytest.mark.gpu

BF16_CASES = ["sn64-7x37", "mv_mini-10x45"]
GRID = [(c, "f16") for c in CASES] + [(c, "bf16") for c in BF16_CASES]
MASK_FILL = 0xA5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


class Guarded:
    """tensors with one guard row (masks: 64 guard bytes) behind them, everything pre-filled"""

    def __init__(self, dev):
        self.dev, self.all = dev, []

    def like(self, t):
        if t.dtype == torch.uint8:
            big = torch.full((t.numel() + 64,), MASK_FILL, dtype=torch.uint8, device=self.dev)
            view = big[:t.numel()]
        else:
            big = torch.full((t.shape[0] + 1, t.shape[1]), float("nan"), dtype=t.dtype, device=self.dev)
            view = big[:t.shape[0]]
        assert view.is_contiguous() and view.data_ptr() == big.data_ptr()
        self.all.append((big, view))
        return view

    def refill(self):
        for big, _ in self.all:
            big.fill_(MASK_FILL if big.dtype == torch.uint8 else float("nan"))

    def check(self, what):
        for i, (big, view) in enumerate(self.all):
            if big.dtype == torch.uint8:
                assert bool((big[view.numel():] == MASK_FILL).all()), (what, i, "guard bytes written")
            else:
                assert bool(torch.isnan(big[view.shape[0]]).all()), (what, i, tuple(view.shape), "guard row written")
                assert not bool(torch.isnan(view).any()), (what, i, tuple(view.shape), "rows left unwritten (or NaN)")


def guarded_train_dumps(ops, P, NS, precision, dev):
    """a TrainDumps set whose buffers are guarded, parked in the pool so that eval_ray_samples_train picks it up"""
    d, g = ops.TrainDumps(P, NS, precision, dev), Guarded(dev)
    d.d_in, d.d_z, d.d_x5, d.d_mask = g.like(d.d_in), g.like(d.d_z), g.like(d.d_x5), g.like(d.d_mask)
    d.d_a, d.d_n = [g.like(t) for t in d.d_a], [g.like(t) for t in d.d_n]
    s = d.struct
    s.d_in, s.d_z, s.d_x5, s.d_mask = d.d_in.data_ptr(), d.d_z.data_ptr(), d.d_x5.data_ptr(), d.d_mask.data_ptr()
    for b in range(5):
        s.d_a[b], s.d_n[b] = d.d_a[b].data_ptr(), d.d_n[b].data_ptr()
    ops.dump_pool_clear()
    d._pool_key, d._free = ("fwd", int(P), int(NS), int(precision), str(dev)), False
    d.release()
    return d, g


def guarded_backward_dumps(ops, fwd, dev):
    o, g = ops.BackwardDumps(fwd, dev), Guarded(dev)
    o.g_fc1, o.g_fc0 = [g.like(t) for t in o.g_fc1], [g.like(t) for t in o.g_fc0]
    o.g_x0, o.d_zlat, o.d_in = g.like(o.g_x0), g.like(o.d_zlat), g.like(o.d_in)
    s = o.struct
    s.g_x0, s.d_zlat, s.d_in = o.g_x0.data_ptr(), o.d_zlat.data_ptr(), o.d_in.data_ptr()
    for b in range(5):
        s.g_fc1[b], s.g_fc0[b] = o.g_fc1[b].data_ptr(), o.g_fc0[b].data_ptr()
    o._pool_key = ("bwd", int(fwd.P), int(fwd.NS), str(fwd.dtype), str(dev))
    return o, g


def park(ops, obj):
    ops.dump_pool_clear()
    obj._free = False
    obj.release()


def show(tag, r):
    print(f"MLP16 {tag}: " + " ".join(f"{k}={v:.3f}" for k, v in r.items()))


@pytest.mark.parametrize("net", [11, "surface"])
@pytest.mark.parametrize("case,prec", GRID)
def test_chain_matches_teacher_forced_fp64_reference(dev, case, prec, net):
    from pixelnerf_amd import ops
    fmt = M.FMTS[prec]
    scene_name, n_rays, K = CASES[case]
    scene, meta = scene_for(scene_name)
    NS = scene["NS"]
    sc = ops.make_scene(scene["latent"].to(dev), scene["poses"].to(dev), scene["focal"].to(dev), scene["c"].to(dev),
                        scene["image_shape"], NS)
    rays = synthetic.target_rays(meta, n_rays=n_rays).reshape(-1, 8)
    u = torch.sort(torch.rand(rays.shape[0], K, generator=torch.Generator().manual_seed(2)), dim=-1)[0]
    z = (rays[:, 6:7] + (rays[:, 7:8] - rays[:, 6:7]) * u).to(dev).contiguous()
    rays = rays.to(dev)
    P = rays.shape[0] * K
    params = network(net)
    state = {k: v.to(dev) for k, v in params.items()}
    pk, pkb = ops.pack_mlp(state, prec), ops.pack_mlp(state, prec, backward=True)
    perm = ops.storage_perm()
    assert torch.equal(perm, M.storage_perm())

    # ---- the training forward
    want, guard = guarded_train_dumps(ops, P, NS, pk.precision, dev)
    out, dumps = ops.eval_ray_samples_train(sc, pk, rays, z)
    torch.cuda.synchronize()
    assert dumps is want and dumps.dtype == fmt.dtype
    guard.check(f"{case} forward")
    ntiles = (P + 63) // 64
    words = dumps.d_mask.cpu().view(torch.int64).reshape(N_GATES, NS, ntiles, 512)
    untouched = torch.full((8,), MASK_FILL, dtype=torch.uint8).view(torch.int64)[0]
    assert bool((words[PER_VIEW_GATES:, 1:] == untouched).all()), "pooled mask layers: only view 0 may be written"
    d_in = dumps.d_in.cpu().double()
    assert not bool(d_in[:, M.D_IN:].any()), "padding columns of the lin_in operand"
    D = {"d_in": d_in[:, :M.D_IN].contiguous(), "d_z": dumps.d_z.cpu().double(), "d_x5": M.from_storage(dumps.d_x5, perm),
         "d_a": [M.from_storage(t, perm) for t in dumps.d_a], "d_n": [M.from_storage(t, perm) for t in dumps.d_n],
         "out": out.reshape(P, 4).cpu().double(), "gates": gates_from_masks(dumps.d_mask, P, NS)}
    M.assert_masks_match_dumps(D["gates"], D)
    fwd_items = M.forward_items(params, D, NS, fmt)
    M.assert_preconditions(fwd_items, torch.zeros(1), fmt)
    tag = f"{case} {prec} net={net} P={P} NS={NS}"
    r = M.ratios(fwd_items)
    show(tag + " forward", r)
    bad = {k: v for k, v in r.items() if not v <= 1.0}

    # ---- the data-gradient chain, two g_out on the same forward
    bwant, bguard = guarded_backward_dumps(ops, dumps, dev)
    for kind in ("randn", "hostile"):
        g_out = M.g_out_variant(kind, P)
        bguard.refill()
        park(ops, bwant)
        s = ops.grad_scale(g_out.to(dev))
        bd = ops.mlp_backward(pkb, dumps, g_out.to(dev), s[0:1])
        torch.cuda.synchronize()
        assert bd is bwant
        sc_, inv_ = float(s[0].item()), float(s[1].item())
        assert sc_ == M.grad_scale_for(g_out) and inv_ == 1.0 / sc_
        bguard.check(f"{case} backward {kind}")
        D.update(g_fc1=[M.from_storage(t, perm) for t in bd.g_fc1], g_fc0=[M.from_storage(t, perm) for t in bd.g_fc0],
                 g_x0=M.from_storage(bd.g_x0, perm), d_zlat=bd.d_zlat.cpu().double(), d_in_grad=bd.d_in.cpu().double())
        if NS > 1:
            g = bd.g_fc1[2].reshape(NS, P, 512)
            assert all(torch.equal(g[0], g[v]) for v in range(1, NS)), "g_fc1[2] differs between views"
        items = M.backward_items(params, D, g_out, sc_, NS, fmt)
        M.assert_preconditions(items, g_out, fmt)
        rb = M.ratios(items)
        show(f"{tag} backward g={kind}", rb)
        print(f"MLP16-HEADROOM {tag} g={kind}: " + " ".join(f"{k}={v:.2e}" for k, v in M.headroom(D, fmt).items()))
        bad.update({f"{k} (g={kind})": v for k, v in rb.items() if not v <= 1.0})
    ops.dump_pool_clear()
    assert not bad, (tag, bad)
