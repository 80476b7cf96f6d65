"""
Host tests (no GPU) of tests/mlp16_ref.py, the teacher-forced fp64 reference and the derived per-element bounds that
tests/test_hip_mlp16_stage.py holds the 16-bit training chain (eval_kernel<.., TRAIN>, bwd_kernel) to.

  * emulate() is a small fp32 torch emulation of both kernels: fp32 accumulation, the 16-bit conversion at the dump points, masks
    from the dumps.  It passes every bound at every case shape, with torch's summation order and with a scrambled one (chunks
    of 16 summed in reverse), on both networks and both g_out of the GPU test -- which also shows, before any GPU run, that the
    preconditions of the reference hold there (finite g_out, nothing near the type's largest finite value).
  * the bounds BITE: each of the listed wrong kernels misses the bound on the dump it touches, by at least 10x -- except
    truncation instead of round-to-nearest, whose error is below one ulp = 2u |ref| by construction, so that no bound that admits
    round-to-nearest (u |ref|) can be missed by more than 2x: it is required to FAIL (ratio > 1), and does.
  * the same wrong kernels stay inside the 3e-2 relative L2 that the end-to-end tests allow, on the dump they touch -- all but
    those that are wrong on a large part of a tensor: the dropped / doubled 1/NS (a whole tensor x 2, x 1/2), the x5 gate taken
    from x_4 and view 1 gated by view 0's masks (half the gates of a layer differ between two activations of a random network).
    For these the test asserts the opposite (they would NOT pass 3e-2 on that dump) and adds the variant that does hide: a 1/NS
    that is 1.5 % off, and the two gate mix-ups confined to ONE thread's 64-bit mask word.
"""
import functools
from unittest import mock

import pytest
import torch

import mlp16_ref as M
from helpers import mlp_params, scene_for
from mlp_bwd_ref import rel_l2
from oracle import pnr_oracle as O
from test_hip_mlp_backward_stage import CASES, network

OLD_BAR = 3e-2  # tests/test_hip_backward.py: per-tensor relative L2 of the f16 path


@functools.lru_cache(maxsize=None)
def network_input(case, seed=13):
    """-> (in42 (NS*P,42), zlat (NS*P,512) float32 in the library's [view][point] rows, P, NS): what models.py:227 hands to the MLP
    for random points in the case's scene, P = the case's point count"""
    scene_name, n_rays, K = CASES[case]
    scene, _ = scene_for(scene_name)
    SB, NS, B = scene["SB"], scene["NS"], n_rays * K
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
    zx = seen["zx"].reshape(SB, NS, B, 512 + 42).permute(1, 0, 2, 3).reshape(NS * SB * B, 512 + 42)  # [object][view][point] -> [view][object][point]
    return zx[:, 512:].contiguous(), zx[:, :512].contiguous(), SB * B, NS


def mm_plain(v, W):
    return v @ W.t()


def mm_scrambled(v, W):
    """the same products, chunks of 16 summed in reverse order"""
    acc = torch.zeros(v.shape[0], W.shape[0], dtype=torch.float32)
    for k in reversed(range(0, W.shape[1], 16)):
        acc = acc + v[:, k:k + 16] @ W[:, k:k + 16].t()
    return acc


# what ONE 64-bit mask word covers (pnr_device.h; thread 0 of a tile): points 0 and 32 of the tile, the 32 features
# 32 it + (r & 3) + 8 (r >> 2) of wave 0, half 0
WORD_POINTS = (0, 64)
WORD_FEATURES = [f for f in range(64) if f % 8 < 4]


def trunc16(t, dt):
    """fp32 -> 16-bit toward zero"""
    h = t.to(dt)
    bits = h.view(torch.int16)
    return torch.where(h.float().abs() > t.abs(), bits - 1, bits).view(dt).float()


def emulate(params, in42, zlat, NS, fmt, g_out, s, mm=mm_plain, mut=None):
    """fp32 emulation of eval_kernel<.., TRAIN> + bwd_kernel -> D of mlp16_ref (feature order, float64).  mut: one wrong kernel."""
    dt = fmt.dtype
    r16 = (lambda t: trunc16(t, dt)) if mut == "trunc" else (lambda t: t.to(dt).float())
    W = lambda k: params[k + ".weight"].to(dt).float()  # noqa: E731
    Bf = lambda *ks: sum(params[k + ".bias"].float() for k in ks)  # noqa: E731
    rows = in42.shape[0]
    P = rows // NS
    inv = torch.tensor(1.0, dtype=torch.float32) / NS
    inv = {"no_inv_ns": inv * NS, "inv_ns_twice": inv * inv, "inv_ns_15pm": inv * 1.015}.get(mut, inv)
    D = {"d_a": [], "d_n": [], "g_fc1": [None] * 5, "g_fc0": [None] * 5}
    d_in, d_z = in42.float().to(dt).float(), zlat.float().to(dt).float()
    x = Bf("lin_in", "lin_z.0").expand(rows, 512) + mm(d_in, W("lin_in"))
    x = x + mm(d_z, W("lin_z.0"))
    for b in range(5):
        if b == 3 and NS > 1:
            xs = x.reshape(NS, P, 512)
            acc = xs[0]
            for v in range(1, NS):
                acc = acc + xs[v]
            x = acc * inv
        a = r16(torch.relu(x))
        net = mm(a, W(f"blocks.{b}.fc_0"))
        if not (mut == "no_bias" and b == 1):
            net = Bf(f"blocks.{b}.fc_0") + net
        n = r16(torch.relu(net))
        if mut == "ragged_row" and b == 2:  # the last valid row of the (ragged) last tile of view 0 <- its neighbour
            n[P - 1] = n[P - 2]
        D["d_a"].append(a)
        D["d_n"].append(n)
        x = x + (Bf(f"blocks.{b}.fc_1", f"lin_z.{b + 1}") if b + 1 < 3 else Bf(f"blocks.{b}.fc_1"))
        x = x + mm(n, W(f"blocks.{b}.fc_1"))
        if b + 1 < 3:
            x = x + mm(d_z, W(f"lin_z.{b + 1}"))
    x5 = r16(torch.relu(x))
    pre = mm(x5, W("lin_out")) + params["lin_out.bias"].float()
    out = torch.cat([torch.sigmoid(pre[:, :3]), torch.relu(pre[:, 3:])], dim=1)
    dumps = []
    for b in range(5):
        dumps += [D["d_a"][b], D["d_n"][b]]
    dumps.append(x5)
    gates = [(d != 0).float() for d in dumps]
    # ---- the data-gradient chain
    inv_s = 1.0 / float(s)
    g16 = r16(g_out.float() * float(s))
    g5 = gates[8 if mut == "x5_gate_from_x4" else 10]
    if mut == "x5_gate_word":  # the same for ONE thread's mask word
        g5 = g5.clone()
        g5[WORD_POINTS[0]:WORD_POINTS[1]:32, WORD_FEATURES] = gates[8][WORD_POINTS[0]:WORD_POINTS[1]:32, WORD_FEATURES]
    G = mm(g16, W("lin_out").t()) * g5
    for b in range(4, -1, -1):
        if b == 2 and NS > 1:
            G = (G * inv).repeat(NS, 1)
        g1 = r16(G)
        Wt1 = W(f"blocks.{b}.fc_1").t().contiguous()  # (in, out): row = this wave's feature, K = the layer's output feature
        if mut == "wfrag_swap" and b == 3:  # one 8-element fragment swapped between wave 0's and wave 1's feature ranges
            Wt1[5, 40:48], Wt1[64 + 5, 40:48] = Wt1[64 + 5, 40:48].clone(), Wt1[5, 40:48].clone()
        t = mm(g1, Wt1)
        gn, ga = gates[2 * b + 1], gates[2 * b]
        if mut == "mask_bit" and b == 1:  # ONE wrong bit: the element with the largest |t|
            gn = gn.clone()
            i = int(t.abs().argmax())
            D["touched"] = (i // 512, i % 512)
            gn[i // 512, i % 512] = 1.0 - gn[i // 512, i % 512]
        if mut == "view_mask" and b == 2 and NS > 1:  # view 1 gated with view 0's mask words
            gn, ga = gn.clone(), ga.clone()
            gn[P:2 * P], ga[P:2 * P] = gn[:P], ga[:P]
        if mut == "view_mask_word" and b == 2 and NS > 1:  # the same for ONE thread's two mask words
            gn, ga = gn.clone(), ga.clone()
            for g in (gn, ga):
                g[P + WORD_POINTS[0]:P + WORD_POINTS[1]:32, WORD_FEATURES] = g[WORD_POINTS[0]:WORD_POINTS[1]:32, WORD_FEATURES]
        g0 = r16(gn * t)
        G = G + ga * mm(g0, W(f"blocks.{b}.fc_0").t().contiguous())
        D["g_fc1"][b], D["g_fc0"][b] = g1, g0
    g_x0 = r16(G)
    Z = mm(D["g_fc1"][1], W("lin_z.2").t().contiguous())
    Z = Z + mm(D["g_fc1"][0], W("lin_z.1").t().contiguous())
    Z = Z + mm(g_x0, W("lin_z.0").t().contiguous())
    D.update(d_in=d_in, d_z=d_z, d_x5=x5, out=out, g_x0=g_x0, d_zlat=Z * inv_s,
             d_in_grad=mm(g_x0, W("lin_in").t().contiguous()) * inv_s, gates=[g.double() for g in gates])
    for k in ("d_in", "d_z", "d_x5", "out", "g_x0", "d_zlat", "d_in_grad"):
        D[k] = D[k].double()
    for k in ("d_a", "d_n", "g_fc1", "g_fc0"):
        D[k] = [t.double() for t in D[k]]
    return D


def run(case, net, prec, kind, mm=mm_plain, mut=None):
    in42, zlat, P, NS = network_input(case)
    fmt = M.FMTS[prec]
    params = network(net)
    g_out = M.g_out_variant(kind, P)
    s = M.grad_scale_for(g_out)
    D = emulate(params, in42, zlat, NS, fmt, g_out, s, mm=mm, mut=mut)
    items = M.forward_items(params, D, NS, fmt) + M.backward_items(params, D, g_out, s, NS, fmt)
    return D, items, g_out, fmt, NS, P


BF16_CASES = ["sn64-7x37", "mv_mini-10x45"]
GRID = [(c, "f16") for c in CASES] + [(c, "bf16") for c in BF16_CASES]


@pytest.mark.parametrize("net,kind,mm", [(11, "randn", mm_plain), ("surface", "hostile", mm_scrambled),
                                         (11, "hostile", mm_scrambled), ("surface", "randn", mm_plain)])
@pytest.mark.parametrize("case,prec", GRID)
def test_emulation_is_inside_every_bound_and_preconditions_hold(case, prec, net, kind, mm):
    D, items, g_out, fmt, NS, P = run(case, net, prec, kind, mm=mm)
    M.assert_preconditions(items, g_out, fmt)
    M.assert_masks_match_dumps(D["gates"], D)
    r = M.assert_within(items, (case, prec, net, kind))
    assert len(r) == 5 + 5 + 1 + 1 + 5 + 5 + 1 + 2
    if NS > 1:
        g = D["g_fc1"][2].reshape(NS, P, 512)
        assert all(torch.equal(g[0], g[v]) for v in range(1, NS))
    k = max(r, key=r.get)
    print(f"MLP16-HOST {case} {prec} net={net} g={kind}: worst {r[k]:.3f} ({k}); headroom {max(M.headroom(D, fmt).values()):.2e}")


def test_hostile_g_out_is_what_it_says():
    for P in (1, 63, 259, 900):
        g = M.g_out_variant("hostile", P)
        n = g.abs().amax(dim=1)
        assert torch.isfinite(g).all() and int(n.argmax()) == P - 1
        if P > 10:
            assert int((n == 0).sum()) >= P // 6 and float(n.max() / n[n > 0].min()) >= 1e4


MV = "mv_mini-10x45"   # 2 objects x 2 views, 900 points: ragged last tile, pooling
BIG = "train-24x37"    # 3552 points: one wrong row of 3552
# mutation -> (case, the dumps it touches = exactly the items that must miss their bound, required factor)
MUTATIONS = {
    "mask_bit": (MV, ["g_fc0[1]"], 10.0),
    "no_inv_ns": (MV, ["d_a[3]", "d_a[4]", "d_x5", "g_fc1[2]"], 10.0),
    "inv_ns_twice": (MV, ["d_a[3]", "d_a[4]", "d_x5", "g_fc1[2]"], 10.0),
    "inv_ns_15pm": (MV, ["d_a[3]", "d_a[4]", "d_x5", "g_fc1[2]"], 10.0),
    "wfrag_swap": (MV, ["g_fc0[3]"], 10.0),
    "no_bias": (MV, ["d_n[1]"], 10.0),
    "ragged_row": (BIG, ["d_n[2]"], 10.0),
    "x5_gate_from_x4": (MV, ["g_fc1[4]"], 10.0),
    "x5_gate_word": (MV, ["g_fc1[4]"], 10.0),
    "trunc": (MV, None, 1.0),  # every dump; below 2x by construction (module docstring)
    "view_mask": (MV, ["g_fc0[2]", "g_fc1[1]"], 10.0),
    "view_mask_word": (MV, ["g_fc0[2]", "g_fc1[1]"], 10.0),
}
# wrong on a large part of a tensor (a factor 2 or 1/2; the gates of a whole layer): these do NOT hide under 3e-2 on the dump they
# touch -- asserted as such; their one-word / 1.5 % variants above do hide
NOT_UNDER_OLD_BAR = {"no_inv_ns", "inv_ns_twice", "x5_gate_from_x4", "view_mask"}


@functools.lru_cache(maxsize=None)
def clean(case):
    return run(case, 11, "f16", "randn")


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_each_wrong_kernel_misses_the_bound_and_hides_under_the_old_bar(mut):
    case, touched, factor = MUTATIONS[mut]
    D0, items0, *_ = clean(case)
    M.assert_within(items0, "clean")
    D, items, *_ = run(case, 11, "f16", "randn", mut=mut)
    r = M.ratios(items)
    failing = sorted(k for k, v in r.items() if v > 1.0)
    if touched is None:  # truncation: every 16-bit dump is rounded the wrong way
        touched = [k for k in r if k not in ("out", "d_zlat", "d_in_grad")]
        assert failing and set(failing) <= set(touched), (mut, failing)
        assert len(failing) >= 10, (mut, failing)
        # g_fc1[4] is the exception: its operand r16(s g_out) is staged inside the kernel and not dumped, the reference rounds it
        # to nearest itself, and a one-ulp difference there is amplified by lin_out^T (>= 10x here)
        assert all(1.0 < r[k] < 2.0 + 1e-6 for k in failing if k != "g_fc1[4]"), (mut, {k: r[k] for k in failing})
        assert r["g_fc1[4]"] >= 10.0, r["g_fc1[4]"]
    else:
        # teacher forcing names the step: exactly the touched dumps miss, nothing downstream does
        assert failing == sorted(touched), (mut, failing, {k: r[k] for k in failing})
        for k in touched:
            assert r[k] >= factor, (mut, k, r[k])
    if mut == "mask_bit":  # on the very element
        row, f = D["touched"]
        assert float(M.ratio_map(items, "g_fc0[1]")[row, f]) >= factor

    # the old measure on the same step: relative L2 of the touched dump against the reference of that step (teacher-forced like
    # the bound; a free-running comparison also counts the relu gates that any 1e-3 perturbation flips further down)
    old = {it.name: rel_l2(it.got, it.ref) for it in items if it.name in (failing if mut == "trunc" else touched)}
    print(f"MLP16-MUT {mut} on {case}: error/bound " + " ".join(f"{k}={r[k]:.3g}" for k in failing)
          + " | relative L2 of the dump " + " ".join(f"{k}={v:.2e}" for k, v in old.items()))
    if mut not in NOT_UNDER_OLD_BAR:
        assert max(old.values()) <= OLD_BAR, (mut, old)
    else:
        assert min(old.values()) > OLD_BAR, (mut, old)  # (if this ever hid under 3e-2 it would belong with the others)


def test_a_mask_bit_wrong_in_the_forward_fails_the_exact_check():
    D, *_ = clean(MV)
    M.assert_masks_match_dumps(D["gates"], D)
    for li in (0, 5, 10):
        gates = [g.clone() for g in D["gates"]]
        gates[li][gates[li].shape[0] - 1, 511] = 1.0 - gates[li][gates[li].shape[0] - 1, 511]
        with pytest.raises(AssertionError):
            M.assert_masks_match_dumps(gates, D)


def test_storage_perm_is_a_permutation_with_the_documented_inverse():
    perm = M.storage_perm()
    assert sorted(perm.tolist()) == list(range(512))
    f = torch.arange(512)
    slot = (f & ~31) + 16 * ((f >> 2) & 1) + (f & 3) + 4 * ((f & 31) >> 3)  # pnr_layout.h slot_of
    assert torch.equal(perm[slot], f)
    t = torch.randn(3, 512)
    assert torch.equal(M.from_storage(t[:, perm]), t.double())
