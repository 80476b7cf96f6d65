"""
fp64 reference of the 16-bit training chain (precision "f16" / "bf16"): the training forward eval_kernel<.., TRAIN> of
pnr_mlp.hip (pnr_eval_ray_samples_train) and the data-gradient chain bwd_kernel of pnr_bwd.hip (pnr_mlp_backward), layer by
layer, TEACHER-FORCED: CPU, torch only.

Every GEMM operand of both kernels leaves the chip as a 16-bit dump, and the residual stream and its gradient live in fp32
accumulators in between.  So every dump is a float64-computable function of dumps the kernel wrote EARLIER, followed by ONE
conversion to the 16-bit type; the reference recomputes each one from the kernel's own earlier dumps and never from its own
earlier results, which names the layer a wrong value was born in.

  rows     the library's: [view][point], points object-major (tests/mlp_bwd_ref.py); the view mean is reshape(NS, P, 512).mean(0)
  columns  FEATURE order here.  The hidden dumps lie in storage order in memory: from_storage() undoes ops.storage_perm, which
           storage_perm() below restates (pnr_layout.h feat_of).  d_in, d_z, d_zlat and the input gradient are in natural order.
  masks    the same words as the fp32-class path's: write_act / nonzero_bits8 of pnr_device.h are shared by both forward kernels
           and lin_out's x5_bits of eval_kernel uses the same bit (xit*JT + jt)*16 + 8*rr + k, so mlp_bwd_ref.decode_relu_masks
           and gates_from_masks are imported, not copied.
  W16      a weight rounded to the run's type as the pack kernels round it: `(T)v` of an fp32 value in pack_weights_kernel
           (pnr_pack.hip) and pack_weights_bwd_kernel (pnr_bwd.hip) is round-to-nearest-even = params[k].to(dtype).
  biases   fp32; slots shared by two layers hold their fp32 sum (pack_bias_kernel: b_in + b_z[0], b_fc1[b] + b_z[b+1]).
  r16      pack8 / pack2 of pnr_device.h: __builtin_convertvector = fptrunc, round-to-nearest-even for BOTH types (gfx950 has a
           native bf16 conversion; nothing truncates), subnormals kept (f16 denormals are on by default, bf16 shares fp32's
           exponent range).  So u = 2^-11 (f16), 2^-8 (bf16), floor = the type's subnormal step.

The chain (what forward_items / backward_items restate; x_b = residual stream in front of block b, G = its gradient):

  x_0      = W16_in . d_in[:, :42] + W16_z0 . d_z + (b_in + b_z0)
  d_a[b]   = r16(relu(x_b))                         d_n[b] = r16(relu(W16_fc0[b] . d_a[b] + b_fc0[b]))
  x_{b+1}  = x_b + (b_fc1[b] [+ b_z[b+1]]) + W16_fc1[b] . d_n[b] [+ W16_z[b+1] . d_z]        (lin_z for b + 1 < 3)
  x_3      = view mean of x_3 (NS > 1)              d_x5 = r16(relu(x_5))
  rgbsigma = (sigmoid x 3, relu)(W16_out . d_x5 + b_out)
  x_b is rebuilt in float64 from the dumped operands of ALL earlier layers (d_in, d_z, d_n[0..b-1]), never from d_a.

  G_5      = gate_x5 . (W16_out^T . r16(s g_out))   g_fc1[4] = r16(G_5)
  g_fc0[b] = r16(gate_net[b] . (W16_fc1[b]^T . g_fc1[b]))
  g_fc1[b-1] (g_x0 for b = 0) = r16(g_fc1[b] + gate_x[b] . (W16_fc0[b]^T . g_fc0[b])), behind block 3 divided by NS and
             broadcast to every view (so g_fc1[2] is bit-identical across views)
  d_zlat   = inv_s . (g_fc1[1] . W16_z2 + g_fc1[0] . W16_z1 + g_x0 . W16_z0)      d_in = inv_s . g_x0 . W16_in
  gates are the decoded mask bits: inputs, not recomputed.

THE BOUND, per element, derived (nothing here was measured on the kernel):

  |got - ref| <= u (|ref| + |carried|) + (1 + u) E + floor                                    (16-bit dumps)
  |got - ref| <= E + 2^-23 |ref| + 2^-149                                                     (fp32 outputs)

  * got = r16(v) with v the kernel's fp32 value: |got - v| <= u |v| + floor (round to nearest), |v - ref| <= E, hence
    u |ref| + (1 + u) E + floor.  ref is the UNROUNDED float64 value: rounding it too would only add a second u.
  * E, the fp32 accumulation error of v.  One GEMM of reduction length K adds K products into an accumulator that holds
    a = the value before it.  Whatever the order (the MFMA's 16-term groups, the K split of lin_out and lin_in^T over the
    waves and the sum of the partials), every intermediate sum is a sub-sum of {a, w_1 v_1, ..., w_K v_K}, so its magnitude
    is at most |a| + sum_k |w_k v_k|, and there are at most K roundings, each at most 2^-23 of the intermediate: one ulp,
    not half, because the f16 matrix instruction's sum rounds toward minus infinity (profiles/mlp_backward_stage_notes.md).
        E += K 2^-23 (|a| + E + sum_k |w_k| |v_k|)          K = 512; 64 for lin_in and lin_out^T (their padded length)
    summed over the GEMMs that feed the accumulator since it last started from an exact value; a bias added in front of a
    GEMM and the masked add G += t count one rounding more.  The products themselves are exact (16-bit x 16-bit in fp32).
  * carried: the gradient chain keeps G in fp32, the reference restarts every step from the DUMPED g_fc1[b] = r16(G).  The
    two differ by at most u |G| + floor <= u (1 + 2u) |g_fc1[b]| + floor: that is the carried term.  It is zero elsewhere.
  * view mean / its backward: NS - 1 adds and one multiplication by fl(1 / NS): (NS + 1) 2^-23 of the summed magnitudes,
    2 x 2^-23 |ref| for the backward's single multiplication.
  * sigmoid: |sigmoid'| <= 1/4, expf + add + divide in fp32 stay inside 8 x 2^-23 of a value in (0, 1).
  * floor: 2^-24 (f16 subnormal step), 2^-133 (bf16), 2^-149 (fp32).  No flush to zero is assumed anywhere.

Preconditions (assert_preconditions, on the reference alone): g_out finite, every reference value below the type's largest
finite number -- the comparison then exercises no saturation (the forward clamps, the backward would produce inf) and no inf.
"""
from collections import namedtuple

import torch

from mlp_bwd_ref import COMBINE_LAYER, D_HID, D_IN, N_BLOCKS, N_GATES, PARAM_KEYS, PER_VIEW_GATES, decode_relu_masks, gates_from_masks

assert (N_BLOCKS, COMBINE_LAYER, D_HID, D_IN, N_GATES, PER_VIEW_GATES) == (5, 3, 512, 42, 11, 6) and len(PARAM_KEYS) == 30

U23 = 2.0 ** -23
Fmt = namedtuple("Fmt", "name dtype u floor max")
F16 = Fmt("f16", torch.float16, 2.0 ** -11, 2.0 ** -24, 65504.0)
BF16 = Fmt("bf16", torch.bfloat16, 2.0 ** -8, 2.0 ** -133, 3.3895313892515355e38)
FMTS = {"f16": F16, "bf16": BF16}
K_BIG, K_SMALL = 512, 64

Item = namedtuple("Item", "name got ref bound")


def storage_perm():
    """perm[e] = hidden feature at storage position e of a dump row (pnr_layout.h feat_of(e / 32, (e % 32) / 16, e % 16))"""
    e = torch.arange(D_HID)
    r = e % 16
    return 32 * (e // 32) + (r & 3) + 8 * (r >> 2) + 4 * ((e % 32) // 16)


def from_storage(t, perm=None):
    """a (rows, 512) dump in storage order -> float64 in feature order"""
    perm = storage_perm() if perm is None else perm.cpu()
    out = torch.empty(t.shape, dtype=torch.float64)
    out[:, perm] = t.detach().cpu().double()
    return out


def w16(params, key, fmt):
    return params[key + ".weight"].detach().cpu().to(fmt.dtype).double()


def bias32(params, *keys):
    """the fp32 sum the bias table holds for a slot (pack_bias_kernel)"""
    b = params[keys[0] + ".bias"].detach().cpu().float()
    for k in keys[1:]:
        b = b + params[k + ".bias"].detach().cpu().float()
    return b.double()


def grad_scale_for(g_out):
    """ops.grad_scale on the host: 2^(6 - ceil(log2 max|g|)), 1 for an all-zero g"""
    import math
    m = float(g_out.abs().max())
    return 1.0 if m == 0.0 else 2.0 ** (6 - math.ceil(math.log2(m)))


def g_out_variant(kind, P, seed=5):
    """the two g_out (P,4) of the stage tests.  randn: 0.02 randn.  hostile: row magnitudes spread over 1e4 (log-uniform, the
    extremes present from 8 rows on), every fifth row all zero, the LAST valid row the largest."""
    gen = torch.Generator().manual_seed(seed)
    g = 0.02 * torch.randn(P, 4, generator=gen)
    if kind == "hostile":
        e = torch.rand(P, generator=gen)
        if P >= 8:
            e[1], e[2] = 0.0, 1.0
        g = g * (10.0 ** (-4.0 * e))[:, None]
        g[::5] = 0.0
        m = max(float(g.abs().max()), 0.02)
        g[P - 1] = 1.5 * m * torch.tensor([1.0, -1.0, 1.0, -1.0])
    else:
        assert kind == "randn", kind
    return g


def _gemm(v, W):
    """v (rows,K) . W (out,K)^T and the same of the magnitudes"""
    return v @ W.t(), v.abs() @ W.abs().t()


def _acc(a, E, v, W, K):
    """one GEMM into an accumulator holding a (error bound E): -> (a + v W^T, E')"""
    y, S = _gemm(v, W)
    return a + y, E + K * U23 * (a.abs() + E + S)


def _dump_bound(fmt, ref, E, carried=None):
    c = 0.0 if carried is None else carried.abs()
    return fmt.u * (ref.abs() + c) + (1.0 + fmt.u) * E + fmt.floor


def forward_items(params, D, NS, fmt):
    """D: the kernel's dumps in feature order, float64: d_in (rows,42), d_z (rows,512), d_a[5], d_n[5], d_x5, out (P,4).
    -> [Item]: d_a[0..4], d_n[0..4], d_x5, out"""
    rows = D["d_in"].shape[0]
    assert rows % NS == 0 and D["d_in"].shape[1] == D_IN
    P = rows // NS
    items = []
    x = bias32(params, "lin_in", "lin_z.0").expand(rows, D_HID)
    E = torch.zeros_like(x)
    x, E = _acc(x, E, D["d_in"], w16(params, "lin_in", fmt), K_SMALL)
    x, E = _acc(x, E, D["d_z"], w16(params, "lin_z.0", fmt), K_BIG)
    for b in range(N_BLOCKS):
        if b == COMBINE_LAYER and NS > 1:  # (v0 + v1) + ..., then * fl(1 / NS)
            mag = (x.abs() + E).reshape(NS, P, D_HID).sum(0)
            x, E = x.reshape(NS, P, D_HID).mean(0), E.reshape(NS, P, D_HID).mean(0) + (NS + 1) * U23 * mag / NS
        ref = torch.relu(x)
        items.append(Item(f"d_a[{b}]", D["d_a"][b], ref, _dump_bound(fmt, ref, E)))
        bn = bias32(params, f"blocks.{b}.fc_0").expand(x.shape)
        net, En = _acc(bn, torch.zeros_like(x), D["d_a"][b], w16(params, f"blocks.{b}.fc_0", fmt), K_BIG)
        ref = torch.relu(net)
        items.append(Item(f"d_n[{b}]", D["d_n"][b], ref, _dump_bound(fmt, ref, En)))
        with_z = b + 1 < COMBINE_LAYER
        bias = bias32(params, f"blocks.{b}.fc_1", f"lin_z.{b + 1}") if with_z else bias32(params, f"blocks.{b}.fc_1")
        x = x + bias
        E = E + U23 * x.abs()
        x, E = _acc(x, E, D["d_n"][b], w16(params, f"blocks.{b}.fc_1", fmt), K_BIG)
        if with_z:
            x, E = _acc(x, E, D["d_z"], w16(params, f"lin_z.{b + 1}", fmt), K_BIG)
    ref = torch.relu(x)
    items.append(Item("d_x5", D["d_x5"], ref, _dump_bound(fmt, ref, E)))
    # lin_out: every wave contracts its 64 features, the 8 partials and the bias are added in fp32
    bo = params["lin_out.bias"].detach().cpu().double()
    y, S = _gemm(D["d_x5"], w16(params, "lin_out", fmt))
    pre, Eo = y + bo, (K_BIG + 9) * U23 * (S + bo.abs())
    ref = torch.cat([torch.sigmoid(pre[:, :3]), torch.relu(pre[:, 3:])], dim=1)
    bound = torch.cat([0.25 * Eo[:, :3] + 8 * U23, Eo[:, 3:] + U23 * ref[:, 3:] + 2.0 ** -149], dim=1)
    items.append(Item("out", D["out"], ref, bound))
    return items


def backward_items(params, D, g_out, s, NS, fmt):
    """D: gates (11 float64 0/1 arrays: (NS*P,512) for the per-view layers, (P,512) for the pooled ones) and the chain's dumps in
    feature order, float64: g_fc1[5], g_fc0[5], g_x0, d_zlat (NS*P,512), d_in_grad (NS*P,42).  g_out (P,4) fp32, s = the scale.
    -> [Item]: g_fc1[4], g_fc0[4], g_fc1[3], ..., g_fc0[0], g_x0, d_zlat, d_in_grad"""
    gates = D["gates"]
    assert len(gates) == N_GATES
    P = g_out.shape[0]
    inv_s = 1.0 / float(s)
    g16 = (g_out.detach().cpu().float() * float(s)).to(fmt.dtype).double()  # staged as 16-bit operand rows
    items = []
    Wo = w16(params, "lin_out", fmt)
    G, S = g16 @ Wo, g16.abs() @ Wo.abs()  # lin_out^T g_out: K = 64 (4 real, zero padded)
    G, E = gates[10] * G, gates[10] * (K_SMALL * U23 * S)
    carried = None
    for b in range(N_BLOCKS - 1, -1, -1):
        if b == COMBINE_LAYER - 1 and NS > 1:  # backward of the view mean: G * fl(1 / NS), the same bits for every view
            G, E = (G / NS).repeat(NS, 1), (E / NS + 2 * U23 * G.abs() / NS).repeat(NS, 1)
            carried = None if carried is None else (carried / NS).repeat(NS, 1)
        items.append(Item(f"g_fc1[{b}]", D["g_fc1"][b], G, _dump_bound(fmt, G, E, carried)))
        g1 = D["g_fc1"][b]
        t, S = _gemm(g1, w16(params, f"blocks.{b}.fc_1", fmt).t())
        gn = gates[2 * b + 1]
        ref = gn * t
        items.append(Item(f"g_fc0[{b}]", D["g_fc0"][b], ref, _dump_bound(fmt, ref, gn * (K_BIG * U23 * S))))
        t2, S2 = _gemm(D["g_fc0"][b], w16(params, f"blocks.{b}.fc_0", fmt).t())
        ga = gates[2 * b]
        carried = g1
        G = g1 + ga * t2
        # the fp32 G the kernel adds to differs from the dump g1 = r16(G) by the carried term (in _dump_bound); the GEMM starts from
        # zero, the masked add rounds once
        E = ga * (K_BIG * U23 * S2) + U23 * G.abs() + 2 * fmt.u * fmt.u * g1.abs() + fmt.floor
    items.append(Item("g_x0", D["g_x0"], G, _dump_bound(fmt, G, E, carried)))
    return items + tail_items(params, D, inv_s, fmt)


def tail_items(params, D, inv_s, fmt):
    """the last four GEMMs of the chain from its own dumps g_fc1[1], g_fc1[0], g_x0 -> [Item]: d_zlat, d_in_grad"""
    items = []
    Z, Ez = torch.zeros_like(D["g_x0"]), torch.zeros_like(D["g_x0"])
    for dY, b in ((D["g_fc1"][1], 2), (D["g_fc1"][0], 1), (D["g_x0"], 0)):
        Z, Ez = _acc(Z, Ez, dY, w16(params, f"lin_z.{b}", fmt).t(), K_BIG)
    ref = Z * inv_s
    items.append(Item("d_zlat", D["d_zlat"], ref, Ez * inv_s + U23 * ref.abs() + 2.0 ** -149))
    y, S = _gemm(D["g_x0"], w16(params, "lin_in", fmt).t())  # K split over the 8 waves, partials summed
    ref = y * inv_s
    items.append(Item("d_in_grad", D["d_in_grad"], ref, (K_BIG + 8) * U23 * S * inv_s + U23 * ref.abs() + 2.0 ** -149))
    return items


def assert_preconditions(items, g_out, fmt):
    assert torch.isfinite(g_out).all(), "g_out must be finite"
    for it in items:
        m = float(it.ref.abs().max()) if it.ref.numel() else 0.0
        assert m < fmt.max, (it.name, m, fmt.max)  # no saturation, no inf


def ratios(items):
    """-> {name: worst |got - ref| / bound}; every element of every row takes part, a non-finite `got` counts as inf"""
    out = {}
    for it in items:
        assert it.got.shape == it.ref.shape == it.bound.shape, (it.name, it.got.shape, it.ref.shape, it.bound.shape)
        assert bool((it.bound > 0).all()), it.name
        r = (it.got.double() - it.ref).abs() / it.bound
        r = torch.where(torch.isfinite(it.got.double()), r, torch.full_like(r, float("inf")))
        out[it.name] = float(r.max()) if r.numel() else 0.0
    return out


def ratio_map(items, name):
    it = next(i for i in items if i.name == name)
    return (it.got.double() - it.ref).abs() / it.bound


def assert_within(items, what=""):
    r = ratios(items)
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, (what, bad)
    return r


# ------------------------------------------------------------------ the exact checks


def assert_masks_match_dumps(gates, D):
    """a mask bit is set if and only if the dumped element is non-zero -- all 11 layers, every view; and a relu'd dump holds no
    negative value (a -0 would set its bit)"""
    dumps = []
    for b in range(N_BLOCKS):
        dumps += [D["d_a"][b], D["d_n"][b]]
    dumps.append(D["d_x5"])
    for li, (g, d) in enumerate(zip(gates, dumps)):
        assert g.shape == d.shape, (li, g.shape, d.shape)
        assert torch.equal(g != 0, d != 0), (li, int(((g != 0) != (d != 0)).sum()))
        assert not bool((d < 0).any()) and not bool(torch.signbit(d).any()), li


def headroom(D, fmt):
    """max |gradient dump| / the type's largest finite value, per dump"""
    out = {}
    for b in range(N_BLOCKS - 1, -1, -1):
        out[f"g_fc1[{b}]"] = float(D["g_fc1"][b].abs().max()) / fmt.max
        out[f"g_fc0[{b}]"] = float(D["g_fc0"][b].abs().max()) / fmt.max
    out["g_x0"] = float(D["g_x0"].abs().max()) / fmt.max
    return out
