"""
fp64 reference of the MLP backward STAGE of the fp32-class training paths (pnr_mlp_backward_split, pnr_mlp_backward_f32 with
split_gemm = 0 / 1): CPU, torch only.

The stage is a pure function of the weights, the network inputs the forward kept, the relu gates and g_out (P,4) =
dL/d(lin_out output).  Its 32 outputs -- the 30 parameter gradients under the reference's state-dict names, d_zlat (NS*P,512)
and d_in (NS*P,42) -- come from torch AUTOGRAD in float64 through a restatement of ResnetFC.forward (resnetfc.py:53-62,132-184,
the lines oracle.pnr_oracle.resnetfc_forward cites; mean pooling in front of block 3), not from a hand-written backward chain.

  rows    the library's: [view][point], points object-major; the view mean is x.reshape(NS, P, 512).mean(0).
  inputs  exactly what the kernel was given: in42[:, :42] and zlat of F32Saved, head + tail of in_op[:, :42] / zlat of SplitSaved.
  gates   INPUTS, not recomputed: relu(t) is t * gate with the 11 gate arrays of the saved state (saved > 0 for F32Saved, the
          decoded 1-bit mask words for SplitSaved).  A pre-activation within rounding of zero would otherwise flip a gate on one
          side only; with the gates forced the stage is smooth and every difference is arithmetic.
"""
import numpy as np
import torch

N_BLOCKS, COMBINE_LAYER, D_HID, D_IN, N_GATES = 5, 3, 512, 42, 11
# gate order = mask-layer order of pnr_device.h: xin[0], net[0], ..., xin[4], net[4], x5; the first 6 are per view (NS*P rows)
PER_VIEW_GATES = 2 * COMBINE_LAYER

PARAM_KEYS = (["lin_in.weight", "lin_in.bias", "lin_out.weight", "lin_out.bias"]
              + [f"blocks.{b}.{fc}.{wb}" for b in range(N_BLOCKS) for fc in ("fc_0", "fc_1") for wb in ("weight", "bias")]
              + [f"lin_z.{b}.{wb}" for b in range(COMBINE_LAYER) for wb in ("weight", "bias")])
OUTPUT_KEYS = PARAM_KEYS + ["d_zlat", "d_in"]
assert len(OUTPUT_KEYS) == 32

# The committed bars of tests/test_hip_mlp_backward_stage.py, per form, on both metrics: 4x the worst figure measured on an
# MI355X over every case (profiles/mlp_backward_stage_notes.md), rounded up to one significant digit, never above the
# project's fp32-class bar 2e-5.  tests/test_mlp_bwd_ref_host.py proves that they bite.
FP32_CLASS_BAR = 2e-5
BARS = {"exact": 3e-6, "gemms": 1e-5, "fused": 1e-5}
assert max(BARS.values()) <= FP32_CLASS_BAR


def decode_relu_masks(masks, P, NS):
    """The 1-bit relu masks of PnrSplitSaved -> bool (11, NS, P, 512), [layer][view][point][feature] (feature order; layers 6..10
    are pooled: only view 0 is written).  Layout (pnr_device.h): [layer][view][tile][thread] 64-bit words, bit (it*2 + jt)*16 + r
    <-> feature 64 wv + 32 it + (r&3) + 8 (r>>2) + 4 h of point 32 jt + (lane & 31) of the 64-point tile, thread = 64 wv + lane,
    h = lane >> 5."""
    ntiles = (P + 63) // 64
    if torch.is_tensor(masks):
        masks = masks.detach().cpu().contiguous().view(torch.int64).numpy()
    words = np.asarray(masks).view(np.uint64).reshape(N_GATES, NS, ntiles, 512)
    k = np.arange(64, dtype=np.uint64)
    bits = ((words[..., None] >> k) & np.uint64(1)).astype(bool)  # (11, NS, ntiles, thread, bit)
    t, kb = np.arange(512)[:, None], np.arange(64)[None, :]
    wv, lane = t >> 6, t & 63
    it, jt, r = kb >> 5, (kb >> 4) & 1, kb & 15
    feat = 64 * wv + 32 * it + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
    pt = 32 * jt + (lane & 31)
    dest = (pt * 512 + feat).reshape(-1)  # a bijection of (thread, bit) onto (point of the tile, feature)
    assert np.unique(dest).size == 64 * 512
    out = np.empty((N_GATES, NS, ntiles, 64 * 512), dtype=bool)
    out[..., dest] = bits.reshape(N_GATES, NS, ntiles, 64 * 512)
    return out.reshape(N_GATES, NS, ntiles * 64, 512)[:, :, :P]


def gates_from_masks(masks, P, NS):
    """SplitSaved.masks -> the 11 gate arrays (float64 0/1), (NS*P,512) for the per-view layers, (P,512) for the pooled ones"""
    g = decode_relu_masks(masks, P, NS)
    return [torch.from_numpy(g[li].reshape(NS * P, 512) if li < PER_VIEW_GATES else g[li, 0]).double() for li in range(N_GATES)]


def gates_from_f32_saved(saved):
    """F32Saved -> the 11 gate arrays: saved > 0 on xin[b], net[b] and x5"""
    pre = []
    for b in range(N_BLOCKS):
        pre += [saved.xin[b], saved.net[b]]
    pre.append(saved.x5)
    return [(t.detach().cpu() > 0).double() for t in pre]


def inputs_from_f32_saved(saved):
    return saved.in42.detach().cpu()[:, :D_IN].double(), saved.zlat.detach().cpu().double()


def inputs_from_split_saved(saved):
    """head + tail of the (2, rows, cols) f16 pairs, summed in float64 (the value the kernel's operands carry)"""
    io, zl = saved.in_op.detach().cpu().double(), saved.zlat.detach().cpu().double()
    return (io[0] + io[1])[:, :D_IN].contiguous(), zl[0] + zl[1]


def forward(p, in42, zlat, NS, gates=None, collect=None):
    """ResnetFC.forward (resnetfc.py:132-184 with ResnetBlockFC.forward :53-62 inlined) on the library's rows.  gates: 11 arrays
    that replace every relu(t) by t * gate; None: plain relu, and `collect` (a list) receives the gates this forward takes."""
    F = torch.nn.functional
    n = [0]

    def act(t):
        if gates is None:
            if collect is not None:
                collect.append((t.detach() > 0).to(t.dtype))
            return torch.relu(t)
        g = gates[n[0]]
        n[0] += 1
        assert g.shape == t.shape, (n[0] - 1, g.shape, t.shape)
        return t * g

    x = F.linear(in42, p["lin_in.weight"], p["lin_in.bias"])  # :147
    for b in range(N_BLOCKS):
        if b == COMBINE_LAYER and NS > 1:  # util.combine_interleaved (util.py:461-471), rows [view][point]
            x = x.reshape(NS, -1, D_HID).mean(0)
        if b < COMBINE_LAYER:
            x = x + F.linear(zlat, p[f"lin_z.{b}.weight"], p[f"lin_z.{b}.bias"])  # :175-180
        net = F.linear(act(x), p[f"blocks.{b}.fc_0.weight"], p[f"blocks.{b}.fc_0.bias"])  # :55
        x = x + F.linear(act(net), p[f"blocks.{b}.fc_1.weight"], p[f"blocks.{b}.fc_1.bias"])  # :56-62
    return F.linear(act(x), p["lin_out.weight"], p["lin_out.bias"])  # :183


def own_gates(params, in42, zlat, NS, dtype=torch.float64):
    """the gates the reference's own (ungated) forward takes"""
    got = []
    with torch.no_grad():
        forward({k: v.to(dtype) for k, v in params.items()}, in42.to(dtype), zlat.to(dtype), NS, collect=got)
    assert len(got) == N_GATES
    return got


class StageRef:
    """One gated forward, any number of backwards: StageRef(...).backward(g_out) -> {the 32 OUTPUT_KEYS: tensor of `dtype`}.
    dtype = torch.float32 is the same chain as a plain fp32 torch run (what a correct fp32 implementation looks like)."""

    def __init__(self, params, in42, zlat, gates, NS, dtype=torch.float64):
        self.p = {k: params[k].detach().to(dtype).clone().requires_grad_(True) for k in PARAM_KEYS}
        self.in42 = in42.detach().to(dtype).clone().requires_grad_(True)
        self.zlat = zlat.detach().to(dtype).clone().requires_grad_(True)
        assert self.in42.shape[1] == D_IN and self.zlat.shape == (self.in42.shape[0], 512) and self.in42.shape[0] % NS == 0
        assert len(gates) == N_GATES
        self.dtype = dtype
        self.out = forward(self.p, self.in42, self.zlat, NS, gates=[g.to(dtype) for g in gates])

    def backward(self, g_out):
        leaves = [self.p[k] for k in PARAM_KEYS] + [self.zlat, self.in42]
        got = torch.autograd.grad(self.out, leaves, grad_outputs=g_out.detach().to(self.dtype).reshape(self.out.shape),
                                  retain_graph=True)
        return dict(zip(OUTPUT_KEYS, got))


def rel_l2(a, b):
    """|a - b| / |b| in float64; a zero reference asks for an exactly zero result"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    nb = float(b.norm())
    if nb == 0.0:
        return 0.0 if float(a.norm()) == 0.0 else float("inf")
    return float((a - b).norm()) / nb


def row_metric(a, b):
    """largest row error over the largest row norm: a wrong tail tile cannot hide in the norm of a long tensor"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    nb = float(b.norm(dim=1).max())
    e = float((a - b).norm(dim=1).max())
    if nb == 0.0:
        return 0.0 if e == 0.0 else float("inf")
    return e / nb


def stage_errors(got, ref):
    """-> {key: relative L2} over the 32 outputs plus {"d_zlat.rows", "d_in.rows"}: the row metric"""
    errs = {}
    for k in OUTPUT_KEYS:
        assert torch.isfinite(got[k]).all(), k
        errs[k] = rel_l2(got[k], ref[k])
    for k in ("d_zlat", "d_in"):
        errs[k + ".rows"] = row_metric(got[k], ref[k])
    return errs


def worst(errs):
    k = max(errs, key=errs.get)
    return k, errs[k]
