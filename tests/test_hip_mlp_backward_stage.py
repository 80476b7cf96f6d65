"""
GPU tests (-m gpu) of the MLP backward STAGE of the fp32-class training paths at its own resolution: the three forms of one
arithmetic

  fused   pnr_eval_ray_samples_split_train + pnr_mlp_backward_split (bwd_split_kernel of pnr_bwd_split.hip, the batched split-operand weight-gradient
          launch, lin_out's gradient): what precision "f16x3" trains with
  gemms   pnr_eval_ray_samples_f32_train(split) + pnr_mlp_backward_f32(split_gemm = 1): one split-operand GEMM per layer
  exact   the same with split_gemm = 0: exact fp32 MFMA products, the yardstick

each against tests/mlp_bwd_ref.py: float64 autograd through a restatement of ResnetFC.forward, fed with exactly the inputs and the
relu gates that run's forward saved.  All 32 outputs (30 parameter gradients, d_zlat, d_in) by relative L2, d_zlat and d_in also
by largest row error / largest row norm; nothing is left out of a comparison.

The bars (mlp_bwd_ref.BARS) are 4x the worst figure measured on an MI355X over every case below, one significant digit, capped by
the project's fp32-class bar 2e-5: the table is in profiles/mlp_backward_stage_notes.md (exact 6.6e-7 -> 3e-6, both split forms
2.4e-6 / 2.5e-6 -> 1e-5; the split forms' worst tensors are bias gradients at the largest point count: the f16 matrix
instruction's sum rounds toward minus infinity, and that bias adds up linearly over rows -- measured and explained there).
tests/test_hip_backward_f32.py keeps guarding the whole render at 1e-3 (sampling discontinuities live there);
tests/test_mlp_bwd_ref_host.py shows that a dropped tail product, one layer's wrong tail stream or ONE wrong mask bit misses these
bars by more than 10x.
"""
import pytest
import torch

import mlp_bwd_ref as R
from helpers import mlp_params, scene_for
from testdata import synthetic

pytestmark = pytest.mark.gpu

FORMS = ["exact", "gemms", "fused"]

# name -> (scene, rays per object, samples per ray).  The tile is 64 points.
CASES = {
    "sn64-1x1": ("sn64", 1, 1),          # one point
    "sn64-1x63": ("sn64", 1, 63),        # one short of a tile
    "sn64-1x64": ("sn64", 1, 64),        # exactly one tile
    "sn64-5x13": ("sn64", 5, 13),        # 65: one point in the second tile
    "sn64-7x37": ("sn64", 7, 37),        # 259: ragged last tile
    "train-24x37": ("train", 24, 37),    # 4 objects x 1 view: object boundaries inside tiles
    "mv_mini-10x45": ("mv_mini", 10, 45),     # 2 objects x 2 views: pooled backward (1/NS), per-view masks
    "train_mv3-6x37": ("train_mv3", 6, 37),   # 2 objects x 3 views: multi-view workspace
}
MV_MINI = "mv_mini-10x45"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def network(net):
    if net == "surface":  # lin_out's sigma row x 100: the range the device-picked scale has to cover
        return synthetic.surface_variant(mlp_params(11), 100.0, 4.3)
    return mlp_params(int(net))


class Stage:
    """one training forward of a form on a case: the saved state on the device and the float64 reference built from it"""

    def __init__(self, dev, form, case, net):
        from pixelnerf_amd import ops
        scene_name, n_rays, K = CASES[case]
        scene, meta = scene_for(scene_name)
        self.form, self.NS = form, scene["NS"]
        sc = ops.make_scene(scene["latent"].to(dev), scene["poses"].to(dev), scene["focal"].to(dev), scene["c"].to(dev),
                            scene["image_shape"], self.NS)
        rays = synthetic.target_rays(meta, n_rays=n_rays).reshape(-1, 8)
        u = torch.sort(torch.rand(rays.shape[0], K, generator=torch.Generator().manual_seed(2)), dim=-1)[0]
        z = rays[:, 6:7] + (rays[:, 7:8] - rays[:, 6:7]) * u
        rays, z = rays.to(dev), z.to(dev).contiguous()
        self.P = rays.shape[0] * K
        self.params = network(net)
        state = {k: v.to(dev) for k, v in self.params.items()}
        self.weights = ops.pack_mlp(state, "f32")
        if form == "fused":
            _, self.saved = ops.eval_ray_samples_split_train(sc, ops.pack_mlp(state, "f16x3"), ops.fold_latent(sc, state, "f16x3"), rays, z)
            in42, zlat = R.inputs_from_split_saved(self.saved)
            gates = R.gates_from_masks(self.saved.masks, self.P, self.NS)
        else:
            _, self.saved = ops.eval_ray_samples_f32_train(sc, self.weights, rays, z, split=(form == "gemms"))
            in42, zlat = R.inputs_from_f32_saved(self.saved)
            gates = R.gates_from_f32_saved(self.saved)
        torch.cuda.synchronize()
        self.ref = R.StageRef(self.params, in42, zlat, gates, self.NS)
        self._keep = (sc, state)

    def backward(self, g_out, want_d_in=True, want_grads=True):
        from pixelnerf_amd import ops
        fn = ops.mlp_backward_split if self.form == "fused" else ops.mlp_backward_f32
        grads, d_zlat, d_in = fn(self.weights, self.saved, g_out, want_d_in=want_d_in, want_grads=want_grads)
        torch.cuda.synchronize()
        return grads, d_zlat, d_in

    def outputs(self, g_out):
        grads, d_zlat, d_in = self.backward(g_out.to(self.saved.x5.device))
        assert set(grads) == set(R.PARAM_KEYS)
        got = {k: v.cpu() for k, v in grads.items()}
        got["d_zlat"], got["d_in"] = d_zlat.cpu(), d_in.cpu()
        return got


_STAGES = {}


def mv_mini_stage(dev, form):
    """the mv_mini case with mlp_params(11): shared by the g_out variants and the properties (one forward, one reference graph)"""
    if form not in _STAGES:
        _STAGES[form] = Stage(dev, form, MV_MINI, 11)
    return _STAGES[form]


def g_out_variant(kind, P):
    g = 1e-3 * torch.randn(P, 4, generator=torch.Generator().manual_seed(5))
    if kind == "sigma":  # only the density column
        g[:, :3] = 0.0
    elif kind == "rows7":  # every seventh row zero
        g[::7] = 0.0
    elif kind == "span":  # row magnitudes 1e-6 ... 1, shuffled over the rows
        mag = 10.0 ** (-6.0 * torch.arange(P, dtype=torch.float32) / max(P - 1, 1))
        g = 1e3 * g * mag[torch.randperm(P, generator=torch.Generator().manual_seed(6))][:, None]
    elif kind == "zero":
        g.zero_()
    else:
        assert kind == "randn", kind
    return g


def check(stage, g_out, what):
    errs = R.stage_errors(stage.outputs(g_out), stage.ref.backward(g_out))
    k, e = R.worst({k: v for k, v in errs.items() if not k.endswith(".rows")})
    print(f"STAGE {stage.form} {what} P={stage.P} NS={stage.NS}: worst {e:.2e} ({k}) d_zlat {errs['d_zlat']:.2e} d_in {errs['d_in']:.2e} "
          f"rows {max(errs['d_zlat.rows'], errs['d_in.rows']):.2e}")
    bar = R.BARS[stage.form]
    bad = {k: v for k, v in errs.items() if not v <= bar}
    assert not bad, (stage.form, what, bar, bad)


@pytest.mark.parametrize("net", [11, 12])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("form", FORMS)
def test_stage_matches_fp64_reference(dev, form, case, net):
    stage = mv_mini_stage(dev, form) if (case, net) == (MV_MINI, 11) else Stage(dev, form, case, net)
    check(stage, g_out_variant("randn", stage.P), f"{case} net={net} g=randn")


@pytest.mark.parametrize("form", FORMS)
def test_stage_with_a_large_lin_out_row(dev, form):
    stage = Stage(dev, form, MV_MINI, "surface")
    check(stage, g_out_variant("randn", stage.P), f"{MV_MINI} net=surface g=randn")


@pytest.mark.parametrize("kind", ["sigma", "rows7", "span"])
@pytest.mark.parametrize("form", FORMS)
def test_stage_g_out_variants(dev, form, kind):
    """span: the rows of g_out cover 1e-6 ... 1; small rows legitimately lose bits to the single power-of-two scale of the split
    forms, so the row metric is relative to the LARGEST row (as everywhere) and the tensor norms are dominated by the large rows"""
    stage = mv_mini_stage(dev, form)
    check(stage, g_out_variant(kind, stage.P), f"{MV_MINI} net=11 g={kind}")


@pytest.mark.parametrize("form", FORMS)
def test_zero_g_out_gives_exact_zeros(dev, form):
    stage = mv_mini_stage(dev, form)
    got = stage.outputs(g_out_variant("zero", stage.P))
    for k in R.OUTPUT_KEYS:
        assert torch.isfinite(got[k]).all() and not got[k].any(), k


def same(a, b, what):
    assert a.shape == b.shape and torch.equal(a, b), (what, float((a.double() - b.double()).abs().max()))


@pytest.mark.parametrize("form", FORMS)
def test_stage_outputs_do_not_depend_on_what_is_asked_for(dev, form):
    """bit for bit: want_grads=False and want_d_in=False change nothing else; a second call reproduces every output"""
    stage = mv_mini_stage(dev, form)
    g = g_out_variant("randn", stage.P).to(dev)
    grads, d_zlat, d_in = stage.backward(g)
    none, d_zlat_a, d_in_a = stage.backward(g, want_grads=False)
    assert none is None
    same(d_zlat_a, d_zlat, "d_zlat without grads")
    same(d_in_a, d_in, "d_in without grads")
    grads_b, d_zlat_b, none = stage.backward(g, want_d_in=False)
    assert none is None
    same(d_zlat_b, d_zlat, "d_zlat without d_in")
    grads_c, d_zlat_c, d_in_c = stage.backward(g)
    same(d_zlat_c, d_zlat, "d_zlat again")
    same(d_in_c, d_in, "d_in again")
    for k in R.PARAM_KEYS:
        same(grads_b[k], grads[k], k + " without d_in")
        same(grads_c[k], grads[k], k + " again")


@pytest.mark.parametrize("shift", [20, -20])
@pytest.mark.parametrize("form", FORMS)
def test_stage_is_exactly_homogeneous_in_powers_of_two(dev, form, shift):
    """g_out * 2^+-20 gives exactly 2^+-20 times every output: the split forms run the chain at a power-of-two scale picked from
    max |g_out| on the device and un-scale exactly on the way out, the exact form has no scale at all (every value stays far
    inside the normal fp32 range here, so a power of two only moves exponents)"""
    stage = mv_mini_stage(dev, form)
    g = g_out_variant("randn", stage.P).to(dev)
    f = 2.0 ** shift
    grads, d_zlat, d_in = stage.backward(g)
    grads_s, d_zlat_s, d_in_s = stage.backward(g * f)
    same(d_zlat_s, d_zlat * f, "d_zlat")
    same(d_in_s, d_in * f, "d_in")
    for k in R.PARAM_KEYS:
        same(grads_s[k], grads[k] * f, k)
