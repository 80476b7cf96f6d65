"""
Host test (no GPU): the formula of composite_bwd_kernel, restated in fp32 torch (tests/composite_bwd_ref.py), against fp64
autograd through the oracle's compositing, on the cases and density families of tests/test_hip_stage_sweep_backward.py and at its
bar (10 x the error of torch's fp32 autograd on the same inputs, floor 2e-6, cap 2e-5).

The division-free suffix recurrence meets the bar everywhere.  The form it replaced, suffix = total - prefix divided by
1 - alpha + 1e-10, misses it on the hostile R=64, K=64 case (d_z off by ~1e-3 of its largest entry): kept as a test so that the
sweep's sensitivity to this loss of digits is itself on record.
"""
import pytest
import torch

import composite_bwd_ref as CR

NAMES = ("d_rgbsigma", "d_z", "d_far")


def _compare(case, family, white, pre_activation=False, old_form=False):
    inp = CR.make_inputs(case, family, pre_activation)
    ref64 = CR.autograd_ref(inp, white, torch.float64, pre_activation)
    assert all(bool(torch.isfinite(r).all()) for r in ref64)
    err32 = CR.errors(CR.autograd_ref(inp, white, torch.float32, pre_activation), ref64)
    got = CR.composite_backward_ref(inp["rays"], inp["z"], inp["rgbsigma"], white, inp["d_rgb"], inp["d_depth"], inp["d_w"],
                                    pre_activation=pre_activation, old_form=old_form)
    assert all(bool(torch.isfinite(g).all()) for g in got)
    err = CR.errors(got, ref64)
    bars = [CR.bar_from(e) for e in err32]
    for n, e, e32, b in zip(NAMES, err, err32, bars):
        print(f"{case} {family} white={white} preact={pre_activation} old={old_form} {n}: err {e:.2e} torch-fp32 {e32:.2e} bar {b:.1e}")
    return err, bars


@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("family", CR.FAMILIES)
@pytest.mark.parametrize("case", CR.CASES, ids=CR.CASE_IDS)
def test_restated_formula_matches_fp64_autograd(case, family, white):
    err, bars = _compare(case, family, white)
    for n, e, b in zip(NAMES, err, bars):
        assert e <= b, f"{n}: {e:.3e} > {b:.1e}"


@pytest.mark.parametrize("case", CR.CASES, ids=CR.CASE_IDS)
def test_restated_formula_pre_activation(case):
    err, bars = _compare(case, "hostile", True, pre_activation=True)
    for n, e, b in zip(NAMES, err, bars):
        assert e <= b, f"{n}: {e:.3e} > {b:.1e}"


def test_reduced_forms_equal_zero_upstream():
    """d_depth / d_weights left out == zeros passed in their place"""
    inp = CR.make_inputs(CR.CASES[5], "hostile")
    a = (inp["rays"], inp["z"], inp["rgbsigma"], True, inp["d_rgb"])
    zd, zw = torch.zeros_like(inp["d_depth"]), torch.zeros_like(inp["d_w"])
    for dd, dw, dd0, dw0 in ((None, inp["d_w"], zd, inp["d_w"]), (inp["d_depth"], None, inp["d_depth"], zw), (None, None, zd, zw)):
        for x, y in zip(CR.composite_backward_ref(*a, dd, dw), CR.composite_backward_ref(*a, dd0, dw0)):
            assert torch.equal(x, y)


def test_old_suffix_form_misses_the_bar():
    """total - prefix, divided by tf: the rounding of the difference (~eps sum|g w|) over a tiny tf, times sigma ex in d_z.
    Sequential fp32 sums, hostile R=64 K=64: d_z error 7.8e-6 (black) / 3.2e-6 (white background) of max|d_z| against a bar of
    2e-6 (torch fp32 autograd: 1.7e-7) and 2.0e-7 / 2.1e-7 for the recurrence; the old form's worst over the sweep is 1.9e-5
    (shell, R=9 K=63)."""
    case = CR.CASES[CR.CASE_IDS.index("R64_K64")]
    for white in (False, True):
        err_new, bars = _compare(case, "hostile", white)
        err_old, _ = _compare(case, "hostile", white, old_form=True)
        assert err_new[1] <= bars[1]
        assert err_old[1] > bars[1], f"old form d_z error {err_old[1]:.3e}: the sweep would not see the cancellation"
        assert err_old[1] > 10 * err_new[1]
