"""Child process of tests/test_hip_position_stage.py::test_latent_scatter_atomic_fallback (not a test): started with
PIXELNERF_SCATTER_TILED=0, so that a 72 x 80 grid takes latent_scatter_kernel, the global-atomic form of pnr_latent_scatter.  Runs
position_ref.CHILD_CASE, asserts the form and holds d_latent to the fp64 reference at the case's bar.  Exit code 0 = passed."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

import position_ref as PR  # noqa: E402


def main():
    from pixelnerf_amd import ops
    assert os.environ.get("PIXELNERF_SCATTER_TILED") == "0"
    dev = torch.device("cuda:0")
    case = PR.CHILD_CASE
    inp, ref64, ref32 = PR.reference(case)
    assert inp["SB"] == 1 and inp["NS"] == 2 and (inp["R"] * inp["K"]) % 16 != 0
    sc = ops.make_scene(inp["latent"].to(dev), inp["poses"].to(dev), inp["focal"].to(dev), inp["c"].to(dev), inp["image_shape"],
                        inp["NS"])
    assert not ops.latent_scatter_single_owner(sc, inp["R"], inp["K"]), "the tiled form is still selected"
    NV, _, Hl, Wl = inp["latent"].shape
    out = ops.latent_scatter(sc, inp["rays"].to(dev), inp["z"].to(dev), inp["g_z"].to(dev), torch.zeros(NV, Hl, Wl, 512, device=dev))
    got = out.permute(0, 3, 1, 2).cpu()
    err, err32 = PR.error(got, ref64["latent"]), PR.error(ref32["latent"], ref64["latent"])
    bar = PR.bar_from(err32)
    print(f"latent scatter (atomic) {case.name} d_latent: HIP {err:.2e} torch-fp32 {err32:.2e} bar {bar:.1e}")
    assert bool(torch.isfinite(got).all())
    assert err <= bar, f"{err:.3e} > {bar:.1e}"


if __name__ == "__main__":
    main()
