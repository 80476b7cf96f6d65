"""
NeRFRenderer / _RenderWrapper with the reference's API (src/render/nerf.py:15-371); the work
is done by libpixelnerf_hip.so.

With a pixelnerf_amd PixelNeRFNet the whole forward (coarse sampling -> fused network ->
compositing -> inverse-CDF + depth resampling + sort -> fused network -> compositing) is one
C call (pnr_render_forward).  Any other `model(xyz, coarse=, viewdirs=)` callable still works:
sampling and compositing run as HIP kernels around the caller's model, chunked by
eval_batch_size exactly like the reference -- and differentiably (autograd.composite_autograd /
sample_fine_autograd), so a renderer around an arbitrary nn.Module trains as it does in the reference.

What the reference does not have -- occupancy-grid culling, skip_empty, early ray termination of inference renders -- is in
render/accel.py; forward and render_views document its keywords and hand the call over as one accel.Accel record.

Random numbers.  `rng="philox"` (default in eval mode with a pixelnerf_amd net): the sampling kernels draw from a
counter-based generator (Philox4x32-10) keyed by a 64-bit seed -- `torch.initial_seed()` of the ray device's generator
mixed with that generator's Philox offset (advanced per call, host side), so `torch.manual_seed(s)` makes a run
reproducible exactly as it does for the reference, without any device-side launch or HBM traffic for noise; a draw depends only on (seed, global ray id, draw, index), so chunked or multi-GPU
sharded renders give the same image as one call.  `rng="torch"` (and training, and generic model callables): torch's
generator on the ray device, in the reference's draw order (nerf.py:111,135,141,158).  Tests inject pre-drawn noise
through `_noise`.
"""
import torch

from .. import ops
from ..util.dotmap import DotMap
from . import accel as _accel


TERMINATE_STAGES = 8  # default number of stages of a terminated fine pass: the fastest of 2 / 4 / 8 without a grid (profiles/termination_notes.md)


class _RenderWrapper(torch.nn.Module):
    """src/render/nerf.py:15-42."""

    def __init__(self, net, renderer, simple_output):
        super().__init__()
        self.net = net
        self.renderer = renderer
        self.simple_output = simple_output

    def forward(self, rays, want_weights=False, occupancy=None, tighten=False, skip_empty=False, terminate=None,
                terminate_stages=TERMINATE_STAGES):
        if rays.shape[0] == 0:
            return (torch.zeros(0, 3, device=rays.device), torch.zeros(0, device=rays.device))
        with torch.profiler.record_function("render_par"):
            outputs = self.renderer(self.net, rays, want_weights=want_weights and not self.simple_output, occupancy=occupancy,
                                    tighten=tighten, skip_empty=skip_empty, terminate=terminate, terminate_stages=terminate_stages)
        if self.simple_output:
            if self.renderer.using_fine:
                return outputs.fine.rgb, outputs.fine.depth
            return outputs.coarse.rgb, outputs.coarse.depth
        return outputs.toDict()

    def render_views(self, poses_c2w, W, H, focal, z_near, z_far, c=None, gt_rgb=None, want_u8=False, views_per_call=None,
                     _noise=None, occupancy=None, tighten=False, skip_empty=False, terminate=None, terminate_stages=TERMINATE_STAGES):
        """Images of the target views from their cameras, with depth normalisation and, given ground truth, PSNR and SSIM per
        view, all on the device (NeRFRenderer.render_views; the loop of eval/eval.py:247-331 as one call).  Inference only:
        runs under torch.no_grad()."""
        with torch.profiler.record_function("render_par"):
            return self.renderer.render_views(self.net, poses_c2w, W, H, focal, z_near, z_far, c=c, gt_rgb=gt_rgb, want_u8=want_u8,
                                              views_per_call=views_per_call, _noise=_noise, occupancy=occupancy, tighten=tighten,
                                              skip_empty=skip_empty, terminate=terminate, terminate_stages=terminate_stages)


class NeRFRenderer(torch.nn.Module):
    """NeRF renderer; parameters as src/render/nerf.py:45-96."""

    def __init__(self, n_coarse=128, n_fine=0, n_fine_depth=0, noise_std=0.0, depth_std=0.01,
                 eval_batch_size=100000, white_bkgd=False, lindisp=False, sched=None, rng="philox"):
        super().__init__()
        if rng not in ("philox", "torch"):
            raise ValueError("rng must be 'philox' (in-kernel counter-based draws) or 'torch'")
        self.rng = rng
        self._seed_override = None  # set by the multi-device wrapper: every shard of one call uses the same key
        self.ray_id_offset = 0  # placement of this call's rays inside a larger ray set (set by sharding wrappers)
        self.ray_id_stride = 0
        self.last_skip_stats = None  # of the last call with skip_empty=True: {"coarse": (kept, total), "fine": (kept, total)} samples
        # of the last call with terminate=eps: {"evaluated", "total" (fine samples), "stopped_rays", "rays", "stages": [(kept, in_stage), ...]}
        self.last_terminate_stats = None
        self.n_coarse, self.n_fine, self.n_fine_depth = n_coarse, n_fine, n_fine_depth
        self.noise_std, self.depth_std = noise_std, depth_std
        self.eval_batch_size = eval_batch_size
        self.white_bkgd = white_bkgd
        self.lindisp = lindisp
        if lindisp:
            print("Using linear displacement rays")
        self.using_fine = n_fine > 0
        self.sched = sched
        if sched is not None and len(sched) == 0:
            self.sched = None
        self.register_buffer("iter_idx", torch.tensor(0, dtype=torch.long), persistent=True)
        self.register_buffer("last_sched", torch.tensor(0, dtype=torch.long), persistent=True)

    # ---- stage methods (same names / shapes as the reference; HIP kernels underneath) ----
    def sample_coarse(self, rays, _u=None):
        """nerf.py:98-118.  rays (B,8) -> (B,Kc)."""
        u = torch.rand(rays.shape[0], self.n_coarse, device=rays.device) if _u is None else _u
        if torch.is_grad_enabled() and rays.requires_grad:  # near / far carry gradient (nerf.py:113-115)
            from ..autograd import sample_coarse_autograd
            return sample_coarse_autograd(rays, u, self.lindisp)
        return ops.sample_coarse(rays, u, self.lindisp)

    def sample_fine(self, rays, weights, _u2=None, _u3=None):
        """nerf.py:120-148.  -> (B, Kf-Kfd), unsorted, like the reference."""
        n = self.n_fine - self.n_fine_depth
        B, dev = rays.shape[0], rays.device
        u2 = torch.rand(B, n, dtype=torch.float32, device=dev) if _u2 is None else _u2
        u3 = torch.rand(B, n, dtype=torch.float32, device=dev) if _u3 is None else _u3
        # the kernel returns sorted([z_coarse, z_fine]); feeding `near` as every coarse sample and
        # dropping the Kc smallest leaves the sorted importance samples (their order is irrelevant
        # downstream: forward() sorts everything, :295)
        Kc = weights.shape[1]
        z0 = rays[:, 6:7].expand(-1, Kc).contiguous()
        z = ops.sample_fine(rays, weights.detach(), None, z0, u2, u3, None, self.depth_std, self.lindisp)
        return z[:, Kc:].contiguous()

    def sample_fine_depth(self, rays, depth, _n=None):
        """nerf.py:150-161.  -> (B, Kfd)."""
        n = torch.randn(rays.shape[0], self.n_fine_depth, device=rays.device) if _n is None else _n
        z0 = rays[:, 6:7].contiguous()
        z = ops.sample_fine(rays, None, depth, z0, None, None, n, self.depth_std, self.lindisp)
        return z[:, 1:].contiguous()  # drop the placeholder coarse sample (= near, the minimum)

    def composite(self, model, rays, z_samp, coarse=True, sb=0):
        """nerf.py:163-249 for an arbitrary model callable: points/viewdirs, chunked model
        calls (eval_batch_size), then the HIP compositing kernel.
        :return weights (B,K), rgb (B,3), depth (B)"""
        with torch.profiler.record_function("renderer_composite"):  # nerf.py:175
            return self._composite(model, rays, z_samp, coarse, sb)

    def _composite(self, model, rays, z_samp, coarse, sb):
        B, K = z_samp.shape
        points = (rays[:, None, :3] + z_samp.unsqueeze(2) * rays[:, None, 3:6]).reshape(-1, 3)
        use_viewdirs = hasattr(model, "use_viewdirs") and model.use_viewdirs
        if sb > 0:
            points = points.reshape(sb, -1, 3)
            eval_batch_size = (self.eval_batch_size - 1) // sb + 1
            dim = 1
        else:
            eval_batch_size = self.eval_batch_size
            dim = 0
        val_all = []
        split_points = torch.split(points, eval_batch_size, dim=dim)
        if use_viewdirs:
            viewdirs = rays[:, None, 3:6].expand(-1, K, -1)
            viewdirs = viewdirs.reshape(sb, -1, 3) if sb > 0 else viewdirs.reshape(-1, 3)
            for pnts, dirs in zip(split_points, torch.split(viewdirs, eval_batch_size, dim=dim)):
                val_all.append(model(pnts.contiguous(), coarse=coarse, viewdirs=dirs.contiguous()))
        else:
            for pnts in split_points:
                val_all.append(model(pnts.contiguous(), coarse=coarse))
        out = torch.cat(val_all, dim=dim).reshape(B, K, -1)
        if self.training and self.noise_std > 0.0:
            out = torch.cat([out[..., :3], out[..., 3:4] + torch.randn_like(out[..., 3:4]) * self.noise_std], -1)
        rgbs = out[..., :4].contiguous()
        if torch.is_grad_enabled() and (rgbs.requires_grad or z_samp.requires_grad or rays.requires_grad):
            # training with an arbitrary model: the compositing kernels as an autograd node (pnr_composite /
            # pnr_composite_backward); gradients reach the model through its outputs and, for the depth samples of the fine
            # pass, through the sample positions (points above are torch ops on z_samp)
            from ..autograd import composite_autograd
            return composite_autograd(rays, z_samp, rgbs, self.white_bkgd)
        return ops.composite(rays, z_samp, rgbs, self.white_bkgd, want_weights=True)

    # ---- forward ----
    def _draw_noise(self, R, dev):
        """torch draws in the reference's order: rand_like (R,Kc) :111, rand (R,Kf-Kfd) :135,
        rand_like :141, randn_like (R,Kfd) :158."""
        noise = {"u1": torch.rand(R, self.n_coarse, device=dev)}
        if self.using_fine:
            n_imp = self.n_fine - self.n_fine_depth
            if n_imp > 0:
                noise["u2"] = torch.rand(R, n_imp, dtype=torch.float32, device=dev)
                noise["u3"] = torch.rand(R, n_imp, dtype=torch.float32, device=dev)
            if self.n_fine_depth > 0:
                noise["n4"] = torch.randn(R, self.n_fine_depth, device=dev)
        return noise

    def forward(self, model, rays, want_weights=False, _noise=None, occupancy=None, tighten=False, skip_empty=False, terminate=None,
                terminate_stages=TERMINATE_STAGES):
        """src/render/nerf.py:251-303.
        :param model nerf model: (SB,B,3) points [+ viewdirs] -> (SB,B,4) rgb sigma
        :param rays [origins(3), directions(3), near, far] (SB,B,8)
        :param occupancy a util.occupancy.OccupancyGrid of the ONE encoded object (inference only): only the rays that pass through
        an occupied cell are rendered, the others are filled with what the compositing yields for sigma == 0 (nerf.py:223-249: rgb 0,
        or 1 with white_bkgd; depth 0; weights 0).  With rng="philox" a rendered ray has exactly the bits of the call without
        `occupancy` (it keeps the draws of its global ray id); with rng="torch" or a generic model callable the draws are made for
        the rendered rays only, so the image is a different sample of the same distribution.  None: the call of the reference.
        :param tighten with `occupancy`: sample every rendered ray between its first and last occupied cell instead of [near, far]
        (the same number of samples over a shorter range: denser, so the image then differs from the dense render everywhere)
        :param skip_empty with `occupancy` and a fused PixelNeRFNet: the rendered rays run the network only on the samples that
        lie in an occupied cell; every other sample gets rgb sigma = 0.  The result is the dense render of those rays with sigma
        forced to 0 in the cells the grid calls empty (so its quality is the grid's: reso, threshold, dilate) -- bit for bit at every
        precision -- at two host synchronisations more per call (the kept samples of the coarse and of the fine pass).  `last_skip_stats` then holds
        {"coarse": (kept, total), "fine": (kept, total)} samples.
        :param terminate eps in (0, 1), with a fused PixelNeRFNet (inference only, ONE object; with or without `occupancy`): early ray
        termination of the FINE pass.  Its K = n_coarse + n_fine sorted samples are cut into stages at fixed sample indices; a ray
        stops at the first stage boundary at which the transmittance in front of it (the compositing's own fp32 product) is <= eps,
        and the network is not run behind it.  The fine outputs are the compositing of the dense fine pass's per-sample outputs with
        rgb sigma = 0 behind each ray's stop (and, with skip_empty, in the cells the grid calls empty), bit for bit at every
        precision: the weights in front of the stop are the dense weights, behind it 0, and the transmittance that is left goes to
        the background.  On a ray whose samples all lie within [near, far] every channel moves by at most eps towards the background
        and the depth by at most eps * far; a ray with a sample beyond `far` (a depth sample drawn past it) has a negative last
        interval and is covered by the identity only.  The coarse pass is untouched -- it places the fine samples -- and the draws are
        taken where the dense call takes them, so under the same torch.manual_seed the coarse outputs are the dense call's bits.
        One host synchronisation per stage.  `last_terminate_stats` then holds {"evaluated", "total", "stopped_rays", "rays",
        "stages": [(kept, in_stage), ...]}: fine samples the network ran on / all of them, rays that stopped / all rendered rays.
        :param terminate_stages the number S of stages -- boundaries at 2 ((K s) // (2 S)) --, or the increasing sequence of the
        boundaries inside (0, K) themselves; 1: no boundary, the dense render
        :return DotMap {coarse:{rgb (SB,B,3), depth (SB,B)[, weights (SB,B,K)]}, fine:{...}}"""
        accel = _accel.Accel.parse(self, occupancy, tighten, skip_empty, terminate, terminate_stages)
        with torch.profiler.record_function("renderer_forward"):  # the reference's scope name (nerf.py:264)
            if accel is not None:  # (render/accel.py: what the reference does not have)
                return _accel.forward(self, model, rays, want_weights, _noise, accel)
            return self._forward(model, rays, want_weights, _noise)

    def _apply_sched(self):
        if self.sched is not None and self.last_sched.item() > 0:
            self.n_coarse = self.sched[1][self.last_sched.item() - 1]
            self.n_fine = self.sched[2][self.last_sched.item() - 1]

    def _fine_counts(self):
        """(Kf, Kfd): the samples of the fine pass (0 without one) and how many of them are depth samples"""
        Kf = self.n_fine if self.using_fine else 0
        return Kf, min(self.n_fine_depth, Kf)

    @staticmethod
    def _is_fused(model):
        # pixelnerf_amd.PixelNeRFNet in the shipped configuration: the fused kernels.  Any other model -- including a PixelNeRFNet
        # configured outside what the fused kernels implement (composed forward) -- is a callable to the reference's control flow.
        return hasattr(model, "scene") and hasattr(model, "packed") and (not hasattr(model, "fused_supported") or model.fused_supported())

    def _forward(self, model, rays, want_weights, _noise):
        self._apply_sched()
        assert len(rays.shape) == 3
        SB = rays.shape[0]
        rays = rays.reshape(-1, 8).float().contiguous()
        R = rays.shape[0]
        fused = self._is_fused(model)
        # (inside a HIP-graph capture the generator's offset cannot be read on the host: torch's own graph-safe draws are used)
        seeded = (_noise is None and fused and self.rng == "philox" and not (self.training and torch.is_grad_enabled())
                  and not (rays.is_cuda and torch.cuda.is_current_stream_capturing()))
        noise = _noise if (_noise is not None or seeded) else self._draw_noise(R, rays.device)
        Kf, Kfd = self._fine_counts()

        if fused:  # pixelnerf_amd.PixelNeRFNet: one C call
            model._check_supported()
            needs_grad = self._fused_needs_grad(model, rays)
            if self.training and self.noise_std > 0.0 and not needs_grad:
                raise NotImplementedError("noise_std > 0 in train mode is implemented on the differentiable path (grad enabled); "
                                          "the reference adds the noise only while training (nerf.py:225-226)")
            if needs_grad:  # training: differentiable path (HIP forward with operand dumps + HIP backward)
                from ..autograd import render_autograd
                model._check_trainable()
                if noise is None:
                    noise = self._draw_noise(R, rays.device)
                guarded = model._guard_begin(training=True)
                try:
                    res = render_autograd(self, model, rays, noise, want_weights)
                finally:
                    if guarded:
                        model._guard_end()
            else:
                seed = self._next_seed(rays.device) if seeded else 0
                res = self._fused_inference(model, Kf, seed, seeded, _noise, noise,
                                            self._rays_launch(model, rays, noise, want_weights),
                                            lambda: rays.reshape(SB, -1, 8))
            outputs = DotMap(coarse=self._format(res["coarse"], SB, want_weights))
            if Kf > 0:
                outputs.fine = self._format(res["fine"], SB, want_weights)
            return outputs

        # generic model callable: reference control flow, HIP kernels for every renderer stage
        z_coarse = self.sample_coarse(rays, _u=noise["u1"])
        wc, rgbc, depthc = self.composite(model, rays, z_coarse, coarse=True, sb=SB)
        outputs = DotMap(coarse=self._format(dict(rgb=rgbc, depth=depthc, weights=wc), SB, want_weights))
        if Kf > 0:
            n4 = noise.get("n4") if Kfd > 0 else None
            if torch.is_grad_enabled() and ((n4 is not None and depthc.requires_grad) or rays.requires_grad):
                # nerf.py:292: the coarse depth is not detached -- the depth samples carry the fine loss back to it
                from ..autograd import sample_fine_autograd
                z_all = sample_fine_autograd(rays, wc.detach(), depthc, z_coarse, noise.get("u2"), noise.get("u3"), n4,
                                             self.depth_std, self.lindisp)
            else:
                z_all = ops.sample_fine(rays, wc.detach(), depthc, z_coarse, noise.get("u2"), noise.get("u3"), n4,
                                        self.depth_std, self.lindisp)
            wf, rgbf, depthf = self.composite(model, rays, z_all, coarse=False, sb=SB)
            outputs.fine = self._format(dict(rgb=rgbf, depth=depthf, weights=wf), SB, want_weights)
        return outputs

    @staticmethod
    def _fused_needs_grad(model, rays):
        """whether a call on a fused PixelNeRFNet takes the differentiable path"""
        return torch.is_grad_enabled() and (
            model.mlp_coarse.any_requires_grad()
            or (model.mlp_fine is not None and model.mlp_fine.any_requires_grad())
            or (model.encoder.latent.requires_grad and not model.stop_encoder_grad)
            or rays.requires_grad  # rays and cameras: pose estimation / refinement (autograd._RenderFunction)
            or any(torch.is_tensor(t) and t.requires_grad for t in (model.poses, model.focal, model.c)))

    def _rays_launch(self, model, rays, noise, want_weights):
        """the launch of _fused_inference for rays (R,8): the seeded / folded one-call renderer"""
        Kf, Kfd = self._fine_counts()

        def launch(pk_c, pk_f, tables, seed):
            return ops.render_forward(model.scene(), pk_c, pk_f, rays, self.n_coarse, Kf, Kfd, noise, depth_std=self.depth_std,
                                      white_bkgd=self.white_bkgd, lindisp=self.lindisp, want_weights=want_weights, tables=tables,
                                      seed=seed, ray_id_offset=self.ray_id_offset, ray_id_stride=self.ray_id_stride)
        return launch

    def _fused_inference(self, model, Kf, seed, seeded, given_noise, noise, launch, calib_rays):
        """The inference (no autograd) call of a fused PixelNeRFNet, shared by forward (rays) and render_views (cameras):
        `launch(packed_coarse, packed_fine|None, tables|None, seed)` is the one C call, everything around it is here -- packed
        streams before tables, the fp16-range guard around fold and launch, the second pass of stream_scale="auto" (which
        calibrates on `calib_rays()` (SB,B,8), the rays of this call, with this call's draws)."""
        # mlp_fine is None (eval/eval.py:140): pass no fine network, so the fine pass re-uses the coarse pass's
        # outputs at the shared sample positions instead of evaluating them again
        own_fine = Kf > 0 and getattr(model, "mlp_fine", None) is not None
        for _ in range(2):  # (twice only for stream_scale="auto" when the first call on new weights saturated)
            pk_c, pk_f = model.packed(True), (model.packed(False) if own_fine else None)  # before tables(): see PixelNeRFNet.tables
            guarded = model._guard_begin()  # fp16-range guard of the fp32-class kernels: first call on new weights / scene
            try:
                # (a fold that happens now is guarded too -- grid values / lin_z weights: word 0 coarse, word 1 fine)
                tc = model.tables(True, guard_slot=0)
                tf = model.tables(False, guard_slot=1) if (own_fine and tc is not None) else None
                res = launch(pk_c, pk_f, None if tc is None else (tc, tf), seed)
            finally:
                if guarded:
                    model._guard_end()
            if not (guarded and getattr(model, "__dict__", {}).get("_auto_first")):
                break
            # the automatic stream scale calibrates on THIS call's rays and draws (same seed / noise), then renders it again
            keep = self._seed_override
            try:
                if seeded:
                    self._seed_override = seed
                redo = model._auto_resolve(rays=calib_rays(), renderer=_FixedNoise(self, given_noise if not seeded else None, noise))
            finally:
                self._seed_override = keep
            if not redo:
                break
        return res

    # ---- cameras -> images ----
    def render_views(self, model, poses_c2w, W, H, focal, z_near, z_far, c=None, gt_rgb=None, want_u8=False,
                     views_per_call=None, _noise=None, occupancy=None, tighten=False, skip_empty=False, terminate=None,
                     terminate_stages=TERMINATE_STAGES):
        """Every pixel of the target views from their cameras, with the evaluation epilogue on the device: what
        eval/eval.py:247-331 does per object (util.gen_rays, render_par over ray batches, clamp, depth normalisation, PSNR and
        SSIM per view) as one call.  An INFERENCE entry: it runs under torch.no_grad() whatever the caller's mode.
        :param poses_c2w (SB,NVt,4,4) camera-to-world of the target views ((NVt,4,4) when the net encoded one object)
        :param focal scalar or (fx, fy); c (cx, cy) or None = the image centre (util.gen_rays)
        :param gt_rgb (SB,NVt,H,W,3) in [0,1]: adds psnr and ssim
        :param views_per_call k: render k views per object at a time (bounds the workspace); the same bits as one call
        :return DotMap: rgb (SB,NVt,H,W,3) and depth (SB,NVt,H,W) -- the fine pass's (the coarse pass's when using_fine is false),
        unclamped, as `simple_output` returns them; depth_norm = (depth - z_near) / (z_far - z_near); rgb_u8 with want_u8;
        psnr, ssim (SB,NVt) float64 of clamp(rgb, 0, 1) against gt_rgb.  All on the device, no host synchronisation beyond what
        forward has on the first call with new weights.
        Under the same torch.manual_seed the image equals, bit for bit, forward over util.gen_rays of the same cameras; a fused
        PixelNeRFNet renders without a ray array (ops.render_views), anything else goes through util.gen_rays + forward.
        :param occupancy a util.occupancy.OccupancyGrid of the ONE encoded object: the rays are materialised (per group of
        views_per_call views), clipped against the grid, and only those that pass through an occupied cell are rendered -- see
        forward.  The return value then also has `hit` (SB,NVt,H,W) bool, the pixels that were rendered, and `n_hit`, their number
        (a host int); every other pixel holds the background (rgb 0, or 1 with white_bkgd; depth 0), and the epilogue (depth_norm,
        rgb_u8, psnr, ssim) runs on the full image as always.  With rng="philox" the pixels of `hit` have the bits of the call
        without `occupancy` under the same torch.manual_seed.  One host synchronisation per group of views.
        :param tighten with `occupancy`: sample the rendered rays between their first and last occupied cell (see forward)
        :param skip_empty with `occupancy`: run the network only on the samples in occupied cells (see forward); `last_skip_stats`
        sums over the groups of views.  Two more host synchronisations per group of views.
        :param terminate eps in (0, 1): early ray termination of the fine pass (see forward), with or without `occupancy`; without a
        grid the rays are materialised per group of views as well, every pixel is rendered and there is no `hit`.
        `last_terminate_stats` sums over the groups of views.  One host synchronisation per stage and group of views.
        :param terminate_stages the number of stages, or the boundaries (see forward)"""
        accel = _accel.Accel.parse(self, occupancy, tighten, skip_empty, terminate, terminate_stages)
        with torch.no_grad(), torch.profiler.record_function("renderer_render_views"):
            return self._render_views(model, poses_c2w, int(W), int(H), focal, z_near, z_far, c, gt_rgb, want_u8, views_per_call, _noise, accel)

    def _render_views(self, model, poses, W, H, focal, z_near, z_far, c, gt_rgb, want_u8, views_per_call, _noise, accel):
        from .. import util
        self._apply_sched()
        if poses.dim() == 3:
            if int(getattr(model, "num_objs", 1) or 1) != 1:
                raise ValueError("render_views: (NVt,4,4) poses need a net that encoded ONE object; pass (SB,NVt,4,4)")
            poses = poses.unsqueeze(0)
        if poses.dim() != 4 or tuple(poses.shape[2:]) != (4, 4):
            raise ValueError(f"render_views: poses_c2w must be (SB,NVt,4,4), got {tuple(poses.shape)}")
        SB, NVt = poses.shape[:2]
        if views_per_call is not None and int(views_per_call) < 1:
            raise ValueError("render_views: views_per_call must be a positive number of views")
        if torch.is_tensor(focal):
            focal = focal.flatten().tolist()
            focal = focal[0] if len(focal) == 1 else (focal[0], focal[1])
        if torch.is_tensor(c):
            c = c.flatten().tolist()
        flat = poses.reshape(-1, 4, 4).float().contiguous()
        HW = H * W
        R, dev = SB * NVt * HW, flat.device
        Kf, Kfd = self._fine_counts()
        fast = (self._is_fused(model) and flat.is_cuda and model._effective_precision() != "f32"
                and not torch.cuda.is_current_stream_capturing() and not (self.training and self.noise_std > 0.0))
        hit = None
        if accel is not None:
            rgb, depth, hit = _accel.render_views(self, model, poses, W, H, focal, z_near, z_far, c, views_per_call, _noise, accel)
        elif not fast:
            # a generic model callable, a composed-path PixelNeRFNet, the exact fp32 path, a capture in progress: the rays, then forward
            rays = util.gen_rays(flat, W, H, focal, z_near, z_far, c).reshape(SB, -1, 8)
            out = self.forward(model, rays, _noise=_noise)
            last = out.fine if self.using_fine else out.coarse
            rgb, depth = last.rgb, last.depth
        else:
            model._check_supported()
            seeded = _noise is None and self.rng == "philox"
            noise = _noise if (_noise is not None or seeded) else self._draw_noise(R, dev)
            seed = self._next_seed(dev) if seeded else 0  # ONE key per call: the generator advances as for one forward over all rays
            k = NVt if views_per_call is None else min(int(views_per_call), NVt)
            if k == NVt:
                def launch(pk_c, pk_f, tables, seed):
                    return ops.render_views(model.scene(), pk_c, pk_f, flat, W, H, focal, z_near, z_far, self.n_coarse, Kf, Kfd,
                                            noise, c=c, depth_std=self.depth_std, white_bkgd=self.white_bkgd, lindisp=self.lindisp,
                                            tables=tables, seed=seed)
                res = self._fused_inference(model, Kf, seed, seeded, _noise, noise, launch,
                                            lambda: ops.gen_rays(flat, W, H, focal, z_near, z_far, c).reshape(SB, -1, 8))
                last = res["fine"] if Kf > 0 else res["coarse"]
                rgb, depth = last["rgb"], last["depth"]
            else:
                rgb, depth = self._render_view_groups(model, poses, k, W, H, focal, z_near, z_far, c, seed, seeded, _noise, noise)
        ret = DotMap(rgb=rgb.reshape(SB, NVt, H, W, 3), depth=depth.reshape(SB, NVt, H, W))
        if hit is not None:
            ret.hit, ret.n_hit = hit[0].reshape(SB, NVt, H, W), hit[1]
        gt = None
        if gt_rgb is not None:
            if tuple(gt_rgb.shape) != (SB, NVt, H, W, 3) and (SB != 1 or tuple(gt_rgb.shape) != (NVt, H, W, 3)):
                raise ValueError(f"render_views: gt_rgb must be (SB,NVt,H,W,3) = {(SB, NVt, H, W, 3)}, got {tuple(gt_rgb.shape)}")
            gt = gt_rgb.reshape(SB * NVt, HW, 3).float()
        ep = ops.eval_epilogue(rgb.reshape(SB * NVt, HW, 3), depth.reshape(SB * NVt, HW), z_near, z_far, gt_rgb=gt, want_u8=want_u8,
                               image_shape=(H, W) if gt is not None else None)
        ret.depth_norm = ep["depth_norm"].reshape(SB, NVt, H, W)
        if want_u8:
            ret.rgb_u8 = ep["rgb_u8"].reshape(SB, NVt, H, W, 3)
        if gt is not None:
            ret.psnr, ret.ssim = ep["psnr"].reshape(SB, NVt), ep["ssim"].reshape(SB, NVt)
        return ret

    def _render_view_groups(self, model, poses, k, W, H, focal, z_near, z_far, c, seed, seeded, given_noise, noise):
        """render_views, k views per object at a time.  pnr_render_views numbers its rays from 0, so a group goes through its
        rays and the ray-batch entry, placed inside the whole (NVt,H,W) ray set of its object by ray_id_offset / ray_id_stride
        (include/pixelnerf_hip.h, "counter-based random draws"); explicit noise is cut to the group's rows.  Same bits as one call."""
        SB, NVt = poses.shape[:2]
        HW = H * W
        dev, Kf = poses.device, self._fine_counts()[0]
        rgb = torch.empty((SB, NVt * HW, 3), dtype=torch.float32, device=dev)
        depth = torch.empty((SB, NVt * HW), dtype=torch.float32, device=dev)
        keep = (self.ray_id_offset, self.ray_id_stride)
        try:
            for v0 in range(0, NVt, k):
                v1 = min(v0 + k, NVt)
                rays = ops.gen_rays(poses[:, v0:v1].reshape(-1, 4, 4).float().contiguous(), W, H, focal, z_near, z_far, c).reshape(-1, 8)
                part = noise if noise is None else {
                    n: t.reshape(SB, NVt * HW, t.shape[-1])[:, v0 * HW:v1 * HW].reshape(-1, t.shape[-1]) for n, t in noise.items()}
                # (the renderer's own placement fields: a calibration pass of stream_scale="auto" renders through forward)
                self.ray_id_offset, self.ray_id_stride = keep[0] + v0 * HW, NVt * HW
                res = self._fused_inference(model, Kf, seed, seeded, None if given_noise is None else part, part,
                                            self._rays_launch(model, rays, part, False),
                                            lambda: rays.reshape(SB, -1, 8))
                last = res["fine"] if Kf > 0 else res["coarse"]
                rgb[:, v0 * HW:v1 * HW] = last["rgb"].reshape(SB, -1, 3)
                depth[:, v0 * HW:v1 * HW] = last["depth"].reshape(SB, -1)
        finally:
            self.ray_id_offset, self.ray_id_stride = keep
        return rgb, depth

    def _next_seed(self, device):
        """64-bit Philox key of this call, from the ray device's torch generator: (seed, Philox offset) mixed by a
        splitmix64 finaliser, and the generator's offset is advanced as a torch.rand launch would advance it.  Host
        arithmetic only (no launch, no sync); `torch.manual_seed(s)` resets it exactly like it resets the reference's
        draws, successive calls get fresh draws."""
        if self._seed_override is not None:
            return self._seed_override
        gen = torch.cuda.default_generators[device.index if device.index is not None else torch.cuda.current_device()]
        base, off = gen.initial_seed(), gen.get_offset()
        gen.set_offset(off + 4)
        x = (base + 0x9E3779B97F4A7C15 * (off // 4 + 1)) & (2 ** 64 - 1)
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
        return x ^ (x >> 31)

    @staticmethod
    def _format(d, SB, want_weights):
        """nerf.py:305-316."""
        ret = DotMap(rgb=d["rgb"].reshape(SB, -1, 3), depth=d["depth"].reshape(SB, -1))
        if want_weights:
            ret.weights = d["weights"].reshape(SB, -1, d["weights"].shape[-1])
        return ret

    def sched_step(self, steps=1):
        """nerf.py:318-338."""
        if self.sched is None:
            return
        self.iter_idx += steps
        while (self.last_sched.item() < len(self.sched[0])
               and self.iter_idx.item() >= self.sched[0][self.last_sched.item()]):
            self.n_coarse = self.sched[1][self.last_sched.item()]
            self.n_fine = self.sched[2][self.last_sched.item()]
            print("INFO: NeRF sampling resolution changed on schedule ==> c", self.n_coarse, "f", self.n_fine)
            self.last_sched += 1

    @classmethod
    def from_conf(cls, conf, white_bkgd=False, lindisp=False, eval_batch_size=100000):
        """nerf.py:340-352."""
        return cls(conf.get_int("n_coarse", 128), conf.get_int("n_fine", 0),
                   n_fine_depth=conf.get_int("n_fine_depth", 0), noise_std=conf.get_float("noise_std", 0.0),
                   depth_std=conf.get_float("depth_std", 0.01), white_bkgd=conf.get_float("white_bkgd", white_bkgd),
                   lindisp=lindisp, eval_batch_size=conf.get_int("eval_batch_size", eval_batch_size),
                   sched=conf.get_list("sched", None), rng=conf.get_string("rng", "philox"))

    def bind_parallel(self, net, gpus=None, simple_output=False):
        """nerf.py:354-371.  Returns a module callable as `(rays (SB,B,8), want_weights=False)`.
        The reference wraps it in single-process torch.nn.DataParallel(dim=1), which re-broadcasts
        the whole network and feature grid on every call.  Here multi-GPU means one process per
        GPU (torchrun) over RCCL: when torch.distributed is initialised with world_size > 1 and
        more than one GPU is requested, rays are sharded on dim 1 across ranks and the results
        all-gathered (pixelnerf_amd.dist.ShardedRenderWrapper)."""
        wrapped = _RenderWrapper(net, self, simple_output=simple_output)
        if gpus is not None and len(gpus) > 1:
            import torch.distributed as dist
            print("Using multi-GPU", gpus)
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                from ..dist import ShardedRenderWrapper
                return ShardedRenderWrapper(wrapped)
            # single process, several devices -- what `eval/eval.py --gpu_id "0 1"` asks for (nerf.py:367-371)
            return _MultiDeviceRenderWrapper(net, self, simple_output, gpus)
        return wrapped


class _FixedNoise:
    """renderer(model, rays) with the noise tensors of one particular call (calibration of an automatic stream scale on that
    call's own samples; seeded draws repeat through the renderer's seed override instead)"""

    def __init__(self, renderer, given, drawn):
        self.renderer, self.noise = renderer, (given if given is not None else drawn)

    def __call__(self, model, rays):
        return self.renderer.forward(model, rays, _noise=self.noise)


def _check_scale_resolved(net, what):
    """sharded renders equal the single-GPU image bit for bit only if every rank / device runs the same stream scale"""
    if hasattr(net, "stream_scale_resolved") and not net.stream_scale_resolved():
        raise RuntimeError(f"{what}: stream_scale='auto' is unresolved -- every rank / device must render at the SAME scale, and an "
                           "automatic one is chosen from the rays a rank happens to see.  Call net.calibrate_stream_scale(rays=..., "
                           "renderer=...) on the same batch on every rank first (or set an integer net.stream_scale).")


class _MultiDeviceRenderWrapper(torch.nn.Module):
    """Single-process counterpart of the reference's DataParallel(_RenderWrapper, gpus, dim=1) (nerf.py:367-371): rays
    are split on dim 1 across the listed devices, every device renders its slice with its own replica of the
    network (weight VALUES copied when they change; the encoded scene -- feature grid, poses, focal, c -- is copied per
    call, as DataParallel's replicate does), results are concatenated on the first device.  Kernel launches are
    asynchronous, so the slices run concurrently.
    Training works as it does through DataParallel (train/train.py:75): under grad, the autograd inputs of a replica's
    render are the SOURCE network's parameters and `encoder.latent` moved to the replica's device with the
    differentiable `.to()`, so every shard's gradient flows back across devices and accumulates in the source
    parameters' `.grad` -- the caller's optimizer steps the source network, the replicas are refreshed on the next call.
    (Across processes: pixelnerf_amd.dist.ShardedRenderWrapper, one all_reduce per step.)"""

    def __init__(self, net, renderer, simple_output, gpus):
        super().__init__()
        self.net, self.renderer, self.simple_output = net, renderer, simple_output
        self.devices = [torch.device("cuda", int(g)) for g in gpus]
        self._replicas = {}  # device index in the list -> [weights fingerprint, net replica, renderer replica]

    def _weights_key(self):
        src = self.net
        mlps = [m for m in (src.mlp_coarse, src.mlp_fine) if m is not None]
        return tuple(m._fingerprint() for m in mlps) + (src.mlp_fine is None,)

    def _replica(self, i):
        import copy
        fp = self._weights_key()
        hit = self._replicas.get(i)
        if hit is None:
            # the copy carries parameters and buffers only: PixelNeRFNet / ResnetFC / SpatialEncoder drop their per-process caches
            # (scene descriptor, folded tables, packed streams, encoder HIP graphs) in __getstate__; the feature grid is not
            # dragged through the copy either -- the replica gets this call's grid below
            src = self.net
            grid, nhwc = src.encoder.latent, getattr(src.encoder, "_nhwc", None)
            src.encoder.latent = torch.empty(0)
            try:
                rep = copy.deepcopy(src).to(self.devices[i])
            finally:
                src.encoder.latent, src.encoder._nhwc = grid, nhwc
            for p in rep.parameters():
                p.requires_grad_(False)  # gradients go to the SOURCE parameters (see forward)
            hit = [fp, rep, copy.deepcopy(self.renderer).to(self.devices[i])]
            self._replicas[i] = hit
        elif hit[0] != fp:
            # the source weights changed (optimizer step, load_state_dict, ...): refresh the VALUES in place, re-pack lazily
            with torch.no_grad():
                for rp, sp in zip(hit[1].parameters(), self.net.parameters()):
                    rp.copy_(sp, non_blocking=True)
            for m in (hit[1].mlp_coarse, hit[1].mlp_fine):
                if m is not None:
                    m.invalidate_packed()
            hit[0] = fp
        _, rep, rend = hit
        dev = self.devices[i]
        src = self.net
        rep.encoder.latent = src.encoder.latent.detach().to(dev, non_blocking=True)
        rep.encoder.latent_scaling = src.encoder.latent_scaling.to(dev, non_blocking=True)
        rep.poses, rep.focal, rep.c = src.poses.to(dev, non_blocking=True), src.focal.to(dev, non_blocking=True), src.c.to(dev, non_blocking=True)
        rep.image_shape = src.image_shape.to(dev, non_blocking=True)
        rep.num_objs, rep.num_views_per_obj, rep.mlp_fine = src.num_objs, src.num_views_per_obj, (rep.mlp_fine if src.mlp_fine is not None else None)
        rep.precision, rep.fold, rep.stop_encoder_grad = src.precision, src.fold, src.stop_encoder_grad
        rep.stream_scale = src.stream_scale  # (resolved: forward checks) an integer pair, the same on every device
        for k in ("n_coarse", "n_fine", "n_fine_depth", "using_fine", "white_bkgd", "lindisp", "depth_std", "noise_std"):
            setattr(rend, k, getattr(self.renderer, k))
        rend.train(self.renderer.training)
        rep.train(src.training)
        return rep, rend

    def render_views(self, *args, **kwargs):
        raise NotImplementedError("render_views is a single-device entry: render with forward(rays) across several devices, or "
                                  "bind_parallel(net) without a device list")

    def forward(self, rays, want_weights=False):
        from ..autograd import PARAM_NAMES
        from ..dist import shard_bounds
        src = self.net
        _check_scale_resolved(src, "bind_parallel (several devices)")
        lat = src.encoder.latent
        training = torch.is_grad_enabled() and (any(p.requires_grad for p in src.parameters())
                                                or (torch.is_tensor(lat) and lat.requires_grad and not src.stop_encoder_grad))
        B, n = rays.shape[1], len(self.devices)
        seed = self.renderer._next_seed(self.devices[0])  # one key per call, shared by all shards
        outs = []
        for i, dev in enumerate(self.devices):
            lo, hi = shard_bounds(B, i, n)
            if hi == lo:
                continue
            rep, rend = self._replica(i)
            rend.ray_id_offset, rend.ray_id_stride, rend._seed_override = lo, B, seed  # same draws as one device
            if training:
                # autograd inputs of this shard = the source tensors, moved differentiably: the shard's gradients arrive in
                # the source parameters' .grad (summed over the shards by autograd's accumulation)
                mlps = [m for m in (src.mlp_coarse, src.mlp_fine) if m is not None]
                src_params = [p for m in mlps for p in m.ordered_params(PARAM_NAMES)]
                rep.encoder.latent.requires_grad_(lat.requires_grad)  # the replica's renderer takes the differentiable path
                for rp, sp in zip([p for m in (rep.mlp_coarse, rep.mlp_fine) if m is not None for p in m.ordered_params(PARAM_NAMES)], src_params):
                    rp.requires_grad_(sp.requires_grad)
                rep._grad_sync = (lambda latent, params, _d=dev, _sp=src_params:
                                  ((lat.to(_d) if lat.requires_grad and not src.stop_encoder_grad else latent), [p.to(_d) for p in _sp]))
            try:
                with torch.cuda.device(dev):
                    part = _RenderWrapper(rep, rend, self.simple_output)(rays[:, lo:hi].to(dev, non_blocking=True), want_weights=want_weights)
            finally:
                if training:
                    rep._grad_sync = None
            outs.append(part)
        home = self.devices[0]
        if self.simple_output:
            return tuple(torch.cat([o[j].to(home) for o in outs], dim=1) for j in range(2))
        return {k: {kk: torch.cat([o[k][kk].to(home) for o in outs], dim=1) for kk in outs[0][k]} for k in outs[0]}
