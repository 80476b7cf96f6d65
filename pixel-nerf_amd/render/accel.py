"""
The acceleration path of inference renders -- what src/render/nerf.py does not have: occupancy-grid culling of rays (`occupancy`,
`tighten`), skipping the network on samples in empty cells (`skip_empty`) and early ray termination of the fine pass (`terminate`,
`terminate_stages`).  The keywords are documented at NeRFRenderer.forward / render_views; here a call that uses any of them is ONE
record (Accel), refused by ONE ordered list (check_call), and rendered by render_culled -- through the renderer's ordinary forward,
or, for skip_empty / terminate, through the stages of the one-call renderer as separate C calls (StagedPass).
"""
from typing import NamedTuple, Optional

import torch

from .. import ops
from ..util.dotmap import DotMap


class Accel(NamedTuple):
    """what a call asked of the acceleration path, field values validated (parse); immutable"""
    occupancy: object           # the util.occupancy.OccupancyGrid of the ONE encoded object, or None (terminate alone)
    tighten: bool
    skip_empty: bool
    eps: Optional[float]        # `terminate`: the transmittance at or below which a ray stops, or None
    bounds: Optional[list]      # the stage boundaries [0, b_1, ..., K] of a terminated fine pass, or None without `terminate`

    @property
    def staged(self):
        """whether the rendered rays go through StagedPass instead of the one-call renderer"""
        return self.skip_empty or self.eps is not None

    @classmethod
    def parse(cls, renderer, occupancy, tighten, skip_empty, terminate, terminate_stages):
        """The five keywords of a call -> its record; None for the dense call (neither `occupancy` nor `terminate`).  ValueError
        for skip_empty without a grid, a bad eps or bad stages; no model and no tensor is looked at.  The stages are cut on the
        sample counts in force for this call, so a pending step of the sampling schedule is applied first.
        terminate_stages an int S: b_s = 2 ((K s) // (2 S)), zeros and duplicates dropped -- for even K no pair (2j, 2j+1) of the
        dense launch straddles a stage; a sequence: the boundaries inside (0, K), as given."""
        if skip_empty and occupancy is None:
            raise ValueError("skip_empty=True needs `occupancy`: the OccupancyGrid that says which cells are empty")
        if occupancy is None and terminate is None:
            return None
        renderer._apply_sched()
        if terminate is None:
            return cls(occupancy, bool(tighten), bool(skip_empty), None, None)
        try:
            eps = float(terminate)
        except (TypeError, ValueError):
            eps = float("nan")
        if not 0.0 < eps < 1.0:
            raise ValueError(f"terminate: eps must lie in (0, 1) -- the transmittance below which a ray stops, e.g. 1e-2 --, got "
                             f"{terminate!r}; pass terminate=None for the dense render")
        K, stages = renderer.n_coarse + renderer._fine_counts()[0], terminate_stages
        if isinstance(stages, (bool, float)) or (torch.is_tensor(stages) and stages.dim() == 0):
            raise ValueError(f"terminate_stages: pass the number of stages as an int >= 1, or the boundaries as a sequence, got {stages!r}")
        if not isinstance(stages, int) and hasattr(stages, "__index__") and not hasattr(stages, "__len__"):
            stages = int(stages)  # (a numpy integer)
        if isinstance(stages, int):
            if stages < 1:
                raise ValueError(f"terminate_stages: needs at least 1 stage (1: no boundary, the dense render), got {stages}")
            inner = []
            for s in range(1, stages):
                b = 2 * ((K * s) // (2 * stages))
                if 0 < b < K and (not inner or b > inner[-1]):
                    inner.append(b)
        else:
            try:
                inner = [int(b) for b in stages]
            except TypeError:
                raise ValueError(f"terminate_stages: pass the number of stages as an int >= 1, or the boundaries as a sequence, got {stages!r}")
            if any(not 0 < b < K for b in inner) or any(b1 <= b0 for b0, b1 in zip(inner, inner[1:])):
                raise ValueError(f"terminate_stages: the boundaries must increase strictly inside (0, K = n_coarse + n_fine = {K}), got "
                                 f"{inner}; or pass the number of stages as an int")
        return cls(occupancy, bool(tighten), bool(skip_empty), eps, [0] + inner + [K])


def check_call(renderer, model, grad_input, SB, accel):
    """The refusals of a call on the acceleration path, each before any device work, in this order:
      1. more (or fewer) than ONE object: SB, or the objects the model encoded (ValueError)
      2. `terminate` on a renderer without a fine pass
      3. the call would take the differentiable path (grad_input: the call's differentiable input -- the rays, or the cameras of
         render_views)
      4. a HIP-graph capture is in progress
      5. `skip_empty` on anything but a fused PixelNeRFNet; then `skip_empty` with noise_std > 0 in train mode
      6. `terminate` on anything but a fused PixelNeRFNet; then `terminate` with noise_std > 0 in train mode
    2 to 6 raise NotImplementedError.  A message opens with the keyword that makes the refusal apply (`occupancy` before
    `terminate` where both do).  Nothing is reset or written: a refused call leaves the renderer, its last_*_stats included, as it
    was."""
    kw = "occupancy" if accel.occupancy is not None else "terminate"
    n_obj = int(getattr(model, "num_objs", 1) or 1)
    if SB != 1 or n_obj != 1:
        raise ValueError(f"{kw}: implemented for ONE object per call -- an OccupancyGrid describes one object, the stages of a "
                         f"terminated pass are counted for one --, this call has {max(SB, n_obj)}; encode one object and pass its rays "
                         "as (1,B,8), object by object")
    if accel.eps is not None and not renderer.using_fine:
        raise NotImplementedError("terminate: early termination applies to the FINE pass (the coarse pass places the fine samples and "
                                  "stays dense); this renderer has none (n_fine = 0) -- call without `terminate`, or render with n_fine > 0")
    fused = renderer._is_fused(model)
    if fused:
        needs_grad = renderer._fused_needs_grad(model, grad_input)
    else:
        params = list(model.parameters()) if hasattr(model, "parameters") else []
        needs_grad = torch.is_grad_enabled() and (grad_input.requires_grad or any(p.requires_grad for p in params))
    if needs_grad:
        raise NotImplementedError(f"{kw}: an inference feature -- this call would take the differentiable path (parameters, feature "
                                  "grid, rays or cameras require grad); call it under torch.no_grad()")
    if grad_input.is_cuda and torch.cuda.is_current_stream_capturing():
        raise NotImplementedError(f"{kw}: the call sizes its launches by counts read on the host (the rays that survive the grid, the "
                                  "samples a stage keeps), which a HIP-graph capture cannot contain; capture the dense call (no "
                                  "`occupancy`, no `terminate`)")
    for name, asked in (("skip_empty", accel.skip_empty), ("terminate", accel.eps is not None)):
        if asked and not fused:
            raise NotImplementedError(f"{name}: runs the staged HIP pass of a fused PixelNeRFNet (the network on a compacted list of "
                                      "samples); a generic model callable and a PixelNeRFNet on the composed (non-fused) path are not "
                                      f"implemented -- call without `{name}`")
        if asked and renderer.training and renderer.noise_std > 0.0:
            raise NotImplementedError(f"{name}: noise_std > 0 in train mode is implemented on the differentiable path only; put the "
                                      f"renderer in eval mode (renderer.eval()) or call without `{name}`")


def begin_call(renderer, model, grad_input, SB, given_noise, accel):
    """check_call; then the call runs: its stats start at zero, and its ONE Philox key is taken exactly where the dense call takes
    its own (the generator advances the same way).  -> the key; None: the draws are torch's (rng="torch", a generic model callable,
    explicit noise)"""
    check_call(renderer, model, grad_input, SB, accel)
    if accel.skip_empty:
        renderer.last_skip_stats = {"coarse": (0, 0), "fine": (0, 0)}
    if accel.eps is not None:
        renderer.last_terminate_stats = {"evaluated": 0, "total": 0, "stopped_rays": 0, "rays": 0, "stages": []}
    seeded = (given_noise is None and renderer._is_fused(model) and renderer.rng == "philox"
              and not (renderer.training and torch.is_grad_enabled()))
    return renderer._next_seed(grad_input.device) if seeded else None


def add_round(renderer, staged):
    """the counts of a StagedPass's last round, ADDED to the renderer's last_skip_stats / last_terminate_stats (render_views sums
    over its groups of views)"""
    if staged.accel.skip_empty:
        renderer.last_skip_stats = {name: (kept + staged.skip[name][0], total + staged.skip[name][1])
                                    for name, (kept, total) in renderer.last_skip_stats.items()}
    if staged.accel.eps is not None:
        acc, new = renderer.last_terminate_stats, staged.term
        stages = [(a[0] + b[0], a[1] + b[1]) for a, b in zip(acc["stages"] or [(0, 0)] * len(new["stages"]), new["stages"])]
        renderer.last_terminate_stats = {k: acc[k] + new[k] for k in ("evaluated", "total", "stopped_rays", "rays")}
        renderer.last_terminate_stats["stages"] = stages


def close_pairs(keep):
    """A keep mask (R,K) uint8 closed over the pairs (2j, 2j+1) of the flat sample order: a kept sample's partner is marked too.
    Needed at precision "f16x3" only.  eval_split_kernel blends the fp32 table rows of an even and of an odd point of the launch
    with differently ordered roundings (its lookup handles two points per step; the compiler contracted w0 v0 + w1 v1 into an FMA
    onto the first product for one of them and onto the second for the other), so there a point's last places depend on the PARITY
    of its place in the launch -- and on nothing else.  A compacted list that carries whole pairs of the dense launch, a kept
    sample's empty partner included, puts every kept sample at a place of its own parity, so it gets the dense launch's bits; the
    partner's output is dropped again after the network (StagedPass.on_mask).  At most one more point per end of a run of kept
    samples."""
    flat = keep.reshape(-1)
    even = flat.numel() - flat.numel() % 2
    p = flat[:even].view(-1, 2)
    return torch.cat([(p | p.flip(1)).reshape(-1), flat[even:]]).view_as(keep)


class StagedPass:
    """The launch of NeRFRenderer._fused_inference for skip_empty and / or early termination on rays (R,8): the stages of the
    one-call renderer as separate C calls, the network on the compacted list of the samples it is needed on (one-sample rays: their
    world point is o + z d rounded as in a dense launch, and eval_kernel / the fp32 path give a point the same bits wherever it
    stands in the launch; "f16x3": close_pairs), zeros elsewhere.
    `skip` {"coarse": (kept, total), "fine": (kept, total)} samples and `term` (the fine pass's last_terminate_stats entry; None
    without `terminate`) are the counts of the LAST ROUND: stream_scale="auto" may call the launch twice."""

    def __init__(self, renderer, model, rays, noise, want_weights, accel):
        self.renderer, self.model, self.rays, self.noise, self.want_weights, self.accel = renderer, model, rays, noise, want_weights, accel
        self.pairs = model._effective_precision() == "f16x3"
        self.skip, self.term = {"coarse": (0, 0), "fine": (0, 0)}, None

    def network(self, packed, tables, slot, rays, z):
        """rgb sigma (N,K,4) of the network `packed` at the samples z (N,K) of rays (N,8); slot: the word of the fp16-range guard
        (when it is armed for this call: 0 coarse, 1 fine)"""
        ops.saturation_guard_slot(rays.device, slot)
        return ops.eval_ray_samples(self.model.scene(), packed, rays, z, tables)

    def on_mask(self, packed, tables, z, slot, keep):
        """the network on the samples of `keep` (R,K) uint8 -> (rgbsigma (R,K,4), zeros elsewhere; the number of kept samples).
        One host synchronisation: the length of the compacted list; an empty list launches no network."""
        run = keep  # the samples the network runs on
        if self.pairs:
            run = close_pairs(keep)
            n_kept = (keep != 0).sum()
        index, rays_c, z_c, M = ops.compact_samples(run, self.rays, z)  # (the host synchronisation)
        part = self.network(packed, tables, slot, rays_c, z_c.unsqueeze(1)).reshape(M, 4) if M > 0 else None
        rgbsigma = ops.expand_rgbsigma(index, part, z.numel()).reshape(*z.shape, 4)
        if self.pairs:
            rgbsigma = torch.where(keep.unsqueeze(-1) != 0, rgbsigma, torch.zeros((), device=z.device))
            M = int(n_kept) if M > 0 else 0  # (already on its way: the stream was drained for the count above)
        return rgbsigma, M

    def terminated(self, packed, tables, z, slot, grid_keep, marks_from=None):
        """A terminated pass, stage by stage: the samples of the stage whose ray has not stopped (pnr_termination_mark on the outputs
        so far, AND the grid's answer, AND the rays that stopped at an earlier boundary -- a stop is final), on_mask, placement of the
        KEPT samples into the (R,K,4) buffer; a stage that keeps nothing launches no network.
        marks_from: finished outputs (R,K,4) to mark on instead of the buffer -- the replay of a call with another `network`
        (tools/gpu_termination_bench.py).  -> (rgbsigma, [(kept, in_stage), ...], the number of rays that stopped)"""
        R, K = z.shape
        eps, bounds = self.accel.eps, self.accel.bounds
        rgbsigma = torch.zeros((R, K, 4), dtype=torch.float32, device=z.device)  # the outputs so far
        live = torch.ones((R, 1), dtype=torch.uint8, device=z.device)             # rays that have not stopped
        counts = []
        for k0, k1 in zip(bounds[:-1], bounds[1:]):
            keep, t_front = ops.termination_mark(self.rays, z, rgbsigma if marks_from is None else marks_from, k0, k1, eps, keep_in=grid_keep)
            live = live & ~(t_front <= eps).unsqueeze(1)
            keep = keep * live
            part, m = self.on_mask(packed, tables, z, slot, keep)
            if m > 0:
                rgbsigma = torch.where(keep.unsqueeze(-1) != 0, part, rgbsigma)
            counts.append((m, R * (k1 - k0)))
        return rgbsigma, counts, R - int(live.sum())

    def one_pass(self, packed, tables, z, slot, name, bounds=None):
        """rgbsigma (R,K,4) of the pass `name` at its samples z, and its counts.  Without a grid and without stages it is the dense
        network call; one stage: nothing can stop."""
        R, N = z.shape[0], z.numel()
        grid_keep = self.accel.occupancy.mark_samples(self.rays, z) if self.accel.skip_empty else None
        stopped = 0
        if bounds is not None and len(bounds) > 2:
            rgbsigma, counts, stopped = self.terminated(packed, tables, z, slot, grid_keep)
        elif grid_keep is None:
            rgbsigma, counts = self.network(packed, tables, slot, self.rays, z), [(N, N)]
        else:
            rgbsigma, M = self.on_mask(packed, tables, z, slot, grid_keep)
            counts = [(M, N)]
        M = sum(m for m, _ in counts)
        if bounds is not None:
            self.term = {"evaluated": M, "total": N, "stopped_rays": stopped, "rays": R, "stages": counts}
        self.skip[name] = (M, N)
        return rgbsigma

    def __call__(self, pk_c, pk_f, tables, seed):
        rend, rays, noise = self.renderer, self.rays, self.noise
        Kf, Kfd = rend._fine_counts()
        tc, tf = tables if tables is not None else (None, None)
        self.skip, self.term = {"coarse": (0, 0), "fine": (0, 0)}, None  # the counts of THIS round
        z_c = ops.sample_coarse(rays, noise["u1"], rend.lindisp)
        w_c, rgb_c, depth_c = ops.composite(rays, z_c, self.one_pass(pk_c, tc, z_c, 0, "coarse"), rend.white_bkgd, True)
        ret = {"coarse": {"rgb": rgb_c, "depth": depth_c}}
        if self.want_weights:
            ret["coarse"]["weights"] = w_c
        if Kf > 0:
            z_f = ops.sample_fine(rays, w_c, depth_c, z_c, noise.get("u2") if Kf > Kfd else None, noise.get("u3") if Kf > Kfd else None,
                                  noise.get("n4") if Kfd > 0 else None, rend.depth_std, rend.lindisp)
            # mlp_fine is None: the coarse network on every kept sample of the fine pass (the one-call renderer merges the
            # coarse pass's outputs instead -- the same bits)
            fine = (pk_f, tf, 1) if pk_f is not None else (pk_c, tc, 0)
            w_f, rgb_f, depth_f = ops.composite(rays, z_f, self.one_pass(fine[0], fine[1], z_f, fine[2], "fine", self.accel.bounds),
                                                rend.white_bkgd, self.want_weights)
            ret["fine"] = {"rgb": rgb_f, "depth": depth_f}
            if self.want_weights:
                ret["fine"]["weights"] = w_f
        return ret


def _background(renderer, R, K, want_weights, dev):
    """what nerf.py:223-249 composites from sigma == 0 on every sample: T = 1 throughout, all weights 0"""
    out = {"rgb": torch.full((R, 3), 1.0 if renderer.white_bkgd else 0.0, dtype=torch.float32, device=dev),
           "depth": torch.zeros((R,), dtype=torch.float32, device=dev)}
    if want_weights:
        out["weights"] = torch.zeros((R, K), dtype=torch.float32, device=dev)
    return out


def render_culled(renderer, model, rays, first_id, want_weights, given_noise, seed, accel):
    """The shared body of forward and render_views on the acceleration path: rays (R,8) of ONE object whose row r has the global
    ray id first_id + r.  Clip against the grid, gather the rays that hit, render them through the ordinary forward with the
    draws of their global ids (seed; given_noise is cut to the hit rows), scatter into outputs pre-filled with the empty-ray
    value.  One host synchronisation: the number of hit rays.  accel.staged: the hit rays go through StagedPass instead (one more
    synchronisation per pass or stage), whose counts are added to the stats.  No grid (terminate alone): every ray is rendered.
    -> ({"coarse": {...}[, "fine": {...}]} flat tensors, hit (R,) bool (None without a grid), the number of rendered rays)"""
    R, dev = rays.shape[0], rays.device
    Kc, (Kf, Kfd) = renderer.n_coarse, renderer._fine_counts()
    if accel.occupancy is None:
        res, hit, idx, sub = None, None, None, rays
        noise = given_noise
        if noise is None and seed is not None:  # the draws of the dense call, as tensors
            noise = ops.philox_noise_ids(torch.arange(R, dtype=torch.int64, device=dev) + int(first_id), Kc, Kf, Kfd, seed)
    else:
        res = {"coarse": _background(renderer, R, Kc, want_weights, dev)}
        if Kf > 0:
            res["fine"] = _background(renderer, R, Kc + Kf, want_weights, dev)
        t_bounds, hit = accel.occupancy.clip_rays(rays)
        hit = hit != 0
        idx = torch.nonzero(hit).flatten()  # ascending; its length reaches the host here
        if idx.numel() == 0:
            return res, hit, 0  # nothing can be hit: no network launch
        sub = rays.index_select(0, idx)
        if accel.tighten:
            sub[:, 6:8] = t_bounds.index_select(0, idx)
        if given_noise is not None:
            noise = {k: v.index_select(0, idx) for k, v in given_noise.items()}
        elif seed is not None:
            noise = ops.philox_noise_ids(idx + int(first_id), Kc, Kf, Kfd, seed)
        else:
            noise = None  # torch draws, for the rendered rays only
    if accel.staged:
        model._check_supported()
        if noise is None:
            noise = renderer._draw_noise(sub.shape[0], dev)
        staged = StagedPass(renderer, model, sub, noise, want_weights, accel)
        out = renderer._fused_inference(model, Kf, 0, False, noise, noise, staged, lambda: sub.unsqueeze(0))
        add_round(renderer, staged)
    else:
        out = renderer._forward(model, sub.unsqueeze(0), want_weights, noise)
    if accel.occupancy is None:
        return out, None, R
    for name, full in res.items():
        part = out[name]
        for key, t in full.items():
            t.index_copy_(0, idx, part[key].reshape(idx.numel(), *t.shape[1:]))
    return res, hit, idx.numel()


def forward(renderer, model, rays, want_weights, given_noise, accel):
    """NeRFRenderer.forward on the acceleration path: rays (1,B,8) -> the DotMap of forward"""
    assert len(rays.shape) == 3
    flat = rays.reshape(-1, 8).float().contiguous()
    seed = begin_call(renderer, model, flat, rays.shape[0], given_noise, accel)
    res = render_culled(renderer, model, flat, renderer.ray_id_offset, want_weights, given_noise, seed, accel)[0]
    outputs = DotMap(coarse=renderer._format(res["coarse"], 1, want_weights))
    if "fine" in res:
        outputs.fine = renderer._format(res["fine"], 1, want_weights)
    return outputs


def render_views(renderer, model, poses, W, H, focal, z_near, z_far, c, views_per_call, given_noise, accel):
    """NeRFRenderer.render_views on the acceleration path: the rays of every group of views (all views without views_per_call)
    through render_culled, under ONE key; ray id = pixel index in the (NVt,H,W) order.
    -> (rgb (R,3), depth (R,), (hit (R,) bool, n_hit) -- None without a grid)"""
    SB, NVt = poses.shape[:2]
    HW = H * W
    flat = poses.reshape(-1, 4, 4).float().contiguous()
    seed = begin_call(renderer, model, flat, SB, given_noise, accel)
    k = NVt if views_per_call is None else min(int(views_per_call), NVt)
    parts, n_hit = [], 0
    for v0 in range(0, NVt, k):
        v1 = min(v0 + k, NVt)
        rays = ops.gen_rays(flat[v0:v1].contiguous(), W, H, focal, z_near, z_far, c).reshape(-1, 8)
        part = given_noise if given_noise is None else {n: t[v0 * HW:v1 * HW] for n, t in given_noise.items()}
        res, hit, n = render_culled(renderer, model, rays, v0 * HW, False, part, seed, accel)
        last = res["fine"] if "fine" in res else res["coarse"]
        parts.append((last["rgb"], last["depth"], hit))
        n_hit += n
    rgb, depth = (torch.cat([p[i] for p in parts]) if len(parts) > 1 else parts[0][i] for i in range(2))
    if accel.occupancy is None:
        return rgb, depth, None
    hit = torch.cat([p[2] for p in parts]) if len(parts) > 1 else parts[0][2]
    return rgb, depth, (hit, n_hit)
