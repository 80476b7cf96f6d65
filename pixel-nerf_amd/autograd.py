"""
Differentiable NeRFRenderer.forward (training; BASELINE config 5, train/train.py:199-215).

forward  : the inference kernels, with the network launches replaced by their training form
           (`pnr_eval_ray_samples_train`: same kernel + 16-bit dumps of every linear's input).
backward : HIP kernels only (no library GEMM, no torch matmul) --
             pnr_composite_backward   d(rgb, depth, weights)      -> d(per-point rgb sigma)
             pnr_mlp_backward         fused data-gradient chain   -> per-layer output gradients dY,
                                      d z_lat = sum_b dY_b W_z[b] and d(code) = dY W_in (transposed weight streams)
             pnr_latent_scatter       d(interpolated latent)      -> d(feature grid)
             pnr_weight_grad_batched  dW = dY^T X, db = sum dY    from the 16-bit dumps (MFMA, fp32 acc), one launch
             pnr_lin_out_grad         lin_out's 4 x 512 weight gradient
             pnr_position_backward    d(network inputs)           -> d(sample positions z)
             pnr_pyramid_to_latent_backward  d(feature grid), channel-last as the scatter wrote it -> d(ResNet stage outputs)
At the default precision "f16x3" (fp32-class) the network calls are replaced by their split-operand forms, fused the same way:
             pnr_eval_ray_samples_split_train   the fp32-class inference kernel in its training instantiation (operand images
                                                + relu masks kept, lin_z through the folded fp32 tables)
             pnr_mlp_backward_split             one launch for all transposed products, one batched split-operand
                                                weight-gradient launch -> all 30 gradients, d z_lat, d(code)
(FUSED_SPLIT_TRAINING = False: the same arithmetic as one split-operand GEMM per layer; precision "f32": exact fp32 MFMA.)
Gradients flow to every ResnetFC parameter of both networks and to `encoder.latent` (hence into
the ResNet-34 through PyTorch autograd), including the reference's one position-gradient path:
fine loss -> positions of the n_fine_depth samples (compositing deltas/depth, positional code,
projection + bilinear lookup) -> sort permutation -> clamp -> coarse depth (nerf.py:157-160,292)
-> coarse network.  When the rays or the scene's cameras (net.poses / focal / c) require grad, every pass also asks for the
network-input gradient and pnr_camera_backward turns it into d rays (origins, directions, near / far through the sampling maps)
and d poses / focal / c (importance weights stay detached, nerf.py:288).
"""

import torch

from . import ops

def _param_names():
    names = ["lin_in", "lin_out"] + [f"blocks.{b}.fc_{j}" for b in range(5) for j in (0, 1)] + [f"lin_z.{b}" for b in range(3)]
    return [n + s for n in names for s in (".weight", ".bias")]


PARAM_NAMES = _param_names()

# precision "f16x3": training runs FUSED -- the split-operand inference kernel in its training instantiation (one launch per
# network pass, operand images + relu masks kept), one launch for all transposed products of the backward, one batched
# split-operand weight-gradient launch.  False = the GEMM-per-layer form (~120 split-operand GEMM launches per step: same
# arithmetic class, the A/B twin and the yardstick of the gradient tests)
FUSED_SPLIT_TRAINING = True


def _sigma_noise(rgbs, cfg):
    """nerf.py:225-226 (training only, noise_std > 0): sigmas = sigmas + randn_like(sigmas) * noise_std, drawn from torch's
    generator after each network pass like the reference.  Under a sharding wrapper (cfg["ray_id_stride"] = rays per object of
    the WHOLE batch, cfg["ray_id_offset"] = this shard's first ray) the draw is made for the whole batch and this shard's rows
    are cut out of it: ranks / devices that share a seed then add to every ray exactly the noise a single process would have
    added (identical draws for different rays on different ranks would correlate the shards).
    -> (rgb | noisy sigma, mask of points whose own sigma was positive -- the relu' the compositing backward can no longer
    read off the noisy value) or (rgbs, None)"""
    std = cfg.get("noise_std", 0.0)
    if not std > 0.0:
        return rgbs, None
    live = (rgbs[..., 3] > 0).float()
    noisy = rgbs.clone()
    R, K = rgbs.shape[:2]
    stride, lo = int(cfg.get("ray_id_stride", 0) or 0), int(cfg.get("ray_id_offset", 0) or 0)
    SB = max(int(cfg.get("num_objs", 1) or 1), 1)
    if stride > 0 and R % SB == 0 and lo + R // SB <= stride and R // SB != stride:
        b = R // SB
        n = torch.randn((SB, stride, K), dtype=rgbs.dtype, device=rgbs.device)[:, lo:lo + b].reshape(R, K)
    else:
        n = torch.randn((R, K), dtype=rgbs.dtype, device=rgbs.device)  # one (R,K) draw per pass, reference order
    noisy[..., 3] += n * std
    return noisy, live


class _NoRelease:
    @staticmethod
    def release():
        pass


def _train_eval(net, scene, coarse, rays, z):
    """network forward of one training pass -> (rgbsigma (R,K,4), saved operands).  precision 'f32': the exact, unfused fp32
    chain (validation grade); 'f16x3': the same chain with split-operand (fp32-class) GEMMs on the f16 matrix cores;
    'f16' / 'bf16': the fused kernel's training instantiation (16-bit operand dumps)."""
    ops.saturation_guard_slot(rays.device, 0 if coarse else 1)  # (when the fp16-range guard is armed for this call)
    if net.precision == "f16x3" and FUSED_SPLIT_TRAINING:
        pk = net.packed(coarse, training_pass=True)  # the folded split stream of inference (before tables(): packed() runs the content check)
        return ops.eval_ray_samples_split_train(scene, pk, net.training_tables(coarse, rays, z, scene=scene), rays, z)  # (large grids: only the rows the pass reads)
    if net.precision in ("f32", "f16x3"):
        mlp = net.mlp_coarse if (coarse or net.mlp_fine is None) else net.mlp_fine
        return ops.eval_ray_samples_f32_train(scene, mlp.packed("f32"), rays, z, split=net.precision == "f16x3")
    return ops.eval_ray_samples_train(scene, net.packed(coarse, folded=False, training_pass=True), rays, z)


def _pass_grads(net, mlp, dumps, g_out, scene_NS, want_d_in, want_grads=True):
    """-> (grads, d_zlat, d_in, releasable) of one pass at the network's precision.  want_grads=False (no parameter of this
    network needs a gradient): the data-gradient chain alone, no weight-gradient launch, grads None."""
    if isinstance(dumps, ops.SplitSaved):
        grads, d_zlat, d_in = ops.mlp_backward_split(mlp.packed("f32"), dumps, g_out, want_d_in=want_d_in, want_grads=want_grads)
        return grads, d_zlat, d_in, _NoRelease
    if net.precision in ("f32", "f16x3"):
        grads, d_zlat, d_in = ops.mlp_backward_f32(mlp.packed("f32"), dumps, g_out, want_d_in=want_d_in, want_grads=want_grads)
        return grads, d_zlat, d_in, _NoRelease
    return _mlp_grads(None, mlp.packed_bwd(net.precision), dumps, g_out, scene_NS, want_d_in=want_d_in, want_grads=want_grads)


def _mlp_grads(mlp_state, packed_bwd, fwd, g_out, scene_NS, want_d_in=False, want_grads=True):
    """All parameter gradients of one ResnetFC + d(interpolated latent) [+ d(lin_in operand)] from
    one backward pass.  fwd: ops.TrainDumps of the forward; g_out (P,4) fp32 = dL/d(lin_out output)."""
    # run the 16-bit chain at a power-of-two scale that puts max|g| near 2^6 (exact to undo); the scale is picked
    # on the device (no host sync in the middle of the backward); a non-finite g poisons it with NaN
    sc = ops.grad_scale(g_out)
    bd = ops.mlp_backward(packed_bwd, fwd, g_out, sc[0:1])
    inv_s = sc[1:2]
    if not want_grads:  # data gradients only: the weight-gradient GEMMs are not launched
        return None, bd.d_zlat, (bd.d_in if want_d_in else None), bd

    prec = packed_bwd.precision
    grads = {}
    # weight gradients of the 512x512 linears: HIP MFMA kernel straight from the 16-bit dumps
    # (fp32 accumulation); the kernel's reduction step writes them in feature order
    jobs, names = [], []
    for b in range(5):
        jobs += [(bd.g_fc0[b], fwd.d_a[b], True, True), (bd.g_fc1[b], fwd.d_n[b], True, True)]
        names += [f"blocks.{b}.fc_0", f"blocks.{b}.fc_1"]
    gzs = [bd.g_x0 if b == 0 else bd.g_fc1[b - 1] for b in range(3)]  # dL/d(residual stream entering block b), per view
    for b in range(3):
        jobs.append((gzs[b], fwd.d_z, True, False))  # latent channels are in natural order
        names.append(f"lin_z.{b}")
    jobs.append((bd.g_x0, fwd.d_in, True, False, 64, 42))  # lin_in: operand (rows,64) = code | viewdir | 0-pad
    names.append("lin_in")
    for name, (dW, db) in zip(names, ops.weight_grad_batched(jobs, prec, 1.0, out_scale_dev=inv_s)):  # one launch, 14 linears
        grads[name + ".weight"], grads[name + ".bias"] = dW, db
    grads["lin_out.weight"], grads["lin_out.bias"] = ops.lin_out_grad(g_out, fwd.d_x5, prec)
    # d z_lat = sum_b dY_b W_z[b] and d(code | viewdir) = dY W_in come out of the same fused chain (pnr_mlp_backward:
    # four more transposed-stream GEMMs on gradient images the kernel already holds), fp32, unscaled
    return grads, bd.d_zlat, (bd.d_in if want_d_in else None), bd


class _RenderFunction(torch.autograd.Function):
    """inputs: cfg (python object), rays (R,8), latent (SB*NS,512,Hl,Wl), the scene's cameras (net.poses (SB*NS,3,4)
    world->camera, net.focal, net.c -- the tensors ops.Scene points at), 30 coarse params, 30 fine params (or the coarse
    ones again when mlp_fine is None).
    outputs: rgb_c, depth_c, weights_c[, rgb_f, depth_f, weights_f]."""

    @staticmethod
    def forward(ctx, cfg, rays, latent, poses, focal, c, *params):
        # outputs the loss does not use (depths, weights) arrive in backward as None, not as zero tensors torch would
        # have to fill and the compositing backward would have to read
        ctx.set_materialize_grads(False)
        net, noise = cfg["net"], cfg["noise"]
        Kc, Kf, Kfd = cfg["n_coarse"], cfg["n_fine"], cfg["n_fine_depth"]
        scene = net.scene()
        passes = []
        z_c = ops.sample_coarse(rays, noise["u1"], cfg["lindisp"])
        rgbs_c, dumps_c = _train_eval(net, scene, True, rays, z_c)  # the training instantiation keeps the lin_z GEMMs (operands are dumped)
        rgbs_c, live_c = _sigma_noise(rgbs_c, cfg)
        w_c, rgb_c, depth_c = ops.composite(rays, z_c, rgbs_c, cfg["white_bkgd"], want_weights=True)
        passes.append(dict(z=z_c, rgbs=rgbs_c, dumps=dumps_c, coarse=True, live=live_c))
        outs = [rgb_c, depth_c, w_c]
        if Kf > 0:
            n4 = noise.get("n4") if Kfd > 0 else None
            z_f, ranks = ops.sample_fine(rays, w_c, depth_c, z_c, noise.get("u2"), noise.get("u3"), n4,
                                         cfg["depth_std"], cfg["lindisp"], want_ranks=True)
            rgbs_f, dumps_f = _train_eval(net, scene, False, rays, z_f)
            rgbs_f, live_f = _sigma_noise(rgbs_f, cfg)
            w_f, rgb_f, depth_f = ops.composite(rays, z_f, rgbs_f, cfg["white_bkgd"], want_weights=True)
            # depth_c is an OUTPUT of this Function: keeping the tensor itself in ctx would close the cycle
            # output -> grad_fn -> ctx -> output and pin every dump of the step until the cyclic GC runs
            passes.append(dict(z=z_f, rgbs=rgbs_f, dumps=dumps_f, coarse=False, ranks=ranks, n4=n4, depth_c=depth_c.detach(), live=live_f))
            outs += [rgb_f, depth_f, w_f]
        ctx.cfg, ctx.rays, ctx.scene, ctx.passes = cfg, rays, scene, passes
        ctx.latent_shape = latent.shape
        ctx.cam_shapes = (poses.shape, focal.shape, c.shape)
        ctx.n_params = len(params)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gouts):
        if ctx.passes is None:
            raise RuntimeError("pixelnerf_amd: backward through this render a second time is not supported -- the operand dumps "
                               "of the forward were handed back after the first backward (retain_graph=True keeps the autograd "
                               "graph, not the 12 KB per point and view of saved operands); sum the losses and call backward once")
        cfg, rays, scene = ctx.cfg, ctx.rays, ctx.scene
        net = cfg["net"]
        dev = rays.device
        need_latent = ctx.needs_input_grad[2]
        need_rays, need_poses, need_focal, need_c = ctx.needs_input_grad[1], *ctx.needs_input_grad[3:6]
        need_cam = need_rays or need_poses or need_focal or need_c
        cam = [None, None, None, None]  # d rays, d poses, d focal, d c summed over the passes (fine, then coarse)
        # one zeroed grid gradient PER PASS, summed at the end: pnr_latent_scatter's LDS-slab form leaves at most two atomic adds
        # per element and call (its owner workgroups split the points at most two ways on a full-size batch), and two terms onto
        # zero commute -- the latent gradient, and with it the whole step, is then bit-reproducible.  Accumulating the fine and
        # the coarse pass into ONE buffer made the second call's adds land on non-zero values in either order.
        # Large grids take the scatter's tiled form -- one owner workgroup per element, plain read-add-write -- where accumulation is
        # order-free anyway: ONE buffer for all passes (the same bits as the sum of per-pass buffers: 0 + a is exact), which saves a
        # fill and a sum over a grid-sized tensor (DTU: 3 x 184 MB of traffic per step).
        n_buf = len(ctx.passes)
        if need_latent and n_buf > 1 and all(ops.latent_scatter_single_owner(scene, ps["z"].shape[0], ps["z"].shape[1]) for ps in ctx.passes):
            n_buf = 1
        d_lat = torch.zeros((n_buf, ctx.latent_shape[0], ctx.latent_shape[2], ctx.latent_shape[3], ctx.latent_shape[1]),
                            dtype=torch.float32, device=dev) if need_latent else None
        shared = net.mlp_fine is None  # fine pass ran on the coarse network (models.py:242)
        n_each = len(PARAM_NAMES)
        # per network: does any of its parameters need a gradient (else its weight-gradient launches are skipped)
        need_w = [any(ctx.needs_input_grad[6 + n_each * k:6 + n_each * (k + 1)]) for k in range(ctx.n_params // n_each)]
        gsum = [None, None]
        extra_depth = None  # dL/d(coarse depth) arriving through the fine pass's depth samples
        for i in reversed(range(len(ctx.passes))):  # fine first: it feeds a depth gradient to coarse
            ps = ctx.passes[i]
            d_rgb, d_depth, d_w = gouts[3 * i], gouts[3 * i + 1], gouts[3 * i + 2]
            R, K = ps["z"].shape
            if d_rgb is None:
                d_rgb = torch.zeros((R, 3), device=dev)
            if ps["coarse"] and extra_depth is not None:
                d_depth = extra_depth if d_depth is None else d_depth + extra_depth
            pos = (not ps["coarse"]) and ps.get("ranks") is not None  # depth samples exist
            cb = ops.composite_backward(rays, ps["z"], ps["rgbs"], cfg["white_bkgd"], d_rgb.contiguous().float(),
                                        None if d_depth is None else d_depth.contiguous().float(),
                                        None if d_w is None else d_w.contiguous().float(), want_dz=pos or need_cam,
                                        pre_activation=True,  # also through sigmoid / relu (models.py:260-265)
                                        want_dfar=need_rays)
            d_far = cb[-1] if need_rays else None
            d_pre, dz = (cb[0], cb[1]) if (pos or need_cam) else (cb, None)
            if ps.get("live") is not None:  # sigma noise: the compositing kernel saw relu(sigma) + n; relu' of the network's own sigma
                d_pre[..., 3] *= ps["live"]
            g_out = d_pre.reshape(-1, 4)
            mlp = net.mlp_coarse if (ps["coarse"] or shared) else net.mlp_fine
            slot = 0 if (ps["coarse"] or shared) else 1
            grads, d_zlat, d_in, bd = _pass_grads(net, mlp, ps["dumps"], g_out, scene.NS, pos or need_cam, want_grads=need_w[slot])
            if grads is not None:
                gsum[slot] = grads if gsum[slot] is None else {k: gsum[slot][k] + v for k, v in grads.items()}
            if need_latent:
                ops.latent_scatter(scene, rays, ps["z"], d_zlat, d_lat[i if n_buf > 1 else 0])
            if pos:
                # only the depth samples carry position gradient: compositing part (dz) + network-input part at their
                # sorted positions, through the clamp z = max(min(depth + n*std, far), near)   (nerf.py:157-160,292)
                extra_depth = ops.depth_sample_backward(scene, rays, ps["z"], ps["ranks"], ps["n4"], ps["depth_c"],
                                                        cfg["depth_std"], d_in, d_zlat, dz)
            if need_cam:
                # rays and cameras: every sample's world-space input gradient (pnr_camera_backward), fixed-order sums
                part = ops.camera_backward(scene, rays, ps["z"], d_in, d_zlat, dz_comp=dz, d_far=d_far,
                                           ranks=ps.get("ranks") if pos else None, n4=ps.get("n4") if pos else None,
                                           depth_c=ps.get("depth_c") if pos else None, depth_std=cfg["depth_std"],
                                           lindisp=cfg["lindisp"], want_rays=need_rays, want_poses=need_poses,
                                           want_focal=need_focal, want_c=need_c)
                cam = [p if a is None else (a if p is None else a + p) for a, p in zip(cam, part)]
            # every consumer of this pass's dumps is enqueued: the sets go back to the pool (same-stream reuse)
            bd.release()
            ps["dumps"].release()
            ps["dumps"] = None
        ctx.passes = None  # release the 16-bit operand dumps (~12 KB per point and view) as soon as they are used
        g_lat = None
        if need_latent:
            # the reference's NCHW shape; the channel-last MEMORY stays when the latent's own node reads it that way
            g_lat = (d_lat[0] if d_lat.shape[0] == 1 else d_lat.sum(0)).permute(0, 3, 1, 2)
            if not cfg.get("latent_grad_channel_last", False):
                g_lat = g_lat.contiguous()
        out = [None, cam[0], g_lat]
        out += [None if g is None else g.reshape(shp) for g, shp in zip(cam[1:], ctx.cam_shapes)]
        for slot in range(ctx.n_params // n_each):
            g = gsum[slot]
            out += [None if g is None else g[n] for n in PARAM_NAMES]
        return tuple(out)


class _PointsFunction(torch.autograd.Function):
    """Differentiable PixelNeRFNet.forward on explicit points (src/model/models.py:146-266): (SB*B, 3) points and view
    directions -> (SB*B, 4) = (sigmoid rgb, relu sigma).  The points go through the training kernels as one-sample rays
    (origin = point, direction = viewdir, z = 0).  Gradients: the 30 ResnetFC parameters and the latent grid; the
    points themselves are inputs (no gradient), as on the renderer path."""

    @staticmethod
    def forward(ctx, cfg, xyz, viewdirs, latent, *params):
        ctx.set_materialize_grads(False)
        net, coarse = cfg["net"], cfg["coarse"]
        scene = net.scene()
        R = xyz.shape[0]
        rays = torch.cat([xyz, viewdirs, torch.zeros((R, 2), dtype=torch.float32, device=xyz.device)], dim=1).contiguous()
        z = torch.zeros((R, 1), dtype=torch.float32, device=xyz.device)
        rgbs, dumps = _train_eval(net, scene, coarse, rays, z)
        ctx.cfg, ctx.scene, ctx.rays, ctx.z, ctx.dumps = cfg, scene, rays, z, dumps
        ctx.latent_shape = latent.shape
        out = rgbs.reshape(R, 4)
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return (None,) * (4 + len(PARAM_NAMES))
        if ctx.dumps is None:
            raise RuntimeError("pixelnerf_amd: backward through this forward a second time is not supported (the operand dumps "
                               "were handed back after the first backward); sum the losses and call backward once")
        (out,) = ctx.saved_tensors
        net, coarse = ctx.cfg["net"], ctx.cfg["coarse"]
        g = g.contiguous().float()
        # through the output activations (models.py:260-265): rgb = sigmoid(.), sigma = relu(.)
        d_pre = torch.cat([g[:, :3] * out[:, :3] * (1.0 - out[:, :3]), g[:, 3:] * (out[:, 3:] > 0).float()], dim=1).contiguous()
        mlp = net.mlp_coarse if (coarse or net.mlp_fine is None) else net.mlp_fine
        grads, d_zlat, _, bd = _pass_grads(net, mlp, ctx.dumps, d_pre, ctx.scene.NS, False)
        d_lat = None
        if ctx.needs_input_grad[3]:
            n, c, hl, wl = ctx.latent_shape
            d_lat = torch.zeros((n, hl, wl, c), dtype=torch.float32, device=g.device)
            ops.latent_scatter(ctx.scene, ctx.rays, ctx.z, d_zlat, d_lat)
            d_lat = d_lat.permute(0, 3, 1, 2)
            if not ctx.cfg.get("latent_grad_channel_last", False):
                d_lat = d_lat.contiguous()
        bd.release()
        ctx.dumps.release()
        ctx.dumps = None
        return (None, None, None, d_lat) + tuple(grads[n] for n in PARAM_NAMES)


class _CompositeFunction(torch.autograd.Function):
    """Differentiable alpha compositing around an arbitrary model's per-point (rgb, sigma) (src/render/nerf.py:178-182,
    223-249): forward = pnr_composite, backward = pnr_composite_backward.  Gradients reach the model through `rgbsigma`
    (relu' of the raw sigma is applied inside, as nerf.py:228 applies the relu inside) and the sample positions `z`
    (through the deltas and depth = sum w z) -- the latter is what carries the fine loss back to the coarse depth
    (nerf.py:157-160,292) -- and, when the rays require grad, `far` through the last delta far - z_{K-1}."""

    @staticmethod
    def forward(ctx, rays, z, rgbsigma, white_bkgd):
        ctx.set_materialize_grads(False)
        w, rgb, depth = ops.composite(rays, z, rgbsigma, white_bkgd, want_weights=True)
        ctx.save_for_backward(rays, z, rgbsigma)
        ctx.white_bkgd = bool(white_bkgd)
        return w, rgb, depth

    @staticmethod
    def backward(ctx, d_w, d_rgb, d_depth):
        rays, z, rgbsigma = ctx.saved_tensors
        if d_w is None and d_rgb is None and d_depth is None:
            return None, None, None, None
        if d_rgb is None:
            d_rgb = torch.zeros((rays.shape[0], 3), dtype=torch.float32, device=rays.device)
        want_dz, want_far = ctx.needs_input_grad[1], ctx.needs_input_grad[0]
        res = ops.composite_backward(rays, z, rgbsigma, ctx.white_bkgd, d_rgb.contiguous().float(),
                                     None if d_depth is None else d_depth.contiguous().float(),
                                     None if d_w is None else d_w.contiguous().float(), want_dz=want_dz, pre_activation=False,
                                     want_dfar=want_far)
        res = res if isinstance(res, tuple) else (res,)
        d_rgbs, dz = res[0], (res[1] if want_dz else None)
        d_rays = None
        if want_far:  # the last delta is far - z_{K-1} (nerf.py:181): column 7 of the rays
            d_rays = torch.zeros_like(rays)
            d_rays[:, 7] = res[-1]
        return d_rays, dz, (d_rgbs if ctx.needs_input_grad[2] else None), None


def composite_autograd(rays, z, rgbsigma, white_bkgd):
    """-> weights (R,K), rgb (R,3), depth (R), differentiable with respect to `rgbsigma` (R,K,4) and `z` (R,K)."""
    return _CompositeFunction.apply(rays, z.contiguous().float(), rgbsigma.contiguous().float(), bool(white_bkgd))


class _SampleFineFunction(torch.autograd.Function):
    """The fine pass's merged sample set (nerf.py:285-295: importance samples from the DETACHED coarse weights, depth samples
    around the coarse depth, sort) with the one gradient the reference has there: z_all -> the depth samples at their sorted
    positions -> through the clamp max(min(depth + n * std, far), near) -> coarse depth (the coarse depth is not detached,
    nerf.py:292).  forward = pnr_sample_fine (which also reports the depth samples' sorted positions)."""

    @staticmethod
    def forward(ctx, rays, weights_c, depth_c, z_coarse, u2, u3, n4, depth_std, lindisp):
        z_all, ranks = ops.sample_fine(rays, weights_c, depth_c, z_coarse, u2, u3, n4, depth_std, lindisp, want_ranks=True)
        if ranks is None:  # no depth samples
            ranks = torch.zeros((rays.shape[0], 0), dtype=torch.int32, device=rays.device)
        ctx.save_for_backward(rays, depth_c, n4, ranks, z_all)
        ctx.depth_std, ctx.lindisp = float(depth_std), bool(lindisp)
        ctx.mark_non_differentiable(ranks)
        return z_all, ranks

    @staticmethod
    def backward(ctx, dz_all, _):
        rays, depth_c, n4, ranks, z_all = ctx.saved_tensors
        if dz_all is None:
            return (None,) * 9
        dz_all = dz_all.contiguous().float()
        d_depth = d_rays = None
        has_depth = n4 is not None and ranks.shape[1] > 0
        if has_depth and ctx.needs_input_grad[2]:
            zraw = depth_c.unsqueeze(1) + n4 * ctx.depth_std
            live = (zraw < rays[:, 7:8]) & (zraw > rays[:, 6:7])  # inside the clamp: the gradient passes (nerf.py:160)
            g = torch.gather(dz_all, 1, ranks.long()) * live.to(dz_all.dtype)
            d_depth = g.sum(dim=1)
        if ctx.needs_input_grad[0]:
            # near / far of every sample: the coarse and importance samples through z(s), the depth samples where clamped.
            # (z_coarse gets none here: its own sample_coarse node carries the same samples of the coarse pass)
            d_rays = ops.sample_bounds_backward(rays, z_all, dz_all, ctx.lindisp, ranks=ranks if has_depth else None,
                                                n4=n4 if has_depth else None, depth_c=depth_c.detach() if has_depth else None,
                                                depth_std=ctx.depth_std)
        return d_rays, None, d_depth, None, None, None, None, None, None


class _SampleCoarseFunction(torch.autograd.Function):
    """ops.sample_coarse differentiable with respect to near / far (nerf.py:98-118: z = near (1-s) + far s, lindisp:
    1/z linear in s) -- pnr_sample_bounds_backward."""

    @staticmethod
    def forward(ctx, rays, u1, lindisp):
        z = ops.sample_coarse(rays, u1, lindisp)
        ctx.save_for_backward(rays, z)
        ctx.lindisp = bool(lindisp)
        return z

    @staticmethod
    def backward(ctx, dz):
        rays, z = ctx.saved_tensors
        if dz is None:
            return None, None, None
        return ops.sample_bounds_backward(rays, z, dz.contiguous().float(), ctx.lindisp), None, None


def sample_coarse_autograd(rays, u1, lindisp):
    """ops.sample_coarse, differentiable with respect to the rays' near / far."""
    return _SampleCoarseFunction.apply(rays, u1, bool(lindisp))


def sample_fine_autograd(rays, weights_c, depth_c, z_coarse, u2, u3, n4, depth_std, lindisp):
    """ops.sample_fine, differentiable with respect to the coarse depth (only the n_fine_depth samples depend on it) and the
    rays' near / far."""
    return _SampleFineFunction.apply(rays, weights_c, depth_c, z_coarse, u2, u3, n4, float(depth_std), bool(lindisp))[0]


class _LinearFunction(torch.autograd.Function):
    """y = [residual +] [relu](x) W^T + b as ONE autograd node around pnr_linear / pnr_linear_backward: the building block of
    ResnetFCs of non-shipped shapes (model/resnetfc.py `_forward_composed`; src/model/resnetfc.py:53-62,147,175-183).  Saves x
    (the pre-ReLU input: relu' = [x > 0] is applied inside the data-gradient kernel) -- nothing else."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, relu_in, precision):
        ctx.save_for_backward(x, weight)
        ctx.relu_in, ctx.precision, ctx.has_bias = bool(relu_in), precision, bias is not None
        return ops.linear(x, weight, bias, relu_in=relu_in, residual=residual, precision=precision)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        need_dx, need_dw, need_db, need_res = ctx.needs_input_grad[:4]
        dy = dy.contiguous().float()
        dx = dw = db = None
        if need_dx or need_dw or (need_db and ctx.has_bias):
            dx, dw, db = ops.linear_backward(dy, x, weight, relu_in=ctx.relu_in, need_dx=need_dx, need_dw=need_dw,
                                             need_db=need_db and ctx.has_bias, precision=ctx.precision)
        return dx, (dw if need_dw else None), db, (dy if need_res else None), None, None


def linear_autograd(x, weight, bias=None, relu_in=False, residual=None, precision="f16x3"):
    """Differentiable `ops.linear` (plain kernel call when nothing requires grad)."""
    x = x.float()
    if not x.is_contiguous():
        x = x.contiguous()
    if residual is not None:
        residual = residual.float().contiguous()
    return _LinearFunction.apply(x, weight, bias, residual, bool(relu_in), precision)


class _PyramidFunction(torch.autograd.Function):
    """Encoder output formatting (src/model/encoder.py:150-163) as ONE autograd node: forward = pnr_pyramid_to_latent
    (the reference's NCHW `latent` + the channel-last grid the fused kernels read, not differentiable on its own), backward =
    pnr_pyramid_to_latent_backward.  A gradient that arrives as channel-last memory (what the render backward hands over
    for a latent made here) goes to the kernel as it is; anything else is made contiguous and read as NCHW."""

    @staticmethod
    def forward(ctx, *levels):
        nhwc, nchw = ops.pyramid_to_latent(levels, want_nchw=True)
        ctx.shapes = [tuple(t.shape) for t in levels]
        ctx.mark_non_differentiable(nhwc)
        return nchw, nhwc

    @staticmethod
    def backward(ctx, g, _):
        if g is None:
            return (None,) * len(ctx.shapes)
        g = g.float()
        if g.permute(0, 2, 3, 1).is_contiguous():
            grads = ops.pyramid_to_latent_backward(g.permute(0, 2, 3, 1), ctx.shapes, nchw=False)
        else:
            grads = ops.pyramid_to_latent_backward(g.contiguous(), ctx.shapes, nchw=True)
        return tuple(d if need else None for d, need in zip(grads, ctx.needs_input_grad))


def pyramid_to_latent_autograd(levels):
    """-> (latent (NV,sum C,H0,W0) with the HIP backward behind it, latent_nhwc (NV,H0,W0,sum C) detached)."""
    return _PyramidFunction.apply(*levels)


class _EncoderTrunkFunction(torch.autograd.Function):
    """The encoder's ResNet trunk as ONE autograd node: forward = pnr_encoder_trunk_train_forward (batch norm in batch mode, or
    the frozen form), backward = pnr_encoder_trunk_backward.  Inputs: the image and, per convolution in the order the layers
    run, (weight, gamma, beta); outputs: the pyramid levels.  The running statistics are updated in place by the forward."""

    @staticmethod
    def forward(ctx, cfg, image, *params):
        stats, blocks, n_levels, pool, frozen = cfg
        convs = [(params[3 * i].detach(), params[3 * i + 1].detach(), params[3 * i + 2].detach()) + tuple(stats[i]) for i in range(len(stats))]
        records, keep = ops.encoder_trunk_train_records(convs)
        image = image.detach().contiguous()
        levels, saved = ops.encoder_trunk_train_forward(image, records, blocks, n_levels, pool, frozen)
        ctx.cfg, ctx.records, ctx.keep = (blocks, n_levels, pool, frozen), records, keep
        ctx.save_for_backward(image, saved, *levels)
        return tuple(levels)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *d_levels):
        blocks, n_levels, pool, frozen = ctx.cfg
        image, saved, *levels = ctx.saved_tensors
        d_levels = [g.float().contiguous() for g in d_levels]
        grads, d_image = ops.encoder_trunk_backward(image, ctx.records, blocks, n_levels, pool, frozen, levels, d_levels, saved,
                                                    want_images=ctx.needs_input_grad[1])
        flat = [g if need else None for g, need in zip((g for t in grads for g in t), ctx.needs_input_grad[2:])]
        return (None, d_image, *flat)


def encoder_trunk_autograd(image, params, stats, blocks, n_levels, use_first_pool, frozen):
    """params: [weight, gamma, beta] * n_convs, flat; stats: [(running_mean, running_var, eps, momentum, stride)] per convolution
    -> the list of pyramid levels with the HIP backward behind them"""
    return list(_EncoderTrunkFunction.apply((stats, tuple(blocks), n_levels, use_first_pool, frozen), image, *params))


def _channel_last_grad(net, latent):
    """may the grid gradient of this call stay channel-last memory?  Only for the latent the encoder's own HIP node made."""
    enc = getattr(net, "encoder", None)
    return bool(enc is not None and hasattr(enc, "latent_takes_channel_last_grad") and enc.latent_takes_channel_last_grad(latent))


def _refuse_stream_scale(net):
    """the differentiable paths run the network unscaled: a net that renders at a stream scale cannot be trained through"""
    scales = [int(getattr(m, "stream_scale", 0) or 0) for m in (net.mlp_coarse, net.mlp_fine) if m is not None]
    if any(scales) and net._effective_precision() == "f16x3":
        raise NotImplementedError(f"training through a network with a non-zero stream scale {tuple(scales)} is not implemented: the "
                                  "scale is an inference form of precision 'f16x3' (the operand dumps, the backward chain and the "
                                  "bias gradients would each need their own factor).  Set net.stream_scale = 0 to train, or "
                                  "precision='f32'.")


def points_autograd(net, xyz, viewdirs, coarse):
    """net(xyz, viewdirs) with autograd: (SB,B,3) x 2 -> (SB,B,4)."""
    _refuse_stream_scale(net)
    if xyz.requires_grad or viewdirs.requires_grad:
        raise NotImplementedError("gradients with respect to the query points / view directions are not implemented "
                                  "(the renderer path does not need them: rays are inputs)")
    SB, B, _ = xyz.shape
    latent = net.encoder.latent
    if net.stop_encoder_grad:
        latent = latent.detach()
    mlp = net.mlp_coarse if (coarse or net.mlp_fine is None) else net.mlp_fine
    out = _PointsFunction.apply(dict(net=net, coarse=coarse, latent_grad_channel_last=_channel_last_grad(net, latent)), xyz.reshape(-1, 3).float().contiguous(),
                                viewdirs.reshape(-1, 3).float().contiguous(), latent, *mlp.ordered_params(PARAM_NAMES))
    return out.reshape(SB, B, 4)


def render_autograd(renderer, net, rays, noise, want_weights):
    """Differentiable twin of the one-call inference path; returns {coarse:{...}, fine:{...}} of
    flat tensors like ops.render_forward."""
    _refuse_stream_scale(net)
    Kf = renderer.n_fine if renderer.using_fine else 0
    cfg = dict(net=net, noise=noise, n_coarse=renderer.n_coarse, n_fine=Kf,
               n_fine_depth=min(renderer.n_fine_depth, Kf), depth_std=renderer.depth_std,
               noise_std=float(renderer.noise_std) if renderer.training else 0.0,
               white_bkgd=bool(renderer.white_bkgd), lindisp=bool(renderer.lindisp),
               ray_id_offset=int(getattr(renderer, "ray_id_offset", 0)), ray_id_stride=int(getattr(renderer, "ray_id_stride", 0)),
               num_objs=int(net.num_objs))
    latent = net.encoder.latent
    if net.stop_encoder_grad:
        latent = latent.detach()
    mlps = [net.mlp_coarse] + ([net.mlp_fine] if net.mlp_fine is not None else [])
    params = []
    for m in mlps:
        params += m.ordered_params(PARAM_NAMES)
    sync = getattr(net, "_grad_sync", None)
    cfg["latent_grad_channel_last"] = sync is None and _channel_last_grad(net, latent)  # (the all-reduce buckets take NCHW)
    if sync is not None:  # multi-process training (dist.ShardedRenderWrapper): identity here, ONE gradient all-reduce in backward
        latent, params = sync(latent, params)
    outs = _RenderFunction.apply(cfg, rays, latent, net.poses, net.focal, net.c, *params)
    res = {"coarse": {"rgb": outs[0], "depth": outs[1], "weights": outs[2]}}
    if Kf > 0:
        res["fine"] = {"rgb": outs[3], "depth": outs[4], "weights": outs[5]}
    if not want_weights:
        for v in res.values():
            v.pop("weights")
    return res


def _fp32(g):
    """an upstream gradient as the ops backward entries take it (None stays None)"""
    return None if g is None else g.contiguous().float()


def _checked_source(what, source):
    """source of a baked march: (rays,) or (poses, W, H, focal, c, z_near, z_far), the first a tensor -> the tuple"""
    source = tuple(source)
    if len(source) not in (1, 7) or not isinstance(source[0], torch.Tensor):
        raise ValueError(f"{what}: source must be (rays,) or (poses, W, H, focal, c, z_near, z_far)")
    return source


def _check_obj_poses(what, obj_poses, n):
    if not isinstance(obj_poses, torch.Tensor) or obj_poses.dim() != 3 or tuple(obj_poses.shape[1:]) != (3, 4) \
            or obj_poses.shape[0] != n or not obj_poses.is_floating_point():
        raise ValueError(f"{what}: obj_poses must be a float tensor ({n},3,4) object-to-world")


def _posed(volumes, host):
    """ops.baked_scene_render's objects: every (stored, degree, reso, c1, c2, bits, index) with its pose, a row of `host`, put in"""
    return [ob[:5] + (host[j],) + ob[5:] for j, ob in enumerate(volumes)]


def _scene_source_grads(ctx, rest, obj_poses, d_rays, d_poses):
    """what pnr_baked_scene_backward_* gave -> (d_lead, d_obj) for the inputs that need them: the rays' gradient as it is, the
    cameras' through ops.gen_rays_backward, the object poses' on their own device and dtype"""
    d_lead = d_obj = None
    if ctx.needs_input_grad[0]:
        d_lead = d_rays if not rest else ops.gen_rays_backward(d_rays, rest[0], rest[1], rest[2], rest[3])
    if ctx.needs_input_grad[1]:
        d_obj = d_poses.reshape(-1, 3, 4).to(device=obj_poses.device, dtype=obj_poses.dtype)
    return d_lead, d_obj


class _BakedMarchFunction(torch.autograd.Function):
    """The baked-volume ray march, differentiable with respect to the STORED values (include/pixelnerf_hip.h, "Gradients of the
    baked march").  forward IS the inference entry -- ops.baked_render / baked_sh_render / baked_sparse_render or their _views
    forms, so its outputs are the bytes of util.bake's `render` -- and backward one pnr_baked_backward_* launch into a zeroed
    buffer.  Nothing is saved but the stored tensor: the backward recomputes the samples.  No gradient reaches rays, poses, step
    or the geometry."""

    @staticmethod
    def forward(ctx, stored, source, degree, index, bits, reso, c1, c2, step, white_bkgd, terminate):
        ctx.set_materialize_grads(False)
        out = ops.baked_march(source, stored, degree, reso, c1, c2, step, bits=bits, index=index, white_bkgd=white_bkgd, terminate=terminate)
        ctx.save_for_backward(stored)
        ctx.march = (source, degree, index, bits, reso, c1, c2, step, white_bkgd, terminate)
        return out

    @staticmethod
    def backward(ctx, d_rgb, d_depth, d_alpha):
        (stored,) = ctx.saved_tensors
        source, degree, index, bits, reso, c1, c2, step, white_bkgd, terminate = ctx.march
        if not ctx.needs_input_grad[0] or (d_rgb is None and d_depth is None and d_alpha is None):
            return (None,) * 11
        entry = ops.baked_render_backward if len(source) == 1 else ops.baked_render_views_backward
        d_stored = entry(*source, stored.detach(), degree, reso, c1, c2, step, d_rgb=_fp32(d_rgb), d_depth=_fp32(d_depth),
                         d_alpha=_fp32(d_alpha), bits=bits, index=index, white_bkgd=white_bkgd, terminate=terminate)
        return (d_stored,) + (None,) * 10


def baked_march_autograd(stored, source, degree, reso, c1, c2, step, bits=None, index=None, white_bkgd=False, terminate=0.0):
    """-> (rgb (R,3), depth (R,), alpha (R,)) of the baked march, differentiable with respect to `stored` (fp32: (nx,ny,nz,4) at
    degree None, (nx,ny,nz,B,4) at degree 0, 1, 2, or with `index` the kept rows of a sparse volume).  source: (rays (R,8),) or the
    camera (poses (NV,4,4), W, H, focal, c, z_near, z_far); neither may require grad."""
    if not isinstance(stored, torch.Tensor) or stored.dtype != torch.float32:
        raise TypeError("baked_march_autograd: gradients exist for fp32 volumes only; fit the volume in fp32 and call half() afterwards")
    if isinstance(source[0], torch.Tensor) and source[0].requires_grad:
        raise ValueError(f"baked_march_autograd: no gradient is given with respect to {'rays' if len(source) == 1 else 'poses'}; "
                         "detach them")
    return _BakedMarchFunction.apply(stored, tuple(source), degree, index, bits, tuple(reso), tuple(c1), tuple(c2), float(step),
                                     bool(white_bkgd), float(terminate))


class _BakedMarchRaysFunction(torch.autograd.Function):
    """The baked-volume ray march, differentiable with respect to its RAYS or POSES (include/pixelnerf_hip.h, "Gradients of the baked
    march with respect to the RAYS") and, for an fp32 volume that requires grad, with respect to the stored values too.  forward IS
    the inference entry; backward one pnr_baked_ray_backward_* launch (no atomics: the same bytes on every call), for a camera
    followed by ops.gen_rays_backward, and one pnr_baked_backward_* launch when `stored` asks for its gradient."""

    @staticmethod
    def forward(ctx, stored, lead, rest, degree, index, bits, reso, c1, c2, step, white_bkgd, terminate):
        ctx.set_materialize_grads(False)
        out = ops.baked_march((lead,) + rest, stored, degree, reso, c1, c2, step, bits=bits, index=index, white_bkgd=white_bkgd,
                              terminate=terminate)
        ctx.save_for_backward(stored, lead)
        ctx.march = (rest, degree, index, bits, reso, c1, c2, step, white_bkgd, terminate)
        return out

    @staticmethod
    def backward(ctx, d_rgb, d_depth, d_alpha):
        stored, lead = ctx.saved_tensors
        rest, degree, index, bits, reso, c1, c2, step, white_bkgd, terminate = ctx.march
        if d_rgb is None and d_depth is None and d_alpha is None:
            return (None,) * 12
        source = (lead.detach(),) + rest
        kw = dict(d_rgb=_fp32(d_rgb), d_depth=_fp32(d_depth), d_alpha=_fp32(d_alpha), bits=bits, index=index, white_bkgd=white_bkgd,
                  terminate=terminate)
        d_stored = d_lead = None
        if ctx.needs_input_grad[0]:
            entry = ops.baked_render_backward if not rest else ops.baked_render_views_backward
            d_stored = entry(*source, stored.detach(), degree, reso, c1, c2, step, **kw)
        if ctx.needs_input_grad[1]:
            if not rest:
                d_lead = ops.baked_ray_backward(*source, stored.detach(), degree, reso, c1, c2, step, **kw)
            else:
                W, H, focal, c = rest[:4]
                d_rays = ops.baked_ray_backward_views(*source, stored.detach(), degree, reso, c1, c2, step, **kw)
                d_lead = ops.gen_rays_backward(d_rays, W, H, focal, c)
        return (d_stored, d_lead) + (None,) * 10


def baked_march_rays_autograd(stored, source, degree, reso, c1, c2, step, bits=None, index=None, white_bkgd=False, terminate=0.0):
    """-> (rgb (R,3), depth (R,), alpha (R,)) of the baked march -- the bytes of the inference entry --, differentiable with respect
    to source[0]: the rays (R,8) of source = (rays,), or the poses (NV,4,4) of the camera source = (poses, W, H, focal, c, z_near,
    z_far) (through ops.gen_rays_backward).  `stored` is fp32 or fp16; an fp32 `stored` that requires grad gets its gradient as well
    (pnr_baked_backward_*: fp32 atomics), an fp16 one that requires grad is refused."""
    if not isinstance(stored, torch.Tensor) or stored.dtype not in (torch.float32, torch.float16):
        raise TypeError("baked_march_rays_autograd: stored must be a float32 or float16 tensor")
    if stored.dtype == torch.float16 and stored.requires_grad:
        raise TypeError("baked_march_rays_autograd: gradients exist for fp32 volumes only; fit the volume in fp32 and call half() afterwards")
    source = _checked_source("baked_march_rays_autograd", source)
    return _BakedMarchRaysFunction.apply(stored, source[0], source[1:], degree, index, bits, tuple(reso), tuple(c1), tuple(c2), float(step),
                                         bool(white_bkgd), float(terminate))


class _BakedSceneMarchFunction(torch.autograd.Function):
    """The scene march of several posed baked volumes, differentiable with respect to its world RAYS or camera POSES and to the
    OBJECT poses (include/pixelnerf_hip.h, "Gradients of the scene march").  forward IS the inference entry; backward one
    pnr_baked_scene_backward_* call (no atomics: the same bytes on every call), for a camera followed by ops.gen_rays_backward.
    The stored values are not differentiated."""

    @staticmethod
    def forward(ctx, lead, obj_poses, rest, volumes, step, white_bkgd, terminate):
        ctx.set_materialize_grads(False)
        host = obj_poses.detach().to("cpu", torch.float32)  # the poses are kernel arguments by value: one host read
        objects = _posed(volumes, host)
        entry = ops.baked_scene_render if not rest else ops.baked_scene_render_views
        out = entry(lead, *rest, objects, step, white_bkgd=white_bkgd, terminate=terminate)
        ctx.save_for_backward(lead, obj_poses)
        ctx.march = (rest, objects, step, white_bkgd, terminate)
        return out

    @staticmethod
    def backward(ctx, d_rgb, d_depth, d_alpha):
        lead, obj_poses = ctx.saved_tensors
        rest, objects, step, white_bkgd, terminate = ctx.march
        if (d_rgb is None and d_depth is None and d_alpha is None) or not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return (None,) * 7
        entry = ops.baked_scene_backward if not rest else ops.baked_scene_backward_views
        d_rays, _, d_poses = entry(lead.detach(), *rest, objects, step, d_rgb=_fp32(d_rgb), d_depth=_fp32(d_depth), d_alpha=_fp32(d_alpha),
                                   white_bkgd=white_bkgd, terminate=terminate, want_poses=ctx.needs_input_grad[1])
        return _scene_source_grads(ctx, rest, obj_poses, d_rays, d_poses) + (None,) * 5


def baked_scene_march_autograd(source, objects, obj_poses, step, white_bkgd=False, terminate=0.0):
    """-> (rgb (R,3), depth (R,), alpha (R,)) of the scene march -- the bytes of ops.baked_scene_render / _views --, differentiable
    with respect to source[0] -- the world rays (R,8) of source = (rays,), or the camera poses (NV,4,4) of source = (poses, W, H,
    focal, c, z_near, z_far) (through ops.gen_rays_backward) -- and with respect to obj_poses (N,3,4), the object-to-world poses, on
    any device.  objects: a list of (stored, degree, reso, c1, c2, bits, index) -- ops.baked_scene_render's tuples without the pose.
    The gradient of obj_poses is that of 12 free numbers per object: a caller that parametrises rigid motions (util.bake.moved_poses)
    gets the projection from autograd.  The stored values are not differentiated.
    The object poses are kernel arguments BY VALUE: a differentiable call reads the N x 12 numbers to the host once per forward (a
    synchronisation when they live on the device)."""
    source = _checked_source("baked_scene_march_autograd", source)
    _check_obj_poses("baked_scene_march_autograd", obj_poses, len(objects))
    volumes = tuple(tuple(ob) for ob in objects)
    if any(len(ob) != 7 for ob in volumes):
        raise ValueError("baked_scene_march_autograd: an object must be (stored, degree, reso, c1, c2, bits, index)")
    return _BakedSceneMarchFunction.apply(source[0], obj_poses, source[1:], volumes, float(step), bool(white_bkgd), float(terminate))


class _BakedSceneFitFunction(torch.autograd.Function):
    """The scene march of several posed baked volumes, differentiable with respect to the STORED VALUES of its objects (include/
    pixelnerf_hip.h, "Gradients of the scene march with respect to the STORED VALUES") and, as _BakedSceneMarchFunction, to its world
    rays or camera poses and to the object poses.  forward IS the inference entry; backward one pnr_baked_scene_stored_backward_*
    call when any stored tensor needs its gradient (fp32 atomics: not bit-reproducible) and one pnr_baked_scene_backward_* call when
    the lead or the poses need theirs.  The stored tensors are tensor arguments, one per DISTINCT tensor: `meta` says which of them
    each object marches (slot) -- a volume listed twice is one argument and gets the sum of both listings."""

    @staticmethod
    def forward(ctx, lead, obj_poses, rest, meta, step, white_bkgd, terminate, *stored):
        ctx.set_materialize_grads(False)
        host = obj_poses.detach().to("cpu", torch.float32)  # the poses are kernel arguments by value: one host read
        objects = _posed([(stored[m[0]],) + m[1:] for m in meta], host)
        entry = ops.baked_scene_render if not rest else ops.baked_scene_render_views
        out = entry(lead, *rest, objects, step, white_bkgd=white_bkgd, terminate=terminate)
        ctx.save_for_backward(lead, obj_poses, *stored)
        ctx.march = (rest, meta, host, step, white_bkgd, terminate)
        return out

    @staticmethod
    def backward(ctx, d_rgb, d_depth, d_alpha):
        lead, obj_poses, *stored = ctx.saved_tensors
        rest, meta, host, step, white_bkgd, terminate = ctx.march
        need_stored = ctx.needs_input_grad[7:]
        none = (None,) * (7 + len(stored))
        if (d_rgb is None and d_depth is None and d_alpha is None) or not any(ctx.needs_input_grad):
            return none
        kw = dict(d_rgb=_fp32(d_rgb), d_depth=_fp32(d_depth), d_alpha=_fp32(d_alpha), white_bkgd=white_bkgd, terminate=terminate)
        stored = [s.detach() for s in stored]  # (one tensor object per slot: ops shares a buffer between its listings)
        objects = _posed([(stored[m[0]],) + m[1:] for m in meta], host)
        d_stored = [None] * len(stored)
        if any(need_stored):
            entry = ops.baked_scene_stored_backward if not rest else ops.baked_scene_stored_backward_views
            bufs = entry(lead.detach(), *rest, objects, step, want=[need_stored[m[0]] for m in meta], **kw)
            for m, buf in zip(meta, bufs):
                d_stored[m[0]] = buf
        d_lead = d_obj = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            entry = ops.baked_scene_backward if not rest else ops.baked_scene_backward_views
            d_rays, _, d_poses = entry(lead.detach(), *rest, objects, step, want_poses=ctx.needs_input_grad[1], **kw)
            d_lead, d_obj = _scene_source_grads(ctx, rest, obj_poses, d_rays, d_poses)
        return (d_lead, d_obj) + (None,) * 5 + tuple(d_stored)


def baked_scene_fit_autograd(source, stored, volumes_meta, obj_poses, step, white_bkgd=False, terminate=0.0):
    """-> (rgb (R,3), depth (R,), alpha (R,)) of the scene march -- the bytes of ops.baked_scene_render / _views --, differentiable
    with respect to the STORED VALUES of its objects: stored, a list of one fp32 tensor per object ((nx,ny,nz,4) at degree None,
    (nx,ny,nz,B,4) at degree 0, 1, 2, or with an index the kept rows); a tensor that requires grad gets its gradient
    (pnr_baked_scene_stored_backward_*: fp32 atomics), one that does not is frozen -- it mixes and attenuates and receives nothing.
    The SAME tensor at two positions is one volume listed twice: it gets the sum of both listings' gradients.
    volumes_meta: per object (degree, reso, c1, c2, bits, index) -- baked_scene_march_autograd's tuples without the tensor.
    source and obj_poses: as baked_scene_march_autograd takes them; source[0] and obj_poses may require grad and then get that
    function's gradient (pnr_baked_scene_backward_*)."""
    source = _checked_source("baked_scene_fit_autograd", source)
    stored, volumes_meta = list(stored), [tuple(m) for m in volumes_meta]
    if not stored or len(stored) != len(volumes_meta) or any(len(m) != 6 for m in volumes_meta):
        raise ValueError("baked_scene_fit_autograd: stored and volumes_meta must list the same objects, each meta (degree, reso, c1, c2, "
                         "bits, index)")
    if not all(isinstance(s, torch.Tensor) and s.dtype == torch.float32 for s in stored):
        raise TypeError("baked_scene_fit_autograd: gradients exist for fp32 volumes only; fit the volume in fp32 and call half() afterwards")
    _check_obj_poses("baked_scene_fit_autograd", obj_poses, len(stored))
    unique, slots = [], []
    for s in stored:
        slot = next((k for k, u in enumerate(unique) if u is s), len(unique))
        if slot == len(unique):
            unique.append(s)
        slots.append(slot)
    meta = tuple((slot,) + m for slot, m in zip(slots, volumes_meta))
    return _BakedSceneFitFunction.apply(source[0], obj_poses, source[1:], meta, float(step), bool(white_bkgd), float(terminate), *unique)


class _BakedTvFunction(torch.autograd.Function):
    """The total-variation prior of a baked volume's stored values (include/pixelnerf_hip.h, "Total-variation prior").  forward asks
    pnr_baked_tv for the value alone, backward for the gradient alone with scale = grad_output left on the device: no host read on
    either side.  Nothing is consumed, so a second backward is allowed."""

    @staticmethod
    def forward(ctx, stored, degree, reso, weights, eps, index, ids):
        value32, _ = ops.baked_tv(stored, degree, reso, weights, eps=eps, index=index, ids=ids, want_value=True)
        ctx.save_for_backward(stored)
        ctx.tv = (degree, reso, weights, eps, index, ids)
        return value32

    @staticmethod
    def backward(ctx, g):
        (stored,) = ctx.saved_tensors
        degree, reso, weights, eps, index, ids = ctx.tv
        if not ctx.needs_input_grad[0]:
            return (None,) * 7
        d_stored = torch.zeros_like(stored, memory_format=torch.contiguous_format)
        ops.baked_tv(stored.detach(), degree, reso, weights, eps=eps, index=index, ids=ids, want_value=False, grad_out=d_stored,
                     scale=g.detach().reshape(1).float())
        return (d_stored,) + (None,) * 6


def baked_tv_autograd(stored, degree, reso, weights, eps=1e-8, index=None, ids=None):
    """-> the total variation of `stored` (ops.baked_tv's value32, a 0-dim fp32 tensor), differentiable with respect to `stored`
    (fp32: (nx,ny,nz,4) at degree None, (nx,ny,nz,B,4) at degree 0, 1, 2, or with `index` and `ids` the kept rows of a sparse volume)"""
    if not isinstance(stored, torch.Tensor) or stored.dtype != torch.float32:
        raise TypeError("baked_tv_autograd: gradients exist for fp32 volumes only; fit the volume in fp32 and call half() afterwards")
    return _BakedTvFunction.apply(stored, degree, tuple(reso), tuple(float(w) for w in weights), float(eps), index, ids)
