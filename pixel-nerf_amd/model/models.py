"""
PixelNeRFNet with the reference's constructor, attributes, state_dict and call contract
(src/model/models.py:14-316); its forward is one call into the fused HIP network kernel.

  net = make_model(conf["model"]).to(device)      # same conf keys as the reference
  net.encode(images, poses, focal, c=c)           # ResNet-34 in PyTorch-ROCm (unchanged maths)
  rgbsigma = net(xyz, coarse=True, viewdirs=d)    # (SB,B,3),(SB,B,3) -> (SB,B,4)   [HIP]

State left by encode() (models.py:111-141) is kept in the same attributes (`poses`, `focal`,
`c`, `image_shape`, `num_objs`, `num_views_per_obj`, `encoder.latent`, `encoder.latent_scaling`)
and may be set by hand exactly as with the reference; the device-side scene descriptor is
rebuilt lazily whenever one of them changes.
"""
import os.path as osp
import warnings

import torch

from .. import ops
from ..util import repeat_interleave  # noqa: F401  (re-exported like the reference module)
from .code import PositionalEncoding
from .model_util import make_encoder, make_mlp


class PixelNeRFNet(torch.nn.Module):
    def __init__(self, conf, stop_encoder_grad=False, precision="f16x3", fold=True, stream_scale=0):
        """:param conf PyHocon-like config subtree 'model' (util.Conf or a real ConfigTree)
        :param precision arithmetic of the 512-wide linears:
        'f16x3' (default) -- fp32-CLASS on the f16 matrix cores: every operand a (head, tail) fp16 pair, 3 MFMAs per product, fp32
        accumulation (per-point |rgb| <= 2e-5 against the reference: the reference's own arithmetic class; the benchmark
        headline).  Inference: the fused kernel; training: its training instantiation + a fused backward (gradients <= 1e-3 vs
        the reference's autograd).
        'f16' (opt-in, ~2.7x faster at inference, ~4.5x in training) -- fp16 MFMA operands, fp32 accumulation: PSNR >= 52 dB vs the fp32
        reference; inference and training (gradients <= 3e-2 per tensor).
        'f32' -- the exact, unfused fp32-MFMA validation path (inference and training, ~1/25 of the f16 rate).
        'bf16' -- experiment flag only: 8-bit significands are not enough for surface-like densities (33 dB on the
        adversarial fixtures); not a supported product precision.
        :param fold inference applies lin_z[b] to the encoded grid once per scene (per-texel tables) instead of
        once per sample -- the same function by linearity, 22-28 % fewer FLOPs per sample (ops.fold_latent).
        :param stream_scale precision 'f16x3' inference, for checkpoints whose hidden activations leave the fp16 range (the
        guard's warning): 0 (default, today's behaviour), an integer s in [0, 30] -- both networks carry their hidden stream at
        2**-s --, or "auto" -- the first inference call after the weights or the scene changed waits for the guard's verdict and
        calibrates on its own rays if needed (see `stream_scale` / calibrate_stream_scale below).  Not part of state_dict()."""
        super().__init__()
        self.encoder = make_encoder(conf["encoder"])
        self.use_encoder = conf.get_bool("use_encoder", True)
        self.use_xyz = conf.get_bool("use_xyz", False)
        assert self.use_encoder or self.use_xyz
        self.normalize_z = conf.get_bool("normalize_z", True)
        self.stop_encoder_grad = stop_encoder_grad
        self.use_code = conf.get_bool("use_code", False)
        self.use_code_viewdirs = conf.get_bool("use_code_viewdirs", True)
        self.use_viewdirs = conf.get_bool("use_viewdirs", False)
        self.use_global_encoder = conf.get_bool("use_global_encoder", False)

        d_latent = self.encoder.latent_size if self.use_encoder else 0
        d_in = 3 if self.use_xyz else 1
        if self.use_viewdirs and self.use_code_viewdirs:
            d_in += 3
        if self.use_code and d_in > 0:
            self.code = PositionalEncoding.from_conf(conf["code"], d_in=d_in)
            d_in = self.code.d_out
        if self.use_viewdirs and not self.use_code_viewdirs:
            d_in += 3
        if self.use_global_encoder:
            from .encoder import ImageEncoder
            self.global_encoder = ImageEncoder.from_conf(conf["global_encoder"])
            self.global_latent_size = self.global_encoder.latent_size
            d_latent += self.global_latent_size
        d_out = 4
        self.latent_size = self.encoder.latent_size
        self.mlp_coarse = make_mlp(conf["mlp_coarse"], d_in, d_latent, d_out=d_out)
        self.mlp_fine = make_mlp(conf["mlp_fine"], d_in, d_latent, d_out=d_out, allow_empty=True)
        self.register_buffer("poses", torch.empty(1, 3, 4), persistent=False)
        self.register_buffer("image_shape", torch.empty(2), persistent=False)
        self.d_in, self.d_out, self.d_latent = d_in, d_out, d_latent
        self.register_buffer("focal", torch.empty(1, 2), persistent=False)
        self.register_buffer("c", torch.empty(1, 2), persistent=False)
        self.num_objs = 0
        self.num_views_per_obj = 1
        self.precision = precision
        for m in (self.mlp_coarse, self.mlp_fine):
            if m is not None:  # per-Linear operators of a non-shipped shape: exact fp32 only when the net is 'f32', else fp32-class
                m.composed_precision = "f32" if precision == "f32" else "f16x3"
        self.fold = bool(fold)
        self._scene = None
        self._tables = {}
        self._sparse_tables = {}  # training_tables(): persistent buffers of the row-wise fold
        self._grad_sync = None  # set for the duration of a call by dist.ShardedRenderWrapper (gradient all-reduce across ranks)
        self._stream_auto = None  # None: fixed scales | "pending": "auto", not resolved yet | "resolved": "auto", scales chosen
        self.stream_scale = stream_scale

    # ---- stream scale of precision 'f16x3' (include/pixelnerf_hip.h "stream scale"; ops.pack_mlp).  Stored per network on the
    # ResnetFCs (ResnetFC.stream_scale, part of the key of their packed() cache), never in state_dict().
    def _mlps(self):
        return [m for m in (self.mlp_coarse, self.mlp_fine) if m is not None]

    @property
    def stream_scale(self):
        """"auto" while an automatic scale is unresolved, else (s_coarse, s_fine) -- s_fine repeats s_coarse when mlp_fine is None.
        Settable: 0 | int (both networks) | (s_coarse, s_fine) | "auto"."""
        if self.__dict__.get("_stream_auto") == "pending":
            return "auto"
        sc = int(getattr(self.mlp_coarse, "stream_scale", 0))
        return (sc, sc if self.mlp_fine is None else int(getattr(self.mlp_fine, "stream_scale", 0)))

    @stream_scale.setter
    def stream_scale(self, value):
        if isinstance(value, str):
            if value != "auto":
                raise ValueError(f"stream_scale: expected 0, an integer in [0, {ops.STREAM_SCALE_MAX}], a pair of them or 'auto', got {value!r}")
            pair, auto = (0, 0), "pending"
        elif isinstance(value, (tuple, list)):
            if len(value) != 2:
                raise ValueError("stream_scale: a pair is (s_coarse, s_fine)")
            pair, auto = (ops.check_stream_scale(value[0]), ops.check_stream_scale(value[1])), None
        else:
            pair, auto = (ops.check_stream_scale(value),) * 2, None
        self.mlp_coarse.stream_scale = pair[0]
        if self.mlp_fine is not None:
            self.mlp_fine.stream_scale = pair[1]
        self.__dict__["_stream_auto"] = auto

    def stream_scale_resolved(self):
        """False only for an "auto" that no inference call / calibrate_stream_scale has resolved yet"""
        return self.__dict__.get("_stream_auto") != "pending"

    def calibrate_stream_scale(self, rays=None, xyz=None, viewdirs=None, renderer=None, _restart=True):
        """Choose the stream scale of both networks on a batch of the ENCODED scene: either `rays` (SB,B,8) with the
        `renderer` (NeRFRenderer) they will be rendered with, or points `xyz` + `viewdirs` (SB,B,3).  The batch is rendered
        under the range probe (ops.range_probe_*), every network takes the smallest s that brings the largest of its 11 probed
        maxima to <= 16384 (ops.stream_scale_for), the networks are re-packed and probed again -- downstream of a saturated layer
        a probe under-reports, so the scales only grow from pass to pass.  Stops when a probe at the chosen scales stays at or below
        16384 with finite outputs (the guard's eleven layer bits are implied: it fires at 65488), or after 6 passes with an
        error that prints the maxima.  One host synchronisation per pass; not during stream capture.  -> (s_coarse, s_fine)."""
        import math
        if self._effective_precision() != "f16x3":
            raise ValueError("calibrate_stream_scale: the stream scale belongs to precision 'f16x3' (precision='f32' needs none)")
        self._check_supported()
        if (rays is None) == (xyz is None) or (rays is not None and renderer is None) or (xyz is not None and viewdirs is None):
            raise ValueError("calibrate_stream_scale: pass rays= and renderer=, or xyz= and viewdirs=")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("calibrate_stream_scale synchronises with the host: call it outside stream capture")
        dev = self.encoder.latent.device
        mlps = self._mlps()
        if _restart:
            for m in mlps:
                m.stream_scale = 0
        self.__dict__["_calibrating"] = True
        log = []
        try:
            for _ in range(6):
                ops.range_probe_arm(dev)
                try:
                    with torch.no_grad():
                        if rays is not None:
                            renderer(self, rays)
                        else:
                            self._forward_points(xyz, True, viewdirs)
                            if self.mlp_fine is not None:
                                self._forward_points(xyz, False, viewdirs)
                finally:
                    ops.range_probe_disarm(dev)
                words = ops.range_probe_read(dev)  # the pass's one synchronisation
                self.__dict__["_probe_passes"] = self.__dict__.get("_probe_passes", 0) + 1
                log.append((tuple(m.stream_scale for m in mlps), words[: len(mlps)]))
                settled = True
                for m, w in zip(mlps, words):
                    amax = max(w[:11])
                    if not all(math.isfinite(v) for v in w[:11]):
                        raise RuntimeError(f"calibrate_stream_scale: a probed maximum is not finite -- no stream scale cures that: {w[:11]}")
                    need = ops.stream_scale_for(amax)
                    if need > m.stream_scale:
                        m.stream_scale, settled = need, False
                    elif w[11] != 0.0:
                        settled = False  # a non-finite output at a scale the maxima fit: look again, then give up below
                if settled:
                    self.__dict__["_probe_log"] = log
                    if self.__dict__.get("_stream_auto") == "pending":
                        self.__dict__["_stream_auto"] = "resolved"
                    return self.stream_scale
        finally:
            self.__dict__["_calibrating"] = False
            # the guard rode along: verdicts of the calibration's own (saturated) passes are not findings.  Everything on the
            # stream is done after the probe read, so this wait returns at once.
            ops.saturation_guard_poll(dev, wait=True, owner=id(self))
        raise RuntimeError("calibrate_stream_scale: no scale settled in 6 passes; (scales, probed maxima per network) of every pass: "
                           + "; ".join(f"{sc}: {[[float('%.4g' % v) for v in w] for w in ws]}" for sc, ws in log))

    def __getstate__(self):
        # copies / pickles (copy.deepcopy for EMA or replica nets, torch.save(net)) carry parameters, buffers and encode() state;
        # the device-side scene descriptor (ctypes struct of raw pointers), the folded tables and a sharding wrapper's hook are
        # per-process caches of THIS object and are rebuilt on demand
        d = dict(self.__dict__)
        d["_scene"], d["_tables"], d["_sparse_tables"], d["_grad_sync"] = None, {}, {}, None
        return d

    # ------------------------------------------------------------------ encode (PyTorch-ROCm)
    @staticmethod
    def _per_view_pair(v, what):
        """intrinsics in any of the reference's call forms -- scalar, (2), (n) or (n,2) (models.py:116-141) -- as (n|1, 2)"""
        if v.dim() == 0:
            return v.reshape(1, 1).expand(1, 2).clone()
        if v.dim() == 1:
            return v.reshape(-1, 1).expand(-1, 2).clone()
        if v.dim() == 2 and v.shape[-1] == 2:
            return v.clone()
        raise ValueError(f"{what}: expected a scalar, (n) or (n,2) tensor, got shape {tuple(v.shape)}")

    def encode(self, images, poses, focal, z_bounds=None, c=None):
        """What the reference's encode() leaves behind (src/model/models.py:89-144), same attributes and conventions:
        `encoder.latent` from the source images, `poses` = world -> camera [R^T | -R^T t] of the camera-to-world inputs,
        `image_shape` = (W, H), `focal` with the y component negated, `c` (image centre when not given), object / view counts.
        :param images (NS,3,H,W) or (SB,NS,3,H,W); poses (NS,4,4) / (SB,NS,4,4) camera-to-world;
        focal () | (2) | (NS) | (NS,2); c None | () | (2) | (NS) | (NS,2)."""
        batched = images.dim() == 5
        if batched and (poses.dim() != 4 or poses.shape[1] != images.shape[1]):
            raise ValueError("encode: (SB,NS,...) images need (SB,NS,4,4) poses")
        self.num_objs = images.shape[0]
        self.num_views_per_obj = images.shape[1] if batched else 1
        if batched:
            images, poses = images.flatten(0, 1), poses.reshape(-1, 4, 4)
        self.encoder(images)
        # camera-to-world (R | t)  ->  world-to-camera (R^T | -R^T t)
        r_wc = poses[:, :3, :3].transpose(1, 2)
        self.poses = torch.cat((r_wc, -(r_wc @ poses[:, :3, 3:4])), dim=-1)
        height, width = images.shape[-2:]
        self.image_shape[0], self.image_shape[1] = width, height
        fl = self._per_view_pair(focal, "focal").float()
        fl[..., 1].neg_()  # image y runs down, camera y up (models.py:129-130)
        self.focal = fl
        self.c = (self.image_shape * 0.5).unsqueeze(0) if c is None else self._per_view_pair(c, "c")
        if self.use_global_encoder:
            self.global_encoder(images)  # models.py:143-144

    # ------------------------------------------------------------------ device scene
    def fused_supported(self):
        """True for THE model configuration every shipped experiment resolves to (conf/default.conf + default_mv.conf:
        use_encoder, use_xyz, normalize_z, code{6, 1.5, include_input}, use_viewdirs, use_code_viewdirs=False, latent 512,
        ResnetFC 512 x 5, combine_layer 3, encoder lookups bilinear / border): the fused HIP kernels implement exactly that.  Every other configuration the
        reference's constructor accepts runs the composed forward (`_forward_composed`)."""
        return (self.use_encoder and self.use_xyz and self.normalize_z and self.use_code
                and self.use_viewdirs and not self.use_code_viewdirs and not self.use_global_encoder
                and self.code.num_freqs == 6 and abs(self.code.freq_factor - 1.5) < 1e-12
                and self.code.include_input and self.d_in == 42 and self.d_latent == 512
                # the fused lookup hard-codes grid_sample(bilinear, border, align_corners=True) (encoder.py:100-108)
                and self.encoder.index_interp == "bilinear" and self.encoder.index_padding == "border"
                and self.mlp_coarse.supported() and (self.mlp_fine is None or self.mlp_fine.supported()))

    def _check_supported(self):
        if not self.fused_supported():
            raise NotImplementedError(
                "this entry point is the fused HIP network's: it implements the model configuration every shipped experiment "
                "uses (conf/default.conf + default_mv.conf: use_encoder, use_xyz, normalize_z, "
                "code{6,1.5,include_input}, use_viewdirs, use_code_viewdirs=False, latent 512, ResnetFC 512x5/3); "
                "other configurations run through net(xyz, coarse=, viewdirs=) / NeRFRenderer (composed forward)")

    def _check_trainable(self):
        """the differentiable paths pool the source views with the mean (every shipped config); "max" has inference kernels only"""
        if int(self.num_views_per_obj) > 1 and any(m is not None and m.combine_type != "average" for m in (self.mlp_coarse, self.mlp_fine)):
            raise NotImplementedError("training with combine_type='max' on a multi-view scene is not implemented (the view maximum "
                                      "has inference kernels only; every shipped config pools with 'average')")

    def scene(self):
        """ops.Scene for the current encode() state (rebuilt only when that state changed)."""
        lat = self.encoder.latent
        if not lat.is_cuda:
            raise ops._lib.PixelNerfHipError("PixelNeRFNet must live on a HIP device (no CPU path): net.to('cuda')")
        NS = int(self.num_views_per_obj)
        tens = (lat, self.poses, self.focal, self.c, self.image_shape)
        key = tuple((t.data_ptr(), t._version, tuple(t.shape)) for t in tens) + (NS,)
        if self._scene is None or self._scene[0] != key:
            dev = lat.device
            focal = self.focal.to(dev).float().reshape(-1, 2)
            c = self.c.to(dev).float().reshape(-1, 2)
            SB = lat.shape[0] // NS
            # reference broadcasting (models.py:207-212): 1 row = shared, >1 rows = one per object
            if focal.shape[0] not in (1, SB) or c.shape[0] not in (1, SB):
                raise ValueError("focal / c must have 1 row or one row per object")
            img = self.image_shape.detach().cpu().tolist()
            sc = ops.Scene(self.encoder.latent_nhwc(), self.poses.to(dev).float(), focal, c, img, NS)
            self._scene = (key, sc)
        return self._scene[1]

    def _effective_precision(self):
        return self.precision

    def _folding(self):
        p = self._effective_precision()
        return p == "f16x3" or (self.fold and p != "f32")

    def packed(self, coarse=True, folded=None, training_pass=False):
        """models.py:242: the fine network falls back to the coarse one when mlp_fine is None.
        folded: None = what inference uses (self.fold); the training path asks for the full stream.
        training_pass: the differentiable path is asking (ResnetFC._cached)."""
        mlp = self.mlp_coarse if (coarse or self.mlp_fine is None) else self.mlp_fine
        return mlp.packed(self._effective_precision(), folded=self._folding() if folded is None else folded, training_pass=training_pass)

    def tables(self, coarse=True, guard_slot=None):
        """lin_z folded into the current scene's grid for the coarse / fine network (None when fold is off);
        rebuilt when encode() or the network's parameters change.  guard_slot: the word of an armed fp16-range guard a fold that
        happens now reports into (ops.fold_latent; None = the guard's current slot)."""
        if not self._folding():
            return None
        mlp = self.mlp_coarse if (coarse or self.mlp_fine is None) else self.mlp_fine
        sc = self.scene()
        # (callers fetch packed() BEFORE tables(): packed() runs the cache's content check, and a silent parameter write it
        # detects bumps the fingerprint this key is made of)
        key = (id(sc), mlp._fingerprint(), self._effective_precision())
        slot = "coarse" if mlp is self.mlp_coarse else "fine"
        hit = self._tables.get(slot)
        if hit is None or hit[0] != key:
            self._tables[slot] = (key, ops.fold_latent(sc, dict(mlp.state_dict()), self._effective_precision(), slot=guard_slot), sc)
        return self._tables[slot][1]

    def training_tables(self, coarse, rays, z, scene=None):
        """tables(coarse) for ONE training pass at precision 'f16x3' (autograd._train_eval).  The weights move every step, so a
        training pass always re-folds; on a large grid most texels are not near any ray of the pass, and only the rows it reads are
        folded (ops.fold_latent_rows: the same bits in those rows) into a persistent buffer that is zeroed once.  Rule: grids of
        >= 8192 texels whose pass has fewer (view, point) pairs than the grid has texels -- DTU-sized training; config 5's 4 x 32 x 32
        grids and every inference call keep the dense fold.  PIXELNERF_SPARSE_FOLD=0 / 1 forces the choice (1: any grid >= 8192)."""
        import os
        mlp = self.mlp_coarse if (coarse or self.mlp_fine is None) else self.mlp_fine
        sc = self.scene() if scene is None else scene
        NV, Hl, Wl, _ = sc.latent_nhwc.shape
        M, pairs = NV * Hl * Wl, rays.shape[0] * z.shape[1] * sc.NS
        mode = os.environ.get("PIXELNERF_SPARSE_FOLD", "auto")
        if M < 8192 or mode == "0" or (mode != "1" and pairs > M) or self._effective_precision() != "f16x3":
            return self.tables(coarse)
        slot = "coarse" if mlp is self.mlp_coarse else "fine"
        key = (sc.latent_nhwc.device, NV, Hl, Wl)
        hit = self._sparse_tables.get(slot)
        if hit is None or hit[0] != key:
            hit = (key, torch.zeros((3, NV, Hl, Wl, 512), dtype=torch.float32, device=sc.latent_nhwc.device))
            self._sparse_tables[slot] = hit
        return ops.fold_latent_rows(sc, dict(mlp.state_dict()), rays, z, hit[1])

    # ---- fp16-range guard of the fp32-class precision (ops.saturation_guard_*; include/pixelnerf_hip.h).  "f16x3" represents
    # every operand as an fp16 (head, tail) pair: exact to ~2^-22 up to 65504, SATURATING beyond -- silently outside the
    # reference's fp32 arithmetic for a network whose hidden activations grow that large.  A drop-in for fp32 results must not
    # do that silently, so EVERY inference call runs the guarded instantiation of the kernel by default (round 6; two
    # v_pk_maximum3_f16 per eight operand values, priced in the benchmark line) and every 16th training call does (the weights
    # move slowly; the TRAIN instantiation is the register-tightest one); a verdict arrives asynchronously -- no host
    # synchronisation -- and is reported as a RuntimeWarning by the next call (or by _guard_report(wait=True)).
    # PIXELNERF_SATURATION_GUARD=sample restores the round-5 policy at inference (only the first call after the weights or the
    # encoded scene changed: a later ray batch that alone saturates goes unreported), =always also guards every training call,
    # =off none.
    def _guard_begin(self, training=False):
        """-> True when this call runs guarded (the caller must call _guard_end)"""
        import os
        if torch.cuda.is_current_stream_capturing():
            return False  # (no Event.query() during a capture either: pending verdicts are reported by the next eager call)
        if self.__dict__.get("_calibrating"):  # verdicts of a calibration's own (saturated) passes are not findings
            ops.saturation_guard_poll(self.encoder.latent.device, owner=id(self))
        else:
            self._guard_report()
        if self._effective_precision() != "f16x3":
            return False
        mode = os.environ.get("PIXELNERF_SATURATION_GUARD", "auto")
        if mode == "off":
            return False
        mlps = [m for m in (self.mlp_coarse, self.mlp_fine) if m is not None]
        lat = self.encoder.latent
        key = self._guard_keyval()
        n = self.__dict__.get("_guard_calls", 0)
        self.__dict__["_guard_calls"] = n + 1
        # (training: the weights change every step -- the key would fire every time; every 16th call instead)
        due = (mode == "always" or (training and n % 16 == 0)
               or (not training and (mode != "sample" or key != self.__dict__.get("_guard_key"))))
        if not due:
            return False
        # stream_scale="auto": the first inference call on new weights / a new scene WAITS for its verdict (_auto_resolve)
        self.__dict__["_auto_first"] = (not training and self.__dict__.get("_stream_auto") is not None
                                        and not self.__dict__.get("_calibrating") and key != self.__dict__.get("_guard_key"))
        self.__dict__["_guard_key"] = key
        ops.saturation_guard_arm(lat.device, owner=id(self))
        return True

    def _guard_keyval(self):
        mlps = self._mlps()
        lat = self.encoder.latent
        key = (tuple(m._fingerprint() for m in mlps), lat.data_ptr(), lat._version, tuple(lat.shape))
        scales = tuple(int(getattr(m, "stream_scale", 0)) for m in mlps)
        return key + (scales,) if any(scales) else key

    def _auto_resolve(self, **batch):
        """stream_scale="auto", after the guarded FIRST call on new weights / a new scene (_guard_begin): wait for its verdict
        (the one host synchronisation of the automatic mode); saturated layers -> calibrate on that call's own batch.
        -> True when the caller must render the call again (its first result was out of class and is not to be delivered)."""
        if not self.__dict__.pop("_auto_first", False):
            return False
        dev = self.encoder.latent.device
        got = ops.saturation_guard_poll(dev, wait=True, owner=id(self))
        self.__dict__["_auto_syncs"] = self.__dict__.get("_auto_syncs", 0) + 1
        bits = (0, 0) if got is None else got
        other = (bits[0] & ~0x7FF, bits[1] & ~0x7FF)  # non-finite outputs, the fold's range bit: no scale cures those
        redo = False
        if (bits[0] | bits[1]) & 0x7FF:
            self.calibrate_stream_scale(_restart=False, **batch)
            self.__dict__["_guard_key"] = self._guard_keyval()  # the re-render is this same first call, not a new one
            other = (other[0] & ~0x800, other[1] & ~0x800)  # (a non-finite output of the saturated pass is not a finding)
            redo = True
        self.__dict__["_stream_auto"] = "resolved"
        if other[0] or other[1]:
            self._guard_warn(other)
        return redo

    def _guard_end(self):
        ops.saturation_guard_disarm(self.encoder.latent.device, owner=id(self))

    def _guard_report(self, wait=False):
        lat = self.encoder.latent
        if not (torch.is_tensor(lat) and lat.is_cuda):
            return None
        got = ops.saturation_guard_poll(lat.device, wait=wait, owner=id(self))
        if got is not None and (got[0] or got[1]):
            raised = None
            if self.__dict__.get("_stream_auto") is not None and (got[0] | got[1]) & 0x7FF:
                # automatic mode, a LATER batch saturated on its own: its render is out (it was out of class), the following
                # calls run two more bits down -- and the next one is a "first" call again (the scales are part of the guard key)
                raised = []
                for m, b in zip((self.mlp_coarse, self.mlp_fine), got):
                    if m is not None and b & 0x7FF:
                        m.stream_scale = min(int(m.stream_scale) + 2, ops.STREAM_SCALE_MAX)
                        raised.append(m.stream_scale)
            self._guard_warn(got, raised)
        return got

    def _guard_warn(self, got, raised=None):
        parts = [f"{name} network: {ops.describe_saturation(b)}" for name, b in (("coarse", got[0]), ("fine", got[1])) if b]
        curable = (got[0] | got[1]) & 0x7FF
        if raised is not None:
            tail = (f"  stream_scale='auto': that EARLIER render was out of class; the stream scale was raised to {self.stream_scale} "
                    "for the following calls.")
        elif curable:
            tail = ("  Use make_model(conf, precision='f16x3', stream_scale='auto') (or net.calibrate_stream_scale) to carry the "
                    "hidden stream at a power-of-two scale, or precision='f32' (exact, slower) for this checkpoint.")
        else:
            tail = "  Use make_model(conf, precision='f32') (exact, slower) for this checkpoint."
        warnings.warn("pixelnerf_amd (precision 'f16x3'): hidden activations reached the fp16 range limit of 65504 -- "
                      + "; ".join(parts) + ".  Operand heads saturate there, so these renders are NOT within the fp32-class "
                      "tolerance of the reference." + tail, RuntimeWarning, stacklevel=4)

    def __del__(self):
        try:
            ops.saturation_guard_release(id(self))
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass

    def _wants_grad(self):
        lat = getattr(self.encoder, "latent", None)
        return torch.is_grad_enabled() and (self.mlp_coarse.any_requires_grad()
                                            or (self.mlp_fine is not None and self.mlp_fine.any_requires_grad())
                                            or (torch.is_tensor(lat) and lat.requires_grad))

    # ------------------------------------------------------------------ forward (HIP)
    def forward(self, xyz, coarse=True, viewdirs=None, far=False):
        """Predict (r,g,b,sigma) at world-space points; src/model/models.py:146-266.
        :param xyz (SB,B,3), viewdirs (SB,B,3) -> (SB,B,4)."""
        with torch.profiler.record_function("model_inference"):  # the reference's scope name (models.py:156)
            return self._forward_points(xyz, coarse, viewdirs)

    def _forward_composed(self, xyz, coarse, viewdirs):
        """src/model/models.py:157-265 for the configurations the fused kernels do not cover (normalize_z=False,
        use_code_viewdirs=True -- the reference's DEFAULT --, use_xyz=False, a global encoder, use_encoder=False, other ResnetFC
        shapes): HIP operators for everything with arithmetic weight -- `SpatialEncoder.index` (pnr_grid_index), the positional
        code (pnr_positional_encoding), every nn.Linear (pnr_linear), each with its HIP backward -- and torch ops on HIP tensors
        for the 3x4 camera transforms, the projection and the concatenations in between.  Differentiable end to end."""
        if not xyz.is_cuda:
            raise ops._lib.PixelNerfHipError("PixelNeRFNet must live on a HIP device (no CPU path): net.to('cuda')")
        SB, B, _ = xyz.shape
        NS = int(self.num_views_per_obj)
        rot, trans = self.poses[:, None, :3, :3], self.poses[:, None, :3, 3]       # world -> source camera, (SB*NS, 1, ...)

        def rotate(v):  # (SB*NS, B, 3) -> R v per view, as three broadcast products (a batched 3x3 matmul of B tiny problems is a GEMM launch that costs more than the network's linears)
            return rot[..., 0] * v[..., 0:1] + rot[..., 1] * v[..., 1:2] + rot[..., 2] * v[..., 2:3]
        p_world = repeat_interleave(xyz.float(), NS)                                # (SB*NS, B, 3)
        p_rot = rotate(p_world)
        p_cam = p_rot + trans
        feat = lat = None
        if self.d_in > 0:
            src = p_rot if self.normalize_z else p_cam                              # models.py:169-179
            feat = src.reshape(-1, 3) if self.use_xyz else -src[..., 2].reshape(-1, 1)
            if self.use_code and not self.use_code_viewdirs:
                feat = self.code(feat.contiguous())
            if self.use_viewdirs:
                assert viewdirs is not None  # models.py:186
                d_cam = rotate(repeat_interleave(viewdirs.float().reshape(SB, B, 3), NS))
                feat = torch.cat((feat, d_cam.reshape(-1, 3)), dim=1)
            if self.use_code and self.use_code_viewdirs:
                feat = self.code(feat.contiguous())
        if self.use_encoder:
            fl, pp = self.focal.unsqueeze(1), self.c.unsqueeze(1)                   # (n|1, 1, 2) each
            uv = -p_cam[..., :2] / p_cam[..., 2:3]                                  # models.py:206-212
            uv = uv * repeat_interleave(fl, NS if fl.shape[0] > 1 else 1) + repeat_interleave(pp, NS if pp.shape[0] > 1 else 1)
            lat = self.encoder.index(uv, None, self.image_shape)                    # (SB*NS, L, B)
            if self.stop_encoder_grad:
                lat = lat.detach()
            lat = lat.transpose(1, 2).reshape(-1, self.latent_size)
        if self.use_global_encoder:                                                 # models.py:228-235: in FRONT of the other columns
            g = self.global_encoder.latent
            n_rows = (lat if lat is not None else feat).shape[0]
            assert n_rows % g.shape[0] == 0
            g = repeat_interleave(g, n_rows // g.shape[0])
            lat = g if lat is None else torch.cat((g, lat), dim=-1)
        # mlp_input = (latent columns | code columns): handed over as its two parts (the ResnetFC splits it again at d_latent)
        mlp = self.mlp_coarse if (coarse or self.mlp_fine is None) else self.mlp_fine
        if mlp.d_latent > 0 and (lat is None or lat.shape[-1] != mlp.d_latent):
            raise ValueError("PixelNeRFNet: the network's d_latent does not match the latent columns of this model conf")
        with torch.profiler.record_function("resnetfc_infer"):  # the reference's scope name (resnetfc.py:141)
            out = mlp._forward_composed(None, (NS, B), parts=(lat, feat)).reshape(-1, B, self.d_out)
        return torch.cat((torch.sigmoid(out[..., :3]), torch.relu(out[..., 3:4])), dim=-1).reshape(SB, B, -1)

    def _forward_points(self, xyz, coarse, viewdirs):
        if not self.fused_supported():
            return self._forward_composed(xyz, coarse, viewdirs)
        assert viewdirs is not None  # models.py:186
        SB, B, _ = xyz.shape
        sc = self.scene()
        if SB != sc.SB:
            raise ValueError(f"xyz has {SB} objects but encode() saw {sc.SB}")
        if self._wants_grad():  # differentiable twin: training kernels + HIP backward (parameters and latent grid)
            self._check_trainable()
            if self._effective_precision() not in ("f16", "bf16", "f32", "f16x3"):
                raise NotImplementedError("training precisions: 'f16' / 'bf16' (fused 16-bit kernels), 'f16x3' (fp32-class split-operand "
                                          "GEMMs) or 'f32' (exact fp32 validation path)")
            from .. import autograd
            return autograd.points_autograd(self, xyz, viewdirs.reshape(SB, B, 3), coarse)
        slot = 0 if (coarse or self.mlp_fine is None) else 1
        for _ in range(2):  # (twice only for stream_scale="auto" when the first call on new weights saturated: _auto_resolve)
            pk = self.packed(coarse)
            tab = self.tables(coarse)
            guarded = self._guard_begin()
            try:
                if guarded:
                    ops.saturation_guard_slot(xyz.device, slot)
                if self.__dict__.get("_calibrating"):
                    ops.range_probe_slot(xyz.device, slot)
                out = ops.eval_points(sc, pk, xyz.float(), viewdirs.reshape(SB, B, 3).float(), tables=tab)
            finally:
                if guarded:
                    self._guard_end()
            if not (guarded and self._auto_resolve(xyz=xyz, viewdirs=viewdirs)):
                break
        return out

    # ------------------------------------------------------------------ checkpoints
    # file layout of the reference's trainer (src/model/models.py:268-316): <checkpoints_path>/<name>/pixel_nerf_{latest,init}
    # and one backup generation of each
    @staticmethod
    def _ckpt_file(args, stem):
        return osp.join(args.checkpoints_path, args.name, stem)

    def load_weights(self, args, opt_init=False, strict=True, device=None):
        """Restore from the experiment's checkpoint like the reference: the `init` file seeds a fresh run (or is asked for with
        opt_init), `latest` continues one (args.resume).  A missing file leaves the model as it is, with a warning unless the
        optional init file was the one looked for."""
        if opt_init and not args.resume:
            return
        stem = "pixel_nerf_latest" if (args.resume and not opt_init) else "pixel_nerf_init"
        path = self._ckpt_file(args, stem)
        if osp.exists(path):
            print("Load", path)
            self.load_state_dict(torch.load(path, map_location=self.poses.device if device is None else device), strict=strict)
        elif not opt_init:
            warnings.warn(f"{path} does not exist: nothing loaded, the model keeps its initialisation "
                          "(pretrained weights belong there; pass --resume to continue a run)")
        return self

    def save_weights(self, args, opt_init=False):
        """Write the state_dict to the experiment's `latest` (or `init`) file, keeping the previous one as its backup."""
        from shutil import copyfile
        stem, backup = ("pixel_nerf_init", "pixel_nerf_init_backup") if opt_init else ("pixel_nerf_latest", "pixel_nerf_backup")
        path = self._ckpt_file(args, stem)
        if osp.exists(path):
            copyfile(path, self._ckpt_file(args, backup))
        torch.save(self.state_dict(), path)
        return self
