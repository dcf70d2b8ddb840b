"""SDFRenderer: the reference's differentiable sphere tracer API on top of the MI355X kernels.

Same constructor and method signatures as core/sdfrenderer/renderer.py:12-999 of the reference (cited per
method), but nothing is marched in PyTorch: `render` / `render_depth` / `render_normal` are single calls into
libdistr.so (distr.functions), which run the whole march loop, sample selection and backward on the GPU without
host synchronisation.
"""
import os

import numpy as np
import torch

from distr import binding, decoder_pack, functions


def default_arith():
    """Arithmetic of a renderer constructed without `arith=` -- what the reference's drivers do when they run unchanged
    (`python -m distr.launch [--arith f16x3] run_single_shape.py ...` sets DISTR_ARITH for them): 'f32' unless the environment says
    otherwise; an unknown name is an error, not a silent fallback."""
    a = os.environ.get('DISTR_ARITH') or 'f32'
    if a not in binding.ARITH:
        raise ValueError("DISTR_ARITH=%r: must be one of %s" % (a, sorted(binding.ARITH)))
    return a


class SDFRenderer(object):
    # reference: renderer.py:13
    def __init__(self, decoder, intrinsic, img_hw=None, transform_matrix=None, march_step=50, buffer_size=5,
                 ray_marching_ratio=1.5, use_depth2normal=False, max_sample_dist=0.2, radius=1.0, threshold=5e-5,
                 scale_list=[4, 2, 1], march_step_list=[3, 3, -1], use_gpu=True, is_eval=True, arith=None, decoder_grad=False,
                 normal_decoder_grad=False):
        # arith (not in the reference): 'f32' = exact f32 decoder evaluations (default); 'bf16x6' / 'f16x3' = the opt-in split-bf16 /
        # split-f16 march tiles (values within ~1e-6, 1.5x / 2x the step rate, no cluster tiles: for large dense renders; f16x3 only for
        # decoders inside the f16 range, see distr_render_stats.f16_overflows); None = default_arith(); also settable later (self.arith)
        # normal_decoder_grad (not in the reference, where it is always on): render() also back-propagates a loss on raw autograd normals
        # (normalize_normal=False) through the decoder's second path (decode_sdf_gradient with create_graph=True, decoder_utils.py:76-92),
        # the term the backward omits by default (DESIGN.md sections 5 and 8d); also settable later (self.normal_decoder_grad)
        self.normal_decoder_grad = bool(normal_decoder_grad)
        # decoder_grad (not in the reference, where autograd simply does it): render / render_depth / render_depth_batch also back-propagate
        # to the decoder's parameters that require grad -- fine-tuning the prior on image losses (zdepth, depth, min_sdf, normals from depth).
        # The backward then exports its sample list and runs the layer-wise train path on it: ONE HOST SYNC per backward, not capturable
        # into a graph; off (the default) nothing changes. Also settable later (self.decoder_grad)
        self.decoder_grad = bool(decoder_grad)
        if arith is None:
            arith = default_arith()
        if arith not in binding.ARITH:
            raise ValueError("arith must be one of %s" % sorted(binding.ARITH))
        self.arith = arith
        self._warn_small_split(img_hw, intrinsic)
        if not use_gpu:
            raise ValueError('SDFRenderer(use_gpu=False): this build has no CPU path (MI355X kernels only).')
        if torch.cuda.device_count() == 0:
            raise ValueError('No GPU device found.')
        self.decoder = decoder
        dev = next(decoder.parameters()).device
        if dev.type != 'cuda':
            raise ValueError('decoder parameters must live on the GPU')
        self.device = dev.index if dev.index is not None else torch.cuda.current_device()
        if is_eval:
            decoder.eval()
        self.march_step = march_step
        self.buffer_size = buffer_size
        self.max_sample_dist = max_sample_dist
        self.ray_marching_ratio = ray_marching_ratio
        self.use_depth2normal = use_depth2normal
        self.radius = radius
        self.threshold = threshold
        self.scale_list = list(scale_list)
        self.march_step_list = list(march_step_list)
        # pyramids built here (renderer.py:731-753 builds one level per scale_list entry): 2..4 levels, integer scales ending in 1, every
        # scale a 2..8-fold multiple of the next (the `scale` of get_downscaled_grid_map, :604-629), one march_step_list entry per level
        # (the last may be -1). Fractional ratios ([3, 2, 1]) and more levels are not built.
        sl = self.scale_list
        ok = 2 <= len(sl) <= 4 and len(self.march_step_list) == len(sl) and all(float(v) == int(v) and int(v) >= 1 for v in sl) and int(sl[-1]) == 1 \
            and all(int(a) % int(b) == 0 and 2 <= int(a) // int(b) <= 8 for a, b in zip(sl[:-1], sl[1:]))
        if not ok:
            raise NotImplementedError('pyramid scale_list=%r / march_step_list=%r: implemented are 2..4 integer scales ending in 1, each a 2..8-fold '
                                      'multiple of the next, with one step count per level' % (self.scale_list, self.march_step_list))
        if any(int(v) < 1 for v in self.march_step_list[:-1]):
            raise ValueError('march_step_list %r: every coarse level needs at least one step (renderer.py:765: ray_marching_trivial with 0 steps '
                             'concatenates an empty list)' % (self.march_step_list,))
        if isinstance(intrinsic, torch.Tensor):
            intrinsic = intrinsic.detach().cpu().numpy()
        self.intrinsic = intrinsic
        if img_hw is None:
            img_hw = (int(intrinsic[1, 2] * 2), int(intrinsic[0, 2] * 2))   # renderer.py:31-33
        self.img_hw = (int(img_hw[0]), int(img_hw[1]))
        if transform_matrix is None:
            transform_matrix = np.array([[1., 0., 0.], [0., 0., -1.], [0., 1., 0.]])   # renderer.py:45
        self._M_np = np.asarray(transform_matrix, dtype=np.float64)
        if self._M_np.shape != (3, 3):
            raise NotImplementedError('3x4 sim3 transform matrices are not supported (the reference path ends in an '
                                      'un-imported pdb.set_trace(), renderer.py:116)')

        tdev = torch.device('cuda', self.device)
        h, w = self.img_hw
        ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
        self.homo_2d = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(h * w)], 0).to(tdev)    # (3, H*W)
        self.K = torch.from_numpy(np.asarray(intrinsic)).float().to(tdev)
        self.K_inv = torch.from_numpy(np.linalg.inv(np.asarray(intrinsic, dtype=np.float64))).float().to(tdev)
        self.homo_calib = torch.matmul(self.K_inv, self.homo_2d)                                     # (3, H*W)
        self.imgmap_init = torch.zeros(h, w, device=tdev)
        self.transform_matrix = torch.from_numpy(self._M_np).float().to(tdev)
        self.calib_map = self.normalize_vectors(self.homo_calib)[2, :]
        eng = functions.get_engine(decoder, self.device)    # packs + uploads the weights now (fails early on an unsupported decoder)
        functions.check_split_arith(eng, self.arith)
        self.last_stats = None

    @property
    def _engine(self):
        """Packed decoder of this renderer's module; follows later parameter updates of the live module (load_state_dict,
        fine-tuning steps, .to()) like the reference, which evaluates the module itself on every call."""
        return functions.get_engine(self.decoder, self.device)

    def _decoder_weights(self):
        """W0..W8, b0..b8 of the module on its autograd graph (weight norm folded there) when this call back-propagates to the decoder:
        decoder_grad set, grad enabled and a decoder parameter that requires grad; None otherwise."""
        if not self.decoder_grad or not torch.is_grad_enabled() or not any(p.requires_grad for p in self.decoder.parameters()):
            return None
        if self.normal_decoder_grad:
            raise NotImplementedError('decoder_grad together with normal_decoder_grad: the second path of the normals has no weight gradient '
                                      'here (DESIGN.md section 8h)')
        if self.arith != 'f32':
            raise NotImplementedError("decoder_grad: arith='f32' only (this renderer: %r)" % (self.arith,))
        functions._check_eval(self.decoder)
        Ws, bs = decoder_pack.effective_weights_torch(self.decoder)
        return Ws + bs

    # ---- small accessors (renderer.py:61-68)
    def get_intrinsic(self):
        return self.intrinsic

    def get_threshold(self):
        return self.threshold

    def get_img_hw(self):
        return self.img_hw

    # ---- geometry helpers kept for subclasses / callers (renderer.py:84-120, 171-223); plain torch, tiny
    def transform_points(self, points):
        return torch.matmul(self.transform_matrix, points)

    def inv_transform_points(self, points):
        return torch.matmul(self.transform_matrix.t(), points)

    def normalize_vectors(self, x):
        return x / (torch.norm(x, p=2, dim=0, keepdim=True) + 1e-12)

    def get_camera_location(self, R, T):
        return -torch.matmul(R.t(), T)

    def get_camera_rays(self, R, homo=None):
        homo = self.homo_calib if homo is None else homo
        return self.normalize_vectors(torch.matmul(R.t(), homo))

    def generate_point_samples(self, cam_pos, cam_rays, Zdepth, inv_transform=True, has_zdepth_grad=False):
        if not has_zdepth_grad:
            Zdepth = Zdepth.detach()
        if Zdepth.shape[0] == 0:
            raise ValueError('No valid depth.')
        points = cam_rays * Zdepth[None, :] + cam_pos[:, None]
        if inv_transform:
            points = self.inv_transform_points(points)
        return points

    _warned_small_split = False

    def _warn_small_split(self, img_hw, intrinsic):
        """The opt-in arithmetics pay on compute-bound renders only: their tiles have no cluster / sticky tail, so a small image --
        every step a tail step -- gets SLOWER. One warning per process, with the measured numbers."""
        if self.arith == 'f32' or SDFRenderer._warned_small_split:
            return
        try:
            h, w = (int(img_hw[0]), int(img_hw[1])) if img_hw is not None else (int(2 * intrinsic[1][2]), int(2 * intrinsic[0][2]))
        except Exception:           # noqa: BLE001
            return
        if h * w < 200 * 200:
            import warnings
            SDFRenderer._warned_small_split = True
            warnings.warn("SDFRenderer(arith=%r) on a %dx%d image: the split arithmetics are meant for large, dense renders. Measured single-view "
                          "iteration (render + losses + backward + Adam, MI355X, profiles/r03_arith_loops.log): 137x137 f32 9.2 ms, bf16x6 15.5 ms, "
                          "f16x3 13.5 ms; 64x64 f32 5.5 / 14.0 / 12.3 ms. They win from about 256x256 up (512x512: 52.7 / 35.6 / 26.1 ms). "
                          "Use arith='f32' (the default, exact) here." % (self.arith, h, w), RuntimeWarning, stacklevel=3)

    # ---- C-struct for one call
    def _cfg(self, clamp_dist, ray_marching_type, use_transform, want_normal, normalize_normal=True,
             no_grad_depth=False, no_grad_mask=False, no_grad_camera=False):
        msl = list(self.march_step_list)
        march_step = self.march_step
        if ray_marching_type == 'pyramid_recursive' and int(msl[-1]) != -1:
            march_step = int(sum(msl))        # an explicit last entry is the full-resolution step count (renderer.py:724-725 only fills in a -1)
        general = {}
        if [int(v) for v in self.scale_list] not in ([4, 2, 1], [2, 1]):       # (the default pyramids travel as coarse_steps, include/distr.h)
            general = dict(scale_list=[int(v) for v in self.scale_list], march_step_list=[int(v) for v in msl])
        return binding.make_cfg(self.img_hw, self.intrinsic, march_step=march_step, buffer_size=self.buffer_size,
                                ratio=self.ray_marching_ratio, threshold=self.threshold, radius=self.radius,
                                clamp_dist=clamp_dist, marcher=ray_marching_type, coarse_steps=(msl[0], msl[1] if len(msl) == 3 else 0),
                                transform_matrix=self._M_np, use_transform=use_transform,
                                use_depth2normal=self.use_depth2normal, normalize_normal=normalize_normal,
                                want_normal=want_normal, grad_depth=not no_grad_depth, grad_mask=not no_grad_mask,
                                grad_camera=not no_grad_camera, arith=self.arith, **general)

    @staticmethod
    def _check_marcher(ray_marching_type):
        if ray_marching_type == 'trivial_non_parallel':
            ray_marching_type = 'trivial'      # per-ray debug loop of renderer.py:422: same values as 'trivial'
        if ray_marching_type not in binding.MARCHERS:
            raise ValueError('Error! Invalid type of ray marching: {}.'.format(ray_marching_type))
        return ray_marching_type

    # reference: renderer.py:836
    def render_depth(self, latent, R, T, clamp_dist=0.1, sample_index_type='min_abs', profile=False, no_grad=False,
                     no_grad_depth=False, no_grad_mask=False, no_grad_camera=False, ray_marching_type='recursive',
                     use_transform=True):
        if sample_index_type != 'min_abs':
            raise NotImplementedError("only sample_index_type='min_abs' (the one every caller uses) is implemented")
        if no_grad:
            no_grad_depth, no_grad_mask, no_grad_camera = True, True, True
        cfg = self._cfg(clamp_dist, self._check_marcher(ray_marching_type), use_transform, want_normal=False,
                        no_grad_depth=no_grad_depth, no_grad_mask=no_grad_mask, no_grad_camera=no_grad_camera)
        # (decoder_grad: with all three no_grad flags nothing of this render is on the graph, the decoder included)
        weights = None if (no_grad_depth and no_grad_mask and no_grad_camera) else self._decoder_weights()
        zdepth, mask, min_sdf, _, _ = functions.render_call(self._engine, cfg, latent, R, T, weights=weights)
        self._last = (cfg, zdepth)
        if no_grad_depth:
            zdepth = zdepth.detach()
        if no_grad_mask and no_grad_camera:
            min_sdf = min_sdf.detach()
        return zdepth, mask.bool(), min_sdf          # (H*W), (H*W), (H*W)

    def render_depth_batch(self, latent, Rs, Ts, clamp_dist=0.1, no_grad_depth=None, no_grad_mask=None, no_grad_camera=None,
                           ray_marching_type='recursive', use_transform=True):
        """render_depth (renderer.py:836) of B views in ONE launch sequence (no counterpart in the reference, which renders view by
        view: optimize_multi.py:62-81): Rs (B,3,3) / Ts (B,3) or sequences of per-view tensors, latent (1,L) shared by the views or
        (B,L); no_grad_* = None or one bool per view. Returns (Zdepth (B,P), valid_mask (B,P) bool, min_sdf_sample (B,P)); row v is
        bit-identical to render_depth(latent, Rs[v], Ts[v], no_grad_*=...[v]) and so are the gradients."""
        # sequences of per-view tensors may live on different devices / in different float types (a host-resident f64 camera for one
        # view): each is brought to the renderer's device in f32 before stacking, differentiably, like a stand-alone render_depth does
        dev = self.calib_map.device
        to_dev = lambda t: t.to(device=dev, dtype=torch.float32)
        Rs = torch.stack([to_dev(r) for r in Rs]) if not torch.is_tensor(Rs) else Rs
        Ts = torch.stack([to_dev(t) for t in Ts]) if not torch.is_tensor(Ts) else Ts
        B = Rs.shape[0]
        ngd = [bool(x) for x in (no_grad_depth if no_grad_depth is not None else [False] * B)]
        ngm = [bool(x) for x in (no_grad_mask if no_grad_mask is not None else [False] * B)]
        ngc = [bool(x) for x in (no_grad_camera if no_grad_camera is not None else [False] * B)]
        cfg = self._cfg(clamp_dist, self._check_marcher(ray_marching_type), use_transform, want_normal=False,
                        no_grad_depth=all(ngd), no_grad_mask=all(ngm), no_grad_camera=all(ngc))
        flags = [(0 if ngd[v] else binding.VIEW_GRAD_DEPTH) | (0 if ngm[v] else binding.VIEW_GRAD_MASK) |
                 (0 if ngc[v] else binding.VIEW_GRAD_CAMERA) for v in range(B)]
        zdepth, mask, min_sdf, _, _ = functions.render_batch_call(self._engine, cfg, latent, Rs, Ts, flags, weights=self._decoder_weights())
        # (a view rendered with no_grad_depth ignores the upstream gradient of its Zdepth row in the backward kernel: the
        # per-view flag does what the reference's .detach() does, renderer.py:876-877)
        # min_sdf of a view with BOTH no_grad_mask and no_grad_camera is detached by render_depth (renderer.py:388-389 + 863: with the
        # mask gradient off only the camera term of the rays that miss the sphere is left, and no_grad_camera removes that too): per
        # view here, by routing those rows around the autograd node
        dead = [ngm[v] and ngc[v] for v in range(B)]
        if any(dead) and not all(dead):
            keep = torch.tensor([not d for d in dead], device=min_sdf.device).reshape(B, 1)
            min_sdf = torch.where(keep, min_sdf, min_sdf.detach())
        elif all(dead):
            min_sdf = min_sdf.detach()
        return zdepth, mask.bool(), min_sdf

    def render_normal_batch(self, latent, Rs, Ts, Zdepth, valid_mask, clamp_dist=0.1, normalize=True, use_transform=True):
        """render_normal (renderer.py:880) of B views in one launch sequence -> (B,3,P)."""
        dev = self.calib_map.device
        to_dev = lambda t: t.to(device=dev, dtype=torch.float32)      # (per view, like render_depth_batch)
        Rs = torch.stack([to_dev(r) for r in Rs]) if not torch.is_tensor(Rs) else Rs
        Ts = torch.stack([to_dev(t) for t in Ts]) if not torch.is_tensor(Ts) else Ts
        cfg = self._cfg(clamp_dist, 'recursive', use_transform, want_normal=True, normalize_normal=normalize)
        cfg.use_depth2normal = 0
        cfg.save_for_backward = 0          # gradient-free pass: no ReLU-mask store in the workspace (512 B x P x (buffer_size + 1) per view)
        return functions.render_normal_batch_call(self._engine, cfg, latent, Rs, Ts, Zdepth, valid_mask)

    # reference: renderer.py:880
    def render_normal(self, latent, R, T, Zdepth, valid_mask, clamp_dist=0.1, MAX_POINTS=100000, no_grad=False,
                      normalize=True, use_transform=True):
        cfg = self._cfg(clamp_dist, 'recursive', use_transform, want_normal=True, normalize_normal=normalize)
        cfg.use_depth2normal = 0
        cfg.save_for_backward = 0          # gradient-free pass: no ReLU-mask store in the workspace
        return functions.render_normal_call(self._engine, cfg, latent, R, T, Zdepth, valid_mask)   # (3, H*W)

    # reference: renderer.py:943
    def render(self, latent, R, T, clamp_dist=0.1, sample_index_type='min_abs', profile=False, no_grad=False,
               no_grad_depth=False, no_grad_normal=False, no_grad_mask=False, no_grad_camera=False,
               normalize_normal=True, use_transform=True, ray_marching_type='pyramid_recursive',
               num_forward_sampling=0):
        if sample_index_type != 'min_abs':
            raise NotImplementedError("only sample_index_type='min_abs' is implemented (the other four crash inside the reference "
                                      "itself, oracle/probe_reference_dead_paths.py)")
        if no_grad:
            no_grad_depth, no_grad_normal, no_grad_mask, no_grad_camera = True, True, True, True
        h, w = self.img_hw
        cfg = self._cfg(clamp_dist, self._check_marcher(ray_marching_type), use_transform, want_normal=True,
                        normalize_normal=normalize_normal, no_grad_depth=no_grad_depth, no_grad_mask=no_grad_mask,
                        no_grad_camera=no_grad_camera)
        if profile:
            self._engine.ctx.profile_enable(True)
        # (no_grad_normal detaches the normals inside render_normal, renderer.py:908-909: the decoder-path term goes with them)
        weights = None if (no_grad_depth and no_grad_mask and no_grad_camera) else self._decoder_weights()
        zdepth, mask, min_sdf, depth, normal = functions.render_call(self._engine, cfg, latent, R, T,
                                                                     normal_decoder_grad=self.normal_decoder_grad and not no_grad_normal,
                                                                     weights=weights, normals_detached=no_grad_normal)
        if profile:
            n, ms = self._engine.ctx.profile_read()
            self._engine.ctx.profile_enable(False)
            print('march kernel: {0} launches\t: {1:.4f} ms'.format(n, ms))
        if no_grad_depth:
            depth = depth.detach()
        # no_grad_normal: the reference detaches the normals INSIDE render_normal (renderer.py:908-909), i.e. before `R @ normal`
        # (:978) -- the explicit gradient of that product w.r.t. R survives the flag (golden G18: g_R is the same with and without it).
        # The autograd normal of this build carries exactly that term and nothing else (the terms through the decoder are identically
        # ~0 for a ReLU decoder after normalisation), so the flag has nothing left to remove here. (Round 3 detached the
        # whole image, which also dropped the R term: found by G18.) With normalize_normal=False the decoder-path terms are not
        # identically zero in the reference; this build returns them with normal_decoder_grad=True only, and then the flag switches them
        # off again (above); by default they are omitted for both settings, so the flag is a no-op there too.
        if no_grad_mask and no_grad_camera:
            min_sdf = min_sdf.detach()
        if num_forward_sampling != 0:
            inside = self.forward_sampling(latent, R, T, zdepth, mask.bool(), clamp_dist=clamp_dist,
                                           num_forward_sampling=num_forward_sampling, use_transform=use_transform)
            return depth, normal, mask.reshape(h, w), min_sdf.reshape(h, w), inside.reshape(h, w, num_forward_sampling)
        return depth, normal, mask.reshape(h, w), min_sdf.reshape(h, w)

    def render_mesh(self, verts, faces, R, T, normal_frame='image', details=False):
        """Depth, normal and mask maps of a triangle mesh seen by this renderer's camera (no counterpart in the reference, which loads
        such maps from files its Blender pipeline wrote): distr.mesh.render_mesh with the renderer's own intrinsic, img_hw and
        transform matrix, so a mesh render and an SDF render of the same object cannot disagree about the camera. R (3, 3) / T (3)
        -> (depth (H, W), normal (H, W, 3), mask (H, W) uint8) like the first three results of render; R (B, 3, 3) / T (B, 3) -> a
        leading B. normal_frame='image': the convention of render's normals; 'world': what SDFRenderer_deepsdf.get_samples takes.
        details=True: also (zdepth, face, bary). The maps are observations: nothing here is differentiable."""
        from distr import mesh
        dev = self.calib_map.device
        R = torch.as_tensor(R).detach().to(device=dev, dtype=torch.float32)
        T = torch.as_tensor(T).detach().to(device=dev, dtype=torch.float32)
        if tuple(R.shape[-2:]) != (3, 3) or R.dim() not in (2, 3) or tuple(T.shape) != tuple(R.shape[:-2]) + (3,):
            raise ValueError('render_mesh: R has shape %s and T %s; (3, 3) and (3,), or (B, 3, 3) and (B, 3)' % (tuple(R.shape), tuple(T.shape)))
        RT = torch.cat([R, T.unsqueeze(-1)], -1)
        if not torch.is_tensor(verts) or not verts.is_cuda:
            verts = mesh._cuda(verts, torch.float32, dev)
        return mesh.render_mesh(verts, faces, self.intrinsic, RT, self.img_hw, transform_matrix=self._M_np, normal_frame=normal_frame,
                                details=details)

    # reference: renderer.py:912
    def forward_sampling(self, latent, R, T, Zdepth, valid_mask, clamp_dist=0.1, num_forward_sampling=1, no_grad=False,
                         use_transform=True):
        """Samples BEHIND the rendered surface along every valid ray: inside_samples[px, i] = f(point(Zdepth + g_i)) + g_i with
        g_i = 0.5 * clamp_dist * (i + 1) / k (renderer.py:912-941; zero on invalid pixels). Zdepth is detached, the latent code
        and the camera keep their gradients (decode_sdf with autograd: distr_mlp_backward). One fused launch per offset."""
        if num_forward_sampling <= 0:
            raise AssertionError('num_forward_sampling must be positive')
        P = self.img_hw[0] * self.img_hw[1]
        out = torch.zeros(P, num_forward_sampling, dtype=torch.float32, device=Zdepth.device)
        idx = torch.nonzero(valid_mask.reshape(-1)).reshape(-1)
        if idx.numel() == 0:
            return out
        cam_pos = self.get_camera_location(R, T)
        rays = self.get_camera_rays(R)[:, idx]
        z = Zdepth.reshape(-1)[idx]
        cols = []
        for i in range(num_forward_sampling):
            g = 0.5 * clamp_dist * (i + 1) / num_forward_sampling
            pts = self.generate_point_samples(cam_pos, rays, z + g, inv_transform=use_transform, has_zdepth_grad=False)
            if no_grad:
                with torch.no_grad():
                    sdf = functions.mlp_eval(self._engine, latent, pts.t().contiguous())
            else:
                sdf = functions.mlp_eval_autograd(self._engine, latent, pts.t().contiguous(), None)
            cols.append(sdf.reshape(-1, 1) + g)
        return out.index_copy(0, idx, torch.cat(cols, 1))
