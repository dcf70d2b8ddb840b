"""SDFRenderer_color: textured rendering with a second (colour) decoder + optional point-light shading (reference:
core/sdfrenderer/renderer_rgb.py:12-125). Same constructor / `render` signature and return tuples.

Depth, mask, min-sdf sample and normals come from one fused `distr_render_forward` (the 'recursive' marcher that
`render_depth` defaults to, autograd-style normals); the colour decoder runs on the fused decoder tile too
(`distr_color_eval`: latent = [shape code | colour code] folded into per-call constants, lin8 with three rows). The
colour image is differentiable like the reference's (golden G26): `render_color` / `render` without `no_grad` keep the colour
code, the shape code and -- through the surface points -- the camera on the tape (ColorDecodeFunction -> distr_color_backward)."""
import torch

from distr import decoder_pack, functions

from .renderer import SDFRenderer


class SDFRenderer_color(SDFRenderer):
    # reference: renderer_rgb.py:13
    def __init__(self, decoder, decoder_color, intrinsic, img_hw=None, march_step=50, buffer_size=5, ray_marching_ratio=1.5,
                 max_sample_dist=0.2, threshold=5e-5, use_gpu=True, is_eval=True, color_decoder_grad=False):
        super(SDFRenderer_color, self).__init__(decoder, intrinsic, img_hw=img_hw, march_step=march_step, buffer_size=buffer_size,
                                                ray_marching_ratio=ray_marching_ratio, max_sample_dist=max_sample_dist,
                                                threshold=threshold, use_gpu=use_gpu, is_eval=is_eval)
        nlat = functions.get_engine(decoder, self.device).latent_size
        if nlat != 256:
            raise decoder_pack.UnsupportedDecoder('SDFRenderer_color is built for shape decoders of code length 256 only; this decoder '
                                                  'has code length %d' % nlat)
        self.decoder_color = decoder_color.eval() if is_eval else decoder_color
        functions.get_color_engine(self.decoder_color, self.device)
        # color_decoder_grad (not in the reference, where autograd simply does it): render / render_batch also back-propagate a loss on the
        # colour image to decoder_color.parameters() -- one host sync per backward, so such a backward cannot be captured into a graph
        # (DESIGN.md section 8j); off (the default) nothing changes. Also settable later (self.color_decoder_grad). The SDF decoder gets
        # nothing from the colour image (its points are constants there): decoder_grad keeps its meaning
        self.color_decoder_grad = bool(color_decoder_grad)

    @property
    def _color_engine(self):
        return functions.get_color_engine(self.decoder_color, self.device)

    def _color_decoder_weights(self, no_grad=False):
        """W0..W8, b0..b8 of decoder_color on its autograd graph (weight norm folded there) when this call back-propagates to it:
        color_decoder_grad set, grad enabled, no_grad false and a parameter of decoder_color that requires grad; None otherwise."""
        if not self.color_decoder_grad or no_grad or not torch.is_grad_enabled() or not any(p.requires_grad for p in self.decoder_color.parameters()):
            return None
        functions._check_eval(self.decoder_color)
        Ws, bs = decoder_pack.effective_weights_torch_color(self.decoder_color)
        return Ws + bs

    # reference: renderer_rgb.py:20
    def render_color(self, latent_color, latent, cam_pos, cam_rays, Zdepth, valid_mask, no_grad=False):
        h, w = self.img_hw
        color = torch.zeros(h * w, 3, device=Zdepth.device)
        idx = torch.nonzero(valid_mask.reshape(-1)).reshape(-1)
        if idx.numel() == 0:
            return color.reshape(h, w, 3)
        points = self.generate_point_samples(cam_pos, cam_rays[:, idx], Zdepth.reshape(-1)[idx], has_zdepth_grad=False)
        if no_grad or not torch.is_grad_enabled():
            with torch.no_grad():
                rgb = functions.color_eval(self._color_engine, latent_color, latent, points.t())
        else:
            # renderer_rgb.py:32-36: without no_grad the colours stay on the tape -- gradients to the colour code, the shape code and, through
            # the surface points (Zdepth detached: has_zdepth_grad=False), to the camera (distr_color_backward; golden G26)
            rgb = functions.color_eval_autograd(self._color_engine, latent_color, latent, points.t().contiguous())
        return color.index_copy(0, idx, rgb).reshape(h, w, 3)

    # reference: renderer_rgb.py:39
    def compute_shading_maps(self, R, T, lighting_locations, Zdepth, Znormal, valid_mask):
        """Lambertian n.l terms for M point lights -> (M, H*W); zero off the mask. (The reference's torch.bmm(R[None],
        directions), renderer_rgb.py:58, only runs for M = 1; any M works here.)"""
        idx = torch.nonzero(valid_mask.reshape(-1)).reshape(-1)
        cam_pos, cam_rays = self.get_camera_location(R, T), self.get_camera_rays(R)
        pts = self.generate_point_samples(cam_pos, cam_rays[:, idx], Zdepth.reshape(-1)[idx], inv_transform=False).t()   # (N,3)
        to_light = lighting_locations[:, None, :] - pts[None, :, :]                                                     # (M,N,3)
        to_light = to_light / torch.norm(to_light, p=2, dim=2, keepdim=True)
        z_dirs = torch.matmul(to_light, R.t())                                   # rows = R @ direction
        lambert = (z_dirs * Znormal.reshape(-1, 3)[idx][None]).sum(2)            # (M,N)
        out = torch.zeros(lighting_locations.shape[0], Zdepth.numel(), device=Zdepth.device, dtype=lambert.dtype)
        return out.index_copy(1, idx, lambert)

    # reference: renderer_rgb.py:73
    def render(self, latent_color, latent, R, T, clamp_dist=0.1, profile=False, no_grad=False, lighting_locations=None,
               lighting_energies=None):
        if self._color_decoder_weights(no_grad) is not None:
            # color_decoder_grad: the colours come from the colour stage's node with B = 1 (the node that carries the weight gradients);
            # depth, normal, mask and min_sdf are bit for bit those below, the colours agree to rounding (render_batch's contract)
            R, T = torch.as_tensor(R), torch.as_tensor(T)
            outs = self.render_batch(latent_color, latent, R[None], T[None], clamp_dist=clamp_dist, no_grad=no_grad,
                                     lighting_locations=lighting_locations, lighting_energies=lighting_energies)
            return tuple(o[0] for o in outs)
        h, w = self.img_hw
        cfg = self._cfg(clamp_dist, 'recursive', True, want_normal=True, no_grad_depth=no_grad, no_grad_mask=no_grad,
                        no_grad_camera=no_grad)
        cfg.use_depth2normal = 0
        zdepth, mask, min_sdf, depth, normal = functions.render_call(self._engine, cfg, latent, R, T)
        if no_grad:
            # (the normals are detached inside render_normal, before `R @ normal` (renderer_rgb.py:93-94): their gradient w.r.t. R stays,
            # exactly as in SDFRenderer.render -- golden G18)
            depth, min_sdf = depth.detach(), min_sdf.detach()
        valid = mask.bool()
        color = self.render_color(latent_color, latent, self.get_camera_location(R, T), self.get_camera_rays(R), zdepth.detach(),
                                  valid, no_grad=no_grad)
        mask_img, min_sdf = mask.reshape(h, w), min_sdf.reshape(h, w)
        if lighting_locations is None:
            return depth, normal, color, mask_img, min_sdf
        if lighting_energies is None:
            lighting_energies = torch.ones_like(lighting_locations[:, 0])
        shading = self.compute_shading_maps(R, T, lighting_locations, zdepth.detach(), normal.reshape(-1, 3), valid)
        shading = (shading * lighting_energies[:, None]).sum(0).reshape(h, w)
        return depth, normal, color * shading[:, :, None], mask_img, min_sdf

    def render_batch(self, latent_color, latent, Rs, Ts, clamp_dist=0.1, no_grad=False, lighting_locations=None, lighting_energies=None):
        """render (renderer_rgb.py:73) of B views in ONE launch sequence (no counterpart in the reference, whose demos call render once per
        frame): Rs (B,3,3) / Ts (B,3) or sequences of per-view tensors; latent (1,256) shared by the views or (B,256), latent_color
        (1,cs) or (B,cs); lighting_locations (M,3) shared or (B,M,3), lighting_energies (M,) or (B,M) (default ones). Returns (depth
        (B,H,W), normal (B,H,W,3), color (B,H,W,3), mask (B,H,W), min_sdf (B,H,W)).

        Geometry is one batched render with `render`'s configuration: depth, normal, mask and min_sdf of view v are bit-identical to
        render(latent_color, latent, Rs[v], Ts[v], ...). The colours are one node over the colour stage (distr_color_stage_*: the valid
        pixels compacted on the device, their points rebuilt from the rays, one segmented colour evaluation, one shading epilogue): every
        view's bytes and gradients are those of its own B = 1 call; against `render` the colours agree to rounding (the points are formed
        in another f32 order). Gradients reach both codes, the cameras and, with lights, the normal image -- and through it the render;
        lights and energies are observations (ValueError if one requires grad). no_grad detaches what render(no_grad=True) detaches.
        With color_decoder_grad the backward also reaches decoder_color.parameters() (functions.ColorStageFunction's weights: one host
        sync per backward); every other byte, forward and backward, is that of the flag-off call."""
        h, w = self.img_hw
        dev = self.calib_map.device
        to_dev = lambda t: t.to(device=dev, dtype=torch.float32)      # (per view, like render_depth_batch)
        Rs = torch.stack([to_dev(r) for r in Rs]) if not torch.is_tensor(Rs) else Rs
        Ts = torch.stack([to_dev(t) for t in Ts]) if not torch.is_tensor(Ts) else Ts
        if Rs.dim() != 3 or Ts.dim() != 2 or Rs.shape[0] != Ts.shape[0]:
            raise ValueError('expected Rs (B,3,3) and Ts (B,3) of the same B; got %s and %s' % (tuple(Rs.shape), tuple(Ts.shape)))
        B = Rs.shape[0]
        ceng = self._color_engine
        functions.color_code_rows(ceng, latent_color, latent, B)       # ValueError naming the expected shapes, before anything is rendered
        functions.color_lights(dev, B, lighting_locations, lighting_energies)
        cfg = self._cfg(clamp_dist, 'recursive', True, want_normal=True, no_grad_depth=no_grad, no_grad_mask=no_grad,
                        no_grad_camera=no_grad)
        cfg.use_depth2normal = 0
        zdepth, mask, min_sdf, depth, normal = functions.render_batch_call(self._engine, cfg, latent, Rs, Ts)
        if no_grad:
            depth, min_sdf = depth.detach(), min_sdf.detach()
        color = functions.color_stage_call(ceng, cfg, latent_color, latent, Rs, Ts, zdepth.detach(), mask, normal, lighting_locations,
                                           lighting_energies, detach_color=no_grad, weights=self._color_decoder_weights(no_grad))
        return depth, normal, color, mask.reshape(B, h, w), min_sdf.reshape(B, h, w)

    def relight(self, color, normal, Zdepth, mask, R, T, lighting_locations, lighting_energies=None):
        """F relit frames of ONE rendered view without marching it again (the relighting demo's loop): color (H,W,3) = the UNLIT colour
        image of render / render_batch, normal (H,W,3), mask (H,W) of the same render, Zdepth (H*W) the ray-length depth of
        render_depth for that view (not the `depth` image, which is Zdepth * calib_map); lighting_locations (F,M,3), lighting_energies
        (M,) or (F,M), default ones. Returns (F,H,W,3): frame f is byte for byte the colour image of the lit render_batch of this view
        with lighting_locations[f]. Forward only: nothing is on the tape."""
        cfg = self._cfg(0.1, 'recursive', True, want_normal=True)
        return functions.color_relight(self._color_engine, cfg, color, normal, Zdepth, mask, R, T, lighting_locations, lighting_energies)
