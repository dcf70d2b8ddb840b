"""SDFRenderer_deepsdf: an observed depth / normal map back-projected into SDF samples of the decoder -- the supervision terms of
a DeepSDF-style fit of a shape code (or a camera) to depth scans (reference: core/sdfrenderer/renderer_deepsdf.py:10-64). Same
constructor and method signatures.

`get_samples` lifts every valid pixel (0 < depth < 1e5, row-major order) to its 3-D point p, evaluates the decoder at p +- eta * n and
returns the residuals (f(p + eta n) - eta, f(p - eta n) + eta); `get_freespace_samples` evaluates the decoder at random fractions
of the observed depth along each ray. Each call is one node of libdistr.so (distr.functions.DepthSamplesFunction,
include/distr_samples.h): compaction by a fixed-order scan, one point kernel, ONE decoder evaluation over the whole list (the reference
runs two, or `number`), an epilogue; the backward gives the shape code's gradient and, through the points, RT's. `depth` and `normal`
are observations: a tensor that requires grad is refused, not silently detached.

Not in the reference: keyword-only `eta_map=` / `ratio=` (explicit draws for tests and reproducible fits; by default they are
torch.rand on the device, so torch.manual_seed governs them) and the `*_batch` forms (V views, one list, one evaluation)."""
import torch

from distr import binding, functions

from .renderer import SDFRenderer


class SDFRenderer_deepsdf(SDFRenderer):
    """Debug read-back (not in the reference; tests and diagnostics use it): every call replaces `last_counts` (valid pixels per
    view), `last_eta_map` / `last_ratio` (the draws it used, view after view) and `_last_points` (the point list the decoder saw, in
    the layout of include/distr_samples.h, without gradient). They hold device memory of the last call only: the list lives until
    the next call or `clear_last()`."""

    _last_points = last_counts = last_eta_map = last_ratio = None

    def clear_last(self):
        """Drops the debug read-back of the last call (frees its device memory)."""
        self._last_points = self.last_counts = self.last_eta_map = self.last_ratio = None

    # reference: renderer_deepsdf.py:11
    def __init__(self, decoder, intrinsic, img_hw=None, march_step=50, buffer_size=5, ray_marching_ratio=1.5, max_sample_dist=0.2,
                 threshold=5e-5, use_gpu=True, is_eval=True):
        super(SDFRenderer_deepsdf, self).__init__(decoder, intrinsic, img_hw=img_hw, march_step=march_step, buffer_size=buffer_size,
                                                  ray_marching_ratio=ray_marching_ratio, max_sample_dist=max_sample_dist,
                                                  threshold=threshold, use_gpu=use_gpu, is_eval=is_eval)

    def _observed(self, name, t, views, channels):
        """An observation as (V, H, W[, 3]): shape-checked against img_hw, refused when it carries a gradient."""
        if not torch.is_tensor(t):
            t = torch.stack([torch.as_tensor(x) for x in t])
        if t.requires_grad:
            raise ValueError('%s requires grad: it is an observation, SDFRenderer_deepsdf has no gradient for it (detach it)' % name)
        h, w = self.img_hw
        want = h * w * channels
        if t.numel() == 0 or t.numel() % want or (views is not None and t.numel() != views * want):
            raise ValueError('%s has shape %s; img_hw %s takes %s%d x %d%s' % (name, tuple(t.shape), (h, w), '' if views == 1 else 'V x ', h, w,
                                                                                ' x 3' if channels == 3 else ''))
        return t.reshape(-1, h, w, channels) if channels == 3 else t.reshape(-1, h, w)

    def _samples_cfg(self, clamp_dist, mode, number=1):
        if mode == 'freespace' and not 1 <= int(number) <= binding.SAMPLES_MAX_NUMBER:
            raise ValueError('number must be 1..%d' % binding.SAMPLES_MAX_NUMBER)
        return binding.make_samples_cfg(self.img_hw, self.intrinsic, self._M_np, clamp_dist, mode, number)

    def _count(self, cfg, depth):
        depth, index, counts = functions.depth_samples_count(self._engine, cfg, depth)
        if min(counts) == 0:
            raise ValueError('No valid depth.')          # generate_point_samples (renderer.py:178-179)
        return depth, index, counts

    def _draws(self, given, n, name):
        dev = self.calib_map.device
        if given is None:
            return torch.rand(n, dtype=torch.float32, device=dev)
        given = torch.cat([torch.as_tensor(g).reshape(-1) for g in given]) if isinstance(given, (list, tuple)) else given
        if given.numel() != n:
            raise ValueError('%s has %d entries; the valid pixels need %d' % (name, given.numel(), n))
        return given.detach().to(device=dev, dtype=torch.float32).reshape(-1)

    def _views(self, RT):
        dev = self.calib_map.device
        RT = torch.stack([t.to(device=dev, dtype=torch.float32) for t in RT]) if not torch.is_tensor(RT) else RT
        if RT.dim() != 3 or tuple(RT.shape[1:]) != (3, 4):
            raise ValueError('RT has shape %s; a batch takes (V, 3, 4)' % (tuple(RT.shape),))
        return RT

    # reference: renderer_deepsdf.py:14
    def get_samples(self, latent, RT, depth, normal, clamp_dist=0.1, eta=0.01, use_rand=True, *, eta_map=None):
        """-> (samples_pos (N,), samples_neg (N,)). eta_map (N,): the offsets themselves (overrides eta / use_rand)."""
        if tuple(RT.shape) != (3, 4):
            raise ValueError('RT has shape %s; get_samples takes (3, 4)' % (tuple(RT.shape),))
        out = self._get_samples(latent, RT.reshape(1, 3, 4), self._observed('depth', depth, 1, 1), self._observed('normal', normal, 1, 3),
                                clamp_dist, eta, use_rand, eta_map)
        return out[0]

    def get_samples_batch(self, latent, RT, depth, normal, clamp_dist=0.1, eta=0.01, use_rand=True, *, eta_map=None):
        """get_samples of V views as one list and one decoder evaluation: RT (V,3,4), depth (V,H,W), normal (V,H,W,3), latent (1,C)
        shared or (V,C); eta_map: sum(N_v) offsets, view after view (or a sequence of per-view tensors). Returns
        [(samples_pos, samples_neg) per view]; entry v is byte for byte get_samples of view v with its part of eta_map."""
        RT = self._views(RT)
        V = RT.shape[0]
        return self._get_samples(latent, RT, self._observed('depth', depth, V, 1), self._observed('normal', normal, V, 3), clamp_dist, eta,
                                 use_rand, eta_map)

    def _get_samples(self, latent, RT, depth, normal, clamp_dist, eta, use_rand, eta_map):
        cfg = self._samples_cfg(clamp_dist, 'surface')
        depth, index, counts = self._count(cfg, depth)
        n = sum(counts)
        if eta_map is not None:
            eta_map = self._draws(eta_map, n, 'eta_map')
        elif use_rand:
            eta_map = self._draws(None, n, 'eta_map') * eta          # renderer_deepsdf.py:30
        else:
            eta_map = torch.full((n,), float(eta), dtype=torch.float32, device=self.calib_map.device)
        per_view, self._last_points = functions.samples_call(self._engine, cfg, latent, RT, depth, normal, eta_map, index, counts)
        self.last_counts, self.last_eta_map = counts, eta_map
        return per_view

    # reference: renderer_deepsdf.py:45
    def get_freespace_samples(self, latent, RT, depth, clamp_dist=0.1, number=1, *, ratio=None):
        """-> samples (number * N,), draw after draw. ratio (number, N): the fractions of the observed depth themselves."""
        if tuple(RT.shape) != (3, 4):
            raise ValueError('RT has shape %s; get_freespace_samples takes (3, 4)' % (tuple(RT.shape),))
        return self._get_freespace(latent, RT.reshape(1, 3, 4), self._observed('depth', depth, 1, 1), clamp_dist, number, ratio)[0]

    def get_freespace_samples_batch(self, latent, RT, depth, clamp_dist=0.1, number=1, *, ratio=None):
        """get_freespace_samples of V views as one list and one decoder evaluation; ratio: per view (number, N_v), flattened view after
        view (or a sequence of per-view tensors). Returns [samples (number * N_v,) per view], each byte for byte the stand-alone call."""
        RT = self._views(RT)
        return self._get_freespace(latent, RT, self._observed('depth', depth, RT.shape[0], 1), clamp_dist, number, ratio)

    def _get_freespace(self, latent, RT, depth, clamp_dist, number, ratio):
        cfg = self._samples_cfg(clamp_dist, 'freespace', number)
        depth, index, counts = self._count(cfg, depth)
        ratio = self._draws(ratio, int(number) * sum(counts), 'ratio')          # renderer_deepsdf.py:57: U[0, 1) per draw and valid pixel
        per_view, self._last_points = functions.freespace_call(self._engine, cfg, latent, RT, depth, ratio, index, counts)
        self.last_counts, self.last_ratio = counts, ratio
        return per_view
