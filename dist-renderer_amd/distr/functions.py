"""torch.autograd glue around the C ABI: forward -> distr_render_forward, backward -> distr_render_backward.

Replaces the autograd tape the reference records through ~50 decode_sdf calls per render
(core/sdfrenderer/renderer.py:382-420, 836-878): the forward keeps O(buffer_size) selected rows per ray
in the workspace tensor together with the ReLU masks of those rows, the backward kernel runs the dX chain at exactly those points.
"""
import ctypes as C
import weakref

import numpy as np
import torch

from . import binding, decoder_pack


def _param_key(module):
    """Identity + in-place version of every parameter: changes after load_state_dict / an optimiser step / .to().
    NOT seen: edits through `.data` (`p.data.copy_()`, `p.data.mul_()`, EMA-style updates) -- they do not bump `_version`. Code
    that edits decoder weights that way must call `get_engine(decoder, dev).refresh(decoder)` itself (a content checksum per
    render would cost a device reduction and a host sync in the hot path)."""
    return tuple((p.data_ptr(), p._version) for p in module.parameters())


def _check_eval(module):
    if module.training and getattr(module, 'dropout', None) and float(getattr(module, 'dropout_prob', 0.0) or 0.0) > 0.0:
        raise decoder_pack.UnsupportedDecoder('decoder is in training mode with dropout: the fused kernels evaluate the deterministic '
                                              '(eval) network only -- call decoder.eval() (SDFRenderer(is_eval=True) does)')


class DecoderEngine(object):
    """Packed decoder on one device (distr_ctx). One per (decoder module, device); `weights=(Ws, bs)` instead of a module: an engine
    straight from numpy weights, never re-synchronised."""

    def __init__(self, decoder=None, device_index=0, weights=None):
        self.ctx = binding.Context(device_index)
        self.device = torch.device('cuda', device_index)
        self._key = None
        self.generation = 0    # number of weight uploads so far: a forward remembers it, its backward refuses to run on newer weights
        self._f16_state = {'gen': None, 'n': 0}      # _check_f16_range: the upload last checked, renders since
        if weights is None:
            self.refresh(decoder)
        else:
            self._upload(*self._flatten(*weights))

    _pack = staticmethod(decoder_pack.pack_module_sized)

    @staticmethod
    def _flatten(Ws, bs):
        return decoder_pack.flatten(Ws, bs), decoder_pack.latent_size_of(Ws)

    def _set(self, flat, nlat):
        self.ctx.set_decoder(flat, nlat)

    def _upload(self, flat, nlat):
        self._set(flat, nlat)
        self.latent_size = nlat     # code length C of the uploaded decoder: every latent buffer of this engine has C entries per view
        self.generation += 1

    def refresh(self, decoder):
        """(Re)uploads the weights."""
        self._upload(*self._pack(decoder))
        self._key = _param_key(decoder)

    def sync(self, decoder):
        """The reference reads the live module on every call (decoder_utils.py:53-74); the packed copy follows it: re-packed
        when any parameter was modified in place, replaced or moved since the last upload (a few microseconds to check)."""
        _check_eval(decoder)
        if _param_key(decoder) != self._key:
            self.refresh(decoder)
        return self


class ColorEngine(DecoderEngine):
    """Packed colour decoder on one device (decode_color / SDFRenderer_color)."""
    _pack = staticmethod(decoder_pack.pack_color_module)
    _flatten = staticmethod(decoder_pack.flatten_color)

    def _set(self, flat, nlat):
        self.ctx.set_color_decoder(flat, nlat)


_engines = {DecoderEngine: weakref.WeakKeyDictionary(), ColorEngine: weakref.WeakKeyDictionary()}


def get_engine(decoder, device_index, kind=DecoderEngine):
    per_dec = _engines[kind].setdefault(decoder, {})
    if device_index not in per_dec:
        _check_eval(decoder)
        per_dec[device_index] = kind(decoder, device_index)
    return per_dec[device_index].sync(decoder)


def get_color_engine(decoder_color, device_index):
    return get_engine(decoder_color, device_index, ColorEngine)


def engine_from_weights(Ws, bs, device_index=0):
    """Engine straight from numpy weights (tests / bench; no nn.Module needed)."""
    return DecoderEngine(device_index=device_index, weights=(Ws, bs))


def check_split_arith(engine, arith):
    """The split arithmetics (bf16x6 / f16x3) are built for the code length 256 only."""
    if arith != 'f32' and engine.latent_size != 256:
        raise decoder_pack.UnsupportedDecoder("arith=%r is built for code length 256 only; this decoder's code length is %d: use arith='f32'"
                                              % (arith, engine.latent_size))


def _code(engine, latent, dev, views=False):
    """latent -> flat f32 device buffer of C (views=True: (1, C) shared or (B, C)) entries; ValueError naming (1, C) otherwise."""
    C = engine.latent_size
    lat = _f32c(latent, dev)
    if lat.numel() == 0 or lat.numel() % C or (not views and lat.numel() != C):
        raise ValueError('latent has shape %s; this decoder takes (1, %d)%s' % (tuple(latent.shape), C, ' or (B, %d)' % C if views else ''))
    return lat.reshape(-1, C) if views else lat.reshape(-1)


def _point_list(engine, latent, points, color_code=None):
    """(code, points (n, 3), n) of a plain point-list call as f32 device buffers; with color_code the colour decoder's input
    [shape_code | color_code] (decoder_utils.py:101-103)."""
    dev = engine.device
    if color_code is None:
        lat = _code(engine, latent, dev)
    else:
        lat = torch.cat([_f32c(latent, dev).reshape(-1), _f32c(color_code, dev).reshape(-1)])
        if lat.numel() != engine.latent_size:
            raise ValueError('shape code + colour code have %d entries, the colour decoder expects %d' % (lat.numel(), engine.latent_size))
    x = _f32c(points, dev).reshape(-1, 3)
    return lat, x, x.shape[0]


def _ws(engine, size_fn, *args):
    """Workspace of size_fn(*args) bytes on the engine's device."""
    return torch.empty(size_fn(*args), dtype=torch.uint8, device=engine.device)


def _list_call(engine, fn, size_fn, lat, x, n, *mid):
    """fn(handle, code, points, n, *mid (tensors as pointers), workspace of size_fn(n) bytes, its size, stream), checked."""
    ws = _ws(engine, size_fn, n)
    mid = [binding.ptr(a) if a is None or torch.is_tensor(a) else a for a in mid]
    engine.ctx.check(fn(engine.ctx.h, binding.ptr(lat), binding.ptr(x), n, *mid, binding.ptr(ws), ws.numel(), engine.ctx.stream()))


def _clamp_arg(clamp_dist):
    return -1.0 if clamp_dist is None else float(clamp_dist)


def color_eval(engine, color_code, shape_code, points):
    """decode_color forward (core/utils/decoder_utils.py:94-112): points (n,3) -> rgb (n,3); the decoder input is
    [shape_code | color_code | xyz] (decoder_utils.py:101-103)."""
    L = engine.ctx.L
    lat, x, n = _point_list(engine, shape_code, points, color_code)
    out = torch.empty(n, 3, dtype=torch.float32, device=engine.device)
    _list_call(engine, L.distr_color_eval, L.distr_mlp_workspace_bytes, lat, x, n, out)
    return out


class ColorDecodeFunction(torch.autograd.Function):
    """decode_color with autograd (decoder_utils.py:94-112 called with no_grad=False): (color_code (1,cs), shape_code (1,256),
    points (n,3)) -> rgb (n,3); backward = distr_color_backward (fused forward recompute + dX chain with the 3-row output layer;
    the code gradients come from the per-tile delta sums)."""

    @staticmethod
    def forward(ctx, color_code, shape_code, points, engine):
        out = color_eval(engine, color_code, shape_code, points)
        ctx.engine = engine
        ctx.save_for_backward(color_code.detach(), shape_code.detach(), points.detach())
        ctx.need = (color_code.requires_grad, shape_code.requires_grad, points.requires_grad)
        return out

    @staticmethod
    def backward(ctx, g):
        engine = ctx.engine
        dev, L = engine.device, engine.ctx.L
        color_code, shape_code, points = ctx.saved_tensors
        lat, x, n = _point_list(engine, shape_code, points, color_code)
        gs = _f32c(g, dev).reshape(-1, 3)
        g_x = torch.empty(n, 3, dtype=torch.float32, device=dev) if ctx.need[2] else None
        g_l = torch.empty(engine.latent_size, dtype=torch.float32, device=dev) if (ctx.need[0] or ctx.need[1]) else None
        _list_call(engine, L.distr_color_backward, L.distr_mlp_backward_workspace_bytes, lat, x, n, gs, g_x, g_l)
        ns = shape_code.numel()
        return ((g_l[ns:].reshape(color_code.shape) if ctx.need[0] else None), (g_l[:ns].reshape(shape_code.shape) if ctx.need[1] else None),
                (g_x.reshape(points.shape) if ctx.need[2] else None), None)


def color_eval_autograd(engine, color_code, shape_code, points):
    return ColorDecodeFunction.apply(color_code, shape_code, points, engine)


def _f32c(t, device):
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def _check_generation(ctx):
    """A backward must run on the decoder weights its forward used: the saved ReLU masks (and every selected row) belong to THAT
    evaluation. Rendering A, updating the decoder, rendering B, then back-propagating A would silently mix new weights with old
    masks -- refuse instead."""
    if ctx.engine.generation != ctx.generation:
        raise RuntimeError('the decoder weights were re-uploaded (load_state_dict / optimiser step / refresh) between this render\'s '
                           'forward and its backward; back-propagate before changing the decoder, or render again')


F16_CHECK_EVERY = 256          # renders between two range checks of the split-f16 arithmetic (DISTR_F16_CHECK_EVERY; the first render of
                               # every decoder upload is always checked)


def _check_f16_range(engine, cfg, ws, nviews=1, view_bytes=0, needs_grad=False):
    """arith = 'f16x3' only. A decoder activation that leaves the f16 range makes the march see a NaN sdf, which fails both `stay`
    comparisons and silently ends the ray -- a driver would optimise on corrupted renders. The march kernel counts such evaluations
    (distr_render_stats.f16_overflows); reading the counter costs a device sync, so for gradient-free renders it is read on the
    first render after every decoder upload and then every F16_CHECK_EVERY renders. A render that will be back-propagated
    (`needs_grad`: an optimisation loop moving the shape code, where overflow depends on the current latent) is checked EVERY time:
    a backward taken on NaN-terminated rays is the failure that must not pass silently. Anything but zero RAISES (use
    arith='bf16x6' or 'f32' for this decoder). Residual window: up to F16_CHECK_EVERY - 1 consecutive gradient-free renders."""
    if cfg.arith != binding.ARITH['f16x3']:
        return
    import os
    every = int(os.environ.get('DISTR_F16_CHECK_EVERY', F16_CHECK_EVERY))
    gen, st = engine.generation, engine._f16_state
    first = st['gen'] != gen
    if first:
        st['gen'], st['n'] = gen, 0
    st['n'] += 1
    if not (first or needs_grad or (every > 0 and st['n'] % every == 0)):
        return
    bad = 0
    for v in range(nviews):
        bad += engine.ctx.render_stats(cfg, ws[v * view_bytes:] if nviews > 1 else ws)['f16_overflows']
    if bad:
        raise binding.DistrError("arith='f16x3': %d decoder evaluation(s) of this render left the f16 range (|activation| x 64 >= 65504): the "
                                 "render is not to be trusted. Use arith='bf16x6' or 'f32' for this decoder / shape code." % bad)


def _single_view(engine, latent, R, T):
    """The single-view calls take one code and one camera: ValueError naming (1, C), (3,3), (3) otherwise."""
    if latent.numel() != engine.latent_size:
        raise ValueError('latent has shape %s; this decoder takes (1, %d)' % (tuple(latent.shape), engine.latent_size))
    if R.numel() != 9 or T.numel() != 3:
        raise ValueError('expected latent (1,%d), R (3,3), T (3)' % engine.latent_size)


def _grad_arg(g, n):
    """Upstream gradient of a render output as the backward kernels read it; None for an output that was not produced."""
    if g is None or g.numel() != n:
        return None
    return g.to(dtype=torch.float32).contiguous()


class RenderBatchFunction(torch.autograd.Function):
    """Several views in one launch sequence (distr_render_forward_batch): (latent (1,C) shared by all views or (B,C), R (B,3,3),
    T (B,3)) -> (zdepth (B,P), mask (B,P) uint8, min_sdf (B,P), depth (B,H,W), normal (B,H,W,3)). The one render node: render_call is
    B = 1. Every view's values and gradients are bit-identical to its own B = 1 call; what changes is the schedule (one march launch
    per step for all views: the views' latency-bound tails overlap). `view_flags`: per-view DISTR_VIEW_GRAD_* (the no_grad_* options of
    each view). `normal_decoder_grad`: the backward also returns the term of a normal-map loss that reaches code and camera through the
    decoder (distr_render_normal_grad_backward_batch), added to the gradients of the main backward; without it every
    byte is what it was before the option existed. `weights` (optional, trailing): W0..W8, b0..b8 of the decoder the engine was packed
    from (decoder_pack.effective_weights_torch) -- the backward then also returns their eighteen gradients (render_weight_grads,
    DESIGN.md section 8h): it exports the backward's sample list, reads the B counts on the host (ONE HOST SYNC per backward: such a
    backward cannot be captured into a graph) and runs the layer-wise train path on the list. The gradients of codes and cameras are
    those of the fused backward either way; without weights every byte is what it was before the option existed."""

    @staticmethod
    def forward(ctx, latent, R, T, engine, cfg, view_flags, normal_decoder_grad=False, *weights):
        if weights and len(weights) != 18:
            raise ValueError('expected W0..W8, b0..b8: 18 tensors, got %d' % len(weights))
        dev = engine.device
        H, W = cfg.band_rows, cfg.W
        P = H * W
        Rc, Tc = _f32c(R, dev).reshape(-1, 9), _f32c(T, dev).reshape(-1, 3)
        B = Rc.shape[0]
        lat = _code(engine, latent, dev, views=True)
        if Tc.shape[0] != B or lat.shape[0] not in (1, B) or not (1 <= B <= binding.MAX_VIEWS):
            raise ValueError('expected latent (1,%d) or (B,%d), R (B,3,3), T (B,3) with 1 <= B <= %d'
                             % (engine.latent_size, engine.latent_size, binding.MAX_VIEWS))
        shared = lat.shape[0] == 1
        fwd_bytes, bwd_bytes = engine.ctx.workspace_bytes(cfg)
        ws = torch.empty(B * fwd_bytes, dtype=torch.uint8, device=dev)
        zdepth = torch.empty(B, P, dtype=torch.float32, device=dev)
        mask = torch.empty(B, P, dtype=torch.uint8, device=dev)
        min_sdf = torch.empty(B, P, dtype=torch.float32, device=dev)
        if cfg.want_normal:
            depth = torch.empty(B, H, W, dtype=torch.float32, device=dev)
            normal = torch.empty(B, H, W, 3, dtype=torch.float32, device=dev)
        else:
            depth = torch.empty(0, dtype=torch.float32, device=dev)
            normal = torch.empty(0, dtype=torch.float32, device=dev)
        flags = None if view_flags is None else (C.c_int32 * B)(*[int(f) for f in view_flags])
        p = binding.ptr
        engine.ctx.check(engine.ctx.L.distr_render_forward_batch(
            engine.ctx.h, C.byref(cfg), B, flags, p(lat), 0 if shared else engine.latent_size, p(Rc), p(Tc), p(zdepth), p(mask), p(min_sdf),
            p(depth) if cfg.want_normal else None, p(normal) if cfg.want_normal else None, p(ws), ws.numel(), engine.ctx.stream()))
        _check_f16_range(engine, cfg, ws, B, fwd_bytes, needs_grad=any(ctx.needs_input_grad[:3]))
        ctx.engine, ctx.cfg, ctx.ws, ctx.bwd_bytes, ctx.B, ctx.shared = engine, cfg, ws, bwd_bytes, B, shared
        ctx.nweights = len(weights)
        if weights:
            ctx.save_for_backward(lat, *weights)       # (the codes as the forward used them: the train path decodes with them again)
        ctx.generation = engine.generation
        ctx.shapes = (latent.shape, R.shape, T.shape)
        ctx.in_meta = tuple((t.device, t.dtype) for t in (latent, R, T))
        ctx.view_bytes = fwd_bytes
        ctx.flags = flags
        ctx.normal_grad = bool(normal_decoder_grad) and normal_grad_applies(cfg)
        ctx.mark_non_differentiable(mask)
        return zdepth, mask, min_sdf, depth, normal

    @staticmethod
    def backward(ctx, g_zdepth, g_mask, g_min_sdf, g_depth, g_normal):
        engine, cfg, ws, B = ctx.engine, ctx.cfg, ctx.ws, ctx.B
        _check_generation(ctx)
        dev = engine.device
        P = cfg.band_rows * cfg.W
        gz, gq = _grad_arg(g_zdepth, B * P), _grad_arg(g_min_sdf, B * P)
        gd, gn = (_grad_arg(g_depth, B * P), _grad_arg(g_normal, 3 * B * P)) if cfg.want_normal else (None, None)
        g_lat = torch.empty(B, engine.latent_size, dtype=torch.float32, device=dev)
        g_R = torch.empty(B, 9, dtype=torch.float32, device=dev)
        g_T = torch.empty(B, 3, dtype=torch.float32, device=dev)
        ws_b = torch.empty(B * ctx.bwd_bytes, dtype=torch.uint8, device=dev)
        p = binding.ptr
        engine.ctx.check(engine.ctx.L.distr_render_backward_batch(
            engine.ctx.h, C.byref(cfg), B, p(ws), ws.numel(), p(gz), p(gq), p(gd), p(gn), p(g_lat), p(g_R), p(g_T),
            p(ws_b), ws_b.numel(), engine.ctx.stream()))
        if ctx.normal_grad and gn is not None:
            # the decoder-path term of the normal-map loss: outputs of its own, added here (the main backward's reduction order stays)
            n_lat, n_R, n_T = normal_grad_term(engine, cfg, ws, gn, B, ctx.flags)
            g_lat, g_R, g_T = g_lat + n_lat, g_R + n_R, g_T + n_T
        g_weights = ()
        if ctx.nweights:
            lat, weights = ctx.saved_tensors[0], ctx.saved_tensors[1:]
            grads, _ = render_weight_grads(engine, cfg, ws, ws_b, B, weights, lat, want_latent=False)
            g_weights = tuple(g.reshape(w.shape).to(device=w.device, dtype=w.dtype) for g, w in zip(grads, weights))
        ls, rs, ts = ctx.shapes
        if ctx.shared and B > 1:
            g_lat = g_lat.sum(0)                   # one shape code rendered from B cameras: the views' gradients add up (fixed order)
        return tuple(g.reshape(sh).to(device=d, dtype=dt) for g, sh, (d, dt) in zip((g_lat, g_R, g_T), (ls, rs, ts), ctx.in_meta)) + (None, None, None, None) + g_weights


def normal_grad_term(engine, cfg, ws, g_normal, B, view_flags=None):
    """distr_render_normal_grad_backward_batch on the saved forward workspace `ws` of B views: the decoder-path term of the upstream
    gradient g_normal (B, H, W, 3) alone -> (g_latent (B, C), g_R (B, 9), g_T (B, 3)), one row per view."""
    dev = engine.device
    gn = _f32c(g_normal, dev)
    if gn.numel() != 3 * B * cfg.band_rows * cfg.W:
        raise ValueError('g_normal has %d entries for %d views of %d x %d x 3' % (gn.numel(), B, cfg.band_rows, cfg.W))
    out = (torch.empty(B, engine.latent_size, dtype=torch.float32, device=dev), torch.empty(B, 9, dtype=torch.float32, device=dev),
           torch.empty(B, 3, dtype=torch.float32, device=dev))
    ws_n = torch.empty(engine.ctx.normal_grad_workspace_bytes(cfg, B), dtype=torch.uint8, device=dev)
    p = binding.ptr
    engine.ctx.check(engine.ctx.L.distr_render_normal_grad_backward_batch(
        engine.ctx.h, C.byref(cfg), B, view_flags, p(ws), ws.numel(), p(gn), p(out[0]), p(out[1]), p(out[2]), p(ws_n), ws_n.numel(),
        engine.ctx.stream()))
    return out


def normal_grad_applies(cfg):
    """The decoder-path term of a normal-map loss exists for raw autograd normals only: depth2normal renders have no decoder in their
    normals, and unit normals are scale invariant (the term is zero: golden G27, *_unit cases)."""
    return bool(cfg.want_normal) and not cfg.use_depth2normal and not cfg.normalize_normal


def check_render_weights(cfg, weights, normal_decoder_grad=False, normals_detached=False):
    """What weight gradients through render are defined for; NotImplementedError naming the reason otherwise.
    normals_detached: the caller keeps the decoder out of the autograd normals (render(no_grad_normal=True), renderer.py:908-909)."""
    if len(weights) != 18:
        raise ValueError('weights: W0..W8, b0..b8 (decoder_pack.effective_weights_torch), 18 tensors, got %d' % len(weights))
    if cfg.arith != binding.ARITH['f32']:
        raise NotImplementedError("decoder_grad: arith='f32' only (the layer-wise train path is f32; the split arithmetics' sample lists "
                                  "belong to other ReLU patterns)")
    if cfg.rows != 0:
        raise NotImplementedError('decoder_grad: row bands are not implemented (render the whole image)')
    if cfg.want_normal and not cfg.use_depth2normal and not normals_detached:
        raise NotImplementedError('decoder_grad: the weight gradient of autograd normals (d(grad_x f)/dW, not zero for a ReLU decoder) is not '
                                  'implemented; normals from depth (use_depth2normal=True) are supported, and so is no_grad_normal=True')
    if normal_decoder_grad:
        raise NotImplementedError('decoder_grad together with normal_decoder_grad: the second path of the normals has no weight gradient here')


def render_batch_call(engine, cfg, latent, R, T, view_flags=None, weights=None, normals_detached=False, normal_decoder_grad=False):
    """Batched render_call: R (B,3,3), T (B,3), latent (1,C) (shared) or (B,C). normal_decoder_grad: see RenderBatchFunction; where the
    term is zero or absent (normal_grad_applies) the option does nothing. weights: None, or W0..W8, b0..b8 of the engine's decoder on
    the autograd graph (decoder_pack.effective_weights_torch): the backward also returns their gradients (one host sync per backward,
    see RenderBatchFunction; check_render_weights names what is refused, normals_detached is its argument)."""
    weights = list(weights) if weights is not None else []
    if weights:
        check_render_weights(cfg, weights, normal_decoder_grad, normals_detached)
    need_bwd = torch.is_grad_enabled() and any(getattr(t, 'requires_grad', False) for t in [latent, R, T] + weights)
    cfg = cfg.clone()
    cfg.save_for_backward = 1 if need_bwd else 0
    if normal_decoder_grad and normal_grad_applies(cfg):
        if cfg.rows != 0:
            raise NotImplementedError('normal_decoder_grad: row bands are not implemented (render the whole image)')
        if cfg.arith != binding.ARITH['f32']:
            raise NotImplementedError("normal_decoder_grad: arith='f32' only")
    return RenderBatchFunction.apply(latent, R, T, engine, cfg, view_flags, bool(normal_decoder_grad), *weights)


def render_call(engine, cfg, latent, R, T, normal_decoder_grad=False, weights=None, normals_detached=False):
    """One view: latent (1,C), R (3,3), T (3) -> (zdepth (P), mask (P) uint8, min_sdf (P), depth (H,W), normal (H,W,3))."""
    _single_view(engine, latent, R, T)
    H, W = cfg.band_rows, cfg.W
    z, mask, q, depth, normal = render_batch_call(engine, cfg, latent, R, T, normal_decoder_grad=normal_decoder_grad, weights=weights,
                                                  normals_detached=normals_detached)
    if cfg.want_normal:
        depth, normal = depth.reshape(H, W), normal.reshape(H, W, 3)
    return z.reshape(-1), mask.reshape(-1), q.reshape(-1), depth, normal


def render_normal_batch_call(engine, cfg, latent, R, T, zdepth, mask):
    """Batched render_normal_call: R (B,3,3), T (B,3), zdepth / mask (B,P) -> (B,3,P)."""
    dev = engine.device
    P = cfg.band_rows * cfg.W
    Rc, Tc = _f32c(R, dev).reshape(-1, 9), _f32c(T, dev).reshape(-1, 3)
    B = Rc.shape[0]
    lat = _code(engine, latent, dev, views=True)
    if lat.shape[0] not in (1, B) or not (1 <= B <= binding.MAX_VIEWS):
        raise ValueError('expected latent (1,%d) or (B,%d), R (B,3,3), T (B,3) with 1 <= B <= %d'
                         % (engine.latent_size, engine.latent_size, binding.MAX_VIEWS))
    z = _f32c(zdepth, dev).reshape(B, P)
    m = mask.detach().to(device=dev).reshape(B, P).to(torch.uint8).contiguous()
    fwd_bytes, _ = engine.ctx.workspace_bytes(cfg)
    ws = torch.empty(B * fwd_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty(B, 3, P, dtype=torch.float32, device=dev)
    p = binding.ptr
    engine.ctx.check(engine.ctx.L.distr_render_normal_batch(engine.ctx.h, C.byref(cfg), B, p(lat), 0 if lat.shape[0] == 1 else engine.latent_size, p(Rc), p(Tc),
                                                            p(z), p(m), p(out), p(ws), ws.numel(), engine.ctx.stream()))
    return out


HALO = 4   # rows; depth2normal needs 1, the 4x4 pyramid parents need the band aligned to 4


def band_cfg(cfg, r0, r1):
    """cfg of the launch that produces rows [r0, r1): the band plus its depth2normal halo. Returns (cfg, b0, b1)."""
    H = cfg.H
    if not (0 <= r0 < r1 <= H) or (r0 & 3) or ((r1 & 3) and r1 != H):
        raise ValueError('band [%d, %d) must lie in [0, %d) on multiples of 4 (or end at H)' % (r0, r1, H))
    halo = HALO if (cfg.want_normal and cfg.use_depth2normal) else 0
    b0, b1 = max(0, r0 - halo), min(H, r1 + halo)
    bcfg = cfg.clone()
    bcfg.row0, bcfg.rows = b0, b1 - b0
    return bcfg, b0, b1


def render_band_call(engine, cfg, latent, R, T, r0, r1):
    """Rows [r0, r1) of the render `cfg` describes (r0, r1 multiples of 4, or r1 == H): what one rank computes when one
    large view is split over several GPUs (row-band tiles whose height is a multiple of 4 px, halo
    recomputed locally for depth2normal). Renders the band plus a HALO-row halo and crops it; autograd through the crop
    zero-pads the halo's upstream gradients, so the sum over a partition of [0, H) of the bands' input gradients equals
    the full render's. Returns (zdepth (n*W), mask (n*W) uint8, min_sdf (n*W), depth (n, W), normal (n, W, 3)), n = r1 - r0;
    every value is bit-identical to the same pixel of the full render."""
    W = cfg.W
    bcfg, b0, b1 = band_cfg(cfg, r0, r1)
    z, mask, q, depth, normal = render_call(engine, bcfg, latent, R, T)
    lo, n = r0 - b0, r1 - r0
    z, mask, q = (t.reshape(b1 - b0, W)[lo:lo + n].reshape(-1) for t in (z, mask, q))
    if cfg.want_normal:
        depth, normal = depth[lo:lo + n], normal[lo:lo + n]
    return z, mask, q, depth, normal


def render_normal_call(engine, cfg, latent, R, T, zdepth, mask):
    """SDFRenderer.render_normal forward (renderer.py:880-910) -> (3, P). Gradient-free: for ReLU decoders the
    normalised SDF gradient is piecewise constant in (latent, point), its autograd contribution is identically ~0
    (SURVEY.md A.6-1)."""
    _single_view(engine, latent, R, T)
    return render_normal_batch_call(engine, cfg, latent, R, T, zdepth, mask)[0]


def mlp_eval(engine, latent, points, clamp_dist=None, arith='f32'):
    """decode_sdf forward (core/utils/decoder_utils.py:53-74): points (n,3) -> (n,1). arith='f32' (default): exact f32 MFMA, bit-identical
    to the oracle; 'bf16x6': six-product split-bf16 arithmetic (distr_mlp_eval_bf16x6: f32-equivalent accuracy, faster, not bit-identical);
    'f16x3': three-product split-f16 arithmetic (distr_mlp_eval_f16x3: the same for decoders inside the f16 range, faster again; NaN
    for a point whose activations leave that range)."""
    if arith not in binding.ARITH:
        raise ValueError("arith must be one of %s" % sorted(binding.ARITH))
    check_split_arith(engine, arith)
    L = engine.ctx.L
    lat, x, n = _point_list(engine, latent, points)
    out = torch.empty(n, 1, dtype=torch.float32, device=engine.device)
    fn = {'f32': L.distr_mlp_eval, 'bf16x6': L.distr_mlp_eval_bf16x6, 'f16x3': L.distr_mlp_eval_f16x3}[arith]
    _list_call(engine, fn, L.distr_mlp_workspace_bytes, lat, x, n, _clamp_arg(clamp_dist), out)
    return out


class DecodeSdfFunction(torch.autograd.Function):
    """decode_sdf with autograd (decoder_utils.py:53-74 called without no_grad): (latent (1,C), points (n,3)) -> (n,1);
    backward = distr_mlp_backward (one fused forward-recompute + dX chain per point, latent gradient from the delta sums)."""

    @staticmethod
    def forward(ctx, latent, points, engine, clamp_dist):
        out = mlp_eval(engine, latent, points, clamp_dist)
        ctx.engine, ctx.clamp = engine, clamp_dist
        ctx.save_for_backward(latent.detach(), points.detach())
        ctx.need = (latent.requires_grad, points.requires_grad)
        return out

    @staticmethod
    def backward(ctx, g):
        engine = ctx.engine
        dev, L = engine.device, engine.ctx.L
        latent, points = ctx.saved_tensors
        lat, x, n = _point_list(engine, latent, points)
        gs = _f32c(g, dev).reshape(-1)
        g_x = torch.empty(n, 3, dtype=torch.float32, device=dev) if ctx.need[1] else None
        g_l = torch.empty(engine.latent_size, dtype=torch.float32, device=dev) if ctx.need[0] else None
        _list_call(engine, L.distr_mlp_backward, L.distr_mlp_backward_workspace_bytes, lat, x, n, gs, _clamp_arg(ctx.clamp), g_x, g_l)
        return (None if g_l is None else g_l.reshape(latent.shape)), (None if g_x is None else g_x.reshape(points.shape)), None, None


def mlp_eval_autograd(engine, latent, points, clamp_dist=None):
    return DecodeSdfFunction.apply(latent, points, engine, clamp_dist)


def segment_plan(counts, max_segments=binding.MAX_SEGMENTS, tile=binding.SEG_TILE):
    """Host-side plan of a segmented point list (pure Python, no GPU): counts[s] >= 0 points per segment ->
    dict(counts: as a list of int, offsets: first point of every segment, tiles: ceil(n_s / 64) tiles each (a tile never holds two
    segments; an empty segment gets none), total: points, chunks: [(s0, s1)] runs of at most 64 segments, one distr_mlp_*_multi call each)."""
    counts = [int(c) for c in counts]
    if not counts:
        raise ValueError('a segmented point list needs at least one segment')
    if min(counts) < 0:
        raise ValueError('segment sizes must be >= 0, got %r' % (counts,))
    offsets, at = [], 0
    for c in counts:
        offsets.append(at)
        at += c
    S = len(counts)
    return dict(counts=counts, offsets=offsets, tiles=[(c + tile - 1) // tile for c in counts], total=at,
                chunks=[(s0, min(S, s0 + max_segments)) for s0 in range(0, S, max_segments)])


def _multi_args(engine, latents, points, counts):
    """(codes (S, C) or (1, C) shared, flat points (N, 3), plan) of a segmented call; ValueError on a shape that does not fit."""
    dev = engine.device
    plan = segment_plan(counts)
    S, Cn = len(plan['tiles']), engine.latent_size
    lat = _f32c(latents, dev)
    if lat.numel() not in (Cn, S * Cn):
        raise ValueError('latents have shape %s; %d segments take (S, C) = (%d, %d) (or (1, %d): one shared code)'
                         % (tuple(latents.shape), S, S, Cn, Cn))
    x = _f32c(points, dev).reshape(-1, 3)
    if x.shape[0] != plan['total']:
        raise ValueError('counts sum to %d, but there are %d points' % (plan['total'], x.shape[0]))
    return lat.reshape(-1, Cn), x, plan


def _multi_chunks(lat, plan):
    """Per chunk of at most 64 segments: (first segment, segments, first point, first code row, latent_stride); a shared code (lat (1, C))
    is row 0 with stride 0 in every chunk. Pure Python."""
    shared = lat.shape[0] == 1
    for s0, s1 in plan['chunks']:
        yield s0, s1 - s0, plan['offsets'][s0], (0 if shared else s0), (0 if shared else lat.shape[1])


def _multi_run(engine, latents, points, counts, ws_bytes, outputs, call):
    """The plumbing every segmented call shares. Checks the arguments, allocates `outputs(n points, S)`, then per chunk runs
    call(head, tail, p0, s0, out) with head = the arguments every distr_mlp_*_multi begins with (handle, nseg, counts, codes,
    latent_stride, xyz of the chunk), tail = those it ends with (workspace of ws_bytes(nseg, counts), its size, stream), p0 / s0 = the
    chunk's first point / segment (where its slices of the per-point / per-segment arrays start). Returns the outputs."""
    lat, x, plan = _multi_args(engine, latents, points, counts)
    out = outputs(x.shape[0], len(plan['tiles']))
    ctx, p = engine.ctx, binding.ptr
    for s0, ns, p0, row, stride in _multi_chunks(lat, plan):
        cnt = (C.c_int64 * ns)(*plan['counts'][s0:s0 + ns])
        ws = _ws(engine, ws_bytes, ns, cnt)
        ctx.check(call((ctx.h, ns, cnt, p(lat[row:]), stride, p(x[p0:])), (p(ws), ws.numel(), ctx.stream()), p0, s0, out))
    return out


def mlp_eval_multi(engine, latents, points, counts, clamp_dist=None):
    """decode_sdf of a segmented point list: segment s = counts[s] consecutive rows of points (sum counts, 3), decoded with latents[s]
    (latents (S, C); (1, C) = one shared code) -> (sum counts, 1). One launch sequence per 64 segments (distr_mlp_eval_multi); every
    segment's slice is byte for byte mlp_eval of that segment alone."""
    L, p, dev = engine.ctx.L, binding.ptr, engine.device
    return _multi_run(engine, latents, points, counts, L.distr_mlp_multi_workspace_bytes,
                      lambda n, S: torch.empty(n, 1, dtype=torch.float32, device=dev),
                      lambda head, tail, p0, s0, out: L.distr_mlp_eval_multi(*head, _clamp_arg(clamp_dist), p(out[p0:]), *tail))


def mlp_grad_multi(engine, latents, points, counts):
    """(sdf (sum counts,), d sdf/d xyz (sum counts, 3)) of the unclamped decoder on a segmented point list (see mlp_eval_multi)."""
    L, p, dev = engine.ctx.L, binding.ptr, engine.device
    return _multi_run(engine, latents, points, counts, L.distr_mlp_multi_workspace_bytes,
                      lambda n, S: (torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, 3, dtype=torch.float32, device=dev)),
                      lambda head, tail, p0, s0, out: L.distr_mlp_grad_multi(*head, p(out[0][p0:]), p(out[1][p0:]), *tail))


def mlp_backward_multi(engine, latents, points, counts, g_sdf, clamp_dist=None, need_latent=True, need_points=True):
    """Backward of mlp_eval_multi for the upstream gradient g_sdf (sum counts,): (g_latent (S, C): one row per segment, also for a
    shared code (the caller sums), g_points (sum counts, 3)); either is None when not needed."""
    L, p, dev = engine.ctx.L, binding.ptr, engine.device
    gs = _f32c(g_sdf, dev).reshape(-1)

    def outputs(n, S):
        if gs.numel() != n:
            raise ValueError('g_sdf has %d entries for %d points' % (gs.numel(), n))
        return (torch.empty(S, engine.latent_size, dtype=torch.float32, device=dev) if need_latent else None,
                torch.empty(n, 3, dtype=torch.float32, device=dev) if need_points else None)

    def call(head, tail, p0, s0, out):
        g_l, g_x = out
        return L.distr_mlp_backward_multi(*head, p(gs[p0:]), _clamp_arg(clamp_dist), p(None if g_x is None else g_x[p0:]),
                                          p(None if g_l is None else g_l[s0:]), *tail)
    return _multi_run(engine, latents, points, counts, L.distr_mlp_backward_multi_workspace_bytes, outputs, call)


class DecodeSdfMultiFunction(torch.autograd.Function):
    """mlp_eval_multi with autograd: (latents (S, C) or (1, C), points (sum counts, 3)) -> (sum counts, 1); backward =
    distr_mlp_backward_multi, one launch sequence per 64 segments. Row s of the latent gradient is the stand-alone call's, bit for bit;
    a shared code gets the sum of the rows."""

    @staticmethod
    def forward(ctx, latents, points, engine, counts, clamp_dist):
        out = mlp_eval_multi(engine, latents, points, counts, clamp_dist)
        ctx.engine, ctx.clamp, ctx.counts = engine, clamp_dist, [int(c) for c in counts]
        ctx.save_for_backward(latents.detach(), points.detach())
        ctx.need = (latents.requires_grad, points.requires_grad)
        return out

    @staticmethod
    def backward(ctx, g):
        engine = ctx.engine
        latents, points = ctx.saved_tensors
        g_rows, g_x = mlp_backward_multi(engine, latents, points, ctx.counts, g, ctx.clamp, need_latent=ctx.need[0], need_points=ctx.need[1])
        if g_rows is not None:
            g_rows = (g_rows.sum(0) if latents.numel() == engine.latent_size and g_rows.shape[0] > 1 else g_rows).reshape(latents.shape)
        return g_rows, (None if g_x is None else g_x.reshape(points.shape)), None, None, None


def mlp_eval_multi_autograd(engine, latents, points, counts, clamp_dist=None):
    return DecodeSdfMultiFunction.apply(latents, points, engine, counts, clamp_dist)


# ---- the layer-wise decoder path: decode_sdf with gradients to the decoder's weights (include/distr_train.h)
TRAIN_ROW_TILE = 64                 # every segment is padded to a multiple of 64 workspace rows
TRAIN_SLAB_MIN = 256                # smallest K slab of a weight-gradient GEMM (rows)
TRAIN_MAX_SLABS = 64                # DISTR_TRAIN_MAX_SLABS
TRAIN_MAX_BYTES_DEFAULT = 32 << 30  # DISTR_TRAIN_MAX_BYTES: largest workspace decode_sdf_train allocates for one call


def train_slab_plan(rows):
    """(slab length, number of slabs) of the weight-gradient GEMMs over `rows` workspace rows: g_W = Delta^T X sums over the rows in
    slabs that are added up in slab order. A pure function of the row count (never of the GPU): the length is a multiple of 64 rows, at
    least 256, and long enough for 64 slabs to cover the list. Mirror of distr_train_slab_plan."""
    rows = max(0, int(rows))
    per = -(-rows // TRAIN_MAX_SLABS)
    length = max(TRAIN_SLAB_MIN, -(-per // TRAIN_ROW_TILE) * TRAIN_ROW_TILE)
    return length, -(-rows // length)


def train_segment_rows(counts):
    """First workspace row of every segment, and behind them the number of rows in all (mirror of distr_train_segment_row)."""
    rows, at = [], 0
    for c in counts:
        rows.append(at)
        at += -(-int(c) // TRAIN_ROW_TILE) * TRAIN_ROW_TILE
    return rows + [at]


def train_max_bytes():
    import os
    return int(os.environ.get('DISTR_TRAIN_MAX_BYTES', TRAIN_MAX_BYTES_DEFAULT))


_train_contexts = {}


def _train_context(device_index):
    """The context of the train calls on one device: it supplies the device and the stream, no decoder is set on it."""
    if device_index not in _train_contexts:
        _train_contexts[device_index] = binding.Context(device_index)
    return _train_contexts[device_index]


def train_dropout_params(module, seed, segment_base=0):
    """The dropout of one train call from a decoder's `dropout` / `dropout_prob`: (layer_mask, threshold, scale)
    with threshold = min(2^32 - 1, floor(p * 2^32)) and scale = float32(1 / (1 - p)), both from double arithmetic. None when nothing is
    dropped: the module in eval mode, p == 0 or an empty list. ValueError for p outside [0, 1) and a layer outside 0..7. `seed` and
    `segment_base` are checked here and travel separately (train_forward(..., dropout=(mask, threshold, scale, seed, segment_base)))."""
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError('dropout seed %r: an integer in 0 .. 2^64 - 1' % (seed,))
    if int(segment_base) < 0:
        raise ValueError('segment_base %r: >= 0' % (segment_base,))
    layers = getattr(module, 'dropout', None)
    p = float(getattr(module, 'dropout_prob', 0.0) or 0.0)
    layers = [] if layers is None else [int(l) for l in layers]
    if not 0.0 <= p < 1.0:
        raise ValueError('dropout_prob %r: 0 <= p < 1' % (p,))
    mask = 0
    for l in layers:
        if not 0 <= l <= 7:
            raise ValueError('dropout layer %d: this decoder has relu outputs lin0..lin7' % l)
        mask |= 1 << l
    if not module.training or p == 0.0 or mask == 0:
        return None
    threshold = min((1 << 32) - 1, int(np.floor(np.float64(p) * 4294967296.0)))
    return mask, threshold, float(np.float32(1.0 / (1.0 - np.float64(p))))


def draw_dropout_seed(generator=None):
    """A seed below 2^63 - 1 from torch's CPU generator (the default one, or `generator`): no device sync, reproducible under
    torch.manual_seed."""
    return int(torch.randint(0, (1 << 63) - 1, (1,), generator=generator, dtype=torch.int64, device='cpu').item())


def _train_dropout_struct(dropout, chunk_base=0):
    """dropout = None or (layer_mask, threshold, scale, seed, segment_base) -> distr_train_dropout (None: the plain calls)"""
    if dropout is None:
        return None
    mask, threshold, scale, seed, base = dropout
    return binding.TrainDropout(layer_mask=int(mask), threshold=int(threshold), scale=float(scale), seed=int(seed), segment_base=int(base) + int(chunk_base))


class TrainSaved(object):
    """What train_forward keeps for train_backward: the workspace with the saved layer inputs, and the call it belongs to."""

    def __init__(self, ctx, ws, net, counts, weights, lat, stride, clamp, dropout=None, grad=False):
        self.ctx, self.ws, self.net, self.counts = ctx, ws, net, list(counts)       # net: (L, lin3_rows, out_dim), the SDF decoder's too
        self.weights, self.lat, self.stride, self.clamp, self.dropout = weights, lat, stride, clamp, dropout
        self.grad = grad        # the workspace of train_grad_forward (section 8m): train_grad_backward follows, not train_backward
        self.latent_size, self.lin3_rows, self.out_dim = net
        self.seg_rows = train_segment_rows(counts)

    def call_args(self):
        """(distr_train_net*, nseg, counts_host) as every distr_train_net_* function takes them first"""
        return C.byref(_train_net_struct(self.weights, self.net)), len(self.counts), (C.c_int64 * len(self.counts))(*self.counts)

    def rows(self, s):
        """(first row, last row + 1) of segment s's points in the workspace (its padded rows follow)."""
        return self.seg_rows[s], self.seg_rows[s] + self.counts[s]

    def activations(self, layer):
        """(rows, width) f32 view of X_layer (1..8), the saved input of lin_layer = relu of lin_(layer-1); width 512, lin3_rows (the SDF
        decoder: 509 - C) for layer 4."""
        off = self.ctx.L.distr_train_net_activation_offset(*(self.call_args() + (int(layer),)))
        if not off:
            raise ValueError('layer %r: 1..8' % (layer,))
        R = self.seg_rows[-1]
        base = (-self.ws.data_ptr()) % 256
        x = self.ws[base + off: base + off + R * 512 * 4].view(torch.float32).reshape(R, 512)
        return x[:, :self.lin3_rows] if layer == 4 else x


def _train_net_struct(weights, net):
    """net = (L, lin3_rows, out_dim) -> distr_train_net on the eighteen tensors"""
    tn = binding.TrainNet(latent_size=int(net[0]), lin3_rows=int(net[1]), out_dim=int(net[2]))
    for l in range(9):
        tn.W[l] = weights[l].data_ptr()
        tn.b[l] = weights[9 + l].data_ptr()
    return tn


def train_net_shapes(net):
    """The eighteen shapes [W0..W8, b0..b8] a net description (L, lin3_rows, out_dim) implies (include/distr_train.h)."""
    L, n3, nout = (int(v) for v in net)
    W = [(512, L + 3), (512, 512), (512, 512), (n3, 512), (512, n3 + L + 3), (512, 512), (512, 512), (512, 512), (nout, 512)]
    return W + [(o,) for o, _ in W]


def train_forward(weights, latents, points, counts, clamp_dist=None, ws_bytes=None, dropout=None, ws=None, out=None, net=None, caller='train_forward',
                  grad=False):
    """Layer-wise decode of one segmented list of at most 64 segments (distr_train_net_forward): weights = [W0..W8, b0..b8] f32 device
    tensors, row-major; latents (S, C) or (1, C) shared; points (sum counts, 3). Returns (sdf (sum counts, 1), saved: TrainSaved).
    A workspace above DISTR_TRAIN_MAX_BYTES is refused (the message names `caller`). ws_bytes (tests): the workspace size to pass
    instead of the one needed. ws, out (tests): a uint8 device tensor to use as the workspace and an f32 (sum counts, 1) tensor for
    sdf, instead of fresh ones.
    dropout: None, or (layer_mask, threshold, scale, seed, segment_base) -- train_dropout_params(...) + (seed, global index of segment 0);
    the saved activations are then those behind the dropout, and train_backward follows.
    net: (L, lin3_rows, out_dim), the described network (the colour decoder is (256 + cs, 253, 3)): the weights
    have train_net_shapes(net), latents are (S, L) or (1, L), the output is (sum counts, out_dim), and a clamp belongs to out_dim 1.
    None = the SDF decoder, (C, 509 - C, 1) with the code length C of W0; a C outside 1..508 is refused here.
    grad: train_grad_forward's call (it documents it): no clamp, out = (sdf, grad), returns ((sdf, grad), saved)."""
    counts = [int(c) for c in counts]
    dev = points.device
    if dev.type != 'cuda':
        raise RuntimeError('train_forward: tensors must be on the GPU (no CPU path in this build)')
    if not 1 <= len(counts) <= binding.MAX_SEGMENTS:
        raise ValueError('%d segments: one train_forward call takes 1..%d' % (len(counts), binding.MAX_SEGMENTS))
    ctx = _train_context(dev.index if dev.index is not None else torch.cuda.current_device())
    weights = [_f32c(t, dev) for t in weights]
    if net is None:
        C_len = weights[0].shape[1] - 3
        if not 1 <= C_len <= 508:
            raise binding.DistrError('train_forward: latent_size %d: 1..508 (the SDF decoder is the network (C, 509 - C, 1))' % C_len)
        net = (C_len, 509 - C_len, 1)
    net = tuple(int(v) for v in net)
    if len(net) != 3:
        raise ValueError('net %r: (L, lin3_rows, out_dim)' % (net,))
    if len(weights) != 18 or [tuple(t.shape) for t in weights] != train_net_shapes(net):
        raise ValueError('net (L, lin3_rows, out_dim) = %r takes W0..W8, b0..b8 of shapes %r, got %r'
                         % (net, train_net_shapes(net), [tuple(t.shape) for t in weights]))
    C_len, nout = net[0], net[2]
    lat = _f32c(latents, dev).reshape(-1, C_len)
    if lat.shape[0] not in (1, len(counts)):
        raise ValueError('latents have shape %s; %d segments take (%d, %d) or (1, %d)' % (tuple(latents.shape), len(counts), len(counts), C_len, C_len))
    x = _f32c(points, dev).reshape(-1, 3)
    if x.shape[0] != sum(counts):
        raise ValueError('counts sum to %d, but there are %d points' % (sum(counts), x.shape[0]))
    stride = 0 if lat.shape[0] == 1 else C_len
    if grad and (nout != 1 or clamp_dist is not None):
        raise ValueError('%s: the spatial gradient belongs to a net with out_dim 1 (got %d) and takes no clamp (got %r)' % (caller, nout, clamp_dist))
    saved = TrainSaved(ctx, ws, net, counts, weights, lat, stride, clamp_dist, dropout, grad)
    need = (ctx.L.distr_train_grad_workspace_bytes if grad else ctx.L.distr_train_net_workspace_bytes)(*saved.call_args())
    if not need:
        raise ValueError('net (L, lin3_rows, out_dim) = %r: L >= 1, lin3_rows in 1..509, out_dim 1 or 3' % (net,))
    if grad and need > train_max_bytes():
        raise binding.DistrError('%s: %d points need a workspace of %d bytes (40 KB per point -- the layer inputs and the tangents -- and the slabs '
                                 'of the weight gradients), more than DISTR_TRAIN_MAX_BYTES = %d; split the batch (the sum order of a gradient '
                                 'follows the batch)' % (caller, x.shape[0], need, train_max_bytes()))
    if need > train_max_bytes():
        raise binding.DistrError('%s: %d points need a workspace of %d bytes (24 KB per point and the slabs of the weight gradients), '
                                 'more than DISTR_TRAIN_MAX_BYTES = %d; split the batch (the sum order of a gradient follows the batch)'
                                 % (caller, x.shape[0], need, train_max_bytes()))
    if ws is None:
        ws = saved.ws = torch.empty(need if ws_bytes is None else ws_bytes, dtype=torch.uint8, device=dev)
    if grad:
        sdf, gx = (torch.empty(x.shape[0], 1, dtype=torch.float32, device=dev), torch.empty(x.shape[0], 3, dtype=torch.float32, device=dev)) if out is None else out
        if ws.dtype != torch.uint8 or not ws.is_contiguous() or any(t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != x.shape[0] * k
                                                                    for t, k in ((sdf, 1), (gx, 3))):
            raise ValueError('train_grad_forward: ws is a contiguous uint8 tensor, out contiguous f32 tensors of %d and %d values' % (x.shape[0], 3 * x.shape[0]))
        td = _train_dropout_struct(dropout)
        ctx.check(ctx.L.distr_train_grad_forward(*((ctx.h,) + saved.call_args() + (binding.ptr(lat), stride, binding.ptr(x), binding.ptr(sdf), binding.ptr(gx),
                                                                                    binding.ptr(ws), ws.numel(), ctx.stream(), None if td is None else C.byref(td)))))
        return (sdf, gx), saved
    if out is None:
        out = torch.empty(x.shape[0], nout, dtype=torch.float32, device=dev)
    if ws.dtype != torch.uint8 or not ws.is_contiguous() or out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != x.shape[0] * nout:
        raise ValueError('train_forward: ws is a contiguous uint8 tensor, out a contiguous f32 tensor of %d values' % (x.shape[0] * nout))
    p = binding.ptr
    td = _train_dropout_struct(dropout)
    ctx.check(ctx.L.distr_train_net_forward(*((ctx.h,) + saved.call_args() + (p(lat), stride, p(x), _clamp_arg(clamp_dist), p(out), p(ws), ws.numel(), ctx.stream(),
                                                                               None if td is None else C.byref(td)))))
    return out, saved


def train_backward(saved, g_sdf, out=None):
    """Backward of train_forward (distr_train_net_backward): g_sdf (sum counts, out_dim) -> ([g_W0..g_W8, g_b0..g_b8], g_latent (S, C):
    one row per segment, also for a shared code). out (tests): (the eighteen gradient tensors, g_latent) to write into instead of fresh
    ones."""
    ctx, dev = saved.ctx, saved.ws.device
    if saved.grad:
        raise ValueError('train_backward: this workspace belongs to train_grad_forward; its backward is train_grad_backward')
    gs = _f32c(g_sdf, dev).reshape(-1)
    if gs.numel() != sum(saved.counts) * saved.out_dim:
        raise ValueError('g_sdf has %d entries for %d points of %d channel(s)' % (gs.numel(), sum(saved.counts), saved.out_dim))
    grads, g_lat, tg = _train_grad_tensors(saved, out, 'train_backward')
    p = binding.ptr
    td = _train_dropout_struct(saved.dropout)
    ctx.check(ctx.L.distr_train_net_backward(*((ctx.h,) + saved.call_args() + (p(saved.lat), saved.stride, p(gs), _clamp_arg(saved.clamp), p(saved.ws), C.byref(tg),
                                                                                p(g_lat), ctx.stream(), None if td is None else C.byref(td)))))
    return grads, g_lat


def _train_grad_tensors(saved, out, name):
    """(the eighteen gradient tensors, g_latent (S, C), distr_train_grads on them) of a backward call: fresh ones, or `out` checked"""
    dev = saved.ws.device
    if out is None:
        grads = [torch.empty_like(w) for w in saved.weights]
        g_lat = torch.empty(len(saved.counts), saved.latent_size, dtype=torch.float32, device=dev)
    else:
        grads, g_lat = out
        if [(g.shape, g.dtype, g.is_contiguous()) for g in grads] != [(w.shape, torch.float32, True) for w in saved.weights] \
                or (g_lat.shape, g_lat.dtype, g_lat.is_contiguous()) != ((len(saved.counts), saved.latent_size), torch.float32, True):
            raise ValueError('%s: out is (eighteen contiguous f32 tensors of the weights\' shapes, g_latent (S, C))' % name)
    tg = binding.TrainGrads()
    for l in range(9):
        tg.g_W[l] = grads[l].data_ptr()
        tg.g_b[l] = grads[9 + l].data_ptr()
    return grads, g_lat, tg


def train_grad_forward(weights, latents, points, counts, ws_bytes=None, dropout=None, ws=None, out=None, caller='train_grad_forward'):
    """f AND its spatial gradient g = grad_x f on the layer-wise path, for losses that reach the weights through g (DESIGN.md section
    8m; distr_train_grad_forward): arguments as train_forward for the SDF decoder. Returns ((sdf (sum counts, 1), grad (sum counts, 3)),
    saved). sdf is tanh(z) without a clamp, grad the true gradient (not decode_sdf_gradient's 3 x, no clamp mask). The workspace takes
    40 KB per point; out (tests): (sdf, grad) tensors to write into."""
    return train_forward(weights, latents, points, counts, None, ws_bytes=ws_bytes, dropout=dropout, ws=ws, out=out, caller=caller, grad=True)


def train_grad_backward(saved, g_sdf, g_grad, out=None):
    """Backward of train_grad_forward (distr_train_grad_backward), ONE pass for both upstreams: g_sdf = dL/df (sum counts, 1) and
    g_grad = dL/dg (sum counts, 3), either may be None (zero) -> ([g_W0..g_W8, g_b0..g_b8], g_latent (S, C)) as train_backward. May be
    called again on the same `saved`."""
    ctx, dev = saved.ctx, saved.ws.device
    if not saved.grad:
        raise ValueError('train_grad_backward: this workspace belongs to train_forward; its backward is train_backward')
    n = sum(saved.counts)
    ups = []
    for name, g, k in (('g_sdf', g_sdf, 1), ('g_grad', g_grad, 3)):
        g = None if g is None else _f32c(g, dev).reshape(-1)
        if g is not None and g.numel() != n * k:
            raise ValueError('%s has %d entries for %d points of %d component(s)' % (name, g.numel(), n, k))
        ups.append(g)
    grads, g_lat, tg = _train_grad_tensors(saved, out, 'train_grad_backward')
    p = lambda t: None if t is None else binding.ptr(t)
    td = _train_dropout_struct(saved.dropout)
    ctx.check(ctx.L.distr_train_grad_backward(*((ctx.h,) + saved.call_args() + (p(saved.lat), saved.stride, p(ups[0]), p(ups[1]), p(saved.ws), C.byref(tg), p(g_lat),
                                                                                 ctx.stream(), None if td is None else C.byref(td)))))
    return grads, g_lat


def _add_in_order(total, grads):
    """THE accumulator of the weight gradients of several train calls: the first call's tensors, then `a += b` in call order."""
    if total is None:
        return grads
    for a, b in zip(total, grads):
        a += b
    return total


def _eighteen(weights):
    if len(weights) != 18:
        raise ValueError('expected W0..W8, b0..b8: 18 tensors, got %d' % len(weights))


def _train_chunks_forward(ctx, weights, lat, points, counts, clamp_dist, dropout, net, caller, grad=False):
    """The forward the train nodes share: code rows `lat` (S, L) or (1, L), more than 64 segments in chunks of 64 (a chunk's
    segment_base is the dropout's + its first segment); keeps every chunk's TrainSaved on ctx for _train_chunks_backward.
    grad: train_grad_forward's chunks, -> (sdf, grad)."""
    counts = [int(c) for c in counts]
    x = points.detach().reshape(-1, 3)
    outs, ctx.saved_chunks = [], []
    for s0, ns, p0, row, stride in _multi_chunks(lat, segment_plan(counts)):
        n = sum(counts[s0:s0 + ns])
        drop = None if dropout is None else tuple(dropout[:4]) + (int(dropout[4]) + s0,)
        out, saved = train_forward(weights, lat[row:row + (ns if stride else 1)], x[p0:p0 + n], counts[s0:s0 + ns], clamp_dist, dropout=drop, net=net, caller=caller,
                                   grad=grad)
        outs.append(out)
        ctx.saved_chunks.append((saved, p0, n))
    if grad:
        return outs[0] if len(outs) == 1 else tuple(torch.cat(part) for part in zip(*outs))
    return outs[0] if len(outs) == 1 else torch.cat(outs)


def _train_chunks_backward(ctx, g, g_grad=None):
    """The backward the train nodes share: the upstream gradient of the output -> (the eighteen weight gradients, the chunks' added in
    chunk order; the code-gradient rows (S, L)). Chunks of train_grad_forward: g and g_grad are the upstreams of (sdf, grad), None = 0."""
    grad = ctx.saved_chunks[0][0].grad
    g = None if g is None else g.reshape(-1, ctx.saved_chunks[0][0].out_dim)
    g_grad = None if g_grad is None else g_grad.reshape(-1, 3)
    total, rows = None, []
    for saved, p0, n in ctx.saved_chunks:
        if grad:
            grads, g_lat = train_grad_backward(saved, None if g is None else g[p0:p0 + n], None if g_grad is None else g_grad[p0:p0 + n])
        else:
            grads, g_lat = train_backward(saved, g[p0:p0 + n])
        rows.append(g_lat)
        total = _add_in_order(total, grads)
    return total, (rows[0] if len(rows) == 1 else torch.cat(rows))


class DecodeSdfTrainFunction(torch.autograd.Function):
    """decode_sdf on the layer-wise path with autograd to the codes AND the eighteen weight tensors: (codes (S, C) or (1, C), flat points
    (sum counts, 3), counts, clamp, W0..W8, b0..b8) -> (sum counts, 1). The forward keeps the workspaces (the layer inputs) for the
    backward. More than 64 segments run in chunks of 64; the weight gradients of the chunks are added in chunk order. Points are data.
    dropout: None or (layer_mask, threshold, scale, seed, segment_base); a chunk's segment_base is segment_base + its first segment."""

    @staticmethod
    def forward(ctx, codes, points, counts, clamp_dist, dropout, *weights):
        _eighteen(weights)
        lat = codes.detach().reshape(-1, weights[0].shape[1] - 3)
        ctx.codes_shape, ctx.shared = codes.shape, lat.shape[0] == 1
        return _train_chunks_forward(ctx, weights, lat, points, counts, clamp_dist, dropout, None, 'decode_sdf_train')

    @staticmethod
    def backward(ctx, g):
        total, g_rows = _train_chunks_backward(ctx, g)
        g_codes = (g_rows.sum(0) if ctx.shared and g_rows.shape[0] > 1 else g_rows).reshape(ctx.codes_shape)
        return (g_codes, None, None, None, None) + tuple(total)


def decode_sdf_train_call(weights, codes, points, counts, clamp_dist=None, dropout=None):
    return DecodeSdfTrainFunction.apply(codes, points, counts, clamp_dist, dropout, *weights)


class DecodeSdfGradientTrainFunction(torch.autograd.Function):
    """(sdf, grad_x sdf) on the layer-wise path with autograd to the codes AND the eighteen weight tensors THROUGH BOTH outputs (DESIGN.md
    section 8m): (codes (S, C) or (1, C), flat points (sum counts, 3), counts, dropout, W0..W8, b0..b8) -> ((sum counts, 1), (sum counts,
    3)). The backward receives both upstreams and makes one pass for them (an output that no loss uses arrives as None: zero). Chunks,
    dropout and points as DecodeSdfTrainFunction; no clamp. The ReLU's second derivative is zero, as in torch."""

    @staticmethod
    def forward(ctx, codes, points, counts, dropout, *weights):
        _eighteen(weights)
        lat = codes.detach().reshape(-1, weights[0].shape[1] - 3)
        ctx.codes_shape, ctx.shared = codes.shape, lat.shape[0] == 1
        ctx.set_materialize_grads(False)
        return _train_chunks_forward(ctx, weights, lat, points, counts, None, dropout, None, 'decode_sdf_gradient_train', grad=True)

    @staticmethod
    def backward(ctx, g_f, g_g):
        total, g_rows = _train_chunks_backward(ctx, g_f, g_g)
        g_codes = (g_rows.sum(0) if ctx.shared and g_rows.shape[0] > 1 else g_rows).reshape(ctx.codes_shape)
        return (g_codes, None, None, None) + tuple(total)


def decode_sdf_gradient_train_call(weights, codes, points, counts, dropout=None):
    return DecodeSdfGradientTrainFunction.apply(codes, points, counts, dropout, *weights)


class _CodeLayout(object):
    """What color_code_rows needs of an engine, without one: the code length of the colour net and the device."""

    def __init__(self, latent_size, device):
        self.latent_size, self.device = latent_size, device


def color_train_net(weights):
    """(L, lin3_rows, out_dim) = (256 + cs, 253, 3) of the colour decoder whose W0 is weights[0]."""
    return int(weights[0].shape[1]) - 3, 253, 3


class DecodeColorTrainFunction(torch.autograd.Function):
    """decode_color on the layer-wise path with autograd to both codes AND the eighteen weight tensors:
    (color_codes (S, cs) or (1, cs), shape_codes (S, 256) or (1, 256), flat points (sum counts, 3), counts, dropout, W0..W8, b0..b8) ->
    (sum counts, 3). The code rows are [shape | colour] as color_code_rows builds them. More than 64 segments run in chunks of 64; the
    weight gradients of the chunks are added in chunk order. The code gradient rows are split into the two codes; the rows of a shared
    code are summed in segment order. Points are data. dropout as DecodeSdfTrainFunction: the segment is the index into the code rows."""

    @staticmethod
    def forward(ctx, color_codes, shape_codes, points, counts, dropout, *weights):
        _eighteen(weights)
        net = color_train_net(weights)
        lat = color_code_rows(_CodeLayout(net[0], points.device), color_codes.detach(), shape_codes.detach(), len(counts))
        ctx.code_like = (color_codes.detach(), shape_codes.detach())
        ctx.need = (color_codes.requires_grad, shape_codes.requires_grad)
        return _train_chunks_forward(ctx, weights, lat, points, counts, None, dropout, net, 'decode_color_train')

    @staticmethod
    def backward(ctx, g):
        total, g_rows = _train_chunks_backward(ctx, g)
        g_c, g_s = _split_code_grad(g_rows, *ctx.code_like)
        return ((g_c if ctx.need[0] else None), (g_s if ctx.need[1] else None), None, None, None) + tuple(total)


def decode_color_train_call(weights, color_codes, shape_codes, points, counts, dropout=None):
    return DecodeColorTrainFunction.apply(color_codes, shape_codes, points, counts, dropout, *weights)


# ---- weight gradients through render: the backward's sample list on the layer-wise path (include/distr_render_train.h)
def render_samples(engine, cfg, ws, ws_b, B, want_src=False):
    """distr_render_samples_export_batch on the forward workspace `ws` and the backward workspace `ws_b` as distr_render_backward_batch
    of B views of `cfg` left them (tests and tools; render_weight_grads): -> (xyz (B, cap, 3), coef (B, cap), src (B, cap) int32 or None,
    counts_dev (B,) int32 on the device), cap = distr_render_max_samples(cfg). View v's list is its first counts_dev[v] rows; the rows
    behind them are not written (uninitialised memory)."""
    dev = engine.device
    cap = int(engine.ctx.L.distr_render_max_samples(C.byref(cfg)))
    if cap <= 0:
        raise ValueError('render_samples: a cfg the render calls refuse')
    xyz = torch.empty(B, cap, 3, dtype=torch.float32, device=dev)
    coef = torch.empty(B, cap, dtype=torch.float32, device=dev)
    src = torch.empty(B, cap, dtype=torch.int32, device=dev) if want_src else None
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    p = binding.ptr
    engine.ctx.check(engine.ctx.L.distr_render_samples_export_batch(
        engine.ctx.h, C.byref(cfg), B, p(ws), ws.numel(), p(ws_b), ws_b.numel(), p(xyz), p(coef), p(src), cap, p(counts), engine.ctx.stream()))
    return xyz, coef, src, counts


def train_plan_bytes(counts, out_dim=1):
    """Workspace bytes of one train_forward call on segments of `counts` points: distr_train_net_workspace_bytes on a description with
    that out_dim (host code of the library, no GPU; a function of the counts and out_dim alone -- the code length and lin3's rows do
    not enter the size, so fixed legal ones stand in). About 20 KB per 64-padded row and the slabs of the weight gradients; the three
    per-row arrays z, tanh, dz have out_dim floats per row. ValueError for a list or an out_dim the calls refuse."""
    counts = [int(c) for c in counts]
    net = binding.TrainNet(latent_size=256, lin3_rows=253, out_dim=int(out_dim))
    need = int(binding.lib().distr_train_net_workspace_bytes(C.byref(net), len(counts), (C.c_int64 * len(counts))(*counts)))
    if not need:
        raise ValueError('train_plan_bytes: %d segments of %r points, out_dim %r: not a list of one train call' % (len(counts), counts[:4], out_dim))
    return need


def render_train_chunks(counts, max_bytes, out_dim=1):
    """The plan of the train calls over the sample lists of B views: counts[v] rows per view -> a list of pieces, each a list of segments
    (view, first row, rows). Every piece fits max_bytes (train_plan_bytes of its segments' rows, for a net of out_dim outputs: 1 the SDF
    decoder, 3 the colour decoder) and has at most 64 segments; a view's list is cut only at multiples of 64 rows from its start (whole
    tiles of the train path: a cut moves no row to another tile); views without rows get no segment; pieces and segments follow the
    view order. A function of the counts, the limit and out_dim alone: the same inputs give the same plan, and so the same bytes.
    ValueError when not even 64 rows fit the limit."""
    counts = [int(c) for c in counts]
    if min(counts + [0]) < 0:
        raise ValueError('counts must be >= 0, got %r' % (counts,))
    max_bytes = int(max_bytes)
    pieces, cur = [], []
    for v, c in enumerate(counts):
        at = 0
        while at < c:
            have = [n for _, _, n in cur]
            left = c - at
            fits = lambda n: train_plan_bytes(have + [n], out_dim) <= max_bytes
            if len(cur) < binding.MAX_SEGMENTS and fits(min(left, TRAIN_ROW_TILE)):
                if fits(left):
                    n = left
                else:               # the most whole tiles that fit (bytes grow with the rows)
                    lo, hi = 1, -(-left // TRAIN_ROW_TILE)          # lo tiles fit, hi tiles do not
                    while hi - lo > 1:
                        mid = (lo + hi) // 2
                        lo, hi = (mid, hi) if fits(mid * TRAIN_ROW_TILE) else (lo, mid)
                    n = lo * TRAIN_ROW_TILE
                cur.append((v, at, n))
                at += n
            elif cur:
                pieces.append(cur)
                cur = []
            else:
                raise ValueError('render_train_chunks: %d bytes do not hold one tile of 64 samples (%d bytes)'
                                 % (max_bytes, train_plan_bytes([TRAIN_ROW_TILE], out_dim)))
    if cur:
        pieces.append(cur)
    return pieces


def render_weight_grads(engine, cfg, ws, ws_b, B, weights, codes, max_bytes=None, want_latent=True):
    """Weight gradients of one render backward: dL/dW_l, dL/db_l = sum over the backward's sample list of coef * d f / d(W_l, b_l)
    (DESIGN.md section 8h). ws / ws_b: the workspaces as distr_render_backward_batch of B views left them; weights: W0..W8, b0..b8 as the
    engine packed them; codes (1, C) shared or (B, C). Exports the list, READS THE B COUNTS ON THE HOST (one sync), cuts the views' rows
    into train calls (render_train_chunks under DISTR_TRAIN_MAX_BYTES or max_bytes), runs train_forward / train_backward per piece and
    adds the pieces' gradients in piece order. -> ([g_W0..g_W8, g_b0..g_b8], g_latent (B, C): the layer-wise code gradient of every
    view, the sum of its segments' rows in order -- a cross-check of the fused g_latent, which is the one autograd returns; None
    without want_latent)."""
    xyz, coef, _, counts_dev = render_samples(engine, cfg, ws, ws_b, B)
    counts = [int(c) for c in counts_dev.cpu().tolist()]
    weights = [_f32c(w, engine.device) for w in weights]
    lat = _f32c(codes, engine.device).reshape(-1, engine.latent_size)
    total = None
    g_lat = torch.zeros(B, engine.latent_size, dtype=torch.float32, device=engine.device) if want_latent else None
    for piece in render_train_chunks(counts, train_max_bytes() if max_bytes is None else max_bytes):
        pts = torch.cat([xyz[v, a:a + n] for v, a, n in piece])
        cf = torch.cat([coef[v, a:a + n] for v, a, n in piece])
        seg_codes = lat if lat.shape[0] == 1 else lat[[v for v, _, _ in piece]]
        _, saved = train_forward(weights, seg_codes, pts, [n for _, _, n in piece], clamp_dist=None)
        grads, rows = train_backward(saved, cf)
        del saved
        total = _add_in_order(total, grads)
        if want_latent:
            for (v, _, _), row in zip(piece, rows):
                g_lat[v] += row
    return (total if total is not None else [torch.zeros_like(w) for w in weights]), g_lat


def depth_samples_count(engine, cfg, depth):
    """Valid pixels (0 < depth < 1e5) of V depth maps (V, H, W), compacted on the GPU in row-major order (distr_depth_samples_count: a
    fixed-order scan, one host read). Returns (depth as the f32 device tensor the kernels read, index (V, H*W) int32 whose first
    counts[v] entries of row v are the valid pixels of view v, counts: list of V ints)."""
    dev = engine.device
    d = _f32c(depth, dev).reshape(-1, cfg.H * cfg.W)
    V = d.shape[0]
    L, p = engine.ctx.L, binding.ptr
    nb = C.c_size_t()
    engine.ctx.check(L.distr_depth_samples_workspace_bytes(engine.ctx.h, C.byref(cfg), V, None, C.byref(nb), None, None))
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    index = torch.empty(V, cfg.H * cfg.W, dtype=torch.int32, device=dev)
    counts = (C.c_int64 * V)()
    engine.ctx.check(L.distr_depth_samples_count(engine.ctx.h, C.byref(cfg), V, p(d), p(index), counts, p(ws), ws.numel(), engine.ctx.stream()))
    return d, index, [int(c) for c in counts]


class DepthSamplesFunction(torch.autograd.Function):
    """SDFRenderer_deepsdf.get_samples / get_freespace_samples (core/sdfrenderer/renderer_deepsdf.py:14-64) of V views as one node:
    (latent (1,C) shared or (V,C), RT (V,3,4)) -> the list of distr_depth_samples_forward (include/distr_samples.h: per view
    [pos | neg] or [draw][pixel]). `obs` = (depth, normal or None, draws, index, counts): observations and random draws, no gradient.
    backward = distr_depth_samples_backward: g_latent (summed over the views of a shared code), g_RT."""

    @staticmethod
    def forward(ctx, latent, RT, engine, cfg, obs):
        depth, normal, draws, index, counts = obs
        dev = engine.device
        V = len(counts)
        lat = _code(engine, latent, dev, views=True)
        if lat.shape[0] not in (1, V):
            raise ValueError('latent has shape %s; %d views take (1, %d) or (%d, %d)' % (tuple(latent.shape), V, engine.latent_size, V, engine.latent_size))
        rt = _f32c(RT, dev).reshape(V, 3, 4)
        m = 2 if cfg.mode == binding.SAMPLES_MODES['surface'] else cfg.number
        n = m * sum(counts)
        L, p = engine.ctx.L, binding.ptr
        cnt = (C.c_int64 * V)(*counts)
        fb, bb = C.c_size_t(), C.c_size_t()
        engine.ctx.check(L.distr_depth_samples_workspace_bytes(engine.ctx.h, C.byref(cfg), V, cnt, None, C.byref(fb), C.byref(bb)))
        xyz = torch.empty(n, 3, dtype=torch.float32, device=dev)
        out = torch.empty(n, dtype=torch.float32, device=dev)
        ws = torch.empty(fb.value, dtype=torch.uint8, device=dev)
        stride = 0 if lat.shape[0] == 1 else engine.latent_size
        engine.ctx.check(L.distr_depth_samples_forward(engine.ctx.h, C.byref(cfg), V, cnt, p(index), p(lat), stride, p(rt), p(depth), p(normal),
                                                       p(draws), p(xyz), p(out), p(ws), ws.numel(), engine.ctx.stream()))
        ctx.engine, ctx.cfg, ctx.obs, ctx.cnt, ctx.stride, ctx.bwd_bytes = engine, cfg, obs, cnt, stride, bb.value
        ctx.shapes = (latent.shape, RT.shape)
        ctx.need = (latent.requires_grad, RT.requires_grad)
        ctx.save_for_backward(lat, rt, xyz)
        ctx.mark_non_differentiable(xyz)
        return out, xyz

    @staticmethod
    def backward(ctx, g_out, _g_xyz):
        engine, cfg = ctx.engine, ctx.cfg
        depth, normal, draws, index, counts = ctx.obs
        lat, rt, xyz = ctx.saved_tensors
        dev = engine.device
        V = len(counts)
        g = _f32c(g_out, dev).reshape(-1)
        g_l = torch.empty(V, engine.latent_size, dtype=torch.float32, device=dev) if ctx.need[0] else None
        g_rt = torch.empty(V, 3, 4, dtype=torch.float32, device=dev) if ctx.need[1] else None
        ws = torch.empty(ctx.bwd_bytes, dtype=torch.uint8, device=dev)
        L, p = engine.ctx.L, binding.ptr
        engine.ctx.check(L.distr_depth_samples_backward(engine.ctx.h, C.byref(cfg), V, ctx.cnt, p(index), p(lat), ctx.stride, p(rt), p(depth), p(draws),
                                                        p(xyz), p(g), p(g_l), p(g_rt), p(ws), ws.numel(), engine.ctx.stream()))
        if g_l is not None:
            g_l = (g_l.sum(0) if ctx.stride == 0 and V > 1 else g_l).reshape(ctx.shapes[0])
        return g_l, (None if g_rt is None else g_rt.reshape(ctx.shapes[1])), None, None, None


def _samples_list(engine, cfg, latent, RT, obs):
    out, xyz = DepthSamplesFunction.apply(latent, RT, engine, cfg, obs)
    counts = obs[4]
    m = 2 if cfg.mode == binding.SAMPLES_MODES['surface'] else cfg.number
    return list(torch.split(out, [m * c for c in counts])), xyz


def samples_call(engine, cfg, latent, RT, depth, normal, eta_map, index, counts):
    """get_samples of V views: eta_map = sum(counts) floats (view after view). Returns ([(samples_pos (N_v,), samples_neg (N_v,))
    per view], the point list (2 sum N, 3) the decoder saw, without gradient)."""
    dev = engine.device
    obs = (depth, _f32c(normal, dev).reshape(len(counts), -1), _f32c(eta_map, dev).reshape(-1), index, counts)
    if obs[2].numel() != sum(counts) or obs[1].shape[1] != 3 * cfg.H * cfg.W:
        raise ValueError('eta_map needs %d entries (one per valid pixel), normal (%d, %d, %d, 3)' % (sum(counts), len(counts), cfg.H, cfg.W))
    per_view, xyz = _samples_list(engine, cfg, latent, RT, obs)
    return [tuple(torch.split(o, [c, c])) for o, c in zip(per_view, counts)], xyz


def freespace_call(engine, cfg, latent, RT, depth, ratio, index, counts):
    """get_freespace_samples of V views: ratio = number * sum(counts) floats (per view [draw][pixel]). Returns ([samples
    (number * N_v,) per view], the point list)."""
    dev = engine.device
    obs = (depth, None, _f32c(ratio, dev).reshape(-1), index, counts)
    if obs[2].numel() != cfg.number * sum(counts):
        raise ValueError('ratio needs number * N = %d entries' % (cfg.number * sum(counts)))
    return _samples_list(engine, cfg, latent, RT, obs)


def mlp_grad(engine, latent, points):
    """(sdf (n,), d sdf/d xyz (n,3)) of the unclamped decoder."""
    L, dev = engine.ctx.L, engine.device
    lat, x, n = _point_list(engine, latent, points)
    sdf = torch.empty(n, dtype=torch.float32, device=dev)
    g = torch.empty(n, 3, dtype=torch.float32, device=dev)
    _list_call(engine, L.distr_mlp_grad, L.distr_mlp_workspace_bytes, lat, x, n, sdf, g)
    return sdf, g


def debug_mlp_layer(engine, latent, points, layer):
    """Test aid: post-activation of hidden layer `layer` -> (n,512)."""
    L = engine.ctx.L
    lat, x, n = _point_list(engine, latent, points)
    out = torch.empty(n, 512, dtype=torch.float32, device=engine.device)
    _list_call(engine, L.distr_debug_mlp_layer, L.distr_mlp_workspace_bytes, lat, x, n, int(layer), out)
    return out


def debug_mlp_layer32(engine, latent, points, layer):
    """Test aid: debug_mlp_layer on 32-point tiles, as the step kernel's 32-ray role runs them (compacted or dense by the engine's knobs)."""
    L = engine.ctx.L
    lat, x, n = _point_list(engine, latent, points)
    out = torch.empty(n, 512, dtype=torch.float32, device=engine.device)
    _list_call(engine, L.distr_debug_mlp_layer32, L.distr_mlp_workspace_bytes, lat, x, n, int(layer), out)
    return out


def debug_tile_timing(engine, latent, points, tile):
    """Test aid: (sdf (n,), stamps (tiles, 20, 2) int64 [shader clock, 100 MHz wall clock]) of the decoder tile phases; tile = 64, or 32 for
    the 32-point tile of the step kernel's 32-ray role."""
    L, dev = engine.ctx.L, engine.device
    if tile not in (32, 64):
        raise ValueError('tile: 64 or 32')
    lat, x, n = _point_list(engine, latent, points)
    sdf = torch.empty(n, dtype=torch.float32, device=dev)
    ts = torch.zeros((n + tile - 1) // tile, 20, 2, dtype=torch.int64, device=dev)
    _list_call(engine, L.distr_debug_tile_timing if tile == 64 else L.distr_debug_tile_timing32, L.distr_mlp_workspace_bytes, lat, x, n, sdf, ts)
    return sdf, ts


# ------------------------------------------------------------------------------------------ fused losses (rows f2, f3)
def _u8c(t, device):
    t = t.detach().to(device=device)
    return (t if t.dtype == torch.uint8 else (t != 0).to(torch.uint8)).contiguous()


def _loss_ws(engine, H, W):
    return _ws(engine, engine.ctx.L.distr_loss_workspace_bytes, H, W)


class SingleViewLossFunction(torch.autograd.Function):
    """(depth (H,W), normal (H,W,3), min_sdf (H,W)) + constants -> losses[4] = (mask_gt, mask_out, depth, normal):
    distr_single_loss_forward / _backward (core/utils/loss_utils.py:59-172 in two element-wise kernels)."""

    @staticmethod
    def forward(ctx, depth, normal, min_sdf, engine, mask, gt_depth, gt_normal, gt_mask, threshold):
        dev = engine.device
        H, W = min_sdf.shape[0], min_sdf.shape[1]
        d, n, q = _f32c(depth, dev), _f32c(normal, dev), _f32c(min_sdf, dev)
        m, gm = _u8c(mask, dev), _u8c(gt_mask, dev)
        gd = None if gt_depth is None else _f32c(gt_depth, dev)
        gn = None if gt_normal is None else _f32c(gt_normal, dev)
        out8 = torch.empty(8, dtype=torch.float32, device=dev)
        ws = _loss_ws(engine, H, W)
        p = binding.ptr
        engine.ctx.check(engine.ctx.L.distr_single_loss_forward(engine.ctx.h, H, W, p(d), p(n), p(m), p(q), p(gd), p(gn), p(gm),
                                                               float(threshold), p(out8), p(ws), ws.numel(), engine.ctx.stream()))
        ctx.engine, ctx.hw, ctx.threshold = engine, (H, W), float(threshold)
        ctx.saved = (d, n, q, m, gd, gn, gm, out8)
        return out8[:4].clone()

    @staticmethod
    def backward(ctx, g):
        engine = ctx.engine
        d, n, q, m, gd, gn, gm, out8 = ctx.saved
        H, W = ctx.hw
        g4 = g.to(dtype=torch.float32).contiguous()
        g_d, g_n, g_q = torch.empty_like(d), torch.empty_like(n), torch.empty_like(q)
        p = binding.ptr
        engine.ctx.check(engine.ctx.L.distr_single_loss_backward(engine.ctx.h, H, W, p(d), p(n), p(m), p(q), p(gd), p(gn), p(gm),
                                                                ctx.threshold, p(out8), p(g4), p(g_d), p(g_n), p(g_q),
                                                                engine.ctx.stream()))
        return g_d, g_n, g_q, None, None, None, None, None, None


def single_view_losses(engine, depth, normal, mask, min_sdf, gt_depth, gt_normal, gt_mask, threshold):
    """-> tensor [mask_gt, mask_out, depth, normal] (terms whose ground truth is None are 0)."""
    return SingleViewLossFunction.apply(depth, normal, min_sdf, engine, mask, gt_depth, gt_normal, gt_mask, threshold)


class WarpLossFunction(torch.autograd.Function):
    """(Zdepth1 (P), R1, T1, R2, T2) + constants -> (loss_color, keep (P) uint8, color1 (H,W,3), color2 (H,W,3)):
    distr_warp_loss_forward / _backward (core/sdfrenderer/renderer_warp.py:18-101)."""

    @staticmethod
    def forward(ctx, z1, R1, T1, R2, T2, engine, wcfg, m1, z2, img1, img2):
        dev = engine.device
        H, W = wcfg.H, wcfg.W
        P = H * W
        z1c, z2c = _f32c(z1, dev).reshape(-1), _f32c(z2, dev).reshape(-1)
        m1c = _u8c(m1, dev).reshape(-1)
        i1, i2 = _f32c(img1, dev).reshape(-1), _f32c(img2, dev).reshape(-1)
        cams = [_f32c(t, dev).reshape(-1) for t in (R1, T1, R2, T2)]
        if z1c.numel() != P or i1.numel() != 3 * P or i2.numel() != 3 * P:
            raise ValueError('render_warp: image / depth sizes do not match img_hw')
        out3 = torch.empty(3, dtype=torch.float32, device=dev)
        keep = torch.empty(P, dtype=torch.uint8, device=dev)
        c1, c2 = torch.empty(H, W, 3, dtype=torch.float32, device=dev), torch.empty(H, W, 3, dtype=torch.float32, device=dev)
        ws = _loss_ws(engine, H, W)
        p = binding.ptr
        engine.ctx.check(engine.ctx.L.distr_warp_loss_forward(engine.ctx.h, C.byref(wcfg), p(z1c), p(m1c), p(z2c), p(i1), p(i2),
                                                             p(cams[0]), p(cams[1]), p(cams[2]), p(cams[3]), p(out3), p(keep),
                                                             p(c1), p(c2), p(ws), ws.numel(), engine.ctx.stream()))
        ctx.engine, ctx.wcfg = engine, wcfg
        ctx.saved = (z1c, m1c, z2c, i1, i2, cams, out3)
        ctx.shapes = (z1.shape, R1.shape, T1.shape, R2.shape, T2.shape)
        ctx.mark_non_differentiable(keep, c1, c2)
        return out3[0].clone(), keep, c1, c2

    @staticmethod
    def backward(ctx, g_loss, g_keep, g_c1, g_c2):
        engine, wcfg = ctx.engine, ctx.wcfg
        z1c, m1c, z2c, i1, i2, cams, out3 = ctx.saved
        dev = engine.device
        gl = g_loss.to(dtype=torch.float32).reshape(1).contiguous()
        g_z = torch.empty_like(z1c)
        g_cam = torch.empty(24, dtype=torch.float32, device=dev)
        ws = _loss_ws(engine, wcfg.H, wcfg.W)
        p = binding.ptr
        engine.ctx.check(engine.ctx.L.distr_warp_loss_backward(engine.ctx.h, C.byref(wcfg), p(z1c), p(m1c), p(z2c), p(i1), p(i2),
                                                              p(cams[0]), p(cams[1]), p(cams[2]), p(cams[3]), p(out3), p(gl),
                                                              p(g_z), p(g_cam), p(ws), ws.numel(), engine.ctx.stream()))
        zs, r1s, t1s, r2s, t2s = ctx.shapes
        return (g_z.reshape(zs), g_cam[0:9].reshape(r1s), g_cam[9:12].reshape(t1s), g_cam[12:21].reshape(r2s),
                g_cam[21:24].reshape(t2s), None, None, None, None, None, None)


def warp_loss(engine, wcfg, z1, m1, z2, img1, img2, R1, T1, R2, T2):
    return WarpLossFunction.apply(z1, R1, T1, R2, T2, engine, wcfg, m1, z2, img1, img2)


# ------------------------------------------------------------------------------------------ colour on a segmented list; the colour stage
SHAPE_CODE = 256        # code length of the shape decoder the colour path is built for (SDFRenderer_color refuses any other)


def color_code_rows(engine, color_codes, shape_codes, S):
    """[shape code | colour code] rows of S segments (or views) as one f32 device tensor: (S, 256 + cs), or (1, 256 + cs) when both
    codes are shared. Each of the two is (1, .) shared or (S, .); ValueError naming the expected shapes otherwise. Runs without a GPU
    on CPU tensors (engine: anything with latent_size and device)."""
    cs = engine.latent_size - SHAPE_CODE
    sc, cc = _f32c(shape_codes, engine.device), _f32c(color_codes, engine.device)
    ok = sc.dim() == 2 and cc.dim() == 2 and sc.shape[1] == SHAPE_CODE and cc.shape[1] == cs and sc.shape[0] in (1, S) and cc.shape[0] in (1, S)
    if not ok:
        raise ValueError('shape codes have shape %s and colour codes %s; %d segments take shape codes (1, %d) or (%d, %d) and colour codes '
                         '(1, %d) or (%d, %d)' % (tuple(shape_codes.shape), tuple(color_codes.shape), S, SHAPE_CODE, S, SHAPE_CODE, cs, S, cs))
    rows = max(sc.shape[0], cc.shape[0])
    return torch.cat([sc.expand(rows, -1), cc.expand(rows, -1)], 1).contiguous()


def _split_code_grad(g_rows, color_codes, shape_codes):
    """Rows [shape | colour] of a code gradient (one per segment) -> (g_color_codes, g_shape_codes) in the inputs' shapes; a shared
    code gets the sum of the rows (fixed order)."""
    def part(g, like):
        g = g.sum(0, keepdim=True) if like.shape[0] == 1 and g.shape[0] > 1 else g
        return g.reshape(like.shape).to(device=like.device, dtype=like.dtype)
    return part(g_rows[:, SHAPE_CODE:], color_codes), part(g_rows[:, :SHAPE_CODE], shape_codes)


def color_eval_multi(engine, color_codes, shape_codes, points, counts):
    """decode_color of a segmented point list: segment s = counts[s] consecutive rows of points (sum counts, 3), decoded with
    [shape_codes[s] | color_codes[s]] (each (S, .) or (1, .) shared) -> (sum counts, 3). One launch sequence per 64 segments
    (distr_color_eval_multi); every segment's slice is byte for byte color_eval of that segment alone."""
    L, p, dev = engine.ctx.L, binding.ptr, engine.device
    lat = color_code_rows(engine, color_codes, shape_codes, len(segment_plan(counts)['tiles']))
    return _multi_run(engine, lat, points, counts, L.distr_color_multi_workspace_bytes,
                      lambda n, S: torch.empty(n, 3, dtype=torch.float32, device=dev),
                      lambda head, tail, p0, s0, out: L.distr_color_eval_multi(*head, p(out[p0:]), *tail))


def color_backward_multi(engine, color_codes, shape_codes, points, counts, g_rgb, need_codes=True, need_points=True):
    """Backward of color_eval_multi for the upstream gradient g_rgb (sum counts, 3): (g_rows (S, 256 + cs): one [shape | colour] row per
    segment, also for shared codes (the caller sums), g_points (sum counts, 3)); either is None when not needed."""
    L, p, dev = engine.ctx.L, binding.ptr, engine.device
    lat = color_code_rows(engine, color_codes, shape_codes, len(segment_plan(counts)['tiles']))
    gs = _f32c(g_rgb, dev).reshape(-1, 3)

    def outputs(n, S):
        if gs.shape[0] != n:
            raise ValueError('g_rgb has %d rows for %d points' % (gs.shape[0], n))
        return (torch.empty(S, engine.latent_size, dtype=torch.float32, device=dev) if need_codes else None,
                torch.empty(n, 3, dtype=torch.float32, device=dev) if need_points else None)

    def call(head, tail, p0, s0, out):
        g_l, g_x = out
        return L.distr_color_backward_multi(*head, p(gs[p0:]), p(None if g_x is None else g_x[p0:]), p(None if g_l is None else g_l[s0:]), *tail)
    return _multi_run(engine, lat, points, counts, L.distr_color_backward_multi_workspace_bytes, outputs, call)


class ColorDecodeMultiFunction(torch.autograd.Function):
    """color_eval_multi with autograd: (color_codes, shape_codes, points (sum counts, 3)) -> (sum counts, 3); backward =
    distr_color_backward_multi. Row s of the code gradients is the stand-alone call's, bit for bit; a shared code gets the sum of the rows."""

    @staticmethod
    def forward(ctx, color_codes, shape_codes, points, engine, counts):
        out = color_eval_multi(engine, color_codes, shape_codes, points, counts)
        ctx.engine, ctx.counts = engine, [int(c) for c in counts]
        ctx.save_for_backward(color_codes.detach(), shape_codes.detach(), points.detach())
        ctx.need = (color_codes.requires_grad, shape_codes.requires_grad, points.requires_grad)
        return out

    @staticmethod
    def backward(ctx, g):
        color_codes, shape_codes, points = ctx.saved_tensors
        g_rows, g_x = color_backward_multi(ctx.engine, color_codes, shape_codes, points, ctx.counts, g, need_codes=ctx.need[0] or ctx.need[1],
                                           need_points=ctx.need[2])
        g_c, g_s = _split_code_grad(g_rows, color_codes, shape_codes) if g_rows is not None else (None, None)
        return (g_c if ctx.need[0] else None), (g_s if ctx.need[1] else None), (None if g_x is None else g_x.reshape(points.shape)), None, None


def color_eval_multi_autograd(engine, color_codes, shape_codes, points, counts):
    return ColorDecodeMultiFunction.apply(color_codes, shape_codes, points, engine, counts)


def color_lights(dev, sets, locations, energies):
    """Point lights of `sets` views (or frames) as the colour stage reads them: locations (M, 3) shared or (sets, M, 3), energies (M,) or
    (sets, M), default ones. Returns (locations, energies as f32 device tensors, binding.ColorLights), or (None, None, None) without
    lights. Lights and energies are observations: ValueError when one requires grad."""
    if locations is None:
        return None, None, None
    for name, t in (('lighting_locations', locations), ('lighting_energies', energies)):
        if t is not None and getattr(t, 'requires_grad', False):
            raise ValueError('%s requires grad: lights and energies are observations here, no gradient reaches them (detach them)' % name)
    loc = _f32c(locations, dev)
    if loc.dim() not in (2, 3) or loc.shape[-1] != 3 or loc.shape[-2] < 1 or (loc.dim() == 3 and loc.shape[0] != sets):
        raise ValueError('lighting_locations has shape %s; expected (M, 3) or (%d, M, 3)' % (tuple(locations.shape), sets))
    M = loc.shape[-2]
    en = torch.ones(M, dtype=torch.float32, device=dev) if energies is None else _f32c(energies, dev)
    if en.shape not in ((M,), (sets, M)):
        raise ValueError('lighting_energies has shape %s; expected (%d,) or (%d, %d)' % (tuple(en.shape), M, sets, M))
    st = binding.ColorLights()
    st.nlights = M
    st.locations_dev, st.location_stride = loc.data_ptr(), (3 * M if loc.dim() == 3 else 0)
    st.energies_dev, st.energy_stride = en.data_ptr(), (M if en.dim() == 2 else 0)
    return loc, en, st


def _stage_views(engine, cfg, R, T, zdepth, mask, normal, lit):
    dev = engine.device
    P = cfg.H * cfg.W
    Rc, Tc = _f32c(R, dev).reshape(-1, 9), _f32c(T, dev).reshape(-1, 3)
    B = Rc.shape[0]
    if Tc.shape[0] != B or not (1 <= B <= binding.MAX_VIEWS):
        raise ValueError('expected R (B,3,3), T (B,3) with 1 <= B <= %d' % binding.MAX_VIEWS)
    z, m = _f32c(zdepth, dev).reshape(-1), _u8c(mask, dev).reshape(-1)
    n = _f32c(normal, dev).reshape(-1) if lit else None
    if z.numel() != B * P or m.numel() != B * P or (lit and n.numel() != 3 * B * P):
        raise ValueError('expected zdepth / mask (%d, %d) and, with lights, normal (%d, %d, %d, 3)' % (B, P, B, cfg.H, cfg.W))
    return Rc, Tc, z, m, n, B, P


def color_stage_forward(engine, cfg, color_codes, shape_codes, R, T, zdepth, mask, normal=None, lights=None, energies=None, want_lists=False):
    """distr_color_stage_forward_batch: the colours of B rendered views in one launch sequence -> rgb (B, H, W, 3), zero off the mask,
    times the shading term when lights are given (then `normal` (B, H, W, 3) is read). Returns (rgb, saved): `saved` is what the
    backward needs; with want_lists it also holds 'index' (B, P) int32, 'xyz' (B, P, 3) and 'totals' (B,) int32 -- the compacted valid
    pixels of every view (its first totals[v] entries) and their surface points."""
    dev, L, p = engine.device, engine.ctx.L, binding.ptr
    lit = lights is not None
    Rc, Tc, z, m, n, B, P = _stage_views(engine, cfg, R, T, zdepth, mask, normal, lit)
    lat = color_code_rows(engine, color_codes, shape_codes, B)
    loc, en, st = color_lights(dev, B, lights, energies)
    fb, bb = C.c_size_t(), C.c_size_t()
    engine.ctx.check(L.distr_color_stage_workspace_bytes(engine.ctx.h, C.byref(cfg), B, C.byref(fb), C.byref(bb)))
    ws = torch.empty(fb.value, dtype=torch.uint8, device=dev)
    rgb = torch.empty(B, cfg.H, cfg.W, 3, dtype=torch.float32, device=dev)
    lists = {}
    if want_lists:
        lists = dict(index=torch.empty(B, P, dtype=torch.int32, device=dev), xyz=torch.empty(B, P, 3, dtype=torch.float32, device=dev),
                     totals=torch.empty(B, dtype=torch.int32, device=dev))
    stride = 0 if lat.shape[0] == 1 else engine.latent_size
    engine.ctx.check(L.distr_color_stage_forward_batch(
        engine.ctx.h, C.byref(cfg), B, p(Rc), p(Tc), p(z), p(m), p(n), p(lat), stride, None if st is None else C.byref(st), p(rgb), p(ws), ws.numel(),
        p(lists.get('index')), p(lists.get('xyz')), p(lists.get('totals')), engine.ctx.stream()))
    saved = dict(lists, ws=ws, bwd_bytes=bb.value, views=(Rc, Tc, z, n), lat=lat, stride=stride, lights=(loc, en, st), B=B, P=P)
    return rgb, saved


def color_stage_samples(engine, cfg, saved, ws_b):
    """distr_color_stage_samples_export_batch on `saved` (color_stage_forward's second value: it holds the forward workspace) and the
    backward workspace `ws_b` as distr_color_stage_backward_batch of the same views left it, having been given a g_latent_cat (tests and
    tools; color_stage_weight_grads): -> (xyz (B, P, 3), up (B, P, 3), index (B, P) int32, counts_dev (B,) int32 on the device). View
    v's list is its first counts_dev[v] rows: the surface points of its valid pixels in row-major order, the upstream g_rgb * s that
    reached the decoder there, and the pixels; the rows behind them are not written (uninitialised memory)."""
    dev, B, P = engine.device, saved['B'], saved['P']
    xyz = torch.empty(B, P, 3, dtype=torch.float32, device=dev)
    up = torch.empty(B, P, 3, dtype=torch.float32, device=dev)
    index = torch.empty(B, P, dtype=torch.int32, device=dev)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    p = binding.ptr
    engine.ctx.check(engine.ctx.L.distr_color_stage_samples_export_batch(
        engine.ctx.h, C.byref(cfg), B, p(saved['ws']), saved['ws'].numel(), p(ws_b), ws_b.numel(), p(xyz), p(up), p(index), P, p(counts),
        engine.ctx.stream()))
    return xyz, up, index, counts


def color_stage_weight_grads(engine, cfg, saved, ws_b, weights, max_bytes=None, want_latent=False):
    """Weight gradients of the colour decoder from one colour-stage backward: dL/dW_l, dL/db_l = sum over the valid pixels of every view
    of (g_rgb * s) . d rgb / d(W_l, b_l). saved / ws_b: see color_stage_samples; weights: W0..W8, b0..b8 of the
    colour decoder the engine was packed from. Exports the list, READS THE B COUNTS ON THE HOST (one sync: such a backward cannot be
    captured into a graph), cuts the views' rows into train calls (render_train_chunks with out_dim = 3 under DISTR_TRAIN_MAX_BYTES or
    max_bytes), runs train_forward / train_backward on the net color_train_net(weights) per piece, the code rows [shape | colour] being
    the stage's own, and adds the pieces' gradients in piece order. -> ([g_W0..g_W8, g_b0..g_b8], g_latent_cat (B, 256 + cs): the
    layer-wise code gradient of every view, a cross-check of the fused one, which is the one autograd returns; None without
    want_latent)."""
    _eighteen(weights)
    dev, B = engine.device, saved['B']
    weights = [_f32c(w, dev) for w in weights]
    net = color_train_net(weights)
    if net[0] != engine.latent_size:
        raise ValueError('the weights describe a colour decoder of code length %d, the engine holds one of %d' % (net[0], engine.latent_size))
    xyz, up, _, counts_dev = color_stage_samples(engine, cfg, saved, ws_b)
    counts = [int(c) for c in counts_dev.cpu().tolist()]
    lat = saved['lat']
    total = None
    g_lat = torch.zeros(B, engine.latent_size, dtype=torch.float32, device=dev) if want_latent else None
    for piece in render_train_chunks(counts, train_max_bytes() if max_bytes is None else max_bytes, out_dim=net[2]):
        pts = torch.cat([xyz[v, a:a + n] for v, a, n in piece])
        u = torch.cat([up[v, a:a + n] for v, a, n in piece])
        seg_codes = lat if lat.shape[0] == 1 else lat[[v for v, _, _ in piece]]
        _, sv = train_forward(weights, seg_codes, pts, [n for _, _, n in piece], net=net, caller='color_stage_weight_grads')
        grads, rows = train_backward(sv, u)
        del sv
        total = _add_in_order(total, grads)
        if want_latent:
            for (v, _, _), row in zip(piece, rows):
                g_lat[v] += row
    return (total if total is not None else [torch.zeros_like(w) for w in weights]), g_lat


class ColorStageFunction(torch.autograd.Function):
    """The colour stage of B rendered views as ONE node: (color_codes (1, cs) / (B, cs), shape_codes (1, 256) / (B, 256), R (B,3,3),
    T (B,3), normal (B,H,W,3) or None) + observations (zdepth, mask, lights, energies) -> rgb (B,H,W,3). backward =
    distr_color_stage_backward_batch: gradients to both codes (summed over the views of a shared code), the cameras and -- with lights --
    the normal image. detach_color: the colours are constants (render(no_grad=True)); only the shading terms carry gradient.
    `weights` (optional, trailing): W0..W8, b0..b8 of the colour decoder the engine was packed from
    (decoder_pack.effective_weights_torch_color) -- the backward then also returns their eighteen gradients (color_stage_weight_grads,
    DESIGN.md section 8j: ONE HOST SYNC per backward, so such a backward cannot be captured into a graph). The decoder backward then
    runs whether or not a code requires grad (it writes the upstream the list carries). The gradients of codes, cameras and the normal
    image are those of the fused backward; without weights every byte is what it was before the option existed."""

    @staticmethod
    def forward(ctx, color_codes, shape_codes, R, T, normal, engine, cfg, zdepth, mask, lights, energies, detach_color, *weights):
        if weights:
            _eighteen(weights)
            if detach_color:          # (the backward would export an upstream that was never written)
                raise ValueError('detach_color makes the colours constants: no gradient reaches the colour decoder, pass no weights')
        rgb, saved = color_stage_forward(engine, cfg, color_codes, shape_codes, R, T, zdepth, mask, normal, lights, energies)
        ctx.engine, ctx.cfg, ctx.saved, ctx.detach_color = engine, cfg, saved, bool(detach_color)
        ctx.nweights = len(weights)
        if weights:
            ctx.save_for_backward(*weights)
        ctx.generation = engine.generation
        ctx.codes = (color_codes.detach(), shape_codes.detach())
        ctx.shapes = (R.shape, T.shape, None if normal is None else normal.shape)
        ctx.in_meta = tuple((t.device, t.dtype) for t in (R, T)) + (None if normal is None else (normal.device, normal.dtype),)
        return rgb

    @staticmethod
    def backward(ctx, g):
        engine, cfg, sv = ctx.engine, ctx.cfg, ctx.saved
        _check_generation(ctx)
        dev, L, p = engine.device, engine.ctx.L, binding.ptr
        B, P = sv['B'], sv['P']
        Rc, Tc, z, n = sv['views']
        loc, en, st = sv['lights']
        need_c, need_s, need_R, need_T, need_n = ctx.needs_input_grad[:5]
        gs = _f32c(g, dev).reshape(-1)
        g_lat = torch.empty(B, engine.latent_size, dtype=torch.float32, device=dev) if (need_c or need_s or ctx.nweights) and not ctx.detach_color else None
        g_R = torch.empty(B, 9, dtype=torch.float32, device=dev) if need_R else None
        g_T = torch.empty(B, 3, dtype=torch.float32, device=dev) if need_T else None
        g_n = torch.empty(B, cfg.H, cfg.W, 3, dtype=torch.float32, device=dev) if need_n and st is not None else None
        ws_b = torch.empty(sv['bwd_bytes'], dtype=torch.uint8, device=dev)
        engine.ctx.check(L.distr_color_stage_backward_batch(
            engine.ctx.h, C.byref(cfg), B, p(Rc), p(Tc), p(z), p(n), p(sv['lat']), sv['stride'], None if st is None else C.byref(st), p(sv['ws']),
            sv['ws'].numel(), p(gs), p(g_lat), p(g_R), p(g_T), p(g_n), p(ws_b), ws_b.numel(), engine.ctx.stream()))
        g_weights = ()
        if ctx.nweights:
            weights = ctx.saved_tensors
            grads, _ = color_stage_weight_grads(engine, cfg, sv, ws_b, weights)
            g_weights = tuple(g.reshape(w.shape).to(device=w.device, dtype=w.dtype) for g, w in zip(grads, weights))
        g_c, g_s = _split_code_grad(g_lat, *ctx.codes) if g_lat is not None else (None, None)
        rs, ts, ns = ctx.shapes
        cam = [None if t is None else t.reshape(sh).to(device=d, dtype=dt) for t, sh, (d, dt) in zip((g_R, g_T), (rs, ts), ctx.in_meta[:2])]
        g_n = None if g_n is None else g_n.reshape(ns).to(device=ctx.in_meta[2][0], dtype=ctx.in_meta[2][1])
        return ((g_c if need_c else None), (g_s if need_s else None), cam[0], cam[1], g_n) + (None,) * 7 + g_weights


def color_stage_call(engine, cfg, color_codes, shape_codes, R, T, zdepth, mask, normal=None, lights=None, energies=None, detach_color=False,
                     weights=None):
    """The colour images of B rendered views (color_stage_forward), on the tape unless nothing requires grad. detach_color: see
    ColorStageFunction. weights: None, or W0..W8, b0..b8 of the engine's colour decoder on the autograd graph
    (decoder_pack.effective_weights_torch_color): the backward also returns their gradients (one host sync per backward, see
    ColorStageFunction); they are not taken together with detach_color."""
    weights = list(weights) if weights is not None else []
    if weights:
        _eighteen(weights)
        if cfg.rows != 0:
            raise NotImplementedError('color_decoder_grad: row bands are not implemented (render the whole image)')
    ins = (R, T, normal) if detach_color else (color_codes, shape_codes, R, T, normal) + tuple(weights)
    if lights is None and detach_color:
        ins = ()
    if torch.is_grad_enabled() and any(getattr(t, 'requires_grad', False) for t in ins):
        return ColorStageFunction.apply(color_codes, shape_codes, R, T, normal if lights is not None else None, engine, cfg, zdepth, mask, lights, energies,
                                        detach_color, *weights)
    return color_stage_forward(engine, cfg, color_codes, shape_codes, R, T, zdepth, mask, normal, lights, energies)[0]


class ColorLossFunction(torch.autograd.Function):
    """The photometric loss of B colour images as ONE node (distr_color_loss_forward_batch / _backward_batch):
    rgb (B, H, W, 3) + observations (mask (B, H, W), gt (B, H, W, 3), gt_mask (B, H, W)) -> (l1 (B,), ssim (B,) -- empty without
    want_ssim --, overlap (B,) int32): the masked L1 and the SSIM term of the reference's compute_loss_color(use_ssim=True), per view.
    Gradient flows to rgb only. A view with an empty overlap has l1 = 0 and a zero L1 gradient; `overlap` shows it."""

    @staticmethod
    def forward(ctx, rgb, mask, gt, gt_mask, want_ssim):
        dev = rgb.device
        if dev.type != 'cuda':
            raise RuntimeError('ColorLossFunction: tensors must be on the GPU (no CPU path in this build)')
        c = _train_context(dev.index if dev.index is not None else torch.cuda.current_device())
        r = _f32c(rgb, dev)
        if r.dim() != 4 or r.shape[3] != 3 or not 1 <= r.shape[0] <= binding.MAX_VIEWS:
            raise ValueError('color_output has shape %s; expected (B, H, W, 3) with 1 <= B <= %d' % (tuple(rgb.shape), binding.MAX_VIEWS))
        B, H, W = r.shape[:3]
        g, m, gm = _f32c(gt, dev), _u8c(mask, dev), _u8c(gt_mask, dev)
        if g.shape != r.shape or m.shape != (B, H, W) or gm.shape != (B, H, W):
            raise ValueError('expected color_gt %s and masks %s, got %s, %s and %s' % (tuple(r.shape), (B, H, W), tuple(gt.shape), tuple(mask.shape), tuple(gt_mask.shape)))
        L, p = c.L, binding.ptr
        need = L.distr_color_loss_workspace_bytes(H, W, B, 0)
        if not need:
            raise ValueError('colour loss: images of %d x %d pixels are refused (at most 2^24 pixels)' % (H, W))
        l1 = torch.empty(B, dtype=torch.float32, device=dev)
        ssim = torch.empty(B if want_ssim else 0, dtype=torch.float32, device=dev)
        ov = torch.empty(B, dtype=torch.int32, device=dev)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        c.check(L.distr_color_loss_forward_batch(c.h, H, W, B, p(r), p(m), p(g), p(gm), 1 if want_ssim else 0, p(l1), p(ssim) if want_ssim else None, p(ov),
                                                 p(ws), ws.numel(), c.stream()))
        ctx.c, ctx.dims, ctx.want_ssim, ctx.saved = c, (B, H, W), bool(want_ssim), (r, m, g, gm, ov)
        ctx.in_meta = (rgb.shape, rgb.device, rgb.dtype)
        ctx.mark_non_differentiable(ov)
        return l1, ssim, ov

    @staticmethod
    def backward(ctx, g_l1, g_ssim, _g_ov):
        c, (B, H, W) = ctx.c, ctx.dims
        r, m, g, gm, ov = ctx.saved
        dev = r.device
        gl = _f32c(g_l1, dev).reshape(B)
        gs = _f32c(g_ssim, dev).reshape(B) if ctx.want_ssim else None
        g_rgb = torch.empty_like(r)
        L, p = c.L, binding.ptr
        ws = torch.empty(L.distr_color_loss_workspace_bytes(H, W, B, 1), dtype=torch.uint8, device=dev)
        c.check(L.distr_color_loss_backward_batch(c.h, H, W, B, p(r), p(m), p(g), p(gm), p(ov), p(gl), p(gs), p(g_rgb), p(ws), ws.numel(), c.stream()))
        shape, d, dt = ctx.in_meta
        return g_rgb.reshape(shape).to(device=d, dtype=dt), None, None, None, None


def color_loss_batch(rgb, mask, gt, gt_mask, want_ssim=False):
    """ColorLossFunction on B views: -> (l1 (B,), ssim (B,) or None, overlap (B,) int32). gt is an observation: ValueError if it
    requires grad."""
    if getattr(gt, 'requires_grad', False):
        raise ValueError('color_gt requires grad: the target is an observation here, no gradient reaches it (detach it)')
    l1, ssim, ov = ColorLossFunction.apply(rgb, mask, gt, gt_mask, bool(want_ssim))
    return l1, (ssim if want_ssim else None), ov


def color_relight(engine, cfg, color, normal, zdepth, mask, R, T, lights, energies=None):
    """distr_color_relight: F light sets (F, M, 3) on ONE rendered view -> (F, H, W, 3) = color * shading term of frame f; byte for byte
    the lit colour stage of that view with frame f's lights. Forward only."""
    dev, L, p = engine.device, engine.ctx.L, binding.ptr
    loc = _f32c(lights, dev)
    if loc.dim() != 3 or loc.shape[2] != 3 or loc.shape[0] < 1 or loc.shape[1] < 1:
        raise ValueError('lighting_locations has shape %s; relight takes (F, M, 3)' % (tuple(lights.shape),))
    F = loc.shape[0]
    loc, en, st = color_lights(dev, F, loc, energies)
    Rc, Tc, z, m, n, B, P = _stage_views(engine, cfg, R, T, zdepth, mask, normal, True)
    col = _f32c(color, dev).reshape(-1)
    if B != 1 or col.numel() != 3 * P:
        raise ValueError('relight takes ONE view: R (3,3), T (3), color / normal (%d, %d, 3), Zdepth / mask (%d, %d)' % (cfg.H, cfg.W, cfg.H, cfg.W))
    out = torch.empty(F, cfg.H, cfg.W, 3, dtype=torch.float32, device=dev)
    engine.ctx.check(L.distr_color_relight(engine.ctx.h, C.byref(cfg), F, p(Rc), p(Tc), p(z), p(m), p(n), p(col), C.byref(st), p(out), engine.ctx.stream()))
    return out
