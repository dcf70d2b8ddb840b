"""DeepSDF decoder -> canonical flat f32 weight buffer for `distr_set_decoder` (include/distr.h).

Host-side counterpart of `load_decoder` (core/utils/decoder_utils.py:7-51) + the layer
construction of `Decoder.__init__` (core/graph/deep_sdf_decoder.py:19-73): takes a module or a
state_dict, folds weight-norm (`lin{l}.weight_g/.weight_v` -> W = g * v / ||v||_row), validates that
the architecture is the one the HIP kernels are specialised for (DeepSDF '8x512', code length C in
1..508, latent_in=[4], ReLU, final tanh, no LayerNorm / xyz_in_all / use_tanh; latent_dropout only in eval mode, where it is the identity), and
returns one contiguous float32 array: for l in 0..8: W_l row-major (out,in) followed by b_l.
The LDS/MFMA-fragment packing itself is done natively inside the library.
"""
import numpy as np

from . import fixture

# Code lengths the tile kernels take: 256 <= C <= 508 packs lin3's 509 - C rows zero-padded to 253 (the narrow
# layout, the C = 256 kernels); C < 256 packs them zero-padded to 509, lin3 / lin4 then run as full 512 x 512 layers (the wide layout).
MAX_LATENT = 508


class UnsupportedDecoder(NotImplementedError):
    pass


def _np(t):
    if hasattr(t, 'detach'):
        t = t.detach().cpu().numpy()
    return np.asarray(t)


def effective_weights(state_dict):
    """state_dict (possibly 'module.'-prefixed, possibly weight-normed) -> ([W_l f32], [b_l f32])."""
    sd = {}
    for k, v in state_dict.items():
        k = k[len('module.'):] if k.startswith('module.') else k
        sd[k] = _np(v)
    if any(k.startswith('bn') for k in sd):
        raise UnsupportedDecoder('LayerNorm decoders (weight_norm=False with norm_layers) are not supported')
    Ws, bs = [], []
    l = 0
    while ('lin%d.bias' % l) in sd:
        if ('lin%d.weight_v' % l) in sd:
            v = sd['lin%d.weight_v' % l].astype(np.float32)
            g = sd['lin%d.weight_g' % l].astype(np.float32).reshape(-1, 1)
            nrm = np.sqrt((v.astype(np.float32) ** 2).sum(axis=1, keepdims=True, dtype=np.float32)).astype(np.float32)
            W = (v * (g / nrm)).astype(np.float32)          # torch._weight_norm: v * (g / ||v||)
        elif ('lin%d.parametrizations.weight.original1' % l) in sd:   # new-style parametrization
            v = sd['lin%d.parametrizations.weight.original1' % l].astype(np.float32)
            g = sd['lin%d.parametrizations.weight.original0' % l].astype(np.float32).reshape(-1, 1)
            nrm = np.sqrt((v ** 2).sum(axis=1, keepdims=True, dtype=np.float32)).astype(np.float32)
            W = (v * (g / nrm)).astype(np.float32)
        else:
            W = sd['lin%d.weight' % l].astype(np.float32)
        Ws.append(np.ascontiguousarray(W))
        bs.append(np.ascontiguousarray(sd['lin%d.bias' % l].astype(np.float32)))
        l += 1
    return Ws, bs


def latent_size_of(Ws):
    """Code length C of a decoder: lin0 takes [latent (C) | xyz (3)]."""
    return int(np.shape(Ws[0])[1]) - 3 if len(Ws) and np.ndim(Ws[0]) == 2 else -1


def validate(Ws, bs):
    """Checks all nine shapes against the DeepSDF 8x512 decoder of code length C = lin0's input width - 3; returns C."""
    if len(Ws) != fixture.NUM_LINEAR or len(bs) != fixture.NUM_LINEAR:
        raise UnsupportedDecoder('expected %d linear layers, got %d' % (fixture.NUM_LINEAR, len(Ws)))
    C = latent_size_of(Ws)
    if C < 1 or C > MAX_LATENT:
        raise UnsupportedDecoder('lin0 has shape %s: code length %d is outside 1..%d (lin3 of a latent_in=[4] decoder has 509 - C rows)'
                                 % (np.shape(Ws[0]), C, MAX_LATENT))
    shapes = fixture.layer_shapes(C)
    for l, (W, b) in enumerate(zip(Ws, bs)):
        if tuple(np.shape(W)) != shapes[l] or tuple(np.shape(b)) != (shapes[l][0],):
            raise UnsupportedDecoder('lin%d has shape %s, kernels are specialised for %s (DeepSDF 8x512, '
                                     'latent %d, latent_in=[4], last_dim=1)' % (l, np.shape(W), shapes[l], C))
        # the compacted 64-ray tile skips the products of hidden units that are +0 for a whole tile: the same value only for finite
        # weights (0 * inf is the one product a skipped link would have changed)
        if not (np.isfinite(W).all() and np.isfinite(b).all()):
            raise UnsupportedDecoder('lin%d has non-finite weights or biases' % l)
    return C


def _row_sumsq_f32(v):
    """sum(v ** 2, axis=1) of a 2-D f32 tensor in the order numpy's f32 sum takes along a contiguous row (pairwise: halves down to runs
    of at most 128, eight strided partial sums per run, their fixed tree, then the run's remainder), out of differentiable elementwise
    torch operations: the row norms -- and with them the folded weights -- of effective_weights_torch are those of effective_weights."""
    n = v.shape[1]
    sq = v * v
    if n >= 256 and n % 128 == 0 and (n // 128) & (n // 128 - 1) == 0:     # equal runs of 128: all runs at once
        r = sq.reshape(sq.shape[0], n // 128, 16, 8)
        acc = r[:, :, 0]
        for i in range(1, 16):
            acc = acc + r[:, :, i]
        t = ((acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3])) + ((acc[..., 4] + acc[..., 5]) + (acc[..., 6] + acc[..., 7]))
        while t.shape[1] > 1:
            t = t[:, 0::2] + t[:, 1::2]
        return t[:, 0]

    def run(a):
        m = a.shape[1]
        if m < 8:
            res = a[:, 0] * 0
            for i in range(m):
                res = res + a[:, i]
            return res
        if m <= 128:
            full = m - m % 8
            acc = a[:, :8]
            for i in range(8, full, 8):
                acc = acc + a[:, i:i + 8]
            res = ((acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])) + ((acc[:, 4] + acc[:, 5]) + (acc[:, 6] + acc[:, 7]))
            for i in range(full, m):
                res = res + a[:, i]
            return res
        half = m // 2
        half -= half % 8
        return run(a[:, :half]) + run(a[:, half:])
    return run(sq)


def _fold_weight_norm(v, g):
    """v * (g / ||v||_row), operation for operation what effective_weights computes in numpy (and torch._weight_norm up to the order of
    the norm's sum)."""
    import torch
    # the square root and the quotient through float64: rounding a float64 sqrt / quotient of f32 values to f32 gives the correctly
    # rounded f32 result (53 >= 2 * 24 + 2 bits), whatever the f32 sqrt and division of the device's torch build do
    nrm = torch.sqrt(_row_sumsq_f32(v).double()).float()
    return v * (g.reshape(-1, 1).double() / nrm.reshape(-1, 1).double()).float()


def effective_weights_torch(decoder):
    """nn.Module (optionally DataParallel-wrapped) -> ([W_l], [b_l]) as torch tensors ON THE AUTOGRAD GRAPH of the module's parameters:
    the weights the layer-wise train path (decode_sdf_train) reads in place and returns gradients for. A plain layer
    hands out its own parameters; weight norm, old style (`weight_g` / `weight_v`) or parametrized (`parametrizations.weight.original0 /
    original1`), is folded as effective_weights folds it, W = v * (g / ||v||_row) with the same f32 operations in the same order, so the
    train path and the packed engine see the same weights, and autograd carries g_W on to g and v. Checked as check_module_flags and validate check a decoder that is packed (flags, the nine shapes, finite values)."""
    Ws, bs = _folded_weights_torch(decoder)
    C = int(Ws[0].shape[1]) - 3 if Ws[0].dim() == 2 else -1
    if C < 1 or C > MAX_LATENT:
        raise UnsupportedDecoder('lin0 has shape %s: code length %d is outside 1..%d (lin3 of a latent_in=[4] decoder has 509 - C rows)'
                                 % (tuple(Ws[0].shape), C, MAX_LATENT))
    shapes = fixture.layer_shapes(C)
    for l, (W, b) in enumerate(zip(Ws, bs)):
        if tuple(W.shape) != shapes[l] or tuple(b.shape) != (shapes[l][0],):
            raise UnsupportedDecoder('lin%d has shape %s, kernels are specialised for %s (DeepSDF 8x512, latent %d, latent_in=[4], '
                                     'last_dim=1)' % (l, tuple(W.shape), shapes[l], C))
    _check_finite_torch(Ws, bs)
    return Ws, bs


def effective_weights_torch_color(decoder):
    """effective_weights_torch for the colour decoder (load_decoder(color_size=cs)): ([W_l], [b_l]) on the autograd graph of the module's
    parameters, for decode_color_train. The same flag checks and the same weight-norm fold; the nine shapes are
    those validate_color asks for (fixture.color_layer_shapes(cs), cs >= 1: lin0 (512, 256 + cs + 3), lin3 (253, 512), lin4 (512, 512 +
    cs), lin8 (3, 512)); every value is finite."""
    Ws, bs = _folded_weights_torch(decoder)
    cs = (int(Ws[0].shape[1]) - 3 - fixture.LATENT_SIZE) if Ws[0].dim() == 2 else -1
    if cs <= 0:
        raise UnsupportedDecoder('colour decoder must take latent = 256 + color_size (> 256), got lin0 of shape %s' % (tuple(Ws[0].shape),))
    want = fixture.color_layer_shapes(cs)
    for l, (W, b) in enumerate(zip(Ws, bs)):
        if tuple(W.shape) != want[l] or tuple(b.shape) != (want[l][0],):
            raise UnsupportedDecoder('colour lin%d has shape %s, expected %s (DeepSDF 8x512 with latent 256+%d, latent_in=[4], '
                                     'last_dim=3)' % (l, tuple(W.shape), want[l], cs))
    _check_finite_torch(Ws, bs)
    return Ws, bs


def _folded_weights_torch(decoder):
    """The nine (W_l, b_l) of a module on its autograd graph, weight norm folded; flags and the layer count checked."""
    check_module_flags(decoder)
    d = decoder.module if hasattr(decoder, 'module') else decoder
    params = dict(d.named_parameters())
    if any(k.startswith('bn') for k in params):
        raise UnsupportedDecoder('LayerNorm decoders (weight_norm=False with norm_layers) are not supported')
    Ws, bs = [], []
    l = 0
    while ('lin%d.bias' % l) in params:
        for g_name, v_name in (('weight_g', 'weight_v'), ('parametrizations.weight.original0', 'parametrizations.weight.original1')):
            if ('lin%d.%s' % (l, v_name)) in params:
                v, g = params['lin%d.%s' % (l, v_name)], params['lin%d.%s' % (l, g_name)]
                W = _fold_weight_norm(v, g)
                break
        else:
            W = params['lin%d.weight' % l]
        Ws.append(W)
        bs.append(params['lin%d.bias' % l])
        l += 1
    if len(Ws) != fixture.NUM_LINEAR:
        raise UnsupportedDecoder('expected %d linear layers, got %d' % (fixture.NUM_LINEAR, len(Ws)))
    return Ws, bs


def _check_finite_torch(Ws, bs):
    import torch
    with torch.no_grad():       # one reduction and one host read for all eighteen tensors
        finite = torch.stack([torch.isfinite(t).all() for t in Ws + bs])
        if not bool(finite.all()):
            bad = [i for i, ok in enumerate(finite.tolist()) if not ok][0]
            raise UnsupportedDecoder('lin%d has non-finite weights or biases' % (bad % fixture.NUM_LINEAR))


def validate_color(Ws, bs):
    """Colour decoder (load_decoder(color_size=cs), decoder_utils.py:16-24): returns its latent length 256 + cs."""
    if len(Ws) != 9:
        raise UnsupportedDecoder('expected 9 linear layers, got %d' % len(Ws))
    cs = Ws[0].shape[1] - 3 - fixture.LATENT_SIZE
    if cs <= 0:
        raise UnsupportedDecoder('colour decoder must take latent = 256 + color_size (> 256), got %d' % (Ws[0].shape[1] - 3))
    want = fixture.color_layer_shapes(cs)
    for l, (W, b) in enumerate(zip(Ws, bs)):
        if tuple(W.shape) != want[l] or b.shape != (want[l][0],):
            raise UnsupportedDecoder('colour lin%d has shape %s, expected %s (DeepSDF 8x512 with latent 256+%d, latent_in=[4], '
                                     'last_dim=3)' % (l, W.shape, want[l], cs))
    return fixture.LATENT_SIZE + cs


def flatten_color(Ws, bs):
    """-> (flat f32 array for distr_set_color_decoder, latent length)."""
    nlat = validate_color(Ws, bs)
    parts = []
    for W, b in zip(Ws, bs):
        parts.append(np.asarray(W, np.float32).reshape(-1))
        parts.append(np.asarray(b, np.float32).reshape(-1))
    return np.ascontiguousarray(np.concatenate(parts), dtype=np.float32), nlat


def pack_color_module(decoder_color):
    check_module_flags(decoder_color)
    Ws, bs = effective_weights(decoder_color.state_dict())
    return flatten_color(Ws, bs)


def check_module_flags(decoder):
    """Rejects constructor options of core/graph/deep_sdf_decoder.py:19-73 that change the math."""
    d = decoder.module if hasattr(decoder, 'module') else decoder
    if getattr(d, 'xyz_in_all', None):
        raise UnsupportedDecoder('xyz_in_all decoders are not supported')
    if getattr(d, 'use_tanh', False):
        raise UnsupportedDecoder('use_tanh decoders are not supported')
    if getattr(d, 'latent_dropout', False) and getattr(d, 'training', False):
        # F.dropout(latent, training=self.training), deep_sdf_decoder.py:84-87: the identity in eval mode (what every driver runs:
        # SDFRenderer(is_eval=True) calls decoder.eval()), stochastic in training mode
        raise UnsupportedDecoder('latent_dropout decoder in training mode: the fused kernels evaluate the deterministic (eval) network only '
                                 '-- call decoder.eval() (SDFRenderer(is_eval=True) does)')
    li = tuple(getattr(d, 'latent_in', (4,)))
    if li != (4,):
        raise UnsupportedDecoder('latent_in=%s is not supported (only [4])' % (li,))
    if not hasattr(d, 'th'):
        raise UnsupportedDecoder('decoder without the final tanh is not supported')


def flatten(Ws, bs):
    """-> flat f32 array for distr_set_decoder (its code length: latent_size_of(Ws))."""
    validate(Ws, bs)
    parts = []
    for W, b in zip(Ws, bs):
        parts.append(np.asarray(W, np.float32).reshape(-1))
        parts.append(np.asarray(b, np.float32).reshape(-1))
    return np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)


def pack_module(decoder):
    """nn.Module (optionally DataParallel-wrapped) -> flat f32 array."""
    return pack_module_sized(decoder)[0]


def pack_module_sized(decoder):
    """nn.Module (optionally DataParallel-wrapped) -> (flat f32 array, code length C)."""
    check_module_flags(decoder)
    Ws, bs = effective_weights(decoder.state_dict())
    return flatten(Ws, bs), latent_size_of(Ws)


def fixture_state_dict(Ws, bs, weight_norm=False):
    """state_dict (numpy) of the fixture decoder in plain or DeepSDF weight_norm form."""
    sd = {}
    for l, (W, b) in enumerate(zip(Ws, bs)):
        if weight_norm and l < 8:
            sd['lin%d.weight_v' % l] = W
            sd['lin%d.weight_g' % l] = np.sqrt((W.astype(np.float32) ** 2).sum(axis=1, keepdims=True, dtype=np.float32)).astype(np.float32)
        else:
            sd['lin%d.weight' % l] = W
        sd['lin%d.bias' % l] = b
    return sd
