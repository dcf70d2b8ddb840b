"""decode_sdf / decode_sdf_gradient / load_decoder with the reference's signatures
(core/utils/decoder_utils.py:7-92), evaluated by the fused MFMA decoder kernel instead of nine ATen GEMMs.
No (n,259) latent-concatenated input is ever materialised (decoder_utils.py:61-62) and MAX_POINTS chunking is
unnecessary (accepted and ignored).
"""
import json
import os

import torch

from distr import functions


def _engine(decoder, ref_tensor):
    dev = ref_tensor.device
    if dev.type != 'cuda':
        raise RuntimeError('decode_sdf: tensors must be on the GPU (no CPU path in this build)')
    return functions.get_engine(decoder, dev.index if dev.index is not None else torch.cuda.current_device())


def load_decoder(experiment_directory, checkpoint_num=None, color_size=None, experiment_directory_color=None, parallel=True):
    """specs.json + ModelParameters/<ckpt>.pth -> Decoder (reference: decoder_utils.py:7-51). With `color_size` the
    colour decoder is built instead: latent = CodeLength + color_size, dims[3] += color_size, last_dim = 3, weights from
    `experiment_directory_color` (saved without the DataParallel 'module.' prefix, decoder_utils.py:35-42)."""
    from core.graph.deep_sdf_decoder import Decoder
    specs_filename = os.path.join(experiment_directory, 'specs.json')
    if not os.path.isfile(specs_filename):
        raise Exception('The experiment directory does not include specifications file "specs.json"')
    with open(specs_filename) as f:
        specs = json.load(f)
    net = dict(specs['NetworkSpecs'])
    if color_size is not None:
        net['dims'] = list(net['dims'])
        net['dims'][3] = net['dims'][3] + color_size
        decoder = Decoder(specs['CodeLength'] + color_size, last_dim=3, **net)
    else:
        decoder = Decoder(specs['CodeLength'], **net)
    if parallel:
        decoder = torch.nn.DataParallel(decoder)
    if checkpoint_num is not None:
        root = experiment_directory_color if color_size is not None else experiment_directory
        state = torch.load(os.path.join(root, 'ModelParameters', checkpoint_num + '.pth'), map_location='cpu')
        sd = {(k[len('module.'):] if k.startswith('module.') else k): v for k, v in state['model_state_dict'].items()}
        if parallel:
            sd = {'module.' + k: v for k, v in sd.items()}
        decoder.load_state_dict(sd)
    return decoder


def decode_sdf(decoder, latent_vector, points, clamp_dist=0.1, MAX_POINTS=100000, no_grad=False, arith='f32'):
    """(n,3) points -> (n,1) SDF, optionally clamped (decoder_utils.py:53-74). Differentiable w.r.t. the latent code and
    the points unless `no_grad` (fused backward: distr_mlp_backward); the decoder weights are constants here (decode_sdf_train returns
    gradients to them). `arith` (not in the
    reference): 'f32' = exact f32 MFMA (default); 'bf16x6' / 'f16x3' = split-bf16 / split-f16 arithmetic, forward only, f32-equivalent
    but not bit-identical (distr_mlp_eval_bf16x6 / distr_mlp_eval_f16x3; the latter needs every layer's largest |weight| in [2^-8, 1023.5) -- refused otherwise -- and activations below 1023.75, and returns NaN otherwise)."""
    if latent_vector is None:
        raise NotImplementedError('latent_vector=None (decoder_utils.py:58-59) is not supported')
    eng = _engine(decoder, points)
    if (not no_grad) and torch.is_grad_enabled() and (latent_vector.requires_grad or points.requires_grad):
        if arith != 'f32':
            raise NotImplementedError("arith=%r is forward-only: call decode_sdf(..., no_grad=True)" % arith)
        return functions.mlp_eval_autograd(eng, latent_vector, points, clamp_dist)
    return functions.mlp_eval(eng, latent_vector, points, clamp_dist, arith=arith)


def decode_sdf_gradient(decoder, latent_vector, points, clamp_dist=0.1, MAX_POINTS=100000, no_grad=False):
    """d sdf / d points, (n,3). Keeps the reference's value semantics: the clamp inside decode_sdf zeroes the
    gradient where |f| > clamp_dist, and the (n,3) grad_outputs of decoder_utils.py:84 made torch 1.1 return 3x
    the gradient. Returned detached (second-order terms vanish for ReLU decoders after normalisation)."""
    sdf, g = functions.mlp_grad(_engine(decoder, points), latent_vector, points)
    g = 3.0 * g
    if clamp_dist is not None:
        g = g * (sdf.abs() <= clamp_dist).to(g.dtype)[:, None]
    return g


def _batch_layout(Cn, latent_vectors, points, counts):
    """(flat points (sum N, 3), counts as a list, output shape without the last axis) of a decode_sdf_batch / decode_sdf_gradient_batch
    call for a decoder of code length Cn; ValueError for shapes that do not fit. Pure shape logic: runs without a GPU."""
    if latent_vectors.dim() != 2 or latent_vectors.shape[1] != Cn or latent_vectors.shape[0] < 1:
        raise ValueError('latent_vectors has shape %s; this decoder takes (S, C) = (S, %d): one code per segment' % (tuple(latent_vectors.shape), Cn))
    S = latent_vectors.shape[0]
    if counts is None:
        if points.dim() != 3 or points.shape[0] != S or points.shape[2] != 3:
            raise ValueError('points has shape %s; without counts %d codes take (S, N, 3) = (%d, N, 3)' % (tuple(points.shape), S, S))
        return points.reshape(-1, 3), [points.shape[1]] * S, (S, points.shape[1])
    counts = [int(c) for c in (counts.tolist() if torch.is_tensor(counts) else counts)]
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError('points has shape %s; with counts it is the flat list (sum N, 3)' % (tuple(points.shape),))
    if len(counts) != S or min(counts) < 0:
        raise ValueError('counts %r: %d codes take %d segment sizes >= 0' % (counts, S, S))
    if sum(counts) != points.shape[0]:
        raise ValueError('counts sum to %d, but there are %d points' % (sum(counts), points.shape[0]))
    return points, counts, (points.shape[0],)


def _batch_args(decoder, latent_vectors, points, counts):
    if latent_vectors is None:
        raise NotImplementedError('latent_vectors=None (a code in every input row, decoder_utils.py:58-59) is not supported')
    eng = _engine(decoder, points)
    return (eng,) + _batch_layout(eng.latent_size, latent_vectors, points, counts)


def decode_sdf_batch(decoder, latent_vectors, points, counts=None, clamp_dist=0.1, no_grad=False):
    """decode_sdf for S shape codes in one launch sequence (not in the reference, which loops): latent_vectors (S, C); points either
    (S, N, 3) -> (S, N, 1), or the flat list (sum N, 3) with `counts` (a sequence or a CPU int tensor of S segment sizes >= 0, segment
    s = the next counts[s] rows) -> (sum N, 1). Every segment's slice is byte for byte decode_sdf(decoder, latent_vectors[s:s+1], its
    points); so are, unless `no_grad`, its gradients w.r.t. the points and row s of the gradient w.r.t. latent_vectors
    (distr_mlp_eval_multi / distr_mlp_backward_multi; more than 64 segments run in chunks of 64). f32 arithmetic."""
    eng, x, counts, shape = _batch_args(decoder, latent_vectors, points, counts)
    if (not no_grad) and torch.is_grad_enabled() and (latent_vectors.requires_grad or points.requires_grad):
        out = functions.mlp_eval_multi_autograd(eng, latent_vectors, x, counts, clamp_dist)
    else:
        out = functions.mlp_eval_multi(eng, latent_vectors, x, counts, clamp_dist)
    return out.reshape(shape + (1,))


def _refuse_point_grads(name, points):
    if points.requires_grad:
        raise ValueError('%s: points.requires_grad is set, but points are data on the layer-wise path (no point gradients); '
                         'pass points.detach(), or use %s for gradients to the points' % (name, name.replace('_train', '_batch')))


def _train_layout(Cn, latent_vectors, points, counts):
    """Shape logic of decode_sdf_train: decode_sdf_batch's (_batch_layout), and points that ask for a gradient are refused. Runs
    without a GPU."""
    if latent_vectors is None:
        raise NotImplementedError('latent_vectors=None (a code in every input row, decoder_utils.py:58-59) is not supported')
    _refuse_point_grads('decode_sdf_train', points)
    return _batch_layout(Cn, latent_vectors, points, counts)


def _train_prologue(name, decoder, points, dropout_seed, weights_of, layout):
    """What decode_sdf_train and decode_color_train (`name`) do before their node, in this order: the decoder's checks (eval mode, or
    with a seed the dropout tuple of functions.train_forward), its weights on the autograd graph (weights_of(decoder) -> (Ws, bs)),
    the refusal of points that ask for a gradient, the shapes (layout(Ws) -> (flat points, counts, output shape)), the device.
    -> (W0..W8 + b0..b8, flat points, counts, output shape, dropout)"""
    module = decoder.module if hasattr(decoder, 'module') else decoder
    dropout = None
    if dropout_seed is None:
        functions._check_eval(module)
    else:
        params = functions.train_dropout_params(module, dropout_seed)
        dropout = None if params is None else params + (int(dropout_seed), 0)
    Ws, bs = weights_of(decoder)
    _refuse_point_grads(name, points)
    x, counts, shape = layout(Ws)
    if x.device.type != 'cuda':
        raise RuntimeError('%s: tensors must be on the GPU (no CPU path in this build)' % name)
    return Ws + bs, x, counts, shape, dropout


def decode_sdf_train(decoder, latent_vectors, points, counts=None, clamp_dist=0.1, dropout_seed=None):
    """decode_sdf_batch that is differentiable w.r.t. `decoder.parameters()` AND the codes (not in the reference, which trains through
    the torch Decoder): the layer-wise path of DESIGN.md section 8f -- one f32-MFMA GEMM per layer over the whole point list, the layer
    inputs kept for the backward (24 KB of workspace per point; above DISTR_TRAIN_MAX_BYTES, default 32 GiB, the call is refused
    rather than chunked, since chunking would change the sum order of the gradients). Arguments, shapes and ValueErrors as
    decode_sdf_batch; points with requires_grad are refused. Without `dropout_seed` the decoder must be in eval mode (dropout in
    training mode raises, as everywhere). With an int `dropout_seed` (functions.draw_dropout_seed()) a decoder in training mode gets the
    dropout of its `dropout` / `dropout_prob` behind the relus, by the counter-based mask of DESIGN.md section 8g: a pure function of
    (seed, segment, point in segment, layer, unit), segment = the index into latent_vectors -- the same call gives the same bytes; in
    eval mode the seed changes nothing. latent_dropout in training mode stays refused. Weight norm is folded on the autograd graph, so
    the gradients arrive at weight_g / weight_v. The fused engine is not involved: after an optimiser step the renderers and
    decode_sdf re-pack the weights by themselves."""
    from distr import decoder_pack
    weights, x, counts, shape, dropout = _train_prologue('decode_sdf_train', decoder, points, dropout_seed, decoder_pack.effective_weights_torch,
                                                         lambda Ws: _train_layout(Ws[0].shape[1] - 3, latent_vectors, points, counts))
    out = functions.decode_sdf_train_call(weights, latent_vectors, x, counts, clamp_dist, dropout)
    return out.reshape(shape + (1,))


def _gradient_train_layout(Cn, latent_vectors, points, counts):
    """Shape logic of decode_sdf_gradient_train: decode_sdf_train's, under its own name in the refusal. Runs without a GPU."""
    if latent_vectors is None:
        raise NotImplementedError('latent_vectors=None (a code in every input row, decoder_utils.py:58-59) is not supported')
    _refuse_point_grads('decode_sdf_gradient_train', points)
    return _batch_layout(Cn, latent_vectors, points, counts)


def decode_sdf_gradient_train(decoder, latent_vectors, points, counts=None, dropout_seed=None):
    """(sdf, grad) = (f, grad_x f) of S shape codes, BOTH differentiable w.r.t. `decoder.parameters()` and the codes (not in the
    reference, where such a loss takes torch's double backward through the torch Decoder): what a normal-supervised fit |grad - n|, an
    Eikonal term (|grad| - 1)^2 or any other loss on the spatial gradient needs to train the decoder. The layer-wise path of
    decode_sdf_train with the closed form of DESIGN.md section 8m; the ReLU's second derivative is zero, as in torch. Arguments, shapes
    and ValueErrors as decode_sdf_train: points (S, N, 3) -> ((S, N, 1), (S, N, 3)), or the flat list (sum N, 3) with `counts` ->
    ((sum N, 1), (sum N, 3)). `sdf` is the raw tanh output: there is NO clamp here, clamp it in torch. `grad` is the TRUE gradient: it
    carries neither decode_sdf_gradient's legacy factor 3 nor its clamp mask (decode_sdf_gradient_batch(clamp_dist=None) / 3 has the
    same values, detached). Points are data: points with requires_grad are refused. Dropout as decode_sdf_train (`dropout_seed`, the
    counter-based mask of section 8g; the tangent and the deltas see the forward's mask and scale). Weight norm is folded on the
    autograd graph. The workspace takes 40 KB per point; above DISTR_TRAIN_MAX_BYTES (default 32 GiB) the call is refused, not chunked.
    The backward makes one pass for the upstream gradients of both outputs."""
    from distr import decoder_pack
    weights, x, counts, shape, dropout = _train_prologue('decode_sdf_gradient_train', decoder, points, dropout_seed, decoder_pack.effective_weights_torch,
                                                         lambda Ws: _gradient_train_layout(Ws[0].shape[1] - 3, latent_vectors, points, counts))
    sdf, grad = functions.decode_sdf_gradient_train_call(weights, latent_vectors, x, counts, dropout)
    return sdf.reshape(shape + (1,)), grad.reshape(shape + (3,))


def decode_sdf_gradient_batch(decoder, latent_vectors, points, counts=None, clamp_dist=0.1):
    """decode_sdf_gradient for S shape codes in one launch sequence; arguments as decode_sdf_batch, returns (S, N, 3) or (sum N, 3) with
    decode_sdf_gradient's value semantics (3 x the gradient, zero where |f| > clamp_dist), detached; byte for byte the single call per
    segment."""
    eng, x, counts, shape = _batch_args(decoder, latent_vectors, points, counts)
    sdf, g = functions.mlp_grad_multi(eng, latent_vectors, x, counts)
    g = 3.0 * g
    if clamp_dist is not None:
        g = g * (sdf.abs() <= clamp_dist).to(g.dtype)[:, None]
    return g.reshape(shape + (3,))


def decode_color(decoder, color_code, shape_code, points, MAX_POINTS=100000, no_grad=False):
    """(n,3) surface points -> (n,3) rgb of the colour decoder (decoder_utils.py:94-112); differentiable w.r.t. the colour code,
    the shape code and the points unless `no_grad` (distr_color_backward). MAX_POINTS chunking is unnecessary (accepted, ignored)."""
    dev = points.device
    if dev.type != 'cuda':
        raise RuntimeError('decode_color: tensors must be on the GPU (no CPU path in this build)')
    eng = functions.get_color_engine(decoder, dev.index if dev.index is not None else torch.cuda.current_device())
    needs = (not no_grad) and torch.is_grad_enabled() and any(getattr(t, 'requires_grad', False) for t in (color_code, shape_code, points))
    if needs:
        return functions.color_eval_autograd(eng, color_code, shape_code, points)
    return functions.color_eval(eng, color_code, shape_code, points)


def _color_batch_layout(color_codes, shape_codes, points, counts):
    """(flat points (sum N, 3), counts as a list, output shape without the last axis) of a decode_color_batch call; ValueError for
    shapes that do not fit. The number of segments S comes from the points ((S, N, 3)) or from `counts`; each of the two codes is
    (1, .) shared or (S, .) -- their lengths are checked against the decoder by functions.color_code_rows. Pure shape logic: runs
    without a GPU."""
    if counts is None:
        if points.dim() != 3 or points.shape[2] != 3 or points.shape[0] < 1:
            raise ValueError('points has shape %s; without counts it is (S, N, 3)' % (tuple(points.shape),))
        S = points.shape[0]
        flat, counts, shape = points.reshape(-1, 3), [points.shape[1]] * S, (S, points.shape[1])
    else:
        counts = [int(c) for c in (counts.tolist() if torch.is_tensor(counts) else counts)]
        if points.dim() != 2 or points.shape[1] != 3:
            raise ValueError('points has shape %s; with counts it is the flat list (sum N, 3)' % (tuple(points.shape),))
        if not counts or min(counts) < 0:
            raise ValueError('counts %r: at least one segment, segment sizes >= 0' % (counts,))
        if sum(counts) != points.shape[0]:
            raise ValueError('counts sum to %d, but there are %d points' % (sum(counts), points.shape[0]))
        S = len(counts)
        flat, shape = points, (points.shape[0],)
    for name, t in (('color_codes', color_codes), ('shape_codes', shape_codes)):
        if t.dim() != 2 or t.shape[0] not in (1, S):
            raise ValueError('%s has shape %s; %d segments take (1, C) (shared) or (%d, C)' % (name, tuple(t.shape), S, S))
    return flat, counts, shape


def decode_color_batch(decoder, color_codes, shape_codes, points, counts=None, no_grad=False):
    """decode_color for S [shape | colour] code pairs in one launch sequence (not in the reference, which decodes one view at a time):
    points either (S, N, 3) -> (S, N, 3), or the flat list (sum N, 3) with `counts` (a sequence or a CPU int tensor of S segment sizes
    >= 0) -> (sum N, 3); color_codes (S, cs) and shape_codes (S, 256), or (1, .) for a code all segments share. Every segment's slice is
    byte for byte decode_color of that segment alone; so are, unless `no_grad`, its gradients w.r.t. the points and its rows of the
    code gradients (distr_color_eval_multi / distr_color_backward_multi; more than 64 segments run in chunks of 64)."""
    flat, counts, shape = _color_batch_layout(color_codes, shape_codes, points, counts)
    dev = points.device
    if dev.type != 'cuda':
        raise RuntimeError('decode_color_batch: tensors must be on the GPU (no CPU path in this build)')
    eng = functions.get_color_engine(decoder, dev.index if dev.index is not None else torch.cuda.current_device())
    needs = (not no_grad) and torch.is_grad_enabled() and any(getattr(t, 'requires_grad', False) for t in (color_codes, shape_codes, points))
    if needs:
        out = functions.color_eval_multi_autograd(eng, color_codes, shape_codes, flat, counts)
    else:
        out = functions.color_eval_multi(eng, color_codes, shape_codes, flat, counts)
    return out.reshape(shape + (3,))


def decode_color_train(decoder, color_codes, shape_codes, points, counts=None, dropout_seed=None):
    """decode_color_batch that is differentiable w.r.t. `decoder.parameters()` AND both codes (not in the reference, which trains its
    texture network through the torch Decoder): the colour decoder on the layer-wise path of DESIGN.md section 8i -- the GEMMs of
    decode_sdf_train on the network (L, lin3 rows, outputs) = (256 + cs, 253, 3), tanh and no clamp. Arguments, shapes and ValueErrors
    as decode_color_batch: points (S, N, 3) -> (S, N, 3), or the flat list (sum N, 3) with `counts` -> (sum N, 3); color_codes (S, cs)
    and shape_codes (S, 256), or (1, .) shared. points with requires_grad are refused (points are data here: decode_color_batch gives
    gradients to them). Without `dropout_seed` the decoder must be in eval mode; with an int seed a decoder in training mode gets the
    counter-based mask of section 8g, segment = the index into the code rows; in eval mode the seed changes nothing. latent_dropout in
    training mode stays refused. A workspace above DISTR_TRAIN_MAX_BYTES (24 KB per point) is refused, not chunked. Weight norm is
    folded on the autograd graph. The colour engine is not involved: after an optimiser step decode_color* and SDFRenderer_color
    re-pack the weights by themselves."""
    from distr import decoder_pack
    weights, x, counts, shape, dropout = _train_prologue('decode_color_train', decoder, points, dropout_seed, decoder_pack.effective_weights_torch_color,
                                                         lambda Ws: _color_batch_layout(color_codes, shape_codes, points, counts))
    out = functions.decode_color_train_call(weights, color_codes, shape_codes, x, counts, dropout)
    return out.reshape(shape + (3,))
