"""Float64 restatement of the colour decoder (load_decoder(color_size=cs): latent 256 + cs, lin3 253 rows, lin4 (512, 512 + cs), lin8
(3, 512), tanh, no clamp) for the tests of decode_color_train.

The network is train_restatement.forward's chain -- its widths come from the weights, [code | xyz] is appended at lin4 -- on code rows
[shape | colour]; what is added here: the code rows, an upstream gradient per channel, the two code gradients, optional dropout masks
(given 0/1 arrays times a scale behind the relu, as the reference's F.dropout applies them), and the blocks of the colour net's
gradients. As there, every ReLU is a product with a GIVEN gate when gates are passed.
"""
import numpy as np
import torch

import train_restatement as tr

SHAPE_CODE = 256
to64 = tr.to64


def code_rows(color_codes, shape_codes, S):
    """(S, 256 + cs) rows [shape | colour]; each code (1, .) shared or (S, .). Tensors in, tensor out (autograd passes through)."""
    return torch.cat([shape_codes.expand(S, -1), color_codes.expand(S, -1)], 1)


def forward(Ws, bs, color_codes, shape_codes, pts, counts, gates=None, masks=None, scale=1.0):
    """rgb (sum counts, 3) and the pre-activations of lin0..lin7. masks: None or {layer: (sum counts, units) 0/1 array}: the relu output
    of that layer is multiplied by mask * scale."""
    rows = code_rows(color_codes, shape_codes, len(counts))
    if masks is None:
        return tr.forward(Ws, bs, rows, pts, counts, None, gates)
    cnt = torch.as_tensor([int(c) for c in counts])
    inp = torch.cat([torch.repeat_interleave(rows, cnt, dim=0), pts], 1)
    x, pre = inp, []
    for l in range(9):
        if l == 4:
            x = torch.cat([x, inp], 1)
        z = x @ Ws[l].t() + bs[l]
        if l < 8:
            pre.append(z)
            g = (z > 0) if gates is None else gates[l]
            x = z * g.to(z.dtype)
            if l in masks:
                x = x * (torch.as_tensor(np.asarray(masks[l]), dtype=z.dtype) * scale)
    return torch.tanh(z), pre


def gradients(Ws, bs, color_codes, shape_codes, pts, counts, w, gates=None, masks=None, scale=1.0):
    """(rgb, pre-activations, [g_W], [g_b], g_color_codes, g_shape_codes) of sum(rgb * w), w (sum counts, 3), in float64."""
    W64, b64 = to64(Ws, True), to64(bs, True)
    cc, sc = to64([color_codes, shape_codes], True)
    p64, w64 = to64([pts, w])
    y, pre = forward(W64, b64, cc, sc, p64, counts, gates, masks, scale)
    (y * w64.reshape(-1, 3)).sum().backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return y.detach(), [z.detach() for z in pre], [zero(t) for t in W64], [zero(t) for t in b64], zero(cc), zero(sc)


def gradient_blocks(cs):
    """(name, index into [g_W0..g_W8, g_b0..g_b8], column slice): g_W0 = [shape | colour | xyz], g_W4 = [lin3 cols | shape | colour |
    xyz] -- the parts different kernels write, each judged against its own largest entry."""
    L = SHAPE_CODE + cs
    blocks = [('g_W0 shape', 0, slice(0, 256)), ('g_W0 colour', 0, slice(256, L)), ('g_W0 xyz', 0, slice(L, L + 3)),
              ('g_W4 lin3 cols', 4, slice(0, 253)), ('g_W4 shape', 4, slice(253, 509)), ('g_W4 colour', 4, slice(509, 509 + cs)),
              ('g_W4 xyz', 4, slice(509 + cs, 512 + cs))]
    blocks += [('g_W%d' % l, l, slice(None)) for l in (1, 2, 3, 5, 6, 7, 8)]
    return blocks + [('g_b%d' % l, 9 + l, slice(None)) for l in range(9)]


def blockwise_residuals(got, ref, cs):
    """[(name, max |got - ref| / max |ref| of the block, max |ref|)]; an all-zero reference block: 0 if got is zero there, else inf."""
    out = []
    for name, i, cols in gradient_blocks(cs):
        a, b = np.asarray(got[i], dtype=np.float64)[..., cols], np.asarray(ref[i], dtype=np.float64)[..., cols]
        top, err = np.abs(b).max(), np.abs(a - b).max()
        out.append((name, (err / top) if top > 0 else (0.0 if err == 0 else np.inf), top))
    return out


def code_residuals(got_c, got_s, ref_c, ref_s):
    """The two code gradients as blocks of their own: [(name, relative residual, max |ref|)]"""
    out = []
    for name, a, b in (('g colour code', got_c, ref_c), ('g shape code', got_s, ref_s)):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        top, err = np.abs(b).max(), np.abs(a - b).max()
        out.append((name, (err / top) if top > 0 else (0.0 if err == 0 else np.inf), top))
    return out


def color_module(Ws, bs, weight_norm=False, dropout=None, dropout_prob=0.0, dtype=torch.float64):
    """The torch colour Decoder of this package (core.graph, last_dim=3, latent 256 + cs, dims[3] += cs) holding the given weights."""
    from core.graph.deep_sdf_decoder import Decoder
    from distr import decoder_pack
    cs = Ws[0].shape[1] - 3 - SHAPE_CODE
    dims = [512] * 8
    dims[3] += cs
    dec = Decoder(SHAPE_CODE + cs, dims, dropout=dropout, dropout_prob=dropout_prob, norm_layers=list(range(8)) if weight_norm else (),
                  latent_in=[4], weight_norm=weight_norm, last_dim=3)
    sd = decoder_pack.fixture_state_dict(Ws, bs, weight_norm=weight_norm)
    dec.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()})
    return dec.to(dtype).eval()


def l1_sgd_losses(module64, color_codes, shape_codes, pts, counts, target, lr, steps):
    """Plain SGD on a float64 colour Decoder and the colour codes, loss mean |rgb - target|: (steps + 1 losses -- before every step, and
    after the last --, the colour codes after the last step). The module is updated in place."""
    cc = color_codes.clone().double().requires_grad_(True)
    params = list(module64.parameters()) + [cc]
    cnt = torch.as_tensor([int(c) for c in counts], device=cc.device)
    losses = []
    for i in range(steps + 1):
        for p in params:
            p.grad = None
        rows = code_rows(cc, shape_codes.double(), len(counts))
        y = module64.inference(torch.cat([torch.repeat_interleave(rows, cnt, dim=0), pts.double()], 1))
        loss = (y - target.double()).abs().mean()
        losses.append(loss.item())
        if i == steps:
            break
        loss.backward()
        with torch.no_grad():
            for p in params:
                p -= lr * p.grad
    return losses, cc.detach()


# ---- golden G34 (tests/gen_golden_color_train.py): the reference's decode_color, loss mean |rgb - target|, its gradients
G34_VALUES = ('rgb', 'loss')
G34_ROWS = (0, 255, -1)


def g34_bits(golden, case, kind, layer, rows=210):
    """The (rows, units) bool array `kind` ('pos', 'near', 'keep') of lin_layer's output."""
    if layer == 3:
        packed, units = golden['%s_%s3' % (case, kind)], 253
    else:
        packed, units = golden['%s_%s' % (case, kind)][layer if layer < 3 else layer - 1], 512
    return np.unpackbits(packed)[:rows * units].reshape(rows, units).astype(bool)


def g34_quantities(rgb, loss, g_color, g_shape, grads):
    """Everything G34 records, from full arrays: grads = {'lin<l>.bias' / 'lin<l>.weight_g' / 'lin<l>.weight_v' / 'lin8.weight': gradient}."""
    a = lambda t: np.asarray(t.detach().cpu() if torch.is_tensor(t) else t)
    q = dict(rgb=a(rgb).reshape(-1, 3), loss=a(loss).reshape(1), g_color_codes=a(g_color), g_shape_codes=a(g_shape), g_lin8_weight=a(grads['lin8.weight']))
    for l in range(9):
        q['g_bias%d' % l] = a(grads['lin%d.bias' % l])
    for l in range(8):
        q['g_weight_g%d' % l] = a(grads['lin%d.weight_g' % l])
        gv = a(grads['lin%d.weight_v' % l])
        q['g_v%d_rowsum' % l], q['g_v%d_colsum' % l] = gv.sum(1), gv.sum(0)
        q['g_v%d_rows' % l] = gv[[min(i, gv.shape[0] - 1) if i >= 0 else gv.shape[0] - 1 for i in G34_ROWS]]
    return q


def g34_check(golden, case, q, value_bar, grad_bar, tag):
    """Every recorded quantity, nothing left out: values within max(2 x floor, value_bar) absolute, gradients within
    max(2 x floor, grad_bar) of the quantity's largest entry. Returns (worst value residual, worst gradient residual)."""
    names = sorted(k[len(case) + 1:] for k in golden.files if k.startswith(case + '_') and '_floor_' not in k
                   and not any(k.startswith('%s_%s' % (case, b)) for b in ('pos', 'near', 'keep')))
    assert sorted(q) == names, (sorted(set(q) ^ set(names)))
    worst = {True: 0.0, False: 0.0}
    for k in names:
        want, got = golden['%s_%s' % (case, k)], np.asarray(q[k], dtype=np.float64)
        assert got.shape == want.shape, (k, got.shape, want.shape)
        floor = float(golden['%s_floor_%s' % (case, k)])
        is_value = k in G34_VALUES
        d = np.abs(got - want).max() / (1.0 if is_value else np.abs(want).max())
        bar = max(2 * floor, value_bar if is_value else grad_bar)
        worst[is_value] = max(worst[is_value], d)
        assert d <= bar, (tag, case, k, d, bar)
    print('G34 %s %s: values within %.3e, gradients within %.3e of their largest entry' % (tag, case, worst[True], worst[False]))
    return worst[True], worst[False]
