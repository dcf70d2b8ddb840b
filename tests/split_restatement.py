"""Plane-exact CPU models of the two split arithmetics of the decoder tile (csrc/distr_mlp_split.hpp: FmtB6, FmtH3) and the
function-preserving rescales of a decoder that probe the range of the split-f16 form. Test infrastructure only.

What is modelled exactly: the planes. Every operand of lin1..lin7 is the sum of bf16 (three) or f16 (two, of the operand times 64)
planes, each the round-to-nearest-even conversion of the running remainder (torch's conversions, denormals kept); the products
that are formed are the ones the tiles form (PW / PA of FmtB6 / FmtH3); lin0 and lin8 are plain f32; lin4's latent part is
folded into c4 in f32; biases start the accumulator. What is NOT modelled bit for bit is the order of the f32 accumulation inside
the MFMA: a product of two planes is exact in f32, their sum over k is taken by torch's f32 matmul. The float64 decoder is
tests/train_restatement.py; it is not restated here.
"""
import numpy as np
import torch

H3_S = 64.0                      # FmtH3::SX = FmtH3::SW
F16_MAX = 65504.0
B6_PRODUCTS = ((0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (0, 2))      # (weight plane, activation plane): PW / PA of FmtB6
H3_PRODUCTS = ((0, 0), (1, 0), (0, 1))                              # the same of FmtH3
PRODUCTS = {'bf16x6': B6_PRODUCTS, 'f16x3': H3_PRODUCTS}


def planes(x, n, dtype, ftz=False):
    """x (f32) ~ sum of n planes of `dtype`, each the rounding of the running remainder (pack_fragments_* / split_pair / split2_f16).
    ftz: planes below the format's smallest normal number become zero (what a unit that flushes denormals would see)."""
    out, r = [], x
    tiny = torch.finfo(dtype).tiny
    for _ in range(n):
        p = r.to(dtype).to(torch.float32)
        if ftz:
            p = torch.where(p.abs() < tiny, torch.zeros_like(p), p)
        out.append(p)
        r = r - p
    return out


def f16_overflowed(v):
    """The flag of FmtH3's store4: the leading f16 plane of a (non-negative) scaled value is inf or NaN (bit pattern >= 0x7c00)."""
    return ~torch.isfinite(v.to(torch.float16))


def latent_consts(Ws, bs, latent):
    """c0 = b0 + W0[:, :C] latent, c4 = b4 + W4[:, r3:r3 + C] latent, in f32."""
    W0, W4 = Ws[0], Ws[4]
    C = W0.shape[1] - 3
    r3 = W4.shape[1] - C - 3
    lat = latent.reshape(-1)
    return bs[0] + W0[:, :C] @ lat, bs[4] + W4[:, r3:r3 + C] @ lat


def _f32(arrays):
    return [torch.as_tensor(np.asarray(a), dtype=torch.float32) for a in arrays]


def forward(Ws, bs, latent, pts, mode, drop=None, clamp=None, ftz=False):
    """sdf (n,) f32 and the per-point overflow flag (n,) bool of the decoder in `mode`:
    'f32'   : the exact f32 chain (what the default tile and the oracle compute, up to summation order);
    'bf16x6': six products of three bf16 planes per operand, activations kept in f32 between the layers;
    'f16x3' : three products of two f16 planes of the operands times 64; the activations live as planes, so lin8 reads their sum.
    drop: a (weight plane, activation plane) pair left out of every layer -- a tile that lost a product.
    The flag is always False except for 'f16x3', where it is raised as FmtH3's store4 raises it; a flagged point's sdf is NaN."""
    with torch.no_grad():
        Ws, bs = _f32(Ws), _f32(bs)
        latent, pts = _f32([latent, pts])
        n = pts.shape[0]
        over = torch.zeros(n, dtype=torch.bool)
        c0, c4 = latent_consts(Ws, bs, latent)
        r3 = Ws[3].shape[0]
        W4 = torch.cat([Ws[4][:, :r3], Ws[4][:, -3:]], 1)            # [x3 | xyz]: the tile's lin4, K = 256
        x = torch.relu(pts @ Ws[0][:, -3:].t() + c0)
        if mode == 'f32':
            for l in range(1, 8):
                if l == 4:
                    x = torch.relu(torch.cat([x, pts], 1) @ W4.t() + c4)
                else:
                    x = torch.relu(x @ Ws[l].t() + bs[l])
        elif mode == 'bf16x6':
            prods = [p for p in B6_PRODUCTS if p != drop]
            for l in range(1, 8):
                W, b = (W4, c4) if l == 4 else (Ws[l], bs[l])
                if l == 4:
                    x = torch.cat([x, pts], 1)
                wp, ap = planes(W, 3, torch.bfloat16, ftz), planes(x, 3, torch.bfloat16, ftz)
                acc = b.expand(n, -1).clone()
                for pw, pa in prods:
                    acc = acc + ap[pa] @ wp[pw].t()
                x = torch.relu(acc)
        elif mode == 'f16x3':
            prods = [p for p in H3_PRODUCTS if p != drop]
            v = x * H3_S                                             # SX * activation, split by the producer
            over |= f16_overflowed(v).any(1)
            ap = planes(v, 2, torch.float16, ftz)
            for l in range(1, 8):
                W, b = (W4, c4) if l == 4 else (Ws[l], bs[l])
                if l == 4:                                           # rows 253..255 <- SX * xyz (signed), as planes; not range-checked
                    xp = planes(pts * H3_S, 2, torch.float16, ftz)
                    ap = [torch.cat([a, q], 1) for a, q in zip(ap, xp)]
                wp = planes(W * H3_S, 2, torch.float16, ftz)
                acc = (b * (H3_S * H3_S)).expand(n, -1).clone()
                for pw, pa in prods:
                    acc = acc + ap[pa] @ wp[pw].t()
                v = torch.relu(acc) * (1.0 / H3_S)
                over |= f16_overflowed(v).any(1)
                ap = planes(v, 2, torch.float16, ftz)
            x = (ap[0] + ap[1]) * (1.0 / H3_S)
        else:
            raise ValueError(mode)
        y = torch.tanh((x @ Ws[8].t() + bs[8]).reshape(-1))
        if clamp is not None:
            y = torch.clamp(y, -clamp, clamp)
        return torch.where(over, torch.full_like(y, float('nan')), y), over       # k_eval_split: NaN for a flagged point


def h3_weights_in_range(Ws):
    """split_f16x2's rule (pack_fragments_split) on lin1..lin7: every weight times 64 below the largest finite f16."""
    return all(float(np.abs(np.asarray(Ws[l], np.float32) * np.float32(H3_S)).max()) < F16_MAX for l in range(1, 8))


H3_WMIN, H3_WMAX = 2.0 ** -8, F16_MAX / H3_S         # csrc/distr_mlp_split.hpp


def h3_refused_layer(Ws):
    """distr_set_decoder's rule for arith='f16x3': the first of lin1..lin7 whose largest |weight| (of the columns the tile multiplies:
    lin4 without its latent columns) lies outside [H3_WMIN, H3_WMAX), or None when the mode is available."""
    r3 = np.asarray(Ws[3]).shape[0]
    for l in range(1, 8):
        W = np.asarray(Ws[l], np.float32)
        if l == 4:
            W = np.concatenate([W[:, :r3], W[:, -3:]], 1)
        m = float(np.abs(W).max())
        if not (H3_WMIN <= m < H3_WMAX):
            return l
    return None


# ---- function-preserving rescales by powers of two: the same decoder in exact arithmetic, other magnitudes inside
def _copy(Ws, bs):
    return [np.array(w, dtype=np.float32, copy=True) for w in Ws], [np.array(b, dtype=np.float32, copy=True) for b in bs]


def rescale_pair(Ws, bs, k, layer):
    """lin_layer (weights and bias) times 2^-k, the columns of lin_{layer+1} that read its output times 2^k: only the activations
    of `layer` shrink. layer 3 crosses the seam into lin4: only lin4's first 253 columns grow."""
    Ws, bs = _copy(Ws, bs)
    s = np.float32(2.0 ** k)
    Ws[layer] /= s
    bs[layer] /= s
    Ws[layer + 1][:, :Ws[layer].shape[0]] *= s
    return Ws, bs


def rescale_chain(Ws, bs, k):
    """lin1 times 2^-k, the biases of lin1..lin6 and lin4's latent and xyz columns times 2^-k, lin7's weights times 2^k: the
    activations of lin1..lin6 all shrink by 2^k."""
    Ws, bs = _copy(Ws, bs)
    s = np.float32(2.0 ** k)
    Ws[1] /= s
    for l in range(1, 7):
        bs[l] /= s
    Ws[4][:, Ws[3].shape[0]:] /= s
    Ws[7] *= s
    return Ws, bs


def family(Ws, bs):
    """The members the range tests walk: (name, weights, biases)."""
    out = []
    for k in (0, 4, 6, 8, 10):
        for layer in (1, 3, 5):
            out.append(('pair lin%d/lin%d k=%d' % (layer, layer + 1, k),) + rescale_pair(Ws, bs, k, layer))
        out.append(('chain k=%d' % k,) + rescale_chain(Ws, bs, k))
    return out


def errors(sdf, sdf64):
    """(max, 99th percentile) of |sdf - sdf64|."""
    e = (torch.as_tensor(np.asarray(sdf), dtype=torch.float64).reshape(-1) - torch.as_tensor(np.asarray(sdf64), dtype=torch.float64).reshape(-1)).abs().numpy()
    return float(e.max()), float(np.percentile(e, 99))
