"""Float64 restatement of the DeepSDF 8x512 decoder (latent_in=[4]) for the tests of the layer-wise train path.

Every ReLU is a multiplication with a GIVEN 0/1 gate tensor per layer; autograd differentiates the rest. With the gates of its own
float64 pre-activations this is the torch Decoder in float64 (tests/test_train_host.py pins that); with the gates a GPU run saved it
is the function the GPU differentiated, so a gradient comparison carries no ReLU-side ambiguity: a unit whose pre-activation is ~1e-8
may sit on either side of the ReLU in two summation orders, and that choice is made once, by the run under test.
"""
import numpy as np
import torch


def to64(arrays, requires_grad=False):
    return [torch.as_tensor(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a), dtype=torch.float64).clone().requires_grad_(requires_grad)
            for a in arrays]


def forward(Ws, bs, codes, pts, counts, clamp=None, gates=None):
    """Ws, bs: nine float64 tensors each; codes (S, C) or (1, C) shared; pts (sum counts, 3); gates: None (own ReLU pattern) or eight
    0/1 tensors, gates[l] of lin_l's output shape. Returns (sdf (sum counts, 1), [pre-activations of lin0..lin7])."""
    counts = torch.as_tensor([int(c) for c in counts])
    rows = codes.expand(len(counts), -1) if codes.shape[0] == 1 else codes
    inp = torch.cat([torch.repeat_interleave(rows, counts, dim=0), pts], 1)
    x, pre = inp, []
    for l in range(9):
        if l == 4:
            x = torch.cat([x, inp], 1)
        z = x @ Ws[l].t() + bs[l]
        if l < 8:
            pre.append(z)
            g = (z > 0) if gates is None else gates[l]
            x = z * g.to(z.dtype)
    y = torch.tanh(z)
    if clamp is not None:
        y = torch.clamp(y, -clamp, clamp)
    return y, pre


def gradients(Ws, bs, codes, pts, counts, w, clamp=None, gates=None):
    """(sdf, pre-activations, [g_W], [g_b], g_codes) of sum(sdf * w) in float64; inputs are numpy arrays or tensors of any dtype."""
    W64, b64 = to64(Ws, True), to64(bs, True)
    c64, = to64([codes], True)
    p64, w64 = to64([pts, w])
    y, pre = forward(W64, b64, c64, p64, counts, clamp, gates)
    (y * w64.reshape(-1, 1)).sum().backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return y.detach(), [z.detach() for z in pre], [zero(t) for t in W64], [zero(t) for t in b64], zero(c64)


def gradient_blocks(Cn):
    """The parts of the eighteen gradients that different kernels write, as (name, index into [g_W0..g_W8, g_b0..g_b8], column slice):
    in g_W0 and g_W4 the latent columns and the xyz columns come from the column-sum kernels, the activation columns from the GEMM.
    A residual is judged against the largest entry of its own block, so that a small block cannot hide behind a large one."""
    n3 = 509 - Cn
    blocks = [('g_W0 latent', 0, slice(0, Cn)), ('g_W0 xyz', 0, slice(Cn, Cn + 3)),
              ('g_W4 activations', 4, slice(0, n3)), ('g_W4 latent', 4, slice(n3, 509)), ('g_W4 xyz', 4, slice(509, 512))]
    blocks += [('g_W%d' % l, l, slice(None)) for l in (1, 2, 3, 5, 6, 7, 8)]
    return blocks + [('g_b%d' % l, 9 + l, slice(None)) for l in range(9)]


def blockwise_residuals(got, ref, Cn):
    """got, ref: [g_W0..g_W8, g_b0..g_b8] (tensors or arrays). [(name, max |got - ref| / max |ref| of the block, max |ref|)]; a block whose
    reference is all zero reports 0 when got is all zero there and inf otherwise."""
    out = []
    for name, i, cols in gradient_blocks(Cn):
        a, b = np.asarray(got[i], dtype=np.float64)[..., cols], np.asarray(ref[i], dtype=np.float64)[..., cols]
        top = np.abs(b).max()
        err = np.abs(a - b).max()
        out.append((name, (err / top) if top > 0 else (0.0 if err == 0 else np.inf), top))
    return out


def clamped_l1(sdf, target, clamp):
    return (torch.clamp(sdf, -clamp, clamp) - torch.clamp(target, -clamp, clamp)).abs().mean()


def sgd_losses(module64, codes, pts, counts, target, lr, steps, clamp=0.1):
    """Plain SGD on a float64 torch Decoder and the codes, clamped L1 loss against fixed targets: steps + 1 losses, the one
    before every step and the one after the last."""
    codes = codes.clone().double().requires_grad_(True)
    params = list(module64.parameters()) + [codes]
    cnt = torch.as_tensor([int(c) for c in counts], device=codes.device)
    losses = []
    for i in range(steps + 1):
        for p in params:
            p.grad = None
        y = module64(torch.cat([torch.repeat_interleave(codes, cnt, dim=0), pts.double()], 1))
        loss = clamped_l1(y, target.double(), clamp)
        losses.append(loss.item())
        if i == steps:
            break
        loss.backward()
        with torch.no_grad():
            for p in params:
                p -= lr * p.grad
    return losses
