"""The entry points of the layer-wise path that take distr_train_weights (distr_train_forward / _backward and their _dropout forms,
include/distr_train.h) against the calls on a description (distr_train_net_*): the Python layer describes every network, the SDF
decoder as (C, 509 - C, 1), so these tests are what keeps a value check on the older names. Byte for byte: the output, the real rows of
X_1..X_8 (each workspace read through its own offset function; X_4: its 509 - C written columns), the eighteen gradients and g_latent.

Code lengths 8 and 256; segments (5, 0, 64, 65) -- a short tile, an empty segment, an exact tile, a tile and one row: 256 padded rows;
a code per segment and a shared one (latent_stride 0); clamp 0.1 and none. Dropout: layers 0, 3 and 7, p = 0.5, segment_base 3.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTS = [5, 0, 64, 65]
DROPOUT = dict(layer_mask=(1 << 0) | (1 << 3) | (1 << 7), threshold=1 << 31, scale=2.0, seed=0x5EED0003, segment_base=3)      # p = 0.5
_inputs = {}


def inputs(Cn):
    """(weights [W0..W8, b0..b8], codes (S, C), points, upstream gradient) on the GPU, made once per code length and never written to"""
    import torch
    from distr import fixture
    if Cn not in _inputs:
        Ws, bs, latent = fixture.make_decoder_weights(latent_size=Cn)
        rs = np.random.RandomState(4100 + Cn)
        n = sum(COUNTS)
        codes = (latent + 0.3 * np.abs(latent).max() * rs.standard_normal((len(COUNTS), Cn))).astype(np.float32)
        pts = ((rs.rand(n, 3) - 0.5) * 1.6).astype(np.float32)
        g = rs.standard_normal(n).astype(np.float32)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
        _inputs[Cn] = ([dev(a) for a in list(Ws) + list(bs)], dev(codes), dev(pts), dev(g))
    return _inputs[Cn]


def run(Cn, shared, clamp, legacy, drop):
    """Forward and backward through one family of entry points -> the tensors to compare, by name"""
    import torch
    import train_abi
    from distr import binding, functions
    weights, codes, pts, g = inputs(Cn)
    lat = codes[:1].contiguous() if shared else codes
    stride = 0 if shared else Cn
    ctx = functions._train_context(0)
    L, p = ctx.L, binding.ptr
    S, n = len(COUNTS), sum(COUNTS)
    cnt = (C.c_int64 * S)(*COUNTS)
    net = functions._train_net_struct(weights, (Cn, 509 - Cn, 1))
    tw = train_abi.train_weights(weights, Cn)
    need = L.distr_train_workspace_bytes(Cn, S, cnt) if legacy else L.distr_train_net_workspace_bytes(C.byref(net), S, cnt)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    out = torch.empty(n, 1, device='cuda')
    grads = [torch.empty_like(w) for w in weights]
    g_lat = torch.empty(S, Cn, device='cuda')
    tg = train_abi.train_grads(grads)
    td = binding.TrainDropout(**DROPOUT) if drop else None
    cl = -1.0 if clamp is None else clamp
    fwd = (S, cnt, p(lat), stride, p(pts), cl, p(out), p(ws), need, ctx.stream())
    bwd = (S, cnt, p(lat), stride, p(g), cl, p(ws), C.byref(tg), p(g_lat), ctx.stream())
    if not legacy:
        ctx.check(L.distr_train_net_forward(ctx.h, C.byref(net), *(fwd + (C.byref(td) if drop else None,))))
        ctx.check(L.distr_train_net_backward(ctx.h, C.byref(net), *(bwd + (C.byref(td) if drop else None,))))
    elif drop:
        ctx.check(L.distr_train_forward_dropout(ctx.h, C.byref(tw), *(fwd + (C.byref(td),))))
        ctx.check(L.distr_train_backward_dropout(ctx.h, C.byref(tw), *(bwd + (C.byref(td),))))
    else:
        ctx.check(L.distr_train_forward(ctx.h, C.byref(tw), *fwd))
        ctx.check(L.distr_train_backward(ctx.h, C.byref(tw), *bwd))
    torch.cuda.synchronize()
    res = {'out': out, 'g_latent': g_lat}
    res.update(('g_W%d' % l, grads[l]) for l in range(9))
    res.update(('g_b%d' % l, grads[9 + l]) for l in range(9))
    seg_rows = functions.train_segment_rows(COUNTS)
    assert seg_rows[-1] == 256
    real = torch.tensor([seg_rows[s] + i for s, c in enumerate(COUNTS) for i in range(c)], device='cuda')
    base = (-ws.data_ptr()) % 256
    for layer in range(1, 9):
        off = L.distr_train_activation_offset(Cn, S, cnt, layer) if legacy else L.distr_train_net_activation_offset(C.byref(net), S, cnt, layer)
        assert off > 0
        X = ws[base + off: base + off + 256 * 512 * 4].view(torch.float32).reshape(256, 512)
        res['X_%d' % layer] = X[real][:, :509 - Cn if layer == 4 else 512].contiguous()
    return res


@pytest.mark.parametrize('clamp', [0.1, None], ids=['clamp', 'noclamp'])
@pytest.mark.parametrize('shared', [False, True], ids=['codes', 'shared'])
@pytest.mark.parametrize('Cn', [8, 256])
def test_weight_struct_calls_are_the_net_calls(Cn, shared, clamp):
    """distr_train_forward + _backward equal the net calls on (C, 509 - C, 1) with drop = NULL; distr_train_forward_dropout +
    _backward_dropout equal the net calls with the same struct."""
    import torch
    for drop in (False, True):
        a, b = run(Cn, shared, clamp, True, drop), run(Cn, shared, clamp, False, drop)
        assert sorted(a) == sorted(b) and len(a) == 2 + 18 + 8
        for name in sorted(a):
            assert a[name].shape == b[name].shape and torch.equal(a[name].view(torch.int32), b[name].view(torch.int32)), (name, drop)
        assert torch.isfinite(a['out']).all() and a['out'].abs().max().item() > 0
        if drop:          # the dropout ran: exact zeros behind lin0 where the plain run has none of its own
            assert (a['X_1'] == 0).float().mean().item() > 0.4
