"""CPU-only checks of the spatial-gradient train path (decode_sdf_gradient_train): the float64 closed form the GPU
tests compare against (tests/train_grad_restatement.py) equals float64 torch.autograd double backward through the project's Decoder;
the shape logic and refusals of the public call; the host-side part of the C ABI."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

SIZES = [5, 0, 7]
P_DROP = 0.2
SEED = 0x1234567890ABCDEF


def _module(Ws, bs, weight_norm=False, **kw):
    import torch
    from core.graph.deep_sdf_decoder import Decoder
    from distr import decoder_pack
    dec = Decoder(decoder_pack.latent_size_of(Ws), [512] * 8, norm_layers=tuple(range(8)) if weight_norm else (), latent_in=[4], weight_norm=weight_norm, **kw)
    dec.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in decoder_pack.fixture_state_dict(Ws, bs, weight_norm=weight_norm).items()})
    return dec.eval()


def _library_keeps(Cn, sizes, threshold):
    """keeps[l] (sum sizes, units of lin_l) from distr_train_dropout_keep, one call per (layer, segment, point, unit)"""
    from distr import binding
    binding.build_library()
    L = binding.lib()
    keeps = []
    for l in range(8):
        units = 509 - Cn if l == 3 else 512
        keeps.append(np.array([[L.distr_train_dropout_keep(SEED, threshold, l, s, i, n) for n in range(units)]
                               for s, cnt in enumerate(sizes) for i in range(cnt)], dtype=bool))
    return keeps


@pytest.mark.parametrize('dropout', [False, True])
@pytest.mark.parametrize('weight_norm', [False, True])
@pytest.mark.parametrize('Cn', [256, 64, 300])
def test_restatement_equals_float64_double_backward(fixture_decoder, monkeypatch, Cn, weight_norm, dropout):
    """f, g, the eighteen weight gradients (at weight_g / weight_v under weight norm) and the code rows of L = sum(f phi) + sum(g u):
    the closed form against autograd with create_graph=True through the Decoder in float64, to 1e-10 of each tensor's largest entry.
    With dropout the Decoder's functional.dropout calls take the keeps of distr_train_dropout_keep in layer order."""
    import torch
    import dropout_restatement as dr
    import train_grad_restatement as tg
    from distr import fixture
    Ws, bs, latent = fixture_decoder if Cn == 256 else fixture.make_decoder_weights(latent_size=Cn)
    rs = np.random.RandomState(11 + Cn)
    n = sum(SIZES)
    codes = latent + 0.3 * np.abs(latent).max() * rs.standard_normal((len(SIZES), Cn))
    pts = (rs.rand(n, 3) - 0.5) * 1.6
    phi, u = rs.standard_normal(n), rs.standard_normal((n, 3))
    kw = dict(dropout=list(range(8)), dropout_prob=P_DROP) if dropout else {}
    dec = _module(Ws, bs, weight_norm=weight_norm, **kw).double()
    keeps, scale = None, 1.0
    if dropout:
        keeps, scale = _library_keeps(Cn, SIZES, dr.threshold(P_DROP)), dr.scale(P_DROP)
        assert all(0.6 < k.mean() < 0.95 for k in keeps)
        dec.train()
        masks = iter(keeps)
        monkeypatch.setattr(torch.nn.functional, 'dropout', lambda x, p=0.5, training=True, inplace=False: x * (torch.from_numpy(next(masks)).to(x.dtype) * scale))
    c64 = torch.tensor(codes, dtype=torch.float64, requires_grad=True)
    x64 = torch.tensor(pts, dtype=torch.float64, requires_grad=True)
    y = dec(torch.cat([torch.repeat_interleave(c64, torch.tensor(SIZES), dim=0), x64], 1))
    g, = torch.autograd.grad(y.sum(), x64, create_graph=True)
    ((y[:, 0] * torch.from_numpy(phi)).sum() + (g * torch.from_numpy(u)).sum()).backward()

    params = dict(dec.named_parameters())
    if weight_norm:
        W_eff = [params['lin%d.weight_v' % l].detach().clone().requires_grad_(True) for l in range(8)]
        g_eff = [params['lin%d.weight_g' % l].detach().clone().requires_grad_(True) for l in range(8)]
        Wt = [v * (gg / v.norm(dim=1, keepdim=True)) for v, gg in zip(W_eff, g_eff)] + [params['lin8.weight'].detach()]
    else:
        Wt = [params['lin%d.weight' % l].detach() for l in range(9)]
    bt = [params['lin%d.bias' % l].detach() for l in range(9)]
    r = tg.restate([w.detach().numpy() for w in Wt], [b.numpy() for b in bt], codes, pts, SIZES, phi, u, keeps=keeps, scale=scale)

    def close(name, got, ref):
        ref = ref.detach().numpy()
        top = np.abs(ref).max()
        assert top > 0, name
        assert np.abs(np.asarray(got) - ref).max() <= 1e-10 * top, (name, np.abs(np.asarray(got) - ref).max() / top)
    close('f', r['f'], y)
    close('g', r['g'], g)
    if weight_norm:       # the closed form's g_W on the fold W = v g / |v|, carried to weight_g / weight_v by autograd
        torch.autograd.backward(Wt[:8], [torch.from_numpy(a) for a in r['g_W'][:8]])
        for l in range(8):
            close('lin%d.weight_v' % l, W_eff[l].grad, params['lin%d.weight_v' % l].grad)
            close('lin%d.weight_g' % l, g_eff[l].grad, params['lin%d.weight_g' % l].grad)
        close('lin8.weight', r['g_W'][8], params['lin8.weight'].grad)
    else:
        for l in range(9):
            close('g_W%d' % l, r['g_W'][l], params['lin%d.weight' % l].grad)
    for l in range(9):
        close('g_b%d' % l, r['g_b'][l], params['lin%d.bias' % l].grad)
    close('g_codes', r['g_codes'], c64.grad)
    assert not r['g_codes'][1].any()        # the empty segment


def test_with_u_zero_it_is_the_value_gradient(fixture_decoder):
    """u = 0: the gradients of tests/train_restatement.py (sum(f phi), no clamp)."""
    import train_grad_restatement as tg
    import train_restatement as tr
    Ws, bs, latent = fixture_decoder
    rs = np.random.RandomState(5)
    n = sum(SIZES)
    codes = latent + 0.3 * np.abs(latent).max() * rs.standard_normal((len(SIZES), 256))
    pts, phi = (rs.rand(n, 3) - 0.5) * 1.6, rs.standard_normal(n)
    r = tg.restate(Ws, bs, codes, pts, SIZES, phi, None)
    y, _, gW, gb, gc = tr.gradients(Ws, bs, codes, pts, SIZES, phi, None)
    for got, ref in zip([r['f']] + r['g_W'] + r['g_b'] + [r['g_codes']], [y] + gW + gb + [gc]):
        assert np.abs(got - ref.numpy()).max() <= 1e-12 * np.abs(ref.numpy()).max()


def test_shapes_and_argument_errors(fixture_decoder):
    """decode_sdf_gradient_train's shape logic runs before anything touches the GPU: decode_sdf_train's errors, under its own name."""
    import torch
    from core.utils import decoder_utils as du
    Ws, bs, _ = fixture_decoder
    dec = _module(Ws, bs)
    lat, pts = torch.zeros(2, 256), torch.zeros(8, 3)
    assert du._gradient_train_layout(256, lat, pts, [5, 3])[1:] == ([5, 3], (8,))
    assert du._gradient_train_layout(256, lat, pts.reshape(2, 4, 3), None)[1:] == ([4, 4], (2, 4))
    with pytest.raises(ValueError, match=r'decode_sdf_gradient_train: points.requires_grad.*decode_sdf_gradient_batch'):
        du.decode_sdf_gradient_train(dec, lat, pts.clone().requires_grad_(True), counts=[5, 3])
    with pytest.raises(ValueError, match='counts sum to 7'):
        du.decode_sdf_gradient_train(dec, lat, pts, counts=[5, 2])
    with pytest.raises(ValueError, match=r'takes \(S, C\)'):
        du.decode_sdf_gradient_train(dec, torch.zeros(2, 255), pts, counts=[5, 3])
    with pytest.raises(ValueError, match='without counts'):
        du.decode_sdf_gradient_train(dec, lat, pts)
    with pytest.raises(NotImplementedError, match='latent_vectors=None'):
        du.decode_sdf_gradient_train(dec, None, pts, counts=[5, 3])
    with pytest.raises(RuntimeError, match='decode_sdf_gradient_train: tensors must be on the GPU'):
        du.decode_sdf_gradient_train(dec, lat, pts, counts=[5, 3])
    drop = _module(Ws, bs, dropout=[0, 1], dropout_prob=0.2)
    drop.train()
    from distr import decoder_pack
    with pytest.raises(decoder_pack.UnsupportedDecoder, match='training mode with dropout'):
        du.decode_sdf_gradient_train(drop, lat, pts, counts=[5, 3])
    with pytest.raises(ValueError, match='dropout seed'):
        du.decode_sdf_gradient_train(drop, lat, pts, counts=[5, 3], dropout_seed=-1)
    doc = du.decode_sdf_gradient_train.__doc__
    assert 'NO clamp' in doc and 'factor 3' in doc and 'clamp mask' in doc


def test_grad_abi_declared_and_exported():
    from distr import binding
    names = ['distr_train_grad_workspace_bytes', 'distr_train_grad_forward', 'distr_train_grad_backward']
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'distr_train.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(distr_[a-z0-9_]+)\s*\(', hdr))
    assert set(names) <= declared and set(names) <= set(binding.TRAIN_EXPORTS)
    assert binding.ABI_VERSION == 6
    binding.build_library()
    L = binding.lib()
    for name in names:
        getattr(L, name)


def test_grad_workspace_size_is_host_code():
    """distr_train_grad_workspace_bytes needs no context: the train carve plus eight tangent buffers, the padded upstream and the row
    scalars (40 KB + 44 bytes per padded row against 24 KB); 0 for a refused description and for out_dim = 3."""
    from distr import binding
    binding.build_library()
    L = binding.lib()
    sizes = [1, 64, 65, 0, 130, 63]
    rows = 512
    cnt = (C.c_int64 * len(sizes))(*sizes)
    net = lambda *a: C.byref(binding.TrainNet(latent_size=a[0], lin3_rows=a[1], out_dim=a[2]))
    base = L.distr_train_net_workspace_bytes(net(256, 253, 1), len(sizes), cnt)
    need = L.distr_train_grad_workspace_bytes(net(256, 253, 1), len(sizes), cnt)
    assert base > 0 and base + rows * (8 * 2048 + 44) <= need <= base + rows * (8 * 2048 + 44) + 13 * 256      # (13 arrays, each 256-byte aligned)
    assert L.distr_train_grad_workspace_bytes(net(64, 445, 1), len(sizes), cnt) == need                         # the layout does not depend on C
    assert L.distr_train_grad_workspace_bytes(net(256, 253, 3), len(sizes), cnt) == 0                           # the colour net has no such gradient
    assert L.distr_train_net_workspace_bytes(net(256, 253, 3), len(sizes), cnt) > 0
    neg = (C.c_int64 * 2)(4, -1)
    for bad in ((net(256, 253, 2), 6, cnt), (net(0, 253, 1), 6, cnt), (net(256, 0, 1), 6, cnt), (net(256, 510, 1), 6, cnt), (net(256, 253, 1), 0, cnt),
                (net(256, 253, 1), 65, cnt), (net(256, 253, 1), 2, neg), (net(256, 253, 1), 2, None), (None, 6, cnt)):
        assert L.distr_train_grad_workspace_bytes(*bad) == 0, bad
    tn = binding.TrainNet(latent_size=256, lin3_rows=253, out_dim=1)
    tn.struct_size -= 4
    assert L.distr_train_grad_workspace_bytes(C.byref(tn), len(sizes), cnt) == 0
    assert L.distr_train_grad_forward(None, None, 1, cnt, None, 0, None, None, None, None, 0, None, None) == -1     # no context: DISTR_ERR_INVALID_ARG
    assert L.distr_train_grad_backward(None, None, 1, cnt, None, 0, None, None, None, None, None, None, None) == -1
