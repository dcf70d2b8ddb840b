"""CPU-only checks of the layer-wise train path (decode_sdf_train): the float64 restatement the GPU tests compare
against, the weights on the autograd graph, the shape logic, the slab plan and the host-side part of the C ABI."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

SIZES = [1, 64, 65, 0, 130, 63]


def _module(Ws, bs, weight_norm=False, **kw):
    import torch
    from core.graph.deep_sdf_decoder import Decoder
    from distr import decoder_pack
    dec = Decoder(decoder_pack.latent_size_of(Ws), [512] * 8, norm_layers=tuple(range(8)) if weight_norm else (), latent_in=[4], weight_norm=weight_norm, **kw)
    dec.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in decoder_pack.fixture_state_dict(Ws, bs, weight_norm=weight_norm).items()})
    return dec.eval()


def _weights(Cn, fixture_decoder):
    from distr import fixture
    return fixture_decoder if Cn == 256 else fixture.make_decoder_weights(latent_size=Cn)


@pytest.mark.parametrize('clamp', [0.1, None])
@pytest.mark.parametrize('Cn', [256, 64, 300])
def test_restatement_equals_float64_decoder(fixture_decoder, Cn, clamp):
    """With the gates of its own pre-activations the restatement is autograd through the torch Decoder in float64: every gradient to
    1e-12 of its largest entry."""
    import torch
    import train_restatement as tr
    Ws, bs, latent = _weights(Cn, fixture_decoder)
    rs = np.random.RandomState(3 + Cn)
    sizes = [60, 0, 100]        # (about one point in fifteen lies inside the clamp: enough for a gradient in every tensor)
    codes = latent + 0.3 * np.abs(latent).max() * rs.standard_normal((len(sizes), Cn))
    pts = (rs.rand(sum(sizes), 3) - 0.5) * 1.6
    w = rs.standard_normal(sum(sizes))
    y, pre, gW, gb, gc = tr.gradients(Ws, bs, codes, pts, sizes, w, clamp)
    gates = [z > 0 for z in pre]
    y2, _, gW2, gb2, gc2 = tr.gradients(Ws, bs, codes, pts, sizes, w, clamp, gates=gates)      # given gates = own gates: the same function
    dec = _module(Ws, bs).double()
    c64 = torch.tensor(codes, dtype=torch.float64, requires_grad=True)
    yr = dec(torch.cat([torch.repeat_interleave(c64, torch.tensor(sizes), dim=0), torch.tensor(pts, dtype=torch.float64)], 1))
    if clamp is not None:
        yr = torch.clamp(yr, -clamp, clamp)
    (yr * torch.tensor(w, dtype=torch.float64).reshape(-1, 1)).sum().backward()
    assert (y - yr.detach()).abs().max() <= 1e-14 and torch.equal(y, y2)
    ref = [getattr(dec, 'lin%d' % l).weight.grad for l in range(9)] + [getattr(dec, 'lin%d' % l).bias.grad for l in range(9)] + [c64.grad]
    for name, got in (('own gates', gW + gb + [gc]), ('given gates', gW2 + gb2 + [gc2])):
        for i, (a, b) in enumerate(zip(got, ref)):
            assert b.abs().max() > 0, i
            assert (a - b).abs().max() <= 1e-12 * b.abs().max(), (name, i)
    assert not gc[1].any()          # the empty segment


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize('form', ['plain', 'old_style', 'parametrized', 'data_parallel'])
def test_effective_weights_torch(fixture_decoder, form):
    """The weights on the autograd graph equal the packed path's (decoder_pack.effective_weights) to 1 ulp, and a gradient to W reaches
    the module's parameters: weight_g / weight_v under weight norm."""
    import torch
    from distr import decoder_pack
    Ws, bs, _ = fixture_decoder
    if form == 'parametrized':
        dec = _module(Ws, bs)
        for l in range(8):
            torch.nn.utils.parametrizations.weight_norm(getattr(dec, 'lin%d' % l))
    else:
        dec = _module(Ws, bs, weight_norm=(form == 'old_style'))
    if form == 'data_parallel':
        dec = torch.nn.DataParallel(dec)
    Wt, bt = decoder_pack.effective_weights_torch(dec)
    Wn, bn = decoder_pack.effective_weights(dec.state_dict())
    assert len(Wt) == 9 and len(bt) == 9
    for l in range(9):
        assert Wt[l].dtype == torch.float32 and tuple(Wt[l].shape) == Wn[l].shape
        assert _ulps(Wt[l].detach().numpy(), Wn[l]).max() <= 1.0, l
        assert np.array_equal(bt[l].detach().numpy(), bn[l])
    sum((W * W).sum() + b.sum() for W, b in zip(Wt, bt)).backward()
    params = dict(dec.named_parameters())
    assert len(params) == (26 if form in ('old_style', 'parametrized') else 18)
    for k, p in params.items():
        assert p.grad is not None and p.grad.abs().max() > 0, k
    if form == 'plain':
        assert all(Wt[l] is getattr(dec, 'lin%d' % l).weight for l in range(9))       # the parameters themselves: nothing is copied


def test_effective_weights_torch_refusals(fixture_decoder):
    import torch
    from core.graph.deep_sdf_decoder import Decoder
    from distr import decoder_pack
    Ws, bs, _ = fixture_decoder
    with pytest.raises(decoder_pack.UnsupportedDecoder, match='latent_in'):
        decoder_pack.effective_weights_torch(Decoder(256, [512] * 8, latent_in=[3]))
    with pytest.raises(decoder_pack.UnsupportedDecoder, match='lin3 has shape'):
        decoder_pack.effective_weights_torch(Decoder(256, [512] * 3 + [300] + [512] * 4, latent_in=[4]))
    with pytest.raises(decoder_pack.UnsupportedDecoder, match='LayerNorm'):
        decoder_pack.effective_weights_torch(Decoder(256, [512] * 8, latent_in=[4], norm_layers=(0, 1)))
    dec = _module(Ws, bs, latent_dropout=True)
    dec.train()
    with pytest.raises(decoder_pack.UnsupportedDecoder, match='latent_dropout'):
        decoder_pack.effective_weights_torch(dec)
    dec = _module(Ws, bs)
    with torch.no_grad():
        dec.lin5.bias[7] = float('nan')
    with pytest.raises(decoder_pack.UnsupportedDecoder, match='lin5 has non-finite'):
        decoder_pack.effective_weights_torch(dec)


def test_decode_sdf_train_argument_errors(fixture_decoder):
    import torch
    from core.utils import decoder_utils as du
    from distr import decoder_pack
    Cn = 8
    lat = torch.zeros(len(SIZES), Cn)
    pts = torch.zeros(sum(SIZES), 3)
    x, counts, shape = du._train_layout(Cn, lat, pts, SIZES)
    assert x.shape == (323, 3) and counts == SIZES and shape == (323,)
    x, counts, shape = du._train_layout(Cn, lat[:3], torch.zeros(3, 5, 3), None)
    assert x.shape == (15, 3) and counts == [5, 5, 5] and shape == (3, 5)
    with pytest.raises(ValueError, match=r'\(S, C\) = \(S, 8\)'):
        du._train_layout(Cn, torch.zeros(len(SIZES), Cn + 1), pts, SIZES)
    with pytest.raises(ValueError, match='counts sum to 324, but there are 323 points'):
        du._train_layout(Cn, lat, pts, [2] + SIZES[1:])
    with pytest.raises(ValueError, match='segment sizes'):
        du._train_layout(Cn, lat, pts, SIZES[:-1])
    with pytest.raises(ValueError, match=r'\(S, N, 3\)'):
        du._train_layout(Cn, lat, pts, None)
    with pytest.raises(ValueError, match='requires_grad'):
        du._train_layout(Cn, lat, pts.clone().requires_grad_(True), SIZES)
    with pytest.raises(NotImplementedError):
        du._train_layout(Cn, None, pts, SIZES)
    # through the public function: the decoder's checks come first, then the shapes, then the device
    Ws, bs, _ = fixture_decoder
    dec = _module(Ws, bs)
    lat = torch.zeros(len(SIZES), 256)
    with pytest.raises(ValueError, match='requires_grad'):
        du.decode_sdf_train(dec, lat, pts.clone().requires_grad_(True), counts=SIZES)
    with pytest.raises(ValueError, match=r'\(S, C\) = \(S, 256\)'):
        du.decode_sdf_train(dec, lat[:, :255], pts, counts=SIZES)
    with pytest.raises(RuntimeError, match='must be on the GPU'):
        du.decode_sdf_train(dec, lat, pts, counts=SIZES)
    drop = _module(Ws, bs, dropout=[0, 1], dropout_prob=0.2)
    drop.train()
    with pytest.raises(decoder_pack.UnsupportedDecoder, match='training mode with dropout'):
        du.decode_sdf_train(drop, lat, pts, counts=SIZES)


def test_slab_plan_is_a_pure_function_of_the_row_count():
    """At most 64 slabs, every row in exactly one, the length a multiple of 64 and at least 256; the library's plan is the Python
    mirror's; the smallest slab is short enough for a three-slab test."""
    from distr import binding, functions
    binding.build_library()
    L = binding.lib()
    assert functions.train_slab_plan(1)[0] == functions.TRAIN_SLAB_MIN <= 1024
    for rows in [0, 1, 64, 255, 256, 257, 512, 513, 576, 64 * 256, 64 * 256 + 1, 16384 * 64, 16384 * 64 + 64, 999936, (1 << 30) + 4096]:
        length, n = functions.train_slab_plan(rows)
        ln, nn = C.c_int64(), C.c_int32()
        L.distr_train_slab_plan(rows, C.byref(ln), C.byref(nn))
        assert (ln.value, nn.value) == (length, n), rows
        assert n <= functions.TRAIN_MAX_SLABS == 64 and length % 64 == 0 and length >= 256
        assert (n - 1) * length < rows <= n * length if rows else n == 0        # slabs [z * length, min(rows, (z + 1) * length)): none empty
    L0 = functions.train_slab_plan(1)[0]
    assert functions.train_slab_plan(functions.train_segment_rows([2 * L0 + 1])[-1]) == (L0, 3)


def test_train_abi_declared_and_exported():
    from distr import binding
    hdr = open(os.path.join(ROOT, 'include', 'distr_train.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(distr_[a-z0-9_]+)\s*\(', hdr))
    assert declared == set(binding.TRAIN_EXPORTS)
    distr_h = open(os.path.join(ROOT, 'include', 'distr.h')).read()
    assert '#include "distr_train.h"' in distr_h and re.search(r'#define DISTR_ABI_VERSION %du' % binding.ABI_VERSION, distr_h)
    assert binding.ABI_VERSION == 6
    binding.build_library()
    L = binding.lib()
    for name in binding.TRAIN_EXPORTS:
        getattr(L, name)
    assert 'distr_train.h' in binding.HEADERS and 'distr_train.hpp' in binding.SOURCES


def test_train_workspace_layout_is_host_code():
    """Sizes, activation offsets and segment rows need no context: 0 / -1 for what the calls refuse; 16 KB per row of saved layer inputs."""
    from distr import binding, functions
    binding.build_library()
    L = binding.lib()
    cnt = (C.c_int64 * len(SIZES))(*SIZES)
    rows = functions.train_segment_rows(SIZES)
    assert rows == [0, 64, 128, 256, 256, 448, 512]
    assert [L.distr_train_segment_row(len(SIZES), cnt, s) for s in range(len(SIZES) + 1)] == rows
    assert L.distr_train_segment_row(len(SIZES), cnt, len(SIZES) + 1) == -1 and L.distr_train_segment_row(len(SIZES), cnt, -1) == -1
    need = L.distr_train_workspace_bytes(256, len(SIZES), cnt)
    offs = [L.distr_train_activation_offset(256, len(SIZES), cnt, l) for l in range(1, 9)]
    assert all(b - a == rows[-1] * 512 * 4 for a, b in zip(offs, offs[1:])) and offs[0] % 256 == 0 and offs[0] > 0
    assert need >= offs[-1] + 3 * rows[-1] * 512 * 4 + 512 * 512 * 4        # X_8, two delta buffers, at least one slab
    assert L.distr_train_activation_offset(256, len(SIZES), cnt, 0) == 0 and L.distr_train_activation_offset(256, len(SIZES), cnt, 9) == 0
    neg = (C.c_int64 * 2)(4, -1)
    for bad in ((256, 0, cnt), (256, 65, cnt), (256, 2, neg), (256, 2, None), (0, 6, cnt), (509, 6, cnt)):
        assert L.distr_train_workspace_bytes(*bad) == 0 and L.distr_train_activation_offset(*bad, 1) == 0, bad
    assert L.distr_train_workspace_bytes(1, 6, cnt) == need == L.distr_train_workspace_bytes(508, 6, cnt)      # the layout does not depend on C
    assert L.distr_train_forward(None, None, 1, cnt, None, 0, None, 0.1, None, None, 0, None) == -1           # no context: DISTR_ERR_INVALID_ARG


def test_byte_cap_is_read_at_call_time(monkeypatch):
    from distr import functions
    monkeypatch.delenv('DISTR_TRAIN_MAX_BYTES', raising=False)
    assert functions.train_max_bytes() == 32 << 30
    monkeypatch.setenv('DISTR_TRAIN_MAX_BYTES', '4096')
    assert functions.train_max_bytes() == 4096
