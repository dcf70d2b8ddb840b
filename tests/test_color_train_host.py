"""CPU-only checks of the colour decoder on the layer-wise train path (decode_color_train): the float64 restatement
the GPU tests compare against, the colour weights on the autograd graph, the shape logic, the workspace size and the refusals of the
distr_train_net_* calls that need no GPU."""
import ctypes as C

import numpy as np
import pytest

SIZES = [1, 65, 0, 63, 194]


def _inputs(cs, sizes, seed):
    from distr import fixture
    Ws, bs, cc0 = fixture.make_color_decoder_weights(color_size=cs)
    rs = np.random.RandomState(seed)
    S, n = len(sizes), sum(sizes)
    cc = cc0 + 0.1 * rs.standard_normal((S, cs))
    sc = 0.1 * rs.standard_normal((S, 256))
    pts = (rs.rand(n, 3) - 0.5) * 1.6
    w = rs.standard_normal((n, 3))
    return Ws, bs, cc, sc, pts, w


@pytest.mark.parametrize('weight_norm', [False, True])
@pytest.mark.parametrize('cs', [256, 5])
def test_restatement_equals_float64_decoder(cs, weight_norm):
    """With the gates of its own pre-activations the restatement is autograd through the float64 torch colour Decoder (core.graph,
    last_dim=3, latent 256 + cs, dims[3] += cs): values and every gradient to 1e-12 of the largest entry. Under weight norm the module's
    weight gradient is compared through the fold: the restatement takes the folded float64 weights."""
    import torch
    import color_train_restatement as cr
    from distr import fixture
    sizes = [60, 0, 100]
    Ws, bs, cc, sc, pts, w = _inputs(cs, sizes, 11 + cs)
    assert [W.shape for W in Ws] == fixture.color_layer_shapes(cs)
    dec = cr.color_module(Ws, bs, weight_norm=weight_norm)
    lin = [getattr(dec, 'lin%d' % l) for l in range(9)]
    # (under weight norm: g * v / ||v|| in float64 -- the module's own `weight` attribute is only refreshed by a forward)
    W64 = [(m.weight_v * (m.weight_g / m.weight_v.norm(dim=1, keepdim=True))).detach() if hasattr(m, 'weight_v') else m.weight.detach().clone() for m in lin]
    y, pre, gW, gb, gc, gs = cr.gradients(W64, bs, cc, sc, pts, sizes, w)
    y2, _, gW2, gb2, gc2, gs2 = cr.gradients(W64, bs, cc, sc, pts, sizes, w, gates=[z > 0 for z in pre])
    c64 = torch.tensor(cc, dtype=torch.float64, requires_grad=True)
    s64 = torch.tensor(sc, dtype=torch.float64, requires_grad=True)
    rows = torch.repeat_interleave(torch.cat([s64, c64], 1), torch.tensor(sizes), dim=0)
    Wleaf = []
    if weight_norm:                # gradients w.r.t. the folded weights: evaluate the module's function on leaves that equal them
        Wleaf = [W.clone().requires_grad_(True) for W in W64]
        x = inp = torch.cat([rows, torch.tensor(pts)], 1)
        for l in range(9):
            if l == 4:
                x = torch.cat([x, inp], 1)
            x = torch.nn.functional.linear(x, Wleaf[l], lin[l].bias)
            if l < 8:
                x = torch.relu(x)
        yr = torch.tanh(x)
        assert (yr.detach() - dec(torch.cat([rows, torch.tensor(pts)], 1)).detach()).abs().max() <= 1e-14
    else:
        yr = dec(torch.cat([rows, torch.tensor(pts)], 1))
    assert yr.shape == (160, 3)
    (yr * torch.tensor(w)).sum().backward()
    assert (y - yr.detach()).abs().max() <= 1e-14 and torch.equal(y, y2)
    ref = [(Wleaf[l] if weight_norm else lin[l].weight).grad for l in range(9)] + [m.bias.grad for m in lin] + [c64.grad, s64.grad]
    for name, got in (('own gates', gW + gb + [gc, gs]), ('given gates', gW2 + gb2 + [gc2, gs2])):
        for i, (a, b) in enumerate(zip(got, ref)):
            assert b.abs().max() > 0, i
            assert (a - b).abs().max() <= 1e-12 * b.abs().max(), (name, i)
    assert not gc[1].any() and not gs[1].any()          # the empty segment
    blocks = cr.gradient_blocks(cs)
    assert sum(c.stop - c.start for _, i, c in blocks if i == 0) == 256 + cs + 3 and sum(c.stop - c.start for _, i, c in blocks if i == 4) == 512 + cs


def test_restatement_masks_are_the_dropout_of_the_module():
    """Given masks times the scale behind the relus = the module in training mode with F.dropout handing out those masks."""
    import torch
    import color_train_restatement as cr
    import dropout_restatement as dr
    sizes, cs, p = [5, 9], 5, 0.2
    Ws, bs, cc, sc, pts, w = _inputs(cs, sizes, 3)
    T, scale = dr.threshold(p), dr.scale(p)
    masks = {l: dr.keep_list(77, l, sizes, Ws[l].shape[0], T).astype(np.float64) for l in range(8)}
    y, _ = cr.forward(cr.to64(Ws), cr.to64(bs), *cr.to64([cc, sc, pts]), sizes, masks=masks, scale=scale)
    dec = cr.color_module(Ws, bs, dropout=list(range(8)), dropout_prob=p).train()
    calls = []

    def masked(x, p=0.5, training=True, inplace=False):
        calls.append(len(calls))
        return x * torch.as_tensor(masks[calls[-1]] * scale)
    real = torch.nn.functional.dropout
    torch.nn.functional.dropout = masked
    try:
        rows = torch.repeat_interleave(torch.cat([torch.tensor(sc), torch.tensor(cc)], 1), torch.tensor(sizes), dim=0)
        yr = dec(torch.cat([rows, torch.tensor(pts)], 1))
    finally:
        torch.nn.functional.dropout = real
    assert len(calls) == 8 and (y - yr.detach()).abs().max() <= 1e-14
    assert (y - cr.forward(cr.to64(Ws), cr.to64(bs), *cr.to64([cc, sc, pts]), sizes)[0]).abs().max() > 1e-3


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize('form', ['plain', 'old_style', 'parametrized', 'data_parallel'])
@pytest.mark.parametrize('cs', [256, 5])
def test_effective_weights_torch_color(cs, form):
    """The colour weights on the autograd graph equal decoder_pack.effective_weights on the same module (to 1 ulp under weight norm,
    the parameters themselves without), and a gradient to W reaches weight_g / weight_v."""
    import torch
    import color_train_restatement as cr
    from distr import decoder_pack, fixture
    Ws, bs, _ = fixture.make_color_decoder_weights(color_size=cs)
    if form == 'parametrized':
        dec = cr.color_module(Ws, bs, dtype=torch.float32)
        for l in range(8):
            torch.nn.utils.parametrizations.weight_norm(getattr(dec, 'lin%d' % l))
    else:
        dec = cr.color_module(Ws, bs, weight_norm=(form == 'old_style'), dtype=torch.float32)
    if form == 'data_parallel':
        dec = torch.nn.DataParallel(dec)
    Wt, bt = decoder_pack.effective_weights_torch_color(dec)
    Wn, bn = decoder_pack.effective_weights(dec.state_dict())
    assert decoder_pack.validate_color(Wn, bn) == 256 + cs
    assert [tuple(W.shape) for W in Wt] == fixture.color_layer_shapes(cs)
    for l in range(9):
        assert Wt[l].dtype == torch.float32
        assert _ulps(Wt[l].detach().numpy(), Wn[l]).max() <= (1.0 if form in ('old_style', 'parametrized') else 0.0), l
        assert np.array_equal(bt[l].detach().numpy(), bn[l])
    sum((W * W).sum() + b.sum() for W, b in zip(Wt, bt)).backward()
    params = dict(dec.named_parameters())
    assert len(params) == (26 if form in ('old_style', 'parametrized') else 18)
    assert all(p.grad is not None and p.grad.abs().max() > 0 for p in params.values())
    if form == 'plain':
        assert all(Wt[l] is getattr(dec, 'lin%d' % l).weight for l in range(9))


def test_effective_weights_torch_color_refusals(fixture_decoder):
    import torch
    import color_train_restatement as cr
    from core.graph.deep_sdf_decoder import Decoder
    from distr import decoder_pack, fixture
    Ws, bs, _ = fixture.make_color_decoder_weights(color_size=5)
    ewc = decoder_pack.effective_weights_torch_color
    with pytest.raises(decoder_pack.UnsupportedDecoder, match='latent_in'):
        ewc(Decoder(261, [512] * 8, latent_in=[3], last_dim=3))
    with pytest.raises(decoder_pack.UnsupportedDecoder, match=r'latent = 256 \+ color_size'):        # the SDF decoder: cs = 0
        ewc(Decoder(256, [512] * 8, latent_in=[4]))
    with pytest.raises(decoder_pack.UnsupportedDecoder, match='colour lin3 has shape'):          # dims[3] not widened by cs
        ewc(Decoder(261, [512] * 8, latent_in=[4], last_dim=3))
    with pytest.raises(decoder_pack.UnsupportedDecoder, match='colour lin8 has shape'):
        ewc(Decoder(261, [512] * 3 + [517] + [512] * 4, latent_in=[4], last_dim=1))
    with pytest.raises(decoder_pack.UnsupportedDecoder, match='LayerNorm'):
        ewc(Decoder(261, [512] * 3 + [517] + [512] * 4, latent_in=[4], last_dim=3, norm_layers=(0, 1)))
    dec = cr.color_module(Ws, bs, dtype=torch.float32)
    dec.latent_dropout = True
    dec.train()
    with pytest.raises(decoder_pack.UnsupportedDecoder, match='latent_dropout'):
        ewc(dec)
    dec = cr.color_module(Ws, bs, dtype=torch.float32)
    with torch.no_grad():
        dec.lin4.weight[3, 515] = float('inf')
    with pytest.raises(decoder_pack.UnsupportedDecoder, match='lin4 has non-finite'):
        ewc(dec)
    # the SDF twin keeps refusing the colour decoder
    with pytest.raises(decoder_pack.UnsupportedDecoder):
        decoder_pack.effective_weights_torch(cr.color_module(Ws, bs, dtype=torch.float32))


def test_decode_color_train_argument_errors():
    """Shapes and ValueErrors are decode_color_batch's; points that ask for a gradient and a decoder in training mode without a seed are
    refused; CPU tensors meet the project's RuntimeError (the decoder's checks come first, then the shapes, then the device)."""
    import torch
    import color_train_restatement as cr
    from core.utils import decoder_utils as du
    from distr import decoder_pack, fixture
    assert du.decode_color_train.__module__ == du.decode_color_batch.__module__
    cs = 5
    Ws, bs, _ = fixture.make_color_decoder_weights(color_size=cs)
    dec = cr.color_module(Ws, bs, dtype=torch.float32)
    S, n = len(SIZES), sum(SIZES)
    cc, sc, pts = torch.zeros(S, cs), torch.zeros(S, 256), torch.zeros(n, 3)
    with pytest.raises(RuntimeError, match='decode_color_train: tensors must be on the GPU'):
        du.decode_color_train(dec, cc, sc, pts, counts=SIZES)
    with pytest.raises(RuntimeError, match='must be on the GPU'):
        du.decode_color_train(dec, cc[:1], sc[:1], torch.zeros(S, 7, 3))
    with pytest.raises(ValueError, match='requires_grad'):
        du.decode_color_train(dec, cc, sc, pts.clone().requires_grad_(True), counts=SIZES)
    with pytest.raises(ValueError, match='counts sum to 324, but there are 323 points'):
        du.decode_color_train(dec, cc, sc, pts, counts=[2] + SIZES[1:])
    with pytest.raises(ValueError, match=r'\(S, N, 3\)'):
        du.decode_color_train(dec, cc, sc, pts)
    with pytest.raises(ValueError, match='color_codes has shape'):
        du.decode_color_train(dec, cc[:2], sc, pts, counts=SIZES)
    with pytest.raises(ValueError, match='shape_codes has shape'):
        du.decode_color_train(dec, cc, sc[:3], pts, counts=SIZES)
    drop = cr.color_module(Ws, bs, dropout=[0, 1], dropout_prob=0.2, dtype=torch.float32).train()
    with pytest.raises(decoder_pack.UnsupportedDecoder, match='training mode with dropout'):
        du.decode_color_train(drop, cc, sc, pts, counts=SIZES)
    with pytest.raises(RuntimeError, match='must be on the GPU'):          # with a seed the training-mode decoder is accepted
        du.decode_color_train(drop, cc, sc, pts, counts=SIZES, dropout_seed=5)
    with pytest.raises(ValueError, match='dropout seed'):
        du.decode_color_train(drop, cc, sc, pts, counts=SIZES, dropout_seed=-1)
    drop.latent_dropout = True
    with pytest.raises(decoder_pack.UnsupportedDecoder, match='latent_dropout'):
        du.decode_color_train(drop, cc, sc, pts, counts=SIZES, dropout_seed=5)
    with pytest.raises(decoder_pack.UnsupportedDecoder, match='latent = 256'):          # an SDF decoder
        from core.graph.deep_sdf_decoder import Decoder
        du.decode_color_train(Decoder(256, [512] * 8, latent_in=[4]), cc, sc, pts, counts=SIZES)


def test_code_rows_and_code_gradient_split_run_on_the_host():
    """The code rows are [shape | colour] as color_code_rows builds them; a code of the wrong length is a ValueError naming the shapes;
    the split of the row gradient sums the rows of a shared code."""
    import torch
    from distr import functions
    S, cs = 3, 5
    lay = functions._CodeLayout(256 + cs, torch.device('cpu'))
    cc, sc = torch.arange(S * cs, dtype=torch.float32).reshape(S, cs), -torch.arange(256, dtype=torch.float32).reshape(1, 256)
    rows = functions.color_code_rows(lay, cc, sc, S)
    assert rows.shape == (S, 261) and torch.equal(rows[:, 256:], cc) and torch.equal(rows[:, :256], sc.expand(S, -1))
    assert functions.color_code_rows(lay, cc[:1], sc, S).shape == (1, 261)
    with pytest.raises(ValueError, match=r'colour codes \(1, 5\) or \(3, 5\)'):
        functions.color_code_rows(lay, torch.zeros(S, 6), sc, S)
    g = torch.arange(S * 261, dtype=torch.float32).reshape(S, 261)
    g_c, g_s = functions._split_code_grad(g, cc, sc)
    assert torch.equal(g_c, g[:, 256:]) and g_s.shape == (1, 256) and torch.equal(g_s[0], g[0, :256] + g[1, :256] + g[2, :256])
    assert functions.color_train_net([torch.zeros(512, 256 + cs + 3)]) == (261, 253, 3)
    assert functions.train_net_shapes((261, 253, 3))[:9] == [tuple(s) for s in __import__('distr.fixture', fromlist=['x']).color_layer_shapes(cs)]
    from distr import fixture
    assert functions.train_net_shapes((256, 253, 1))[:9] == [tuple(s) for s in fixture.layer_shapes(256)]


def _net(L, n3, nout):
    from distr import binding
    return binding.TrainNet(latent_size=L, lin3_rows=n3, out_dim=nout)


def test_plan_bytes_with_three_outputs():
    """train_plan_bytes(counts, out_dim) mirrors distr_train_net_workspace_bytes. The carve: z, tanh and dz are three arrays of rows x
    out_dim floats, each rounded up to 256 bytes, so out_dim = 3 costs 3 x (up256(12 rows) - up256(4 rows)) bytes more than out_dim = 1
    -- 3 x rows x (3 - 1) x 4 = 24 bytes per row, rows being a multiple of 64. Nothing else depends on out_dim, nothing on L or
    lin3_rows, and with out_dim = 1 the sizes and offsets are those of the SDF calls."""
    from distr import binding, functions
    binding.build_library()
    L = binding.lib()
    for counts in ([1], [64], SIZES, [0], [700, 1], [65] * 64, [16385]):
        cnt = (C.c_int64 * len(counts))(*counts)
        rows = functions.train_segment_rows(counts)[-1]
        b1, b3 = functions.train_plan_bytes(counts), functions.train_plan_bytes(counts, out_dim=3)
        assert b1 == functions.train_plan_bytes(counts, out_dim=1) == L.distr_train_workspace_bytes(256, len(counts), cnt)
        assert b3 == b1 + 3 * rows * (3 - 1) * 4
        for Lc, n3 in ((512, 253), (257, 253), (1, 1), (769, 509)):
            assert L.distr_train_net_workspace_bytes(C.byref(_net(Lc, n3, 3)), len(counts), cnt) == b3, (counts, Lc, n3)
            assert L.distr_train_net_workspace_bytes(C.byref(_net(Lc, n3, 1)), len(counts), cnt) == b1
            for layer in range(1, 9):
                off = L.distr_train_activation_offset(256, len(counts), cnt, layer)
                assert L.distr_train_net_activation_offset(C.byref(_net(Lc, n3, 3)), len(counts), cnt, layer) == off
                assert L.distr_train_net_activation_offset(C.byref(_net(Lc, n3, 1)), len(counts), cnt, layer) == off


def test_net_refusals_on_the_host():
    """The size functions return 0 for a description the calls refuse; the calls need a context."""
    from distr import binding
    binding.build_library()
    L = binding.lib()
    cnt = (C.c_int64 * len(SIZES))(*SIZES)
    ok = _net(512, 253, 3)
    assert L.distr_train_net_workspace_bytes(C.byref(ok), len(SIZES), cnt) > 0
    bad_size = _net(512, 253, 3)
    bad_size.struct_size -= 4
    for net in (bad_size, _net(512, 253, 2), _net(512, 253, 0), _net(512, 0, 3), _net(512, 510, 3), _net(0, 253, 3), _net(-5, 253, 1)):
        assert L.distr_train_net_workspace_bytes(C.byref(net), len(SIZES), cnt) == 0, (net.latent_size, net.lin3_rows, net.out_dim)
        assert L.distr_train_net_activation_offset(C.byref(net), len(SIZES), cnt, 1) == 0
    assert L.distr_train_net_workspace_bytes(None, len(SIZES), cnt) == 0
    assert L.distr_train_net_workspace_bytes(C.byref(ok), 0, cnt) == 0 and L.distr_train_net_workspace_bytes(C.byref(ok), 65, cnt) == 0
    assert L.distr_train_net_activation_offset(C.byref(ok), len(SIZES), cnt, 0) == 0 and L.distr_train_net_activation_offset(C.byref(ok), len(SIZES), cnt, 9) == 0
    assert L.distr_train_net_forward(None, C.byref(ok), 1, cnt, None, 0, None, -1.0, None, None, 0, None, None) == -1
    assert L.distr_train_net_backward(None, C.byref(ok), 1, cnt, None, 0, None, -1.0, None, None, None, None, None) == -1
    assert C.sizeof(binding.TrainNet) == 16 + 18 * C.sizeof(C.c_void_p)
    assert {'distr_train_net_workspace_bytes', 'distr_train_net_activation_offset', 'distr_train_net_forward', 'distr_train_net_backward'} <= set(binding.TRAIN_EXPORTS)
