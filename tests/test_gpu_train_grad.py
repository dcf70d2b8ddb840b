"""Training through the spatial gradient: decode_sdf_gradient_train, (f, grad_x f) on the layer-wise path with gradients to the weights
and the codes through BOTH outputs (distr_train_grad_*).

References: decode_sdf_batch (2e-6, the project's bar) for f; for g and for every gradient the float64 closed form of
tests/train_grad_restatement.py run WITH THE GATES THE GPU RUN SAVED (tests/test_train_grad_host.py pins it to float64 autograd double
backward through the Decoder), and decode_sdf_gradient_batch(clamp_dist=None) / 3 for g. Bar: 1e-4 of the largest entry -- the project's
bar for a different f32 summation order -- per tensor, per block of a tensor (train_restatement.gradient_blocks) and per code-gradient
row. Three upstream cases: phi = dL/df random with u = dL/dg absent, phi absent with u random, both random. Shapes are those of
tests/test_gpu_train.py: segments [1, 64, 65, 0, 130, 63], a shared code, 2 L + 1 rows (three K slabs), 65 segments (two chunks)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [1, 64, 65, 0, 130, 63]
CODE_LENGTHS = (256, 64, 300)
UPSTREAMS = ('phi', 'u', 'both')
P_DROP, SEED = 0.2, 0x5DEECE66D1234567


def _module(Ws, bs, weight_norm=False, **kw):
    import torch
    from core.graph.deep_sdf_decoder import Decoder
    from distr import decoder_pack
    dec = Decoder(decoder_pack.latent_size_of(Ws), [512] * 8, norm_layers=tuple(range(8)) if weight_norm else (), latent_in=[4], weight_norm=weight_norm, **kw)
    dec.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in decoder_pack.fixture_state_dict(Ws, bs, weight_norm=weight_norm).items()})
    return dec.cuda().eval()


def _weights_of(dec):
    from distr import decoder_pack
    Wt, bt = decoder_pack.effective_weights_torch(dec)
    return [t.detach() for t in Wt + bt]


def _segments(sizes=SIZES):
    at = 0
    for s, n in enumerate(sizes):
        yield s, at, at + n
        at += n


def _gates(saved):
    """[X_(l+1) > 0] at the list's points, in point order: the ReLU gate and the dropout keep at once"""
    import torch
    idx = torch.cat([torch.arange(*saved.rows(s)) for s in range(len(saved.counts))]).cuda()
    return [(saved.activations(l + 1)[idx] > 0).cpu() for l in range(8)]


def _pick(case, phi, u):
    return (phi if case in ('phi', 'both') else None), (u if case in ('u', 'both') else None)


def _run(weights, codes, pts, sizes, phi, u, dropout=None, cases=UPSTREAMS):
    """One forward and one backward per upstream case on the low-level calls, everything on the CPU:
    dict(f, g, gates, case -> (grads [g_W0..g_W8, g_b0..g_b8], g_lat (S, C)))"""
    from distr import functions
    (f, g), saved = functions.train_grad_forward(weights, codes, pts, sizes, dropout=dropout)
    out = dict(f=f.cpu(), g=g.cpu(), gates=_gates(saved))
    for case in cases:
        grads, g_lat = functions.train_grad_backward(saved, *_pick(case, phi, u))
        out[case] = ([t.cpu() for t in grads], g_lat.cpu())
    return out


def _assert_gradients(got, ref, sizes, tag):
    """got = (grads, g_lat) of a GPU run, ref = train_grad_restatement.restate(...): 1e-4 of the largest entry per tensor, per block, per
    code row; prints the worst block"""
    import train_restatement as tr
    grads, g_lat = got
    refs = ref['g_W'] + ref['g_b']
    for i, (a, b) in enumerate(zip(grads, refs)):
        name = ('g_W%d' % i) if i < 9 else ('g_b%d' % (i - 9))
        top = np.abs(b).max()
        assert top > 0, (tag, name)
        rel = np.abs(a.double().numpy() - b).max() / top
        assert rel <= 1e-4, (tag, name, rel)
    blocks = tr.blockwise_residuals([t.numpy() for t in grads], refs, grads[0].shape[1] - 3)
    worst = max(blocks, key=lambda t: t[1])
    print('%s: worst block %s, %.3e of its largest entry' % (tag, worst[0], worst[1]))
    for name, rel, top in blocks:
        assert rel <= 1e-4, (tag, 'block', name, rel, top)
    worst_row = 0.0
    for s, a, b in _segments(sizes):
        if a == b:
            assert not g_lat[s].any(), (tag, 'the empty segment has a code gradient')
            continue
        top = np.abs(ref['g_codes'][s]).max()
        assert top > 0, (tag, s)
        rel = np.abs(g_lat[s].double().numpy() - ref['g_codes'][s]).max() / top
        worst_row = max(worst_row, rel)
        assert rel <= 1e-4, (tag, 'g_latent row', s, rel)
    print('%s: worst code-gradient row %.3e of its largest entry' % (tag, worst_row))
    return worst[1]


def _inputs(latent, Cn, sizes, seed, shared=False):
    rs = np.random.RandomState(seed)
    n = sum(sizes)
    codes = (latent + 0.3 * np.abs(latent).max() * rs.standard_normal((1 if shared else len(sizes), Cn))).astype(np.float32)
    pts = ((rs.rand(n, 3) - 0.5) * 1.6).astype(np.float32)
    phi = rs.standard_normal((n, 1)).astype(np.float32)
    u = rs.standard_normal((n, 3)).astype(np.float32)
    return codes, pts, phi, u


def _refs(Ws, bs, codes, pts, sizes, phi, u, r, cases=UPSTREAMS, **kw):
    import train_grad_restatement as tg
    S = len(sizes)
    rows = np.repeat(codes, S, 0) if codes.shape[0] == 1 else codes
    return {case: tg.restate(Ws, bs, rows, pts, sizes, *_pick(case, phi, u), gates=r['gates'], **kw) for case in cases}


@pytest.fixture(scope='module', params=CODE_LENGTHS)
def case(request, fixture_decoder):
    """Per code length, made once and never modified: decoder, inputs, the GPU run (twice), the fused references and the float64
    closed form with the GPU's gates for the three upstream cases."""
    import torch
    from core.utils.decoder_utils import decode_sdf_batch, decode_sdf_gradient_batch
    from distr import fixture
    Cn = request.param
    Ws, bs, latent = fixture_decoder if Cn == 256 else fixture.make_decoder_weights(latent_size=Cn)
    codes, pts, phi, u = _inputs(latent, Cn, SIZES, 200 + Cn)
    dec = _module(Ws, bs)
    c = dict(Cn=Cn, Ws=Ws, bs=bs, dec=dec, weights=_weights_of(dec), np=(codes, pts, phi, u))
    c['codes'], c['pts'], c['phi'], c['u'] = (torch.from_numpy(a).cuda() for a in (codes, pts, phi, u))
    c['run'] = _run(c['weights'], c['codes'], c['pts'], SIZES, c['phi'], c['u'])
    c['again'] = _run(c['weights'], c['codes'], c['pts'], SIZES, c['phi'], c['u'])
    c['batch'] = decode_sdf_batch(dec, c['codes'], c['pts'], counts=SIZES, clamp_dist=None, no_grad=True).cpu()
    c['gbatch'] = (decode_sdf_gradient_batch(dec, c['codes'], c['pts'], counts=SIZES, clamp_dist=None) / 3).cpu()
    c['ref'] = _refs(Ws, bs, codes, pts, SIZES, phi, u, c['run'])
    return c


def test_values(case):
    r, ref = case['run'], case['ref']['both']
    n = sum(SIZES)
    assert r['f'].shape == (n, 1) and r['g'].shape == (n, 3)
    d_f = (r['f'] - case['batch']).abs().max().item()
    top = np.abs(ref['g']).max()
    d_ref = np.abs(r['g'].double().numpy() - ref['g']).max() / top
    d_fused = (r['g'] - case['gbatch']).abs().max().item() / case['gbatch'].abs().max().item()
    print('C = %d: |f - decode_sdf_batch| <= %.3e; g: %.3e of its largest entry (%.3f) from the closed form, %.3e from decode_sdf_gradient_batch / 3'
          % (case['Cn'], d_f, d_ref, top, d_fused))
    assert d_f <= 2e-6 and np.abs(r['f'].double().numpy() - ref['f']).max() <= 2e-6
    assert top > 0 and d_ref <= 1e-4 and d_fused <= 1e-4


@pytest.mark.parametrize('up', UPSTREAMS)
def test_gradients(case, up):
    _assert_gradients(case['run'][up], case['ref'][up], SIZES, 'C = %d, upstream %s' % (case['Cn'], up))
    assert not case['run'][up][1][3].any()          # the empty segment's code row: exactly zero


def test_without_u_it_is_decode_sdf_train(case):
    """u absent: the gradient of decode_sdf_train(clamp_dist=None) in another sum order (the row scalar sits on the operands here, on
    the delta there): 1e-4 of each tensor's (row's) largest entry."""
    from distr import functions
    _, saved = functions.train_forward(case['weights'], case['codes'], case['pts'], SIZES, None)
    grads, g_lat = functions.train_backward(saved, case['phi'])
    got, got_lat = case['run']['phi']
    for i, (a, b) in enumerate(zip(got, grads)):
        b = b.cpu()
        assert (a - b).abs().max().item() <= 1e-4 * b.abs().max().item(), i
    for s, p0, p1 in _segments():
        b = g_lat[s].cpu()
        assert (got_lat[s] - b).abs().max().item() <= 1e-4 * b.abs().max().item(), s


def test_same_bytes_on_every_run_and_per_segment(case):
    import torch
    from distr import functions
    a, b = case['run'], case['again']
    assert torch.equal(a['f'], b['f']) and torch.equal(a['g'], b['g'])
    for up in UPSTREAMS:
        assert all(torch.equal(x, y) for x, y in zip(a[up][0], b[up][0])) and torch.equal(a[up][1], b[up][1]), up
    for s, p0, p1 in _segments():
        if p0 == p1:
            continue
        (f, g), saved = functions.train_grad_forward(case['weights'], case['codes'][s:s + 1], case['pts'][p0:p1], [p1 - p0])
        assert torch.equal(f.cpu(), a['f'][p0:p1]) and torch.equal(g.cpu(), a['g'][p0:p1]), s
        for up in UPSTREAMS:
            phi, u = _pick(up, case['phi'][p0:p1], case['u'][p0:p1])
            _, g_lat = functions.train_grad_backward(saved, phi, u)
            assert torch.equal(g_lat.cpu(), a[up][1][s:s + 1]), (s, up)


def test_autograd_node_equals_the_low_level_calls(case):
    """decode_sdf_gradient_train hands autograd the bytes of train_grad_forward / train_grad_backward, in ONE backward pass for both
    outputs; an output no loss uses counts as a zero upstream."""
    import torch
    from core.utils.decoder_utils import decode_sdf_gradient_train
    from distr import functions
    dec, r = case['dec'], case['run']
    calls = []
    real = functions.train_grad_backward
    for up in ('both', 'u', 'phi'):
        lat = case['codes'].clone().requires_grad_(True)
        for p in dec.parameters():
            p.grad = None
        f, g = decode_sdf_gradient_train(dec, lat, case['pts'], counts=torch.tensor(SIZES))
        assert f.shape == (sum(SIZES), 1) and g.shape == (sum(SIZES), 3) and f.requires_grad and g.requires_grad
        assert torch.equal(f.detach().cpu(), r['f']) and torch.equal(g.detach().cpu(), r['g'])
        loss = sum(term for term, use in (((f * case['phi']).sum(), up != 'u'), ((g * case['u']).sum(), up != 'phi')) if use)
        functions.train_grad_backward = lambda *a, **k: calls.append(up) or real(*a, **k)
        try:
            loss.backward()
        finally:
            functions.train_grad_backward = real
        assert torch.equal(lat.grad.cpu(), r[up][1]), up
        for l in range(9):
            lin = getattr(dec, 'lin%d' % l)
            assert torch.equal(lin.weight.grad.cpu(), r[up][0][l]) and torch.equal(lin.bias.grad.cpu(), r[up][0][9 + l]), (up, l)
    assert calls == ['both', 'u', 'phi']          # one pass each
    for p in dec.parameters():
        p.grad = None
    with torch.no_grad():
        f3, g3 = decode_sdf_gradient_train(dec, case['codes'][:4], case['pts'][:4 * 65].reshape(4, 65, 3))        # the (S, N, 3) form
        ff, gf = decode_sdf_gradient_train(dec, case['codes'][:4], case['pts'][:4 * 65], counts=[65] * 4)
    assert f3.shape == (4, 65, 1) and g3.shape == (4, 65, 3) and torch.equal(f3.reshape(-1, 1), ff) and torch.equal(g3.reshape(-1, 3), gf)


def test_shared_code(fixture_decoder):
    """latent_stride 0: one code for every segment. g_latent keeps a row per segment; the autograd node hands the code their sum."""
    import torch
    from distr import functions
    Ws, bs, latent = fixture_decoder
    weights = _weights_of(_module(Ws, bs))
    codes, pts, phi, u = _inputs(latent, 256, SIZES, 41, shared=True)
    tc, tp, tphi, tu = (torch.from_numpy(a).cuda() for a in (codes, pts, phi, u))
    r = _run(weights, tc, tp, SIZES, tphi, tu, cases=('both',))
    assert r['both'][1].shape == (len(SIZES), 256)
    _assert_gradients(r['both'], _refs(Ws, bs, codes, pts, SIZES, phi, u, r, cases=('both',))['both'], SIZES, 'shared code')
    lat = tc.clone().requires_grad_(True)
    f, g = functions.decode_sdf_gradient_train_call(weights, lat, tp, SIZES)
    ((f * tphi).sum() + (g * tu).sum()).backward()
    assert torch.equal(f.detach().cpu(), r['f']) and torch.equal(lat.grad.cpu(), r['both'][1].cuda().sum(0).reshape(1, -1).cpu())


def test_three_slabs(fixture_decoder):
    """One list of 2 L + 1 points, L the smallest slab length: the weight-gradient GEMMs run three K slabs, the last with one real row
    and 63 padded ones; then with upstreams at that last point only."""
    import torch
    from distr import functions
    L0 = functions.train_slab_plan(1)[0]
    n = 2 * L0 + 1
    assert L0 <= 1024 and functions.train_slab_plan(functions.train_segment_rows([n])[-1]) == (L0, 3)
    Ws, bs, latent = fixture_decoder
    weights = _weights_of(_module(Ws, bs))
    codes, pts, phi, u = _inputs(latent, 256, [n], 43)
    tc, tp = torch.from_numpy(codes).cuda(), torch.from_numpy(pts).cuda()
    r = _run(weights, tc, tp, [n], torch.from_numpy(phi).cuda(), torch.from_numpy(u).cuda(), cases=('both',))
    _assert_gradients(r['both'], _refs(Ws, bs, codes, pts, [n], phi, u, r, cases=('both',))['both'], [n], 'three slabs')
    phi1, u1 = np.zeros_like(phi), np.zeros_like(u)
    phi1[-1], u1[-1] = phi[-1], u[-1]
    r1 = _run(weights, tc, tp, [n], torch.from_numpy(phi1).cuda(), torch.from_numpy(u1).cuda(), cases=('both',))
    _assert_gradients(r1['both'], _refs(Ws, bs, codes, pts, [n], phi1, u1, r1, cases=('both',))['both'], [n], 'third slab only')


def test_chunks_of_64_segments(fixture_decoder):
    """65 segments of 3 points: two calls (64 + 1) behind one decode_sdf_gradient_train; the weight gradients are the chunks' added in
    chunk order, byte for byte, the code gradient has the chunks' rows."""
    import torch
    from core.utils.decoder_utils import decode_sdf_gradient_train
    Ws, bs, latent = fixture_decoder
    dec = _module(Ws, bs)
    weights = _weights_of(dec)
    S, N = 65, 3
    codes, pts, phi, u = _inputs(latent, 256, [N] * S, 7)
    tc, tp, tphi, tu = (torch.from_numpy(a).cuda() for a in (codes, pts, phi, u))
    lat = tc.clone().requires_grad_(True)
    f, g = decode_sdf_gradient_train(dec, lat, tp.reshape(S, N, 3))
    assert f.shape == (S, N, 1) and g.shape == (S, N, 3)
    ((f.reshape(-1, 1) * tphi).sum() + (g.reshape(-1, 3) * tu).sum()).backward()
    a = _run(weights, tc[:64], tp[:64 * N], [N] * 64, tphi[:64 * N], tu[:64 * N], cases=('both',))
    b = _run(weights, tc[64:], tp[64 * N:], [N], tphi[64 * N:], tu[64 * N:], cases=('both',))
    assert torch.equal(f.detach().reshape(-1, 1).cpu(), torch.cat([a['f'], b['f']])) and torch.equal(g.detach().reshape(-1, 3).cpu(), torch.cat([a['g'], b['g']]))
    assert torch.equal(lat.grad.cpu(), torch.cat([a['both'][1], b['both'][1]]))
    got = [getattr(dec, 'lin%d' % l).weight.grad.cpu() for l in range(9)] + [getattr(dec, 'lin%d' % l).bias.grad.cpu() for l in range(9)]
    for i in range(18):
        assert torch.equal(got[i], a['both'][0][i] + b['both'][0][i]), i
    r = dict(gates=[torch.cat([ga, gb]) for ga, gb in zip(a['gates'], b['gates'])])
    _assert_gradients((got, lat.grad.cpu()), _refs(Ws, bs, codes, pts, [N] * S, phi, u, r, cases=('both',))['both'], [N] * S, '65 segments')


def test_weight_norm_decoder(fixture_decoder):
    """A weight-norm decoder: g_W travels on to weight_g / weight_v through autograd; same bar, against float64 autograd double backward
    through the same fold W = v * (g / ||v||_row) and the GPU's gates."""
    import torch
    import train_restatement as tr
    from core.utils.decoder_utils import decode_sdf_gradient_train
    from distr import functions
    Ws, bs, latent = fixture_decoder
    dec = _module(Ws, bs, weight_norm=True)
    codes, pts, phi, u = _inputs(latent, 256, SIZES, 47)
    tc, tp, tphi, tu = (torch.from_numpy(a).cuda() for a in (codes, pts, phi, u))
    _, saved = functions.train_grad_forward(_weights_of(dec), tc, tp, SIZES)
    gates = _gates(saved)
    lat = tc.clone().requires_grad_(True)
    f, g = decode_sdf_gradient_train(dec, lat, tp, counts=SIZES)
    ((f * tphi).sum() + (g * tu).sum()).backward()
    params = dict(dec.named_parameters())
    assert len(params) == 26
    p64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in params.items()}
    W64 = [p64['lin%d.weight_v' % l] * (p64['lin%d.weight_g' % l] / p64['lin%d.weight_v' % l].norm(dim=1, keepdim=True)) for l in range(8)] + [p64['lin8.weight']]
    b64 = [p64['lin%d.bias' % l] for l in range(9)]
    c64, x64 = tr.to64([codes], True)[0], tr.to64([pts], True)[0]
    phi64, u64 = tr.to64([phi, u])
    yr, _ = tr.forward(W64, b64, c64, x64, SIZES, None, gates)
    gr, = torch.autograd.grad(yr.sum(), x64, create_graph=True)
    ((yr * phi64).sum() + (gr * u64).sum()).backward()
    worst = 0.0
    for k, p in params.items():
        top = p64[k].grad.abs().max().item()
        assert top > 0, k
        rel = (p.grad.cpu().double() - p64[k].grad).abs().max().item() / top
        worst = max(worst, rel)
        assert rel <= 1e-4, (k, rel)
    for s, a, b in _segments():
        if a == b:
            assert not lat.grad[s].any()
        else:
            assert (lat.grad[s].cpu().double() - c64.grad[s]).abs().max().item() <= 1e-4 * c64.grad[s].abs().max().item(), s
    print('weight norm: largest residual %.3e' % worst)


def test_dropout(fixture_decoder):
    """p = 0.2 on all eight layers, a fixed seed: the closed form with the GPU's gates AND the mask of the definition (tests/
    dropout_restatement.py, which tests/test_train_dropout_host.py pins to distr_train_dropout_keep; 512 entries per layer are also
    asked of the library here). The tangent and the deltas see the forward's mask and scale. In eval mode, or with p = 0, the seed
    changes no byte."""
    import torch
    import dropout_restatement as dr
    from core.utils.decoder_utils import decode_sdf_gradient_train
    from distr import binding, functions
    Ws, bs, latent = fixture_decoder
    dec = _module(Ws, bs, dropout=list(range(8)), dropout_prob=P_DROP)
    dec.train()
    codes, pts, phi, u = _inputs(latent, 256, SIZES, 53)
    tc, tp, tphi, tu = (torch.from_numpy(a).cuda() for a in (codes, pts, phi, u))
    mask, T, scale = functions.train_dropout_params(dec, SEED)
    assert (mask, T, scale) == (0xff, dr.threshold(P_DROP), dr.scale(P_DROP))
    r = _run(_weights_of(dec), tc, tp, SIZES, tphi, tu, dropout=(mask, T, scale, SEED, 0))
    keeps = [dr.keep_list(SEED, l, SIZES, 253 if l == 3 else 512, T) for l in range(8)]
    L = binding.lib()
    rs = np.random.RandomState(1)
    seg_of = np.repeat(np.arange(len(SIZES)), SIZES)
    first = np.cumsum([0] + SIZES)
    for l in range(8):
        for row, unit in zip(rs.randint(0, sum(SIZES), 512), rs.randint(0, keeps[l].shape[1], 512)):
            s = int(seg_of[row])
            assert bool(L.distr_train_dropout_keep(SEED, T, l, s, int(row - first[s]), int(unit))) == bool(keeps[l][row, unit]), (l, row, unit)
        assert not (r['gates'][l].numpy() & ~keeps[l]).any(), l          # a dropped unit is stored as zero
    ref = _refs(Ws, bs, codes, pts, SIZES, phi, u, r, keeps=keeps, scale=scale)
    top = np.abs(ref['both']['g']).max()
    assert np.abs(r['f'].double().numpy() - ref['both']['f']).max() <= 2e-6
    assert np.abs(r['g'].double().numpy() - ref['both']['g']).max() <= 1e-4 * top
    for up in UPSTREAMS:
        _assert_gradients(r[up], ref[up], SIZES, 'dropout, upstream %s' % up)
    # the public call: the same bytes with the seed; another seed, another mask
    lat = tc.clone().requires_grad_(True)
    f, g = decode_sdf_gradient_train(dec, lat, tp, counts=SIZES, dropout_seed=SEED)
    ((f * tphi).sum() + (g * tu).sum()).backward()
    assert torch.equal(f.detach().cpu(), r['f']) and torch.equal(g.detach().cpu(), r['g']) and torch.equal(lat.grad.cpu(), r['both'][1])
    assert torch.equal(dec.lin2.weight.grad.cpu(), r['both'][0][2])
    with torch.no_grad():
        assert not torch.equal(decode_sdf_gradient_train(dec, tc, tp, counts=SIZES, dropout_seed=SEED + 1)[1].cpu(), r['g'])
    # eval mode, or p = 0: every byte of the call without a seed
    dec.eval()
    dec0 = _module(Ws, bs, dropout=list(range(8)), dropout_prob=0.0)
    dec0.train()
    outs = []
    for d, seed in ((dec, None), (dec, SEED), (dec0, SEED)):
        lat = tc.clone().requires_grad_(True)
        for p in d.parameters():
            p.grad = None
        f, g = decode_sdf_gradient_train(d, lat, tp, counts=SIZES, dropout_seed=seed)
        ((f * tphi).sum() + (g * tu).sum()).backward()
        outs.append([f.detach(), g.detach(), lat.grad] + [p.grad for p in d.parameters()])
    for other in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(outs[0], other))


EIKONAL_LR = 3e-4


def _eikonal_loss(f, g, target):
    return ((g.norm(dim=-1) - 1) ** 2).mean() + (f - target).abs().mean()


def _eikonal_losses64(module64, codes, pts, counts, target, lr, steps):
    """Plain SGD on a float64 torch Decoder and the codes, mean((|grad_x f| - 1)^2) + mean|f - target| through torch's double backward:
    steps + 1 losses, the one before every step and the one after the last."""
    import torch
    codes = codes.clone().double().requires_grad_(True)
    params = list(module64.parameters()) + [codes]
    cnt = torch.as_tensor([int(c) for c in counts])
    losses = []
    for i in range(steps + 1):
        for p in params:
            p.grad = None
        x = pts.double().clone().requires_grad_(True)
        y = module64(torch.cat([torch.repeat_interleave(codes, cnt, dim=0), x], 1))
        g, = torch.autograd.grad(y.sum(), x, create_graph=True)
        loss = _eikonal_loss(y, g, target.double())
        losses.append(loss.item())
        if i == steps:
            break
        loss.backward()
        with torch.no_grad():
            for p in params:
                p -= lr * p.grad
    return losses


def test_eikonal_fit(fixture_decoder):
    """Three plain SGD steps on the weights and the codes through decode_sdf_gradient_train, loss mean((|g| - 1)^2) + mean|f - target|
    with targets f + 0.05, and the same loop on the float64 torch Decoder (double backward). |g| lies in 0.42 .. 1.36 at the start.
    Learning rate 3e-4, chosen on the CPU in float64: the loss falls 0.0793 -> 0.0717 -> 0.0643 -> 0.0571 (1e-4 falls by 9 %, 1e-3
    overshoots at the third step). The loss goes down, and matches at every step to 1e-4 relative (the tolerance of
    test_gpu_train.py::test_sgd_loop)."""
    import copy
    import torch
    from core.utils.decoder_utils import decode_sdf_batch, decode_sdf_gradient_train
    Ws, bs, latent = fixture_decoder
    dec = _module(Ws, bs)
    codes, pts, _, _ = _inputs(latent, 256, SIZES, 359)
    codes, pts = torch.from_numpy(codes).cuda(), torch.from_numpy(pts).cuda()
    target = decode_sdf_batch(dec, codes, pts, counts=SIZES, clamp_dist=None, no_grad=True) + 0.05
    ref = _eikonal_losses64(copy.deepcopy(dec).cpu().double(), codes.cpu(), pts.cpu(), SIZES, target.cpu(), EIKONAL_LR, 3)
    assert all(b < a for a, b in zip(ref, ref[1:])), ref
    lat = codes.clone().requires_grad_(True)
    params = list(dec.parameters()) + [lat]
    losses = []
    for i in range(4):
        for p in params:
            p.grad = None
        f, g = decode_sdf_gradient_train(dec, lat, pts, counts=SIZES)
        loss = _eikonal_loss(f, g, target)
        losses.append(loss.item())
        if i == 3:
            break
        loss.backward()
        with torch.no_grad():
            for p in params:
                p -= EIKONAL_LR * p.grad
    print('float64: %s\nGPU:     %s' % (' '.join('%.8f' % x for x in ref), ' '.join('%.8f' % x for x in losses)))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    for a, b in zip(losses, ref):
        assert abs(a - b) <= 1e-4 * b, (losses, ref)


def test_refusals(fixture_decoder, monkeypatch):
    import torch
    from core.utils.decoder_utils import decode_sdf_gradient_train
    from distr import binding, functions
    Ws, bs, latent = fixture_decoder
    dec = _module(Ws, bs)
    weights = _weights_of(dec)
    lat = torch.zeros(2, 256, device='cuda')
    pts = torch.zeros(8, 3, device='cuda')
    with pytest.raises(ValueError, match='requires_grad'):
        decode_sdf_gradient_train(dec, lat, pts.clone().requires_grad_(True), counts=[5, 3])
    cnt = (C.c_int64 * 2)(5, 3)
    tn = functions._train_net_struct(weights, (256, 253, 1))
    need = binding.lib().distr_train_grad_workspace_bytes(C.byref(tn), 2, cnt)
    assert need > binding.lib().distr_train_net_workspace_bytes(C.byref(tn), 2, cnt) > 0
    with pytest.raises(binding.DistrError, match=r'error -4: .*workspace too small'):           # DISTR_ERR_WORKSPACE
        functions.train_grad_forward(weights, lat, pts, [5, 3], ws_bytes=need - 1)
    (f, g), saved = functions.train_grad_forward(weights, lat, pts, [5, 3], ws_bytes=need)       # and the size asked for is enough
    assert f.shape == (8, 1) and g.shape == (8, 3)
    with pytest.raises(ValueError, match='train_grad_backward'):                                # the two backwards do not mix
        functions.train_backward(saved, torch.zeros(8, 1, device='cuda'))
    _, plain = functions.train_forward(weights, lat, pts, [5, 3], None)
    with pytest.raises(ValueError, match='train_backward'):
        functions.train_grad_backward(plain, None, torch.zeros(8, 3, device='cuda'))
    with pytest.raises(ValueError, match='g_grad has 21 entries'):
        functions.train_grad_backward(saved, None, torch.zeros(7, 3, device='cuda'))
    monkeypatch.setenv('DISTR_TRAIN_MAX_BYTES', str(need - 1))
    with pytest.raises(binding.DistrError, match=r'decode_sdf_gradient_train: 8 points need a workspace of %d bytes \(40 KB per point.*DISTR_TRAIN_MAX_BYTES' % need):
        decode_sdf_gradient_train(dec, lat, pts, counts=[5, 3])
    monkeypatch.delenv('DISTR_TRAIN_MAX_BYTES')
    # the C ABI's own refusals: out_dim = 3 (the colour net has no such gradient), a null weight pointer, a bad list, a bad stride
    ctx = functions._train_context(0)
    L, p = ctx.L, binding.ptr
    f, g = torch.empty(8, 1, device='cuda'), torch.empty(8, 3, device='cuda')
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')

    def call(tn, nseg=2, counts=cnt, stride=256):
        rc = L.distr_train_grad_forward(ctx.h, C.byref(tn), nseg, counts, p(lat), stride, p(pts), p(f), p(g), p(ws), need, ctx.stream(), None)
        return rc, L.distr_last_error(ctx.h).decode()
    rc, err = call(functions._train_net_struct(weights, (256, 253, 3)))
    assert rc == -1 and 'out_dim 3' in err, (rc, err)
    tg = binding.TrainGrads()
    rc = L.distr_train_grad_backward(ctx.h, C.byref(functions._train_net_struct(weights, (256, 253, 3))), 2, cnt, p(lat), 256, p(f), p(g), p(ws), C.byref(tg), None,
                                     ctx.stream(), None)
    assert rc == -1 and 'out_dim 3' in L.distr_last_error(ctx.h).decode()
    bad = functions._train_net_struct(weights, (256, 253, 1))
    bad.b[6] = None
    rc, err = call(bad)
    assert rc == -1 and 'lin6' in err, (rc, err)
    for kw, word in ((dict(nseg=0), 'nseg'), (dict(counts=(C.c_int64 * 2)(9, -1)), 'negative'), (dict(stride=100), 'latent_stride')):
        rc, err = call(tn, **kw)
        assert rc == -1 and word in err, (kw, rc, err)
    rc = L.distr_train_grad_backward(ctx.h, C.byref(tn), 2, cnt, p(lat), 256, p(f), p(g), p(ws), C.byref(tg), None, ctx.stream(), None)
    assert rc == -1 and 'distr_train_grads' in L.distr_last_error(ctx.h).decode()               # null gradient pointers
    assert call(tn)[0] == 0
    torch.cuda.synchronize()
