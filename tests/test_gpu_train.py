"""Training the decoder: decode_sdf_train, the layer-wise path with weight gradients (distr_train_*).

References: decode_sdf_batch (the fused tiles) for the values, and for the gradients the float64 restatement of tests/train_restatement.py
run WITH THE GATES THE GPU RUN SAVED, so that both differentiate the same piecewise-linear function and no ReLU-side carve-out is needed
(tests/test_train_host.py pins the restatement to the float64 torch Decoder). Bars: 2e-6 on sdf (G11's), 1e-4 of a tensor's largest entry
on gradients (the project's bar for a different f32 summation order), per row for the code gradient so that a wrong small row cannot
hide, and also per block of a tensor (train_restatement.gradient_blocks: the latent, xyz and activation columns of g_W0 / g_W4 come from
different kernels). The reduction order itself is pinned byte for byte by tests/test_gpu_train_edges.py. Shapes are the smallest at which each mechanism can go wrong: segments [1, 64, 65, 0, 130, 63] (block -> segment map, padded rows,
an empty segment), a shared code, one list of 2 L + 1 rows (three K slabs, the last with a single real row), 65 segments (two chunks).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [1, 64, 65, 0, 130, 63]
CODE_LENGTHS = (256, 64, 300)
CLAMPS = (0.1, None)


def _module(Ws, bs, weight_norm=False, **kw):
    import torch
    from core.graph.deep_sdf_decoder import Decoder
    from distr import decoder_pack
    dec = Decoder(decoder_pack.latent_size_of(Ws), [512] * 8, norm_layers=tuple(range(8)) if weight_norm else (), latent_in=[4], weight_norm=weight_norm, **kw)
    dec.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in decoder_pack.fixture_state_dict(Ws, bs, weight_norm=weight_norm).items()})
    return dec.cuda().eval()


def _segments(sizes=SIZES):
    at = 0
    for s, n in enumerate(sizes):
        yield s, at, at + n
        at += n


def _real_rows(saved):
    """Workspace rows of the list's points, in point order (the padded rows are left out by construction)."""
    import torch
    return torch.cat([torch.arange(*saved.rows(s)) for s in range(len(saved.counts))]).cuda()


def _gates(saved):
    idx = _real_rows(saved)
    return [(saved.activations(l + 1)[idx] > 0).cpu() for l in range(8)]


def _run(weights, codes, pts, sizes, w, clamp):
    """One forward + backward on the low-level calls: dict(sdf, gates, grads [g_W0..g_W8, g_b0..g_b8], g_lat (S, C)), on the CPU."""
    from distr import functions
    sdf, saved = functions.train_forward(weights, codes, pts, sizes, clamp)
    grads, g_lat = functions.train_backward(saved, w)
    return dict(sdf=sdf.cpu(), gates=_gates(saved), grads=[g.cpu() for g in grads], g_lat=g_lat.cpu())


def _assert_gradients(got_W, got_b, got_rows, ref_W, ref_b, ref_rows, sizes, tag):
    worst = 0.0
    for l in range(9):
        for name, a, b in (('g_W%d' % l, got_W[l], ref_W[l]), ('g_b%d' % l, got_b[l], ref_b[l])):
            top = b.abs().max().item()
            assert top > 0, (tag, name)
            rel = (a.double() - b).abs().max().item() / top
            worst = max(worst, rel)
            assert rel <= 1e-4, (tag, name, rel)
    # the same bar per block: the latent, xyz and activation columns of g_W0 / g_W4 come from different kernels, and a small block
    # must not hide behind a large one (tests/train_restatement.py::gradient_blocks)
    import train_restatement as tr
    blocks = tr.blockwise_residuals([t.cpu() for t in list(got_W) + list(got_b)], list(ref_W) + list(ref_b), got_W[0].shape[1] - 3)
    for name, rel, top in blocks:
        assert rel <= 1e-4, (tag, 'block', name, rel, top)
    worst_block = max(blocks, key=lambda t: t[1])
    print('%s: worst block %s, %.3e of its largest entry' % (tag, worst_block[0], worst_block[1]))
    for s, a, b in _segments(sizes):
        if a == b:
            assert not got_rows[s].any(), (tag, 'the empty segment has a code gradient')
            continue
        top = ref_rows[s].abs().max().item()
        if top == 0:        # every point of the segment outside the clamp
            assert not got_rows[s].any(), (tag, s)
            continue
        rel = (got_rows[s].double() - ref_rows[s]).abs().max().item() / top
        worst = max(worst, rel)
        assert rel <= 1e-4, (tag, 'g_latent row', s, rel)
    print('%s: largest gradient residual %.3e of a tensor\'s (row\'s) largest entry' % (tag, worst))


@pytest.fixture(scope='module', params=CODE_LENGTHS)
def case(request, fixture_decoder):
    """Per code length, made once and never modified: the decoder, codes (6, C), points, an upstream gradient, and for both clamps the
    GPU run (twice), decode_sdf_batch on the same inputs and the float64 restatement with its own gates and with the GPU's."""
    import torch
    import train_restatement as tr
    from core.utils.decoder_utils import decode_sdf_batch
    from distr import decoder_pack, fixture
    Cn = request.param
    Ws, bs, latent = fixture_decoder if Cn == 256 else fixture.make_decoder_weights(latent_size=Cn)
    rs = np.random.RandomState(100 + Cn)
    codes = (latent + 0.3 * np.abs(latent).max() * rs.standard_normal((len(SIZES), Cn))).astype(np.float32)
    pts = ((rs.rand(sum(SIZES), 3) - 0.5) * 1.6).astype(np.float32)
    w = rs.standard_normal((sum(SIZES), 1)).astype(np.float32)
    dec = _module(Ws, bs)
    c = dict(Cn=Cn, Ws=Ws, bs=bs, dec=dec, codes=torch.from_numpy(codes).cuda(), pts=torch.from_numpy(pts).cuda(), w=torch.from_numpy(w).cuda())
    Wt, bt = decoder_pack.effective_weights_torch(dec)
    c['weights'] = [t.detach() for t in Wt + bt]
    for clamp in CLAMPS:
        r = _run(c['weights'], c['codes'], c['pts'], SIZES, c['w'], clamp)
        r['again'] = _run(c['weights'], c['codes'], c['pts'], SIZES, c['w'], clamp)
        r['batch'] = decode_sdf_batch(dec, c['codes'], c['pts'], counts=SIZES, clamp_dist=clamp, no_grad=True).cpu()
        r['own'] = tr.gradients(Ws, bs, codes, pts, SIZES, w, clamp)
        r['ref'] = tr.gradients(Ws, bs, codes, pts, SIZES, w, clamp, gates=r['gates'])
        c[clamp] = r
    return c


@pytest.mark.parametrize('clamp', CLAMPS)
def test_values(case, clamp):
    r = case[clamp]
    assert r['sdf'].shape == (sum(SIZES), 1)
    d_batch = (r['sdf'] - r['batch']).abs().max().item()
    d_64 = (r['sdf'].double() - r['own'][0]).abs().max().item()
    print('C = %d, clamp %s: |sdf - decode_sdf_batch| <= %.3e, |sdf - float64| <= %.3e; %d of %d values are not byte-identical to decode_sdf_batch'
          % (case['Cn'], clamp, d_batch, d_64, int((r['sdf'] != r['batch']).sum()), sum(SIZES)))
    assert d_batch <= 2e-6 and d_64 <= 2e-6
    assert r['sdf'].abs().max() > 0 and (clamp is None or r['sdf'].abs().max() <= clamp)


def test_gates(case):
    """The saved activations give the ReLU pattern; it may differ from the float64 run's own pattern only at units whose float64
    pre-activation is below 1e-5 in magnitude. Padded rows are not looked at: _real_rows leaves them out."""
    r = case[None]
    pre = r['own'][1]
    ndiff = 0
    for l in range(8):
        assert r['gates'][l].shape == pre[l].shape, l
        diff = r['gates'][l] != (pre[l] > 0)
        ndiff += int(diff.sum())
        assert not diff.any() or pre[l][diff].abs().max().item() < 1e-5, l
        assert r['gates'][l].any() and not r['gates'][l].all(), l
    print('C = %d: %d of %d units sit on the other side of the ReLU than in float64' % (case['Cn'], ndiff, sum(g.numel() for g in r['gates'])))


@pytest.mark.parametrize('clamp', CLAMPS)
def test_gradients(case, clamp):
    r = case[clamp]
    _, _, ref_W, ref_b, ref_rows = r['ref']
    _assert_gradients(r['grads'][:9], r['grads'][9:], r['g_lat'], ref_W, ref_b, ref_rows, SIZES, 'C = %d, clamp %s' % (case['Cn'], clamp))
    assert not r['g_lat'][3].any()


@pytest.mark.parametrize('clamp', CLAMPS)
def test_same_bytes_on_every_run_and_per_segment(case, clamp):
    import torch
    from distr import functions
    r = case[clamp]
    a, b = r, r['again']
    assert torch.equal(a['sdf'], b['sdf']) and torch.equal(a['g_lat'], b['g_lat'])
    assert all(torch.equal(x, y) for x, y in zip(a['grads'], b['grads']))
    assert all(torch.equal(x, y) for x, y in zip(a['gates'], b['gates']))
    for s, p0, p1 in _segments():
        if p0 == p1:
            continue
        sdf, saved = functions.train_forward(case['weights'], case['codes'][s:s + 1], case['pts'][p0:p1], [p1 - p0], clamp)
        _, g_lat = functions.train_backward(saved, case['w'][p0:p1])
        assert torch.equal(sdf.cpu(), r['sdf'][p0:p1]), s
        assert torch.equal(g_lat.cpu(), r['g_lat'][s:s + 1]), s


def test_autograd_node_equals_the_low_level_calls(case):
    """decode_sdf_train hands autograd the bytes of train_forward / train_backward: to the parameters and to the codes."""
    import torch
    from core.utils.decoder_utils import decode_sdf_train
    dec, r = case['dec'], case[0.1]
    lat = case['codes'].clone().requires_grad_(True)
    for p in dec.parameters():
        p.grad = None
    y = decode_sdf_train(dec, lat, case['pts'], counts=torch.tensor(SIZES), clamp_dist=0.1)
    assert y.shape == (sum(SIZES), 1) and y.requires_grad
    (y * case['w']).sum().backward()
    assert torch.equal(y.detach().cpu(), r['sdf']) and torch.equal(lat.grad.cpu(), r['g_lat'])
    for l in range(9):
        lin = getattr(dec, 'lin%d' % l)
        assert torch.equal(lin.weight.grad.cpu(), r['grads'][l]) and torch.equal(lin.bias.grad.cpu(), r['grads'][9 + l]), l
    for p in dec.parameters():
        p.grad = None
    y3 = decode_sdf_train(dec, case['codes'][:4], case['pts'][:4 * 65].reshape(4, 65, 3), clamp_dist=None)        # the (S, N, 3) form
    y3f = decode_sdf_train(dec, case['codes'][:4], case['pts'][:4 * 65], counts=[65] * 4, clamp_dist=None)
    assert y3.shape == (4, 65, 1) and torch.equal(y3.reshape(-1, 1), y3f)


def test_shared_code(fixture_decoder):
    """latent_stride 0: one code for every segment. g_latent keeps a row per segment; the autograd node hands the code their sum."""
    import torch
    import train_restatement as tr
    from distr import decoder_pack, functions
    Ws, bs, latent = fixture_decoder
    dec = _module(Ws, bs)
    Wt, bt = decoder_pack.effective_weights_torch(dec)
    weights = [t.detach() for t in Wt + bt]
    rs = np.random.RandomState(41)
    code = (latent + 0.3 * np.abs(latent).max() * rs.standard_normal((1, 256))).astype(np.float32)
    pts = ((rs.rand(sum(SIZES), 3) - 0.5) * 1.6).astype(np.float32)
    w = rs.standard_normal((sum(SIZES), 1)).astype(np.float32)
    tc, tp, tw = (torch.from_numpy(a).cuda() for a in (code, pts, w))
    r = _run(weights, tc, tp, SIZES, tw, None)
    assert r['g_lat'].shape == (len(SIZES), 256)
    _, _, ref_W, ref_b, ref_rows = tr.gradients(Ws, bs, np.repeat(code, len(SIZES), 0), pts, SIZES, w, None, gates=r['gates'])
    _assert_gradients(r['grads'][:9], r['grads'][9:], r['g_lat'], ref_W, ref_b, ref_rows, SIZES, 'shared code')
    lat = tc.clone().requires_grad_(True)
    y = functions.decode_sdf_train_call(weights, lat, tp, SIZES, None)
    (y * tw).sum().backward()
    assert torch.equal(y.detach().cpu(), r['sdf']) and torch.equal(lat.grad.cpu(), r['g_lat'].cuda().sum(0).reshape(1, -1).cpu())


def test_three_slabs(fixture_decoder):
    """One list of 2 L + 1 points, L the smallest slab length: the weight-gradient GEMMs run three K slabs, the last with one real row
    and 63 padded ones."""
    import torch
    import train_restatement as tr
    from distr import decoder_pack, functions
    L0 = functions.train_slab_plan(1)[0]
    n = 2 * L0 + 1
    assert L0 <= 1024 and functions.train_slab_plan(functions.train_segment_rows([n])[-1]) == (L0, 3)
    Ws, bs, latent = fixture_decoder
    dec = _module(Ws, bs)
    Wt, bt = decoder_pack.effective_weights_torch(dec)
    weights = [t.detach() for t in Wt + bt]
    rs = np.random.RandomState(43)
    code = (latent + 0.3 * np.abs(latent).max() * rs.standard_normal((1, 256))).astype(np.float32)
    pts = ((rs.rand(n, 3) - 0.5) * 1.6).astype(np.float32)
    w = rs.standard_normal((n, 1)).astype(np.float32)
    tc, tp, tw = (torch.from_numpy(a).cuda() for a in (code, pts, w))
    r = _run(weights, tc, tp, [n], tw, None)
    _, _, ref_W, ref_b, ref_rows = tr.gradients(Ws, bs, code, pts, [n], w, None, gates=r['gates'])
    _assert_gradients(r['grads'][:9], r['grads'][9:], r['g_lat'], ref_W, ref_b, ref_rows, [n], 'three slabs')
    # the last point alone sits in the third slab: with an upstream gradient at that point only, the whole gradient comes from it
    w1 = np.zeros_like(w)
    w1[-1] = 1.0
    r1 = _run(weights, tc, tp, [n], torch.from_numpy(w1).cuda(), None)
    _, _, ref_W, ref_b, ref_rows = tr.gradients(Ws, bs, code, pts, [n], w1, None, gates=r1['gates'])
    _assert_gradients(r1['grads'][:9], r1['grads'][9:], r1['g_lat'], ref_W, ref_b, ref_rows, [n], 'third slab only')


def test_chunks_of_64_segments(fixture_decoder):
    """65 segments of 3 points: two calls (64 + 1) behind one decode_sdf_train; the weight gradients are the chunks' added in chunk
    order, the code gradient has the chunks' rows."""
    import torch
    import train_restatement as tr
    from core.utils.decoder_utils import decode_sdf_batch, decode_sdf_train
    from distr import decoder_pack
    Ws, bs, latent = fixture_decoder
    dec = _module(Ws, bs)
    Wt, bt = decoder_pack.effective_weights_torch(dec)
    weights = [t.detach() for t in Wt + bt]
    S, N = 65, 3
    rs = np.random.RandomState(7)
    codes = (latent + 0.3 * np.abs(latent).max() * rs.standard_normal((S, 256))).astype(np.float32)
    pts = ((rs.rand(S, N, 3) - 0.5) * 1.6).astype(np.float32)
    w = rs.standard_normal((S, N, 1)).astype(np.float32)
    tc, tp, tw = (torch.from_numpy(a).cuda() for a in (codes, pts, w))
    lat = tc.clone().requires_grad_(True)
    y = decode_sdf_train(dec, lat, tp, clamp_dist=None)
    assert y.shape == (S, N, 1)
    (y * tw).sum().backward()
    assert (y.detach() - decode_sdf_batch(dec, tc, tp, clamp_dist=None, no_grad=True)).abs().max().item() <= 2e-6
    a = _run(weights, tc[:64], tp[:64].reshape(-1, 3), [N] * 64, tw[:64].reshape(-1), None)
    b = _run(weights, tc[64:], tp[64:].reshape(-1, 3), [N], tw[64:].reshape(-1), None)
    assert torch.equal(y.detach().reshape(-1, 1).cpu(), torch.cat([a['sdf'], b['sdf']]))
    assert torch.equal(lat.grad.cpu(), torch.cat([a['g_lat'], b['g_lat']]))
    got = [getattr(dec, 'lin%d' % l).weight.grad.cpu() for l in range(9)] + [getattr(dec, 'lin%d' % l).bias.grad.cpu() for l in range(9)]
    for i in range(18):
        assert torch.equal(got[i], a['grads'][i] + b['grads'][i]), i
    gates = [torch.cat([ga, gb]) for ga, gb in zip(a['gates'], b['gates'])]
    _, _, ref_W, ref_b, ref_rows = tr.gradients(Ws, bs, codes, pts.reshape(-1, 3), [N] * S, w.reshape(-1), None, gates=gates)
    _assert_gradients(got[:9], got[9:], lat.grad.cpu(), ref_W, ref_b, ref_rows, [N] * S, '65 segments')


@pytest.mark.parametrize('clamp', CLAMPS)
def test_weight_norm_decoder(fixture_decoder, clamp):
    """A weight-norm decoder: g_W travels on to weight_g / weight_v through autograd; same bar, against float64 autograd through the
    same fold W = v * (g / ||v||_row) and the GPU's gates."""
    import torch
    import train_restatement as tr
    from core.utils.decoder_utils import decode_sdf_train
    from distr import decoder_pack, functions
    Ws, bs, latent = fixture_decoder
    dec = _module(Ws, bs, weight_norm=True)
    rs = np.random.RandomState(47)
    codes = (latent + 0.3 * np.abs(latent).max() * rs.standard_normal((len(SIZES), 256))).astype(np.float32)
    pts = ((rs.rand(sum(SIZES), 3) - 0.5) * 1.6).astype(np.float32)
    w = rs.standard_normal((sum(SIZES), 1)).astype(np.float32)
    tc, tp, tw = (torch.from_numpy(a).cuda() for a in (codes, pts, w))
    Wt, bt = decoder_pack.effective_weights_torch(dec)
    _, saved = functions.train_forward([t.detach() for t in Wt + bt], tc, tp, SIZES, clamp)
    gates = _gates(saved)
    lat = tc.clone().requires_grad_(True)
    (decode_sdf_train(dec, lat, tp, counts=SIZES, clamp_dist=clamp) * tw).sum().backward()
    params = dict(dec.named_parameters())
    assert len(params) == 26
    p64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in params.items()}
    W64 = [p64['lin%d.weight_v' % l] * (p64['lin%d.weight_g' % l] / p64['lin%d.weight_v' % l].norm(dim=1, keepdim=True)) for l in range(8)] + [p64['lin8.weight']]
    b64 = [p64['lin%d.bias' % l] for l in range(9)]
    c64, x64, w64 = tr.to64([codes], True)[0], tr.to64([pts])[0], tr.to64([w])[0]
    yr, _ = tr.forward(W64, b64, c64, x64, SIZES, clamp, gates)
    (yr * w64).sum().backward()
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
        elif c64.grad[s].abs().max() > 0:
            assert (lat.grad[s].cpu().double() - c64.grad[s]).abs().max().item() <= 1e-4 * c64.grad[s].abs().max().item(), s
    print('weight norm, clamp %s: largest residual %.3e' % (clamp, worst))


LOOP_LR = 2.5e-4


def test_sgd_loop(fixture_decoder):
    """Three plain SGD steps on the weights and the codes through decode_sdf_train, clamped L1 loss (clamp 0.1) against fixed targets, and
    the same loop on the float64 torch Decoder. Points: per segment the first of 12 000 uniform candidates with |sdf| < 0.03; targets:
    their sdf + 0.06, so every residual starts at 0.06 with one sign and no point is outside the clamp. Learning rate 2.5e-4, chosen on
    the CPU in float64: the loss falls 0.0600 -> 0.0497 -> 0.0392 -> 0.0285, by 53 % (5e-4 still falls monotonically, by 92 %; from
    1e-3 on the L1 loss overshoots). The loss matches at every step to 1e-4 relative; afterwards decode_sdf_batch, whose engine re-packs
    the updated weights through the parameters' _version, agrees with decode_sdf_train to 2e-6."""
    import copy
    import torch
    import train_restatement as tr
    from core.utils.decoder_utils import decode_sdf_batch, decode_sdf_train
    Ws, bs, latent = fixture_decoder
    dec = _module(Ws, bs)
    rs = np.random.RandomState(356)
    codes = torch.from_numpy((latent + 0.3 * np.abs(latent).max() * rs.standard_normal((len(SIZES), 256))).astype(np.float32)).cuda()
    cand = torch.from_numpy(((rs.rand(len(SIZES), 12000, 3) - 0.5) * 1.6).astype(np.float32)).cuda()
    f = decode_sdf_batch(dec, codes, cand, clamp_dist=None, no_grad=True)
    pts = torch.cat([cand[s][(f[s, :, 0].abs() < 0.03).nonzero()[:n, 0]] for s, n in enumerate(SIZES)])
    assert pts.shape == (sum(SIZES), 3)
    target = decode_sdf_batch(dec, codes, pts, counts=SIZES, clamp_dist=None, no_grad=True) + 0.06
    ref = tr.sgd_losses(copy.deepcopy(dec).cpu().double(), codes.cpu(), pts.cpu(), SIZES, target.cpu(), LOOP_LR, 3)
    assert ref[-1] <= 0.9 * ref[0], ref
    lat = codes.clone().requires_grad_(True)
    params = list(dec.parameters()) + [lat]
    losses = []
    for i in range(4):
        for p in params:
            p.grad = None
        loss = tr.clamped_l1(decode_sdf_train(dec, lat, pts, counts=SIZES, clamp_dist=0.1), target, 0.1)
        losses.append(loss.item())
        if i == 3:
            break
        loss.backward()
        with torch.no_grad():
            for p in params:
                p -= LOOP_LR * p.grad
    print('float64: %s\nGPU:     %s' % (' '.join('%.8f' % x for x in ref), ' '.join('%.8f' % x for x in losses)))
    for a, b in zip(losses, ref):
        assert abs(a - b) <= 1e-4 * b, (losses, ref)
    with torch.no_grad():
        y_train = decode_sdf_train(dec, lat, pts, counts=SIZES, clamp_dist=0.1)
        y_batch = decode_sdf_batch(dec, lat, pts, counts=SIZES, clamp_dist=0.1, no_grad=True)
    assert (y_train - y_batch).abs().max().item() <= 2e-6
    assert (y_batch - (target - 0.06)).abs().max().item() > 1e-3          # the engine did follow the updated weights


def test_refusals(fixture_decoder, monkeypatch):
    import torch
    import train_abi
    from core.utils.decoder_utils import decode_sdf_train
    from distr import binding, decoder_pack, functions
    Ws, bs, latent = fixture_decoder
    dec = _module(Ws, bs)
    lat = torch.zeros(2, 256, device='cuda')
    pts = torch.zeros(8, 3, device='cuda')
    drop = _module(Ws, bs, dropout=[0, 1], dropout_prob=0.2)
    drop.train()
    with pytest.raises(decoder_pack.UnsupportedDecoder, match='training mode with dropout'):
        decode_sdf_train(drop, lat, pts, counts=[5, 3])
    ldrop = _module(Ws, bs, latent_dropout=True)
    ldrop.train()
    with pytest.raises(decoder_pack.UnsupportedDecoder, match='latent_dropout'):
        decode_sdf_train(ldrop, lat, pts, counts=[5, 3])
    with pytest.raises(ValueError, match='requires_grad'):
        decode_sdf_train(dec, lat, pts.clone().requires_grad_(True), counts=[5, 3])
    Wt, bt = decoder_pack.effective_weights_torch(dec)
    weights = [t.detach() for t in Wt + bt]
    need = binding.lib().distr_train_workspace_bytes(256, 2, (C.c_int64 * 2)(5, 3))
    with pytest.raises(binding.DistrError, match=r'error -4: .*workspace too small'):           # DISTR_ERR_WORKSPACE
        functions.train_forward(weights, lat, pts, [5, 3], 0.1, ws_bytes=need - 1)
    sdf, _ = functions.train_forward(weights, lat, pts, [5, 3], 0.1, ws_bytes=need)             # and the size asked for is enough
    assert sdf.shape == (8, 1)
    monkeypatch.setenv('DISTR_TRAIN_MAX_BYTES', str(need - 1))
    with pytest.raises(binding.DistrError, match=r'8 points need a workspace of %d bytes.*DISTR_TRAIN_MAX_BYTES' % need):
        decode_sdf_train(dec, lat, pts, counts=[5, 3])
    monkeypatch.delenv('DISTR_TRAIN_MAX_BYTES')
    # the C ABI's own refusals: a code length outside 1..508, a null weight pointer, a bad list
    ctx = functions._train_context(0)
    L, p = ctx.L, binding.ptr
    out = torch.empty(8, 1, device='cuda')
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    cnt = (C.c_int64 * 2)(5, 3)

    def call(tw, nseg=2, counts=cnt, stride=256):
        rc = L.distr_train_forward(ctx.h, C.byref(tw), nseg, counts, p(lat), stride, p(pts), 0.1, p(out), p(ws), need, ctx.stream())
        return rc, L.distr_last_error(ctx.h).decode()
    for bad_c in (0, 509):
        rc, err = call(train_abi.train_weights(weights, bad_c))
        assert rc == -1 and 'latent_size' in err, (bad_c, rc, err)
    tw = train_abi.train_weights(weights, 256)
    tw.b[6] = None
    rc, err = call(tw)
    assert rc == -1 and 'lin6' in err, (rc, err)
    tw = train_abi.train_weights(weights, 256)
    for kw, word in ((dict(nseg=0), 'nseg'), (dict(counts=(C.c_int64 * 2)(9, -1)), 'negative'), (dict(stride=100), 'latent_stride')):
        rc, err = call(tw, **kw)
        assert rc == -1 and word in err, (kw, rc, err)
    assert call(tw)[0] == 0
    torch.cuda.synchronize()
