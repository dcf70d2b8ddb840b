"""Dropout in training mode on the layer-wise train path (distr_train_*_dropout).

The mask is a pure function (tests/dropout_restatement.py restates it in numpy; tests/test_train_dropout_host.py pins the library's
round function to it), so every check here knows which units must be zero. Values and gradients: the float64 restatement of
tests/train_restatement.py with the gates the GPU run saved, `[X > 0] * scale` (1 where the layer has no dropout) -- the function the
GPU differentiated. Bars are section 8f's: 2e-6 on sdf, 1e-4 of a tensor's (code-gradient row's) largest entry on gradients, a ReLU
pattern that may differ from float64's only where |pre-activation| < 1e-5. The decoders are the fixtures with the weights behind a
dropped layer multiplied by 1 - p (_rescaled says why). Shapes are test_gpu_train.py's: segments
[1, 64, 65, 0, 130, 63], one list of three K slabs, 65 segments (two chunks), and golden G32 (3 x 70).
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SIZES = [1, 64, 65, 0, 130, 63]
SEED = 0x5EED0001
CASES = [(Cn, p, tuple(layers)) for Cn in (256, 64, 300) for p in (0.2, 0.5) for layers in (range(8), (0, 3, 7))]


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


def _drop(layers, p, seed=SEED, base=0):
    import dropout_restatement as dr
    return (sum(1 << l for l in layers), dr.threshold(p), dr.scale(p), seed, base)


def _activations(saved):
    """X_1..X_8 of the list's points (the padded rows left out), on the CPU."""
    import torch
    idx = torch.cat([torch.arange(*saved.rows(s)) for s in range(len(saved.counts))]).cuda()
    return [saved.activations(l + 1)[idx].cpu() for l in range(8)]


def _gates(X, layers, scale):
    return [(x > 0).double() * (scale if l in layers else 1.0) for l, x in enumerate(X)]


def _run(weights, codes, pts, sizes, w, clamp, dropout):
    """One forward + backward on the low-level calls: dict(sdf, X, grads [g_W0..g_W8, g_b0..g_b8], g_lat (S, C)), on the CPU."""
    from distr import functions
    sdf, saved = functions.train_forward(weights, codes, pts, sizes, clamp, dropout=dropout)
    grads, g_lat = functions.train_backward(saved, w)
    return dict(sdf=sdf.cpu(), X=_activations(saved), grads=[g.cpu() for g in grads], g_lat=g_lat.cpu())


def _same_bytes(a, b):
    import torch
    return torch.equal(a['sdf'], b['sdf']) and torch.equal(a['g_lat'], b['g_lat']) and all(torch.equal(x, y) for x, y in zip(a['grads'], b['grads'])) \
        and all(torch.equal(x, y) for x, y in zip(a['X'], b['X']))


def _assert_gradients(got_W, got_b, got_rows, ref_W, ref_b, ref_rows, sizes, tag):
    worst = 0.0
    for l in range(9):
        for name, a, b in (('g_W%d' % l, got_W[l], ref_W[l]), ('g_b%d' % l, got_b[l], ref_b[l])):
            top = b.abs().max().item()
            assert top > 0, (tag, name)
            rel = (a.double() - b).abs().max().item() / top
            worst = max(worst, rel)
            assert rel <= 1e-4, (tag, name, rel)
    for s, a, b in _segments(sizes):
        if a == b:
            assert not got_rows[s].any(), (tag, 'the empty segment has a code gradient')
            continue
        top = ref_rows[s].abs().max().item()
        if top == 0:
            assert not got_rows[s].any(), (tag, s)
            continue
        rel = (got_rows[s].double() - ref_rows[s]).abs().max().item() / top
        worst = max(worst, rel)
        assert rel <= 1e-4, (tag, 'g_latent row', s, rel)
    print('%s: largest gradient residual %.3e of a tensor\'s (row\'s) largest entry' % (tag, worst))


CANDIDATES = 8


def _rescaled(Ws, p, layers):
    """The fixture's weights for a run with dropout: the columns of lin_(l+1) that read a dropped layer l are multiplied by 1 - p, which
    undoes the dropout scale in expectation -- the pre-activations then have the eval-mode fixture's size, as those of a decoder that
    was trained with dropout do. Why: the fixture was not; under p = 0.5 its activations double at each of eight layers and every
    prediction saturates (median 0.9995). The backward's 1 - tanh^2, taken from the f32 tanh, then carries a relative error of
    1.2e-7 / (1 - tanh^2): the conditioning of f32 at a saturated output, not the summation order that section 8f's 1e-4 bar is
    about -- and the one-point segment's code-gradient row has no second point to hide it."""
    out = [np.array(W, dtype=np.float32) for W in Ws]
    Cn = out[0].shape[1] - 3
    for l in layers:
        if l + 1 == 4:
            out[4][:, :509 - Cn] *= np.float32(1 - p)
        else:
            out[l + 1] *= np.float32(1 - p)
    return out


def _case(c, p, layers):
    """One case's decoder and points, cached and never modified: the weights of _rescaled, and for slot i of segment s, of its
    CANDIDATES uniform candidates, the one whose float64 prediction under the mask of (SEED, s, i) -- numpy and the restatement
    only, no GPU -- is smallest in magnitude (the same reason: away from the saturated tanh)."""
    import torch
    import dropout_restatement as dr
    key = (p, tuple(layers))
    if key not in c['cases']:
        Ws = _rescaled(c['Ws0'], p, layers)
        W64, b64 = [W.astype(np.float64) for W in Ws], [np.asarray(b, np.float64) for b in c['bs']]
        K, parts = CANDIDATES, []
        for s, a, b in _segments():
            n = b - a
            if n == 0:
                continue
            inp = np.concatenate([np.repeat(c['codes_np'][s:s + 1].astype(np.float64), n * K, 0), c['cand_np'][a:b].astype(np.float64).reshape(-1, 3)], 1)
            x = inp
            for l in range(9):
                if l == 4:
                    x = np.concatenate([x, inp], 1)
                z = x @ W64[l].T + b64[l]
                if l < 8:
                    x = np.maximum(z, 0)
                    if l in layers:
                        x = x * np.repeat(dr.keep(SEED, l, s, n, x.shape[1], dr.threshold(p)), K, 0) * dr.scale(p)
            best = np.abs(np.tanh(z).reshape(n, K)).argmin(1)
            parts.append(c['cand_np'][a:b][np.arange(n), best])
        pts = np.concatenate(parts).astype(np.float32)
        c['cases'][key] = dict(Ws=Ws, weights=_weights_of(_module(Ws, c['bs'])), pts_np=pts, pts=torch.from_numpy(pts).cuda())
    return c['cases'][key]


@pytest.fixture(scope='module')
def inputs(fixture_decoder):
    """Per code length, made once and never modified: the fixture's weights (Ws0), codes (6, C), candidate points, an upstream
    gradient; Ws / weights / pts are those of the case with dropout on all eight layers and p = 0.2 (_case)."""
    import torch
    from distr import fixture
    out = {}
    for Cn in (256, 64, 300):
        Ws, bs, latent = fixture_decoder if Cn == 256 else fixture.make_decoder_weights(latent_size=Cn)
        rs = np.random.RandomState(200 + Cn)
        codes = (latent + 0.3 * np.abs(latent).max() * rs.standard_normal((len(SIZES), Cn))).astype(np.float32)
        cand = ((rs.rand(sum(SIZES), CANDIDATES, 3) - 0.5) * 1.6).astype(np.float32)
        w = rs.standard_normal((sum(SIZES), 1)).astype(np.float32)
        out[Cn] = dict(Ws0=Ws, bs=bs, latent=latent, codes_np=codes, cand_np=cand, w_np=w, cases={},
                       codes=torch.from_numpy(codes).cuda(), w=torch.from_numpy(w).cuda())
        out[Cn].update(_case(out[Cn], 0.2, range(8)))
    return out


@pytest.mark.parametrize('Cn,p,layers', CASES, ids=['C%d-p%.1f-%s' % (c, p, 'all' if len(l) == 8 else '037') for c, p, l in CASES])
def test_mask_values_and_gradients(inputs, Cn, p, layers):
    import dropout_restatement as dr
    import train_restatement as tr
    c = inputs[Cn]
    k = _case(c, p, layers)
    r = _run(k['weights'], c['codes'], k['pts'], SIZES, c['w'], None, _drop(layers, p))
    scale, T = dr.scale(p), dr.threshold(p)
    gates = _gates(r['X'], layers, scale)
    y, pre, ref_W, ref_b, ref_rows = tr.gradients(k['Ws'], c['bs'], c['codes_np'], k['pts_np'], SIZES, c['w_np'], None, gates=gates)
    tag = 'C = %d, p = %.1f, layers %s' % (Cn, p, list(layers))
    d = (r['sdf'].double() - y).abs().max().item()
    flips = 0
    for l in range(8):
        X, z = r['X'][l], pre[l]
        assert X.shape == z.shape and (X >= 0).all(), l
        pos = (X > 0).numpy()
        keep = dr.keep_list(SEED, l, SIZES, X.shape[1], T) if l in layers else np.ones(tuple(X.shape), bool)
        if l in layers:
            dropped = X.numpy()[~keep]
            assert 0 < dropped.size < keep.size and not dropped.any() and not np.signbit(dropped).any(), (tag, l)       # exactly +0
        diff = (pos != (z.numpy() > 0)) & keep          # (a layer without dropout: every unit follows its own ReLU -- no forced zeros)
        flips += int(diff.sum())
        assert not diff.any() or np.abs(z.numpy()[diff]).max() < 1e-5, (tag, l)
        assert pos.any() and not pos.all(), l
    print('%s: |sdf - float64| <= %.3e; %d kept units on the other side of the ReLU than in float64' % (tag, d, flips))
    assert d <= 2e-6, (tag, d)
    _assert_gradients(r['grads'][:9], r['grads'][9:], r['g_lat'], ref_W, ref_b, ref_rows, SIZES, tag)


@pytest.fixture(scope='module')
def base_run(inputs):
    c = inputs[256]
    return _run(c['weights'], c['codes'], c['pts'], SIZES, c['w'], None, _drop(range(8), 0.2))


def test_same_seed_same_bytes_other_seed_other_values(inputs, base_run):
    import torch
    c = inputs[256]
    again = _run(c['weights'], c['codes'], c['pts'], SIZES, c['w'], None, _drop(range(8), 0.2))
    assert _same_bytes(base_run, again)
    other = _run(c['weights'], c['codes'], c['pts'], SIZES, c['w'], None, _drop(range(8), 0.2, seed=SEED + 1))
    assert not torch.equal(base_run['sdf'], other['sdf'])
    plain = _run(c['weights'], c['codes'], c['pts'], SIZES, c['w'], None, None)
    assert not torch.equal(base_run['sdf'], plain['sdf'])
    # a layer mask of 0 and a null struct take the plain path
    assert _same_bytes(plain, _run(c['weights'], c['codes'], c['pts'], SIZES, c['w'], None, _drop((), 0.2)))


def test_a_segment_alone_with_its_global_index(inputs, base_run):
    import torch
    from distr import functions
    c = inputs[256]
    for s, p0, p1 in _segments():
        if p0 == p1:
            continue
        sdf, saved = functions.train_forward(c['weights'], c['codes'][s:s + 1], c['pts'][p0:p1], [p1 - p0], None, dropout=_drop(range(8), 0.2, base=s))
        _, g_lat = functions.train_backward(saved, c['w'][p0:p1])
        assert torch.equal(sdf.cpu(), base_run['sdf'][p0:p1]), s
        assert torch.equal(g_lat.cpu(), base_run['g_lat'][s:s + 1]), s
    s, p0, p1 = 4, 130, 260
    sdf, _ = functions.train_forward(c['weights'], c['codes'][s:s + 1], c['pts'][p0:p1], [p1 - p0], None, dropout=_drop(range(8), 0.2, base=0))
    assert not torch.equal(sdf.cpu(), base_run['sdf'][p0:p1])          # the segment's index is part of the mask


def _drop_module(Ws, bs, layers=tuple(range(8)), p=0.2, weight_norm=False):
    return _module(Ws, bs, weight_norm=weight_norm, dropout=list(layers), dropout_prob=p)


def test_chunks_of_64_segments(fixture_decoder):
    """65 segments of 3 points through decode_sdf_train: two calls (64 + 1); every segment equals the stand-alone call with its global index."""
    import torch
    from core.utils.decoder_utils import decode_sdf_train
    from distr import functions
    Ws, bs, latent = fixture_decoder
    dec = _drop_module(Ws, bs).train()
    weights = _weights_of(dec)
    S, N = 65, 3
    rs = np.random.RandomState(9)
    tc = torch.from_numpy((latent + 0.3 * np.abs(latent).max() * rs.standard_normal((S, 256))).astype(np.float32)).cuda()
    tp = torch.from_numpy(((rs.rand(S, N, 3) - 0.5) * 1.6).astype(np.float32)).cuda()
    tw = torch.from_numpy(rs.standard_normal((S, N, 1)).astype(np.float32)).cuda()
    lat = tc.clone().requires_grad_(True)
    y = decode_sdf_train(dec, lat, tp, clamp_dist=None, dropout_seed=SEED)
    assert y.shape == (S, N, 1)
    (y * tw).sum().backward()
    for s in (0, 1, 63, 64):
        sdf, saved = functions.train_forward(weights, tc[s:s + 1], tp[s], [N], None, dropout=_drop(range(8), 0.2, base=s))
        _, g_lat = functions.train_backward(saved, tw[s])
        assert torch.equal(sdf, y.detach()[s]) and torch.equal(g_lat[0], lat.grad[s]), s
    a = _run(weights, tc[:64], tp[:64].reshape(-1, 3), [N] * 64, tw[:64].reshape(-1), None, _drop(range(8), 0.2))
    b = _run(weights, tc[64:], tp[64:].reshape(-1, 3), [N], tw[64:].reshape(-1), None, _drop(range(8), 0.2, base=64))
    assert torch.equal(y.detach().reshape(-1, 1).cpu(), torch.cat([a['sdf'], b['sdf']]))
    for l in range(9):
        assert torch.equal(getattr(dec, 'lin%d' % l).weight.grad.cpu(), a['grads'][l] + b['grads'][l]), l


def test_three_slabs(fixture_decoder):
    import torch
    import dropout_restatement as dr
    import train_restatement as tr
    from distr import functions
    L0 = functions.train_slab_plan(1)[0]
    n = 2 * L0 + 1
    assert functions.train_slab_plan(functions.train_segment_rows([n])[-1]) == (L0, 3)
    Ws, bs, latent = fixture_decoder
    Ws = _rescaled(Ws, 0.2, range(8))
    weights = _weights_of(_module(Ws, bs))
    rs = np.random.RandomState(45)
    code = (latent + 0.3 * np.abs(latent).max() * rs.standard_normal((1, 256))).astype(np.float32)
    pts = ((rs.rand(n, 3) - 0.5) * 1.6).astype(np.float32)
    w = rs.standard_normal((n, 1)).astype(np.float32)
    tc, tp, tw = (torch.from_numpy(a).cuda() for a in (code, pts, w))
    r = _run(weights, tc, tp, [n], tw, None, _drop(range(8), 0.2))
    assert _same_bytes(r, _run(weights, tc, tp, [n], tw, None, _drop(range(8), 0.2)))
    for l in (0, 3, 7):         # the mask follows the point index through every 64-row block of the one segment
        keep = dr.keep(SEED, l, 0, n, r['X'][l].shape[1], dr.threshold(0.2))
        assert not r['X'][l].numpy()[~keep].any(), l
    _, _, ref_W, ref_b, ref_rows = tr.gradients(Ws, bs, code, pts, [n], w, None, gates=_gates(r['X'], range(8), dr.scale(0.2)))
    _assert_gradients(r['grads'][:9], r['grads'][9:], r['g_lat'], ref_W, ref_b, ref_rows, [n], 'three slabs')


def test_eval_mode_p0_and_empty_list_are_the_plain_call(inputs, fixture_decoder):
    import torch
    from core.utils.decoder_utils import decode_sdf_train
    Ws, bs, _ = fixture_decoder
    c = inputs[256]

    def run(dec, **kw):
        for p in dec.parameters():
            p.grad = None
        lat = c['codes'].clone().requires_grad_(True)
        y = decode_sdf_train(dec, lat, c['pts'], counts=SIZES, clamp_dist=None, **kw)
        (y * c['w']).sum().backward()
        return [y.detach(), lat.grad] + [p.grad for p in dec.parameters()]
    plain = run(_module(Ws, bs))
    for name, dec in (('eval', _drop_module(Ws, bs).eval()), ('p = 0', _drop_module(Ws, bs, p=0.0).train()), ('empty list', _drop_module(Ws, bs, layers=()).train())):
        got = run(dec, dropout_seed=SEED)
        assert len(got) == len(plain) and all(torch.equal(a, b) for a, b in zip(got, plain)), name
    assert not torch.equal(run(_drop_module(Ws, bs).train(), dropout_seed=SEED)[0], plain[0])


def test_autograd_node_equals_the_low_level_calls(inputs, base_run, fixture_decoder):
    import torch
    from core.utils.decoder_utils import decode_sdf_train
    c, r = inputs[256], base_run
    dec = _drop_module(c['Ws'], c['bs']).train()
    lat = c['codes'].clone().requires_grad_(True)
    y = decode_sdf_train(dec, lat, c['pts'], counts=torch.tensor(SIZES), clamp_dist=None, dropout_seed=SEED)
    assert y.shape == (sum(SIZES), 1) and y.requires_grad
    (y * c['w']).sum().backward()
    assert torch.equal(y.detach().cpu(), r['sdf']) and torch.equal(lat.grad.cpu(), r['g_lat'])
    for l in range(9):
        lin = getattr(dec, 'lin%d' % l)
        assert torch.equal(lin.weight.grad.cpu(), r['grads'][l]) and torch.equal(lin.bias.grad.cpu(), r['grads'][9 + l]), l


def test_weight_norm_decoder(inputs, fixture_decoder):
    """Under weight norm the gradients arrive at weight_g / weight_v: against float64 autograd through the same fold and the GPU's gates."""
    import torch
    import dropout_restatement as dr
    import train_restatement as tr
    from core.utils.decoder_utils import decode_sdf_train
    from distr import functions
    c = inputs[256]
    dec = _drop_module(c['Ws'], c['bs'], weight_norm=True).train()
    _, saved = functions.train_forward(_weights_of(dec), c['codes'], c['pts'], SIZES, None, dropout=_drop(range(8), 0.2))
    gates = _gates(_activations(saved), range(8), dr.scale(0.2))
    lat = c['codes'].clone().requires_grad_(True)
    (decode_sdf_train(dec, lat, c['pts'], counts=SIZES, clamp_dist=None, dropout_seed=SEED) * c['w']).sum().backward()
    params = dict(dec.named_parameters())
    assert len(params) == 26
    p64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in params.items()}
    W64 = [p64['lin%d.weight_v' % l] * (p64['lin%d.weight_g' % l] / p64['lin%d.weight_v' % l].norm(dim=1, keepdim=True)) for l in range(8)] + [p64['lin8.weight']]
    b64 = [p64['lin%d.bias' % l] for l in range(9)]
    c64, x64, w64 = tr.to64([c['codes_np']], True)[0], tr.to64([c['pts_np']])[0], tr.to64([c['w_np']])[0]
    yr, _ = tr.forward(W64, b64, c64, x64, SIZES, None, gates)
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
    print('weight norm with dropout: largest residual %.3e' % worst)


G32_GRADS = ['g_codes', 'g_lin8_weight'] + ['g_bias%d' % l for l in range(9)] + ['g_weight_g%d' % l for l in range(8)] + \
    ['g_v%d_%s' % (l, k) for l in range(8) for k in ('rowsum', 'colsum', 'rows')]


@pytest.mark.parametrize('case', ['eval', 'train'])
def test_golden_g32_forward_train(fixture_decoder, case):
    """Decoder.forward_train against the reference's training forward (golden G32: weight norm, dropout on all eight layers, p = 0.2,
    3 x 70 samples, min / max clamp), `train` under the recorded seed. Bars: max(2 x the recorded floor, section 8f's bar)."""
    import torch
    import dropout_restatement as dr
    from distr import fixture, functions
    g = np.load(os.path.join(GOLDEN, 'g32_train_forward.npz'))
    Ws, bs, _ = fixture_decoder
    assert str(g['weights_sha256']) == fixture.weights_sha256(Ws, bs)
    B, S = g['sdf_data'].shape[:2]
    seed, p = int(g['seed']), float(g['p'])
    dec = _drop_module(Ws, bs, p=p, weight_norm=True).train(case == 'train')
    data = torch.from_numpy(g['sdf_data']).cuda()
    lat = torch.from_numpy(g['codes']).cuda().requires_grad_(True)
    lo, hi = torch.from_numpy(g['min_vec']).cuda(), torch.from_numpy(g['max_vec']).cuda()
    pred, l1, l2 = dec.forward_train(data, lat, lo, hi, dropout_seed=seed)
    (l1.mean() + float(g['code_reg']) * l2.mean()).backward()
    assert pred.shape == (B * S, 1) and l1.shape == (B * S,) and l2.shape == (B,)
    for name, got in (('pred_sdf', pred), ('loss_l1', l1), ('loss_l2_size', l2)):
        d = np.abs(got.detach().cpu().numpy() - g['%s_%s' % (case, name)]).max()
        bar = max(2 * float(g['%s_floor_%s' % (case, name)]), 2e-6)
        print('G32 %s %s: residual %.3e (bar %.1e)' % (case, name, d, bar))
        assert d <= bar, (case, name, d)
    params = {k: v.grad.cpu().numpy() for k, v in dec.named_parameters()}
    got = dict(g_codes=lat.grad.cpu().numpy(), g_lin8_weight=params['lin8.weight'])
    for l in range(9):
        got['g_bias%d' % l] = params['lin%d.bias' % l]
    for l in range(8):
        got['g_weight_g%d' % l] = params['lin%d.weight_g' % l]
        gv = params['lin%d.weight_v' % l]
        got['g_v%d_rowsum' % l], got['g_v%d_colsum' % l] = gv.astype(np.float64).sum(1), gv.astype(np.float64).sum(0)
        got['g_v%d_rows' % l] = gv[[min(int(i), gv.shape[0] - 1) if i >= 0 else gv.shape[0] - 1 for i in g['rows']]]
    worst = 0.0
    for name in G32_GRADS:
        want = g['%s_%s' % (case, name)]
        rel = np.abs(got[name] - want).max() / np.abs(want).max()
        bar = max(2 * float(g['%s_floor_%s' % (case, name)]), 1e-4)
        worst = max(worst, rel / bar)
        assert rel <= bar, (case, name, rel, bar)
    print('G32 %s: the largest gradient residual is %.3f of its bar' % (case, worst))
    # the mask the GPU applied: the low-level call on the same inputs (forward_train's bytes), its saved activations
    sdf, saved = functions.train_forward(_weights_of(dec), lat.detach(), data.reshape(-1, 4)[:, :3], [S] * B, None,
                                         dropout=_drop(range(8), p, seed=seed) if case == 'train' else None)
    assert torch.equal(torch.minimum(torch.maximum(sdf, lo), hi), pred.detach())
    for l, X in enumerate(_activations(saved)):
        keep = dr.g32_bits(g, 'train', 'keep', l) if case == 'train' else True
        want = dr.g32_bits(g, case, 'pos', l) & keep
        diff = ((X > 0).numpy() != want) & ~dr.g32_bits(g, case, 'near', l)
        assert not diff.any(), (case, l, int(diff.sum()))


LOOP_LR = 1e-4


def test_sgd_loop(fixture_decoder, monkeypatch):
    """Five plain SGD steps of forward_train in training mode with the seeds s, s + 1, ..., on the weights and the codes, loss =
    loss_l1.mean() + 1e-4 * loss_l2_size.mean(); and the same loop on the float64 torch Decoder with F.dropout substituted by the
    restatement's masks under the same seeds. The decoder is the fixture with _rescaled weights; 5 scenes x 65 samples with
    |sdf| < 0.05 for the fixture itself in eval mode, targets = that sdf + 0.06; the min / max clamp is set so that half of the first
    step's float64 predictions clamp (under dropout this decoder's predictions all leave the reference's -/+ 0.1: no gradient). Learning rate 1e-4, below
    test_gpu_train.py's 2.5e-4 (chosen there on the CPU for a loss without the dropout noise). The losses agree to 1e-4 relative at
    every step (section 8f's loop bar and its caveat on knife-edge units)."""
    import copy
    import torch
    import dropout_restatement as dr
    from core.utils.decoder_utils import decode_sdf_batch
    Ws, bs, latent = fixture_decoder
    B, S, p, steps = 5, 65, 0.2, 5
    dec = _drop_module(_rescaled(Ws, p, range(8)), bs, p=p)
    rs = np.random.RandomState(77)
    codes = torch.from_numpy((latent + 0.3 * np.abs(latent).max() * rs.standard_normal((B, 256))).astype(np.float32)).cuda()
    cand = torch.from_numpy(((rs.rand(B, 12000, 3) - 0.5) * 1.6).astype(np.float32)).cuda()
    dec0 = _module(Ws, bs)          # the fixture itself, in eval mode: where the rescaled decoder's predictions under dropout scatter around
    f = decode_sdf_batch(dec0, codes, cand, clamp_dist=None, no_grad=True)
    pts = torch.stack([cand[s][(f[s, :, 0].abs() < 0.05).nonzero()[:S, 0]] for s in range(B)])
    assert pts.shape == (B, S, 3)
    target = decode_sdf_batch(dec0, codes, pts, clamp_dist=None, no_grad=True) + 0.06
    data = torch.cat([pts, target], 2)

    # float64: the torch Decoder, F.dropout handing out the masks of (seed of the step, layer = call number)
    state = dict(seed=0, call=0)

    def masked(x, p=0.5, training=True, inplace=False):
        assert training
        keep = dr.keep_list(state['seed'], state['call'], [S] * B, x.shape[1], dr.threshold(p))
        state['call'] += 1
        return x * torch.from_numpy(keep.astype(np.float64) * dr.scale(p))
    dec64 = copy.deepcopy(dec).cpu().double().train()
    c64 = codes.cpu().double().requires_grad_(True)
    d64 = data.cpu().double().reshape(-1, 4)
    ref = []
    monkeypatch.setattr(torch.nn.functional, 'dropout', masked)
    # the min / max clamp: half way between the two middle ones of the float64 decoder's |predictions| under the first step's masks
    state.update(seed=SEED, call=0)
    with torch.no_grad():
        y0 = dec64(torch.cat([torch.repeat_interleave(c64, S, dim=0), d64[:, :3]], 1)).abs().reshape(-1).sort().values
    bound = float(np.float32(0.5 * (y0[B * S // 2 - 1] + y0[B * S // 2]).item()))          # (a float32 number: the same bound on both sides)
    assert y0[B * S // 2] - y0[B * S // 2 - 1] > 1e-5 and 0 < bound < 0.99, (bound, y0[B * S // 2 - 1:B * S // 2 + 1])
    lo64, hi64 = torch.full((B * S, 1), -bound, dtype=torch.float64), torch.full((B * S, 1), bound, dtype=torch.float64)
    lo, hi = lo64.float().cuda(), hi64.float().cuda()
    params64 = list(dec64.parameters()) + [c64]
    for i in range(steps):
        for q in params64:
            q.grad = None
        state.update(seed=SEED + i, call=0)
        y = dec64(torch.cat([torch.repeat_interleave(c64, S, dim=0), d64[:, :3]], 1))
        assert state['call'] == 8
        loss = (torch.minimum(torch.maximum(y, lo64), hi64) - torch.minimum(torch.maximum(d64[:, 3:4], lo64), hi64)).abs().mean() + 1e-4 * c64.pow(2).mean(1).mean()
        ref.append(loss.item())
        loss.backward()
        with torch.no_grad():
            for q in params64:
                q -= LOOP_LR * q.grad
    monkeypatch.undo()

    dec.train()
    lat = codes.clone().requires_grad_(True)
    params = list(dec.parameters()) + [lat]
    before = dec.lin4.weight.detach().clone()
    losses = []
    for i in range(steps):
        for q in params:
            q.grad = None
        pred, l1, l2 = dec.forward_train(data, lat, lo, hi, dropout_seed=SEED + i)
        loss = l1.mean() + 1e-4 * l2.mean()
        losses.append(loss.item())
        loss.backward()
        with torch.no_grad():
            for q in params:
                q -= LOOP_LR * q.grad
    print('float64: %s\nGPU:     %s' % (' '.join('%.8f' % x for x in ref), ' '.join('%.8f' % x for x in losses)))
    assert (dec.lin4.weight.detach() - before).abs().max().item() > 0 and len(set(losses)) == steps
    for a, b in zip(losses, ref):
        assert abs(a - b) <= 1e-4 * b, (losses, ref)


def test_refusals(fixture_decoder):
    import ctypes as C
    import torch
    import train_abi
    from core.utils.decoder_utils import decode_sdf_train
    from distr import binding, decoder_pack, functions
    Ws, bs, _ = fixture_decoder
    lat = torch.zeros(2, 256, device='cuda')
    pts = torch.zeros(8, 3, device='cuda')
    drop = _drop_module(Ws, bs).train()
    with pytest.raises(decoder_pack.UnsupportedDecoder, match='training mode with dropout'):
        decode_sdf_train(drop, lat, pts, counts=[5, 3])
    assert decode_sdf_train(drop, lat, pts, counts=[5, 3], dropout_seed=3).shape == (8, 1)
    ldrop = _module(Ws, bs, latent_dropout=True, dropout=[0], dropout_prob=0.2).train()
    with pytest.raises(decoder_pack.UnsupportedDecoder, match='latent_dropout'):
        decode_sdf_train(ldrop, lat, pts, counts=[5, 3], dropout_seed=3)
    with pytest.raises(ValueError, match='dropout_prob'):
        decode_sdf_train(_drop_module(Ws, bs, p=1.0).train(), lat, pts, counts=[5, 3], dropout_seed=3)
    with pytest.raises(ValueError, match='layer 8'):
        decode_sdf_train(_drop_module(Ws, bs, layers=(0, 8)).train(), lat, pts, counts=[5, 3], dropout_seed=3)
    with pytest.raises(ValueError, match='seed'):
        decode_sdf_train(drop, lat, pts, counts=[5, 3], dropout_seed=-1)
    # the C ABI's own refusals
    weights = _weights_of(drop)
    ctx = functions._train_context(0)
    L, p = ctx.L, binding.ptr
    cnt = (C.c_int64 * 2)(5, 3)
    need = L.distr_train_workspace_bytes(256, 2, cnt)
    out = torch.empty(8, 1, device='cuda')
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    tw = train_abi.train_weights(weights, 256)
    good = dict(layer_mask=0xff, threshold=858993459, scale=1.25, seed=1, segment_base=0)

    def call(td):
        rc = L.distr_train_forward_dropout(ctx.h, C.byref(tw), 2, cnt, p(lat), 256, p(pts), 0.1, p(out), p(ws), need, ctx.stream(), C.byref(td))
        return rc, L.distr_last_error(ctx.h).decode()
    short = binding.TrainDropout(**good)
    short.struct_size = 24
    for word, td in (('struct_size', short), ('layer_mask', binding.TrainDropout(**dict(good, layer_mask=0x1ff))),
                     ('scale', binding.TrainDropout(**dict(good, scale=0.99))), ('scale', binding.TrainDropout(**dict(good, scale=float('inf')))),
                     ('segment_base', binding.TrainDropout(**dict(good, segment_base=-2)))):
        rc, err = call(td)
        assert rc == -1 and word in err, (word, rc, err)
    assert call(binding.TrainDropout(**good))[0] == 0
    torch.cuda.synchronize()
