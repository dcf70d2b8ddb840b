"""decode_color_train on the GPU: the colour decoder on the layer-wise train path, against float64.

  values      on 323 points in 5 segments [1, 65, 0, 63, 194], cs = 256: max and p99 of |rgb_train - rgb64| at most 2 x the same
              statistics of the fused decode_color_batch (the parent's code) against float64 on the same inputs, measured here; the
              factor 2 allows for two f32 orderings of the same chains
  gates       the saved gates differ from float64's own only where |pre-activation64| < 1e-5
  gradients   all eighteen and both code gradients against the float64 restatement run with the GPU's gates, per block (g_W0 = [shape |
              colour | xyz], g_W4 = [lin3 cols | shape | colour | xyz], the code gradient in its shape and colour halves) at 1e-4 of the
              block's largest entry -- section 8f's bar. Cases: cs = 256 and 5, a shared colour code with per-segment shape codes and the
              reverse, 65 segments (two chunks), a list of 640 rows (three slabs), a weight-norm decoder
  bytes       two runs agree; a segment's rgb slice and its two code-gradient rows equal a call on that segment alone; the autograd
              node's results equal the low-level calls'
  SGD         three steps on the weights and the colour code against the float64 Decoder: the losses agree to 1e-4 relative; then
              decode_color_batch on the updated module agrees with float64 (the colour engine re-packed by itself)
  dropout     the mask the GPU applied equals distr_train_dropout_keep's; eval mode / p = 0 with a seed = the seedless call, byte for byte
  G34         the reference's decode_color under DeepSDF's specification, cases eval and train
  refusals
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SIZES = [1, 65, 0, 63, 194]
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'g34_color_train.npz')
SEED = 0x5EED0C01

# name -> (cs, counts, shared colour code, shared shape code, weight norm)
_many = [(7 * s) % 5 + (70 if s in (3, 64) else 0) for s in range(65)]        # 65 segments: 0..4 points, two of 70+; two chunks
CASES = {'cs256': (256, SIZES, False, False, False), 'cs5': (5, SIZES, False, False, False),
         'shared-colour': (256, SIZES, True, False, False), 'shared-shape': (5, SIZES, False, True, False),
         '65-segments': (5, _many, False, False, False), 'three-slabs': (256, [300, 277], False, False, False),
         'weight-norm': (256, SIZES, False, False, True)}


class Run(object):
    """One decoder, one list: the module on the GPU, the inputs, and the low-level calls chunk by chunk."""

    def __init__(self, cs, counts, shared_c=False, shared_s=False, weight_norm=False, dropout=None, p=0.0):
        import torch
        import color_train_restatement as cr
        from distr import decoder_pack, fixture
        self.cs, self.counts = cs, list(counts)
        self.Ws, self.bs, cc0 = fixture.make_color_decoder_weights(color_size=cs)
        self.dec = cr.color_module(self.Ws, self.bs, weight_norm=weight_norm, dropout=dropout, dropout_prob=p, dtype=torch.float32).cuda()
        S, n = len(counts), sum(counts)
        rs = np.random.RandomState(600 + cs + 3 * n + S)
        self.cc = (cc0 + 0.1 * rs.standard_normal((1 if shared_c else S, cs))).astype(np.float32)
        self.sc = (0.1 * rs.standard_normal((1 if shared_s else S, 256))).astype(np.float32)
        self.pts = ((rs.rand(n, 3) - 0.5) * 1.6).astype(np.float32)
        self.w = (1.0 + rs.standard_normal((n, 3))).astype(np.float32)
        Wt, bt = decoder_pack.effective_weights_torch_color(self.dec)
        self.weights = [t.detach().contiguous() for t in Wt + bt]          # what the train path reads (weight norm folded)
        self.t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def low_level(self, w=None, dropout=None, keep_saved=False):
        """train_forward / train_backward per chunk of 64 segments, as DecodeColorTrainFunction runs them: (rgb, [gates of lin0..lin7 in
        point order] or None, eighteen gradients added in chunk order, g_latent rows (S, L), [saved])."""
        import torch
        from distr import functions
        S = len(self.counts)
        lat = functions.color_code_rows(functions._CodeLayout(256 + self.cs, torch.device('cuda')), self.t(self.cc), self.t(self.sc), S)
        net = functions.color_train_net(self.weights)
        x, wt = self.t(self.pts), self.t(self.w if w is None else w)
        outs, gates, total, rows, saved_all = [], [[] for _ in range(8)], None, [], []
        for s0 in range(0, S, 64):
            cnt = self.counts[s0:s0 + 64]
            p0, n = sum(self.counts[:s0]), sum(cnt)
            drop = None if dropout is None else tuple(dropout[:4]) + (dropout[4] + s0,)
            out, saved = functions.train_forward(self.weights, lat[s0:s0 + 64] if lat.shape[0] > 1 else lat, x[p0:p0 + n], cnt, None, dropout=drop, net=net)
            idx = torch.cat([torch.arange(*saved.rows(s)) for s in range(len(cnt))]).cuda()
            for l in range(8):
                gates[l].append(saved.activations(l + 1)[idx].clone() if keep_saved else (saved.activations(l + 1)[idx] > 0))
            grads, g_lat = functions.train_backward(saved, wt[p0:p0 + n])
            outs.append(out)
            rows.append(g_lat)
            saved_all.append(saved)
            if total is None:
                total = grads
            else:
                for a, b in zip(total, grads):
                    a += b
        return torch.cat(outs), [torch.cat(g).cpu() for g in gates], total, torch.cat(rows), saved_all

    def autograd(self, w=None, seed=None):
        """decode_color_train + backward of sum(rgb * w): (rgb, {parameter name: grad}, g_color_codes, g_shape_codes)"""
        import torch
        from core.utils.decoder_utils import decode_color_train
        for p in self.dec.parameters():
            p.grad = None
        cc, sc = self.t(self.cc).requires_grad_(True), self.t(self.sc).requires_grad_(True)
        rgb = decode_color_train(self.dec, cc, sc, self.t(self.pts), counts=self.counts, dropout_seed=seed)
        (rgb * self.t(self.w if w is None else w)).sum().backward()
        return rgb.detach(), {k: p.grad.clone() for k, p in self.dec.named_parameters()}, cc.grad, sc.grad

    def split(self, g_rows):
        """(S, L) code-gradient rows -> (g_color_codes, g_shape_codes) in the inputs' shapes (a shared code: the sum of the rows)"""
        g = g_rows.cpu().numpy().astype(np.float64)
        gc, gs = g[:, 256:], g[:, :256]
        return (gc.sum(0, keepdims=True) if self.cc.shape[0] == 1 else gc), (gs.sum(0, keepdims=True) if self.sc.shape[0] == 1 else gs)


_runs = {}


def run_of(name):
    if name not in _runs:
        _runs[name] = Run(*CASES[name])
    return _runs[name]


@pytest.fixture(scope='module')
def base():
    """cs = 256 on SIZES: the run, its float64 values and pre-activations (computed once, left unchanged), the low-level results."""
    import color_train_restatement as cr
    r = run_of('cs256')
    y64, pre64 = cr.forward(cr.to64(r.Ws), cr.to64(r.bs), *cr.to64([r.cc, r.sc, r.pts]), r.counts)
    return dict(run=r, y64=y64.numpy(), pre64=[z.numpy() for z in pre64], low=r.low_level())


def _stats(a, ref):
    d = np.abs(np.asarray(a, np.float64) - ref).ravel()
    return d.max(), np.percentile(d, 99)


def test_values_against_the_fused_path(base):
    import torch
    from core.utils.decoder_utils import decode_color_batch, decode_color_train
    r = base['run']
    with torch.no_grad():
        fused = decode_color_batch(r.dec, r.t(r.cc), r.t(r.sc), r.t(r.pts), counts=r.counts, no_grad=True)
        train = decode_color_train(r.dec, r.t(r.cc), r.t(r.sc), r.t(r.pts), counts=r.counts)
    assert train.shape == fused.shape == (323, 3) and not train.requires_grad
    fm, fp = _stats(fused.cpu().numpy(), base['y64'])
    tm, tp = _stats(train.cpu().numpy(), base['y64'])
    print('values against float64: train path max %.3e p99 %.3e; fused path max %.3e p99 %.3e' % (tm, tp, fm, fp))
    assert tm <= 2 * fm and tp <= 2 * fp, (tm, tp, fm, fp)
    assert torch.equal(train, base['low'][0])
    cube = r.t(r.pts[:300]).reshape(5, 60, 3)
    assert torch.equal(decode_color_train(r.dec, r.t(r.cc), r.t(r.sc), cube).reshape(-1, 3),
                       decode_color_train(r.dec, r.t(r.cc), r.t(r.sc), cube.reshape(-1, 3), counts=[60] * 5))


def test_saved_gates_against_float64(base):
    gates, n_diff = base['low'][1], 0
    for l in range(8):
        diff = gates[l].numpy() != (base['pre64'][l] > 0)
        n_diff += int(diff.sum())
        assert gates[l].shape == base['pre64'][l].shape
        assert not diff.any() or np.abs(base['pre64'][l][diff]).max() < 1e-5, (l, np.abs(base['pre64'][l][diff]).max())
    print('gates: %d of %d differ from float64\'s own, all at |pre-activation| < 1e-5' % (n_diff, sum(g.numel() for g in gates)))


@pytest.mark.parametrize('name', list(CASES))
def test_gradients_blockwise(name, base):
    import torch
    import color_train_restatement as cr
    r = run_of(name)
    rgb, gates, grads, g_rows, _ = base['low'] if name == 'cs256' else r.low_level()
    W32 = [w.cpu().numpy() for w in r.weights]
    y, _, ref_W, ref_b, ref_c, ref_s = cr.gradients(W32[:9], W32[9:], r.cc, r.sc, r.pts, r.counts, r.w, gates=gates)
    assert np.abs(rgb.cpu().numpy() - y.numpy()).max() < 1e-5
    res = cr.blockwise_residuals([g.cpu().numpy() for g in grads], [t.numpy() for t in ref_W + ref_b], r.cs)
    res += cr.code_residuals(*r.split(g_rows), ref_c.numpy(), ref_s.numpy())
    worst = max(res, key=lambda t: t[1])
    print('%s: worst block %s: %.3e of its largest entry (%.3e)' % (name, worst[0], worst[1], worst[2]))
    for bname, rel, top in res:
        assert top > 0 and rel <= 1e-4, (name, bname, rel, top)
    if name == 'three-slabs':
        from distr import functions
        assert functions.train_slab_plan(functions.train_segment_rows(r.counts)[-1]) == (256, 3)
    if name == 'weight-norm':
        # through the fold: autograd carries g_W on to weight_g / weight_v; the float64 chain rule from the reference's g_W
        _, pg, _, _ = r.autograd()
        for l in range(8):
            lin = getattr(r.dec, 'lin%d' % l)
            v, g = lin.weight_v.detach().double().cpu().requires_grad_(True), lin.weight_g.detach().double().cpu().requires_grad_(True)
            (v * (g / v.norm(dim=1, keepdim=True))).backward(ref_W[l])
            for tag, got, ref in (('weight_v', pg['lin%d.weight_v' % l], v.grad), ('weight_g', pg['lin%d.weight_g' % l], g.grad)):
                rel = (got.double().cpu() - ref).abs().max().item() / ref.abs().max().item()
                assert rel <= 1e-4, (l, tag, rel)
        assert torch.equal(pg['lin8.weight'], grads[8])


def test_two_runs_and_the_autograd_node_give_the_same_bytes(base):
    import torch
    r = base['run']
    rgb, _, grads, g_rows, _ = base['low']
    rgb2, _, grads2, g_rows2, _ = r.low_level()
    assert torch.equal(rgb, rgb2) and torch.equal(g_rows, g_rows2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    rgb3, pg, g_c, g_s = r.autograd()
    assert torch.equal(rgb3, rgb) and torch.equal(g_c, g_rows[:, 256:]) and torch.equal(g_s, g_rows[:, :256])
    for l in range(9):
        assert torch.equal(pg['lin%d.weight' % l], grads[l]) and torch.equal(pg['lin%d.bias' % l], grads[9 + l]), l
    # 65 segments: the node's chunks of 64, weight gradients added in chunk order, are the low-level calls' too
    m = run_of('65-segments')
    rgb, _, grads, g_rows, saved = m.low_level()
    assert len(saved) == 2
    rgb3, pg, g_c, g_s = m.autograd()
    assert torch.equal(rgb3, rgb) and torch.equal(g_c, g_rows[:, 256:]) and torch.equal(g_s, g_rows[:, :256])
    assert all(torch.equal(pg['lin%d.weight' % l], grads[l]) and torch.equal(pg['lin%d.bias' % l], grads[9 + l]) for l in range(9))


def test_a_segment_alone(base):
    import torch
    from core.utils.decoder_utils import decode_color_train
    r = base['run']
    rgb, _, _, g_rows, _ = base['low']
    at = 0
    for s, n in enumerate(r.counts):
        cc, sc = r.t(r.cc[s:s + 1]).requires_grad_(True), r.t(r.sc[s:s + 1]).requires_grad_(True)
        one = decode_color_train(r.dec, cc, sc, r.t(r.pts[at:at + n]), counts=[n])
        assert torch.equal(one, rgb[at:at + n]), s
        (one * r.t(r.w[at:at + n])).sum().backward()
        assert torch.equal(cc.grad[0], g_rows[s, 256:]) and torch.equal(sc.grad[0], g_rows[s, :256]), s
        assert n > 0 or not g_rows[s].any()
        at += n


def test_three_sgd_steps_and_the_repack():
    """Weights and the colour code, lr 0.01, loss mean |rgb - target| (2 % per step on the float64 Decoder): the four losses agree to 1e-4
    relative. Then the fused decode_color_batch on the module the steps updated in place agrees with float64 of that module within 2 x
    the fused path's own error before the steps (measured here) -- it re-packed by itself -- and has moved by far more than that."""
    import copy
    import torch
    import color_train_restatement as cr
    from core.utils.decoder_utils import decode_color_batch, decode_color_train
    r = Run(256, [40, 0, 30])
    lr, steps = 0.01, 3
    rs = np.random.RandomState(77)
    cnt = torch.tensor(r.counts)
    rows = lambda cc: torch.repeat_interleave(torch.cat([torch.tensor(r.sc, dtype=torch.float64), cc], 1), cnt, dim=0)
    dec64 = copy.deepcopy(r.dec).double().cpu()
    with torch.no_grad():
        y0 = dec64(torch.cat([rows(torch.tensor(r.cc, dtype=torch.float64)), torch.tensor(r.pts, dtype=torch.float64)], 1))
    target = (y0 + 0.2 * torch.tensor(rs.standard_normal(y0.shape))).float()
    fused0 = decode_color_batch(r.dec, r.t(r.cc), r.t(r.sc), r.t(r.pts), counts=r.counts, no_grad=True)
    err0 = (fused0.double().cpu() - y0).abs().max().item()
    ref, cc64 = cr.l1_sgd_losses(dec64, torch.tensor(r.cc), torch.tensor(r.sc), torch.tensor(r.pts), r.counts, target, lr, steps)
    cc = r.t(r.cc).requires_grad_(True)
    params, losses = list(r.dec.parameters()) + [cc], []
    for i in range(steps + 1):
        for p in params:
            p.grad = None
        loss = (decode_color_train(r.dec, cc, r.t(r.sc), r.t(r.pts), counts=r.counts) - target.cuda()).abs().mean()
        losses.append(loss.item())
        if i == steps:
            break
        loss.backward()
        with torch.no_grad():
            for p in params:
                p -= lr * p.grad
    print('SGD losses: GPU %s, float64 %s' % (losses, ref))
    assert ref[-1] < 0.97 * ref[0]
    for a, b in zip(losses, ref):
        assert abs(a - b) <= 1e-4 * abs(b), (losses, ref)
    own64 = copy.deepcopy(r.dec).double().cpu()
    with torch.no_grad():
        y1 = own64(torch.cat([rows(cc.detach().double().cpu()), torch.tensor(r.pts, dtype=torch.float64)], 1))
    fused1 = decode_color_batch(r.dec, cc.detach(), r.t(r.sc), r.t(r.pts), counts=r.counts, no_grad=True)
    err1 = (fused1.double().cpu() - y1).abs().max().item()
    moved = (fused1 - fused0).abs().max().item()
    print('re-pack: fused path against float64 %.3e before the steps, %.3e after; the steps moved rgb by %.3e' % (err0, err1, moved))
    assert err1 <= 2 * err0 and moved > 100 * err0, (err0, err1, moved)


def test_dropout_mask_is_the_definition():
    """3 x 70 points, dropout [0..7], p = 0.2, training mode: the zeros of the saved activations are the definition's mask
    (distr_train_dropout_keep, a strided sample of it through the C call; tests/dropout_restatement.py in full), a kept unit is positive
    wherever float64 under the same masks has a pre-activation above 1e-5; lin0's output is the plain run's times scale or +0, byte for byte."""
    import torch
    import color_train_restatement as cr
    import dropout_restatement as dr
    from distr import binding, functions
    r = Run(256, [70] * 3, dropout=list(range(8)), p=0.2)
    r.dec.train()
    params = functions.train_dropout_params(r.dec, SEED)
    assert params == (0xff, dr.threshold(0.2), dr.scale(0.2))
    rgb, X, _, _, _ = r.low_level(dropout=params + (SEED, 0), keep_saved=True)
    plain = r.low_level(keep_saved=True)[1]
    L = binding.lib()
    masks = {l: dr.keep_list(SEED, l, r.counts, 253 if l == 3 else 512, params[1]) for l in range(8)}
    y64, pre64 = cr.forward(cr.to64(r.Ws), cr.to64(r.bs), *cr.to64([r.cc, r.sc, r.pts]), r.counts, masks=masks, scale=params[2])
    for l in range(8):
        keep, x = masks[l], X[l].numpy()
        for pt in range(0, 210, 7):
            for u in range(l, keep.shape[1], 16):
                assert L.distr_train_dropout_keep(SEED, params[1], l, pt // 70, pt % 70, u) == int(keep[pt, u]), (l, pt, u)
        assert abs(keep.mean() - 0.8) < 0.01
        assert not x[~keep].any(), l
        z = pre64[l].numpy()
        sure = np.abs(z) >= 1e-5
        assert np.array_equal((x > 0)[sure], (keep & (z > 0))[sure]), l
    x1 = np.where(masks[0], plain[0].numpy() * np.float32(params[2]), np.float32(0))
    assert np.array_equal(X[0].numpy(), x1)
    assert np.abs(rgb.cpu().numpy() - y64.numpy()).max() < 1e-5 and (rgb - r.low_level()[0]).abs().max() > 1e-3


def test_eval_mode_and_p0_ignore_the_seed(base):
    import torch
    r = base['run']
    rgb, pg, g_c, g_s = r.autograd()
    for run in (r, Run(256, SIZES, dropout=list(range(8)), p=0.2), Run(256, SIZES, dropout=list(range(8)), p=0.0)):
        if run is not r:
            run.dec.train(run.dec.dropout_prob == 0.0)          # p = 0.2 in eval mode; p = 0 in training mode
        rgb2, pg2, g_c2, g_s2 = run.autograd(seed=SEED)
        assert torch.equal(rgb, rgb2) and torch.equal(g_c, g_c2) and torch.equal(g_s, g_s2)
        assert all(torch.equal(pg[k], pg2[k]) for k in pg)


@pytest.mark.parametrize('case', ['eval', 'train'])
def test_golden_g34(case):
    """The reference's decode_color (G34) on the GPU: values within max(2 x floor, 2e-6), gradients within max(2 x floor, 1e-4) of the
    quantity's largest entry, everything that was recorded; the gate bits (for `train`: positive and kept) outside `near`."""
    import torch
    import color_train_restatement as cr
    from core.utils.decoder_utils import decode_color_train
    from distr import fixture, functions
    g = np.load(GOLDEN)
    Ws, bs, _ = fixture.make_color_decoder_weights(color_size=256)
    assert str(g['weights_sha256']) == fixture.weights_sha256(Ws, bs)
    seed, p = int(g['seed']), float(g['p'])
    dec = cr.color_module(Ws, bs, weight_norm=True, dropout=list(range(8)), dropout_prob=p, dtype=torch.float32).cuda()
    dec.train(case == 'train')
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    cc, sc = t(g['color_codes']).requires_grad_(True), t(g['shape_codes']).requires_grad_(True)
    rgb = decode_color_train(dec, cc, sc, t(g['points']), dropout_seed=seed)
    assert rgb.shape == (3, 70, 3)
    loss = (rgb.reshape(-1, 3) - t(g['target'])).abs().mean()
    loss.backward()
    q = cr.g34_quantities(rgb, loss, cc.grad, sc.grad, {k: v.grad for k, v in dec.named_parameters()})
    cr.g34_check(g, case, q, 2e-6, 1e-4, 'GPU')
    # the gates: the saved activations of the same call at the low level
    from distr import decoder_pack
    Wt, bt = decoder_pack.effective_weights_torch_color(dec)
    weights = [w.detach().contiguous() for w in Wt + bt]
    params = functions.train_dropout_params(dec, seed)
    assert (params is None) == (case == 'eval')
    lat = torch.cat([sc, cc], 1).detach().contiguous()
    out, saved = functions.train_forward(weights, lat, t(g['points'].reshape(-1, 3)), [70] * 3, None, net=functions.color_train_net(weights),
                                         dropout=None if params is None else params + (seed, 0))
    assert torch.equal(out, rgb.detach().reshape(-1, 3))
    idx = torch.cat([torch.arange(*saved.rows(s)) for s in range(3)]).cuda()
    for l in range(8):
        on = (saved.activations(l + 1)[idx] > 0).cpu().numpy()
        want = cr.g34_bits(g, case, 'pos', l)
        if case == 'train':
            want = want & cr.g34_bits(g, case, 'keep', l)
        assert not ((on != want) & ~cr.g34_bits(g, case, 'near', l)).any(), (case, l)


def test_refusals(base):
    import torch
    from core.utils.decoder_utils import decode_color_train
    from distr import binding, decoder_pack, functions
    r = base['run']
    cc, sc, pts = r.t(r.cc), r.t(r.sc), r.t(r.pts)
    with pytest.raises(ValueError, match='requires_grad'):
        decode_color_train(r.dec, cc, sc, pts.clone().requires_grad_(True), counts=r.counts)
    with pytest.raises(ValueError, match=r'colour codes \(1, 256\) or \(5, 256\)'):
        decode_color_train(r.dec, cc[:, :255], sc, pts, counts=r.counts)
    with pytest.raises(ValueError, match='shape_codes has shape'):
        decode_color_train(r.dec, cc, sc[:2], pts, counts=r.counts)
    with pytest.raises(ValueError, match='counts sum to'):
        decode_color_train(r.dec, cc, sc, pts[:-1], counts=r.counts)
    drop = Run(256, SIZES, dropout=[0, 5], p=0.2)
    drop.dec.train()
    with pytest.raises(decoder_pack.UnsupportedDecoder, match='training mode with dropout'):
        decode_color_train(drop.dec, cc, sc, pts, counts=r.counts)
    assert decode_color_train(drop.dec, cc, sc, pts, counts=r.counts, dropout_seed=1).shape == (323, 3)
    # the C level, through the low-level call
    net = functions.color_train_net(r.weights)
    lat = torch.cat([sc, cc], 1).contiguous()
    with pytest.raises(binding.DistrError, match='clamp_dist 0.1 with out_dim 3'):
        functions.train_forward(r.weights, lat, pts, r.counts, 0.1, net=net)
    need = functions.train_plan_bytes(r.counts, out_dim=3)
    with pytest.raises(binding.DistrError, match='workspace too small'):
        functions.train_forward(r.weights, lat, pts, r.counts, None, net=net, ws_bytes=need - 1)
    assert functions.train_forward(r.weights, lat, pts, r.counts, None, net=net, ws_bytes=need)[0].shape == (323, 3)
    with pytest.raises(ValueError, match='takes W0..W8, b0..b8 of shapes'):
        functions.train_forward(r.weights, lat, pts, r.counts, None, net=(512, 252, 3))
    with pytest.raises(ValueError, match='segments take'):
        functions.train_forward(r.weights, lat[:2], pts, r.counts, None, net=net)
    ctx = functions._train_context(0)
    cnt = (C.c_int64 * 5)(*r.counts)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    out = torch.empty(323, 3, device='cuda')
    p = binding.ptr
    for L_, n3, nout, stride, word in ((512, 253, 2, 512, 'out_dim'), (512, 510, 3, 512, 'lin3_rows'), (0, 253, 3, 512, 'latent_size'), (512, 253, 3, 511, 'latent_stride')):
        tn = functions._train_net_struct(r.weights, (L_, n3, nout))
        rc = ctx.L.distr_train_net_forward(ctx.h, C.byref(tn), 5, cnt, p(lat), stride, p(pts), -1.0, p(out), p(ws), ws.numel(), ctx.stream(), None)
        assert rc == -1 and word in ctx.L.distr_last_error(ctx.h).decode(), (word, rc, ctx.L.distr_last_error(ctx.h).decode())
    tn = functions._train_net_struct(r.weights, net)
    tn.struct_size -= 8
    assert ctx.L.distr_train_net_forward(ctx.h, C.byref(tn), 5, cnt, p(lat), 512, p(pts), -1.0, p(out), p(ws), ws.numel(), ctx.stream(), None) == -1
    assert 'struct_size' in ctx.L.distr_last_error(ctx.h).decode()
    tn = functions._train_net_struct(r.weights, net)
    tn.W[4] = None
    assert ctx.L.distr_train_net_forward(ctx.h, C.byref(tn), 5, cnt, p(lat), 512, p(pts), -1.0, p(out), p(ws), ws.numel(), ctx.stream(), None) == -1
    assert 'null pointer for lin4' in ctx.L.distr_last_error(ctx.h).decode()
    torch.cuda.synchronize()
