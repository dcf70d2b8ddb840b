"""The CPU models of the split arithmetics (tests/split_restatement.py) and the oracle's sample accessor: what the GPU tests of
tests/test_gpu_split_arith.py stand on, checked without a GPU.

Recorded results (this file's points: 2 048 in [-0.8, 0.8]^3, seed 7, fixture F1, its own code; max |sdf - sdf64|, and in brackets
the ratio to the f32 chain's 2.77e-7 / its 99th percentile 1.84e-7):
    bf16x6   2.18e-7 (0.79 / 0.84)        f16x3   2.67e-7 (0.96 / 1.08)
    one product left out, ratio of the maxima:
      bf16x6  w0a0 4.6e6   w1a0 5 207   w0a1 7 910   w1a1 11.6   w2a0 6.8   w0a2 10.4
      f16x3   w0a0 4.6e6   w1a0 491     w0a1 798
    f16x3 on the rescaled decoders (the f32 chain and bf16x6 stay at 2.77e-7 / 2.18e-7 on every member), ratio of the maxima:
      k            0      4      6      7      8      9      10
      pair lin1   0.96   0.92   1.24   1.93   2.92   5.17   10.99
      pair lin3   0.96   1.24   1.07   1.40   1.91   3.61    7.33
      pair lin5   0.96   1.24   1.25   1.56   2.26   4.51    9.06
      chain       0.96   1.00   1.56   2.75   4.78   9.15   19.83
    so the model puts the edge of the accepted range between k = 6 and k = 7, and the bar of the GPU tests (2 x the f32 error)
    between a correct tile (<= 1.1) and the mildest lost product (6.8).
"""
import numpy as np
import pytest
import torch

import split_restatement as sr
import train_restatement as tr

BAR = 2.0            # bar (a) of tests/test_gpu_split_arith.py: a split mode's error may be at most 2 x the f32 error
RECORDED = {'bf16x6': (0.79, 0.84), 'f16x3': (0.96, 1.08)}      # (max, p99) ratios to the f32 chain, see above


@pytest.fixture(scope='module')
def f1(fixture_decoder):
    Ws, bs, latent = fixture_decoder
    pts = (np.random.RandomState(7).rand(2048, 3) * 1.6 - 0.8).astype(np.float32)
    return dict(Ws=Ws, bs=bs, latent=latent, pts=pts, ref=sdf64(Ws, bs, latent, pts))


def sdf64(Ws, bs, latent, pts):
    with torch.no_grad():
        return tr.forward(tr.to64(Ws), tr.to64(bs), tr.to64([latent])[0], tr.to64([pts])[0], [len(pts)])[0].reshape(-1)


@pytest.fixture(scope='module')
def f32_err(f1):
    return sr.errors(sr.forward(f1['Ws'], f1['bs'], f1['latent'], f1['pts'], 'f32')[0], f1['ref'])


@pytest.mark.parametrize('k', [0, 4, 8, 10])
def test_rescales_keep_the_float64_function_exactly(f1, k):
    members = [sr.rescale_chain(f1['Ws'], f1['bs'], k)] + [sr.rescale_pair(f1['Ws'], f1['bs'], k, l) for l in (1, 3, 5)]
    for Ws, bs in members:
        assert torch.equal(sdf64(Ws, bs, f1['latent'], f1['pts']), f1['ref'])
        assert k == 0 or any(not np.array_equal(a, b) for a, b in zip(Ws, f1['Ws']))
        assert sr.h3_weights_in_range(Ws)                    # k = 10: largest weight 332, inside split_f16x2's range


@pytest.mark.parametrize('mode', ['bf16x6', 'f16x3'])
def test_models_sit_at_the_f32_chains_error(f1, f32_err, mode):
    y, over = sr.forward(f1['Ws'], f1['bs'], f1['latent'], f1['pts'], mode)
    e = sr.errors(y, f1['ref'])
    ratios = (e[0] / f32_err[0], e[1] / f32_err[1])
    print('%s: max %.3e p99 %.3e, f32 chain %.3e / %.3e, ratios %.2f / %.2f' % ((mode,) + e + f32_err + ratios))
    assert not over.any()
    assert 2.0e-7 < f32_err[0] < 4.0e-7
    # the recorded ratios, with room for another summation order of the host's matmul (the planes themselves are exact)
    for got, rec in zip(ratios, RECORDED[mode]):
        assert rec / 1.3 <= got <= rec * 1.3, (mode, ratios)
    assert max(ratios) <= BAR


@pytest.mark.parametrize('mode,drop', [(m, d) for m in ('bf16x6', 'f16x3') for d in sr.PRODUCTS[m]])
def test_a_lost_product_exceeds_the_bar(f1, f32_err, mode, drop):
    """Bar (a) separates a correct tile from one that lost any single product: shown once, here."""
    e = sr.errors(sr.forward(f1['Ws'], f1['bs'], f1['latent'], f1['pts'], mode, drop=drop)[0], f1['ref'])
    print('%s without w%da%d: max %.3e (x %.1f), p99 %.3e (x %.1f)' % (mode, drop[0], drop[1], e[0], e[0] / f32_err[0], e[1], e[1] / f32_err[1]))
    assert e[0] > BAR * f32_err[0] and e[1] > BAR * f32_err[1]


def test_model_predicts_the_silent_loss_of_f16x3(f1, f32_err):
    """Inside the range split_f16x2 accepts, small activations cost accuracy with nothing reported (the second f16 plane
    falls into the denormals); bf16x6 has f32's exponent range and does not care."""
    for name, Ws, bs in [('chain k=10',) + sr.rescale_chain(f1['Ws'], f1['bs'], 10), ('pair lin1 k=10',) + sr.rescale_pair(f1['Ws'], f1['bs'], 10, 1)]:
        a = sr.errors(sr.forward(Ws, bs, f1['latent'], f1['pts'], 'f32')[0], f1['ref'])
        y, over = sr.forward(Ws, bs, f1['latent'], f1['pts'], 'f16x3')
        h = sr.errors(y, f1['ref'])
        b = sr.errors(sr.forward(Ws, bs, f1['latent'], f1['pts'], 'bf16x6')[0], f1['ref'])
        print('%s: f32 %.2e, f16x3 %.2e, bf16x6 %.2e' % (name, a[0], h[0], b[0]))
        assert not over.any() and sr.h3_weights_in_range(Ws)
        assert a[0] <= 1.5 * f32_err[0] and b[0] <= BAR * a[0]
        assert h[0] > 5 * a[0]


def test_acceptance_rule_refuses_what_the_model_loses(f1, f32_err):
    """The rule distr_set_decoder applies to f16x3 (every layer's largest |weight| in [2^-8, 1023.5), mirrored by
    split_restatement.h3_refused_layer): every family member on which the model misses bar (a) is refused, with the layer that
    was scaled down; both fixtures are accepted, a weight of 1023 is, one of 1024 is not."""
    from distr import fixture
    assert sr.h3_refused_layer(f1['Ws']) is None and sr.h3_refused_layer(fixture.load_fixture_f2()[0]) is None
    for name, Ws, bs in sr.family(f1['Ws'], f1['bs']):
        refused = sr.h3_refused_layer(Ws)
        if refused is None:
            e = sr.errors(sr.forward(Ws, bs, f1['latent'], f1['pts'], 'f16x3')[0], f1['ref'])
            assert e[0] <= BAR * f32_err[0] and e[1] <= BAR * f32_err[1], (name, e, f32_err)
        else:
            assert ('pair lin%d' % refused in name or (name.startswith('chain') and refused == 1)) and not name.endswith(('k=0', 'k=4', 'k=6')), name
    for value, want in ((1023.0, None), (1024.0, 2)):
        W1 = [w.copy() for w in f1['Ws']]
        W1[2][5, 7] = value
        assert sr.h3_refused_layer(W1) == want


def test_f16x3_model_marks_overflow_at_the_f16_range():
    """FmtH3's store4 flags a ray when the leading f16 plane of 64 x is inf: round to nearest turns into inf from 65520 on, half a unit
    in the last place above the largest finite f16, 65504; values in [65504, 65520) round to 65504, keep a finite second plane and
    stay exact to 2^-22, so nothing is lost where they are not flagged. Below 65504 nothing may be flagged, from 65520 on everything."""
    v = torch.tensor([0.0, 1.0, 65503.0, 65503.996, 65504.0, 65519.996, 65520.0, 65536.0, 1e6, float('inf'), float('nan')])
    flag = sr.f16_overflowed(v)
    assert flag.tolist() == [False] * 6 + [True] * 5
    assert not flag[v < sr.F16_MAX].any() and flag[v >= 65520.0].all()
    p = sr.planes(v[:6], 2, torch.float16)
    assert p[0].tolist() == [0.0, 1.0, 65504.0, 65504.0, 65504.0, 65504.0]
    assert float((p[0] + p[1] - v[:6]).abs().max()) <= 65504.0 * 2.0 ** -22                           # two planes: 22 bits
    # through the decoder: one unit of lin0 pushed to the edge of the range (the later layers stay far inside it) -- the flag is
    # raised for exactly the points whose 64 x0 reaches 65520
    from distr import fixture
    Ws, bs, latent = fixture.make_decoder_weights()
    pts = (np.random.RandomState(1).rand(256, 3) * 1.2 - 0.6).astype(np.float32)
    b2 = [b.copy() for b in bs]
    b2[0][7] += np.float32(1023.75)        # 65520 / 64
    y, over = sr.forward(Ws, b2, latent, pts, 'f16x3')
    c0, _ = sr.latent_consts([torch.from_numpy(w) for w in Ws], [torch.from_numpy(b) for b in b2], torch.from_numpy(latent))
    x0 = torch.relu(torch.from_numpy(pts) @ torch.from_numpy(Ws[0][:, -3:]).t() + c0) * 64
    want = (x0 >= 65520.0).any(1)
    assert 32 <= int(want.sum()) <= 224
    assert torch.equal(over, want) and torch.equal(torch.isnan(y), want)


def test_oracle_sample_list_explains_its_latent_gradient(fixture_decoder, cpu_oracle, orc):
    """RenderState.samples returns the list orc_render_backward differentiates: the oracle's own g_latent is the float64 sum over
    it of coef (1 - y^2) d pre / d code, on the oracle's own ReLU pattern at each point."""
    from distr import fixture
    Ws, bs, latent = fixture_decoder
    H = W = 24
    K = fixture.make_intrinsic(H, W)
    R, T = fixture.make_camera(20, 10, 1.6, 0)
    for kw in (dict(marcher='recursive', march_step=30, buffer_size=2, want_normal=False),
               dict(marcher='pyramid_recursive', march_step=6, buffer_size=5, want_normal=False, threshold=1e-3)):
        out = cpu_oracle.render(orc.make_cfg(H, W, K, **kw), latent, R, T)
        rs = np.random.RandomState(3)
        gz, gq = rs.randn(H * W).astype(np.float32), rs.randn(H * W).astype(np.float32)
        g_lat, _, _, ns = out['state'].backward(g_zdepth=gz, g_min_sdf=gq)
        pix, pts, coef = out['state'].samples(g_zdepth=gz, g_min_sdf=gq)
        assert len(pix) == ns and ns > H * W // 2
        pad = pix < 0
        assert pad.sum() <= 1 and not pad[:-1].any() and not pts[pad].any()
        assert ((pix[~pad] >= 0) & (pix[~pad] < H * W)).all()
        gates = [torch.from_numpy(cpu_oracle.layer_activations(latent, pts, l)[:, :Ws[l].shape[0]] > 0) for l in range(8)]
        ref = tr.gradients(Ws, bs, latent, pts, [len(pts)], coef, gates=gates)[4].numpy()
        res = np.abs(g_lat.astype(np.float64) - ref).max() / np.abs(ref).max()
        print('%s: %d samples (%d pad), g_latent against the float64 sum over them: %.2e of the largest entry' % (kw['marcher'], ns, int(pad.sum()), res))
        assert res <= 1e-4
        # one pixel's min-sdf gradient alone: exactly one sample, at that pixel, with that weight
        one = np.zeros(H * W, np.float32)
        one[(H // 2) * W + W // 2] = -0.75
        pix1, _, coef1 = out['state'].samples(g_min_sdf=one)
        assert pix1.tolist() in ([(H // 2) * W + W // 2], [-1]) and coef1.tolist() == [-0.75]
