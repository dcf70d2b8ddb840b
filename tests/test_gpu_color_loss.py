"""The fused photometric loss on the GPU (distr_color_loss_forward_batch / _backward_batch, functions.ColorLossFunction,
loss_utils.compute_loss_color_batch) against the float64 restatement tests/color_loss_restatement.py.

The bar is not chosen here: sigma = E[x^2] - mu^2 cancels against C2 = 9e-4, so what an f32 evaluation of this formula can reach is read
off the reference's own f32 evaluation -- golden G35 holds the reference's loss_ssim and its gradient on three raw image pairs; their
distance from the restatement, measured on the CPU in the fixture `bars`, times two, is the bar for values (absolute) and for gradients
(of the gradient's largest entry). Shapes: 1 x 1, 1 x 5, 3 x 3, 16 x 16 (exactly one block of 256 pixels), 1 x 257 (two blocks, the second
with one pixel), 17 x 19 (two blocks, windows across the block edge), with full masks and with masks that touch every border."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

import color_loss_restatement as clr
import color_render_train_restatement as crt

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 5), (3, 3), (16, 16), (1, 257), (17, 19)]


@pytest.fixture(scope='module')
def bars():
    """(value bar, gradient bar) = 2 x the largest distance of the reference's f32 records from the float64 restatement"""
    g = np.load(os.path.join(GOLDEN, 'g35_color_render_weight_grad.npz'))
    dv = dg = 0.0
    for i in range(len(crt.SSIM_PAIRS)):
        loss, grad, _ = clr.ssim_loss(g['ssim%d_x' % i], g['ssim%d_y' % i])
        dv = max(dv, abs(float(g['ssim%d_loss' % i]) - loss))
        dg = max(dg, float(np.abs(g['ssim%d_g' % i] - grad).max() / np.abs(grad).max()))
    print('bars from the reference\'s f32 records: value %.3e, gradient %.3e of its largest entry' % (2 * dv, 2 * dg))
    assert 0 < dv < 1e-6 and 0 < dg < 1e-4
    return 2 * dv, 2 * dg


def _t(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _case(h, w, masked, seed):
    rs = np.random.RandomState(seed)
    rgb, gt = rs.rand(h, w, 3).astype(np.float32), rs.rand(h, w, 3).astype(np.float32)
    if not masked:
        return rgb, np.ones((h, w), np.uint8), gt, np.ones((h, w), np.uint8)
    m, gm = (rs.rand(h, w) < 0.75).astype(np.uint8), (rs.rand(h, w) < 0.75).astype(np.uint8)
    for a in (m, gm):                       # the overlap touches every border (and is not empty)
        a[0, :], a[-1, :], a[:, 0], a[:, -1] = 1, 1, 1, 1
    if h * w > 9:
        m[h // 2, w // 2], gm[h // 2, (w // 2 + 1) % w] = 0, 0
    return rgb, m, gt, gm


def run(views, want_ssim=True):
    """views: [(rgb, mask, gt, gt_mask)] of one size -> (l1, ssim, overlap, g of sum(l1) w.r.t. rgb, g of sum(ssim)), numpy"""
    import torch
    from core.utils.loss_utils import compute_loss_color_batch
    rgb = _t(np.stack([v[0] for v in views])).requires_grad_(True)
    m, gt, gm = _t(np.stack([v[1] for v in views]), np.uint8), _t(np.stack([v[2] for v in views])), _t(np.stack([v[3] for v in views]), np.uint8)
    l1, ssim, ov = compute_loss_color_batch(rgb, m, gt, gm, use_ssim=want_ssim)
    g1, = torch.autograd.grad(l1.sum(), rgb, retain_graph=want_ssim)
    g2 = torch.autograd.grad(ssim.sum(), rgb)[0].cpu().numpy() if want_ssim else None
    torch.cuda.synchronize()
    return l1.detach().cpu().numpy(), None if ssim is None else ssim.detach().cpu().numpy(), ov.cpu().numpy(), g1.cpu().numpy(), g2


def check(tag, view, got, v, bars, grad_scale=None):
    """view v of `got` against the restatement of `view`; returns the residuals (l1, ssim, g_l1, g_ssim)"""
    ref = clr.color_loss(*view)
    l1, ssim, ov, g1, g2 = got
    assert int(ov[v]) == ref['overlap'], tag
    top1 = max(np.abs(ref['g_l1']).max(), 1e-300)
    top2 = np.abs(ref['g_ssim']).max() if grad_scale is None else grad_scale
    # (the value bar was measured on losses below 1: for an l1 above 1 -- the clamp-edge pair's pixels reach 12 -- it is taken relative)
    res = (abs(float(l1[v]) - ref['l1']) / max(1.0, ref['l1']), abs(float(ssim[v]) - ref['ssim']), float(np.abs(g1[v] - ref['g_l1']).max() / top1),
           float(np.abs(g2[v] - ref['g_ssim']).max() / top2))
    print('%s: l1 %.2e ssim %.2e (bar %.2e); g_l1 %.2e g_ssim %.2e (bar %.2e)' % ((tag,) + res[:2] + (bars[0],) + res[2:] + (bars[1],)))
    assert res[0] <= bars[0] and res[1] <= bars[0] and res[2] <= bars[1] and res[3] <= bars[1], (tag, res, bars)
    off = ~((view[1] != 0) & (view[3] != 0))
    assert not g1[v][off].any() and not g2[v][off].any(), 'gradient off the overlap'
    return res


@pytest.mark.parametrize('masked', [False, True], ids=['full', 'masked'])
@pytest.mark.parametrize('hw', SHAPES, ids=['%dx%d' % s for s in SHAPES])
def test_values_and_gradients_against_float64(bars, hw, masked):
    view = _case(hw[0], hw[1], masked, 100 * hw[0] + hw[1])
    got = run([view])
    check('%d x %d %s' % (hw + ('masked' if masked else 'full',)), view, got, 0, bars)
    again = run([view])
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()
    # without the SSIM term: the same L1 bytes, nothing else
    l1, ssim, ov, g1, g2 = run([view], want_ssim=False)
    assert ssim is None and g2 is None and l1.tobytes() == got[0].tobytes() and g1.tobytes() == got[3].tobytes() and ov.tobytes() == got[2].tobytes()


def test_batch_with_an_empty_overlap(bars):
    """B = 3, the middle view's masks do not overlap: l1 = 0 with a zero gradient there (the one divergence from the reference, which
    yields NaN), overlap = 0 shows it, its SSIM term is that of two zero images; every view is byte for byte its B = 1 call."""
    h, w = 17, 19
    views = [_case(h, w, True, 7), None, _case(h, w, False, 9)]
    e = _case(h, w, False, 8)
    board = (np.arange(h * w).reshape(h, w) % 2).astype(np.uint8)
    views[1] = (e[0], board, e[2], 1 - board)
    got = run(views)
    assert list(got[2]) == [int(((v[1] != 0) & (v[3] != 0)).sum()) for v in views] and got[2][1] == 0
    assert got[0][1] == 0.0 and not got[3][1].any() and not got[4][1].any() and np.isfinite(got[1]).all()
    for v in range(3):
        check('batch view %d' % v, views[v], got, v, bars) if v != 1 else None
        alone = run([views[v]])
        for a, b in zip(got, alone):
            assert a[v:v + 1].tobytes() == b.tobytes(), v
    ref = clr.color_loss(*views[1])
    assert abs(float(got[1][1]) - ref['ssim']) <= bars[0]
    again = run(views)
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()


def test_clamp_edge(bars):
    """The pair of tests/test_color_render_train_host.py whose ssim is within 1e-4 of -1 in every interior window: (1 - ssim) / 2 sits
    at the clamp's upper edge, where rounding decides on which side an f32 evaluation lands (inside: the gradient passes; outside: it is
    zero). The value is held to the value bar. The gradient there is what is left of three terms that cancel (2e-7 from 1e-3), so the
    relative bar applies to the size of those terms (color_loss_restatement.ssim_grad_terms), not to their cancelled sum: an entry may
    also be zero where the clamp cut it, which is inside the same bound since the entry itself is smaller than the bar times the terms."""
    from test_color_render_train_host import clamp_pair
    x, y = clamp_pair()
    full = np.ones(x.shape[1:], np.uint8)
    view = (y.transpose(1, 2, 0).astype(np.float32), full, x.transpose(1, 2, 0).astype(np.float32), full)
    terms = clr.ssim_grad_terms(view[2].transpose(2, 0, 1), view[0].transpose(2, 0, 1))
    got = run([view])
    print('clamp edge: largest gradient entry %.3e, largest term %.3e' % (np.abs(clr.color_loss(*view)['g_ssim']).max(), terms.max()))
    check('clamp edge', view, got, 0, bars, grad_scale=terms.max())


def test_compute_loss_color_returns_three_values():
    """compute_loss_color(use_ssim=True) of one view: (l1, ssim, visualizer), with or without the reference's package."""
    import torch
    from core.utils.loss_utils import compute_loss_color
    rgb, m, gt, gm = _case(17, 19, True, 11)
    t = _t(rgb).requires_grad_(True)
    out = compute_loss_color(t, _t(m, np.uint8).bool(), _t(gt), _t(gm, np.uint8).bool(), use_ssim=True)
    assert len(out) == 3 and out[2] is None
    ref = clr.color_loss(rgb, m, gt, gm)
    assert abs(out[0].item() - ref['l1']) <= 1e-6 and abs(out[1].item() - ref['ssim']) <= 1e-6
    (out[0] + out[1]).backward()
    want = ref['g_l1'] + ref['g_ssim']
    assert np.abs(t.grad.cpu().numpy() - want).max() <= 1e-4 * np.abs(want).max()
    assert len(compute_loss_color(_t(rgb), _t(m, np.uint8).bool(), _t(gt), _t(gm, np.uint8).bool())) == 2


def test_refusals():
    import torch
    from core.utils.loss_utils import compute_loss_color_batch
    rgb, m, gt, gm = (_t(a, d)[None] for a, d in zip(_case(3, 3, False, 1), (np.float32, np.uint8, np.float32, np.uint8)))
    with pytest.raises(ValueError, match='color_gt requires grad'):
        compute_loss_color_batch(rgb, m, gt.clone().requires_grad_(True), gm)
    with pytest.raises(ValueError, match=r'expected \(B, H, W, 3\)'):
        compute_loss_color_batch(rgb[0], m, gt, gm)
    with pytest.raises(ValueError, match='expected color_gt'):
        compute_loss_color_batch(rgb, m[:, :2], gt, gm)
    with pytest.raises(RuntimeError, match='must be on the GPU'):
        compute_loss_color_batch(rgb.cpu(), m.cpu(), gt.cpu(), gm.cpu())
