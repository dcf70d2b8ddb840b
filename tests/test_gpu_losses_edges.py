"""The fused losses at their edges (csrc/distr_losses.hpp: block_sum, k_single_loss_partial / _final / _bwd, k_warp_fwd / _final / _bwd,
k_sum_partials) against the float64 restatement of tests/losses_restatement.py, on synthetic inputs (tests/losses_edges_inputs.py).
tests/test_losses_edges_host.py asserts on the CPU what every case here assumes of its inputs.

Every bar is k 2^-24 A: A from the restatement (float64, never from the library), k counted from the kernels (the table is the
restatement's docstring): losses 1 | 1 | 1 | 15 + 10 + nblk; g_min_sdf, g_depth 1; g_normal 30; warp loss 74 + nblk; c2 60;
g_z1 1; camera entries 10 + nblk. Counts, kept sets and colour1 are exact; entries outside a set are exactly zero.

f3  sizes P = 1, 63, 64, 65, 255, 256, 257, 513, 16 641, each as 1 x P and ragged; with and without gt_depth / gt_normal; per set a
    one-member case at pixels 0, 63, 64, 255, 256, P - 1, a full and an empty case; the special values on wave and block boundaries;
    poison where nothing may be read; run-to-run bytes; 17 038 590 members (the count as an integer sum).
f2  (a) border scene, (b) one-hot masks, (c) sizes, (d) threshold straddlers and exact colour ties, (e) ambiguous pixels are cleared
    from mask1 on both sides and the run repeated, at most 3 % of the valid pixels, (f) no valid pixel, nothing kept.

Residuals of the library on the MI355X are recorded in profiles/losses_edges.md; every test prints its own.
"""
import numpy as np
import pytest

import losses_edges_inputs as inp
import losses_restatement as lr

pytestmark = pytest.mark.gpu
U = lr.U


def _t(a, grad=False):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().requires_grad_(grad)


def _np(t):
    return t.detach().cpu().numpy()


# ============================================================================================ f3
def _f3_raw(engine, g, H, W):
    """distr_single_loss_forward through the binding -> out8 = losses[4], counts[4]. Arrays that are None go in as null."""
    import torch
    from distr import binding, functions
    dev = [None if g.get(k) is None else _t(g[k]) for k in ('depth', 'normal', 'mask', 'min_sdf', 'gt_depth', 'gt_normal', 'gt_mask')]
    out8 = torch.full((8,), -7.0, dtype=torch.float32, device='cuda')
    ws = functions._loss_ws(engine, H, W)
    p = binding.ptr
    engine.ctx.check(engine.ctx.L.distr_single_loss_forward(engine.ctx.h, H, W, *[p(t) for t in dev], float(g['threshold']), p(out8), p(ws), ws.numel(),
                                                           engine.ctx.stream()))
    return _np(out8)


def _f3_run(engine, g, hw):
    """-> (out8, g_depth (P), g_normal (P, 3), g_min_sdf (P)) of one forward through the binding and one forward + backward through autograd."""
    from distr import functions
    H, W = hw
    out8 = _f3_raw(engine, g, H, W)
    c = lambda k, s: None if g.get(k) is None else _t(np.asarray(g[k]).reshape(s))
    d, n, q = _t(g['depth'].reshape(H, W), True), _t(g['normal'].reshape(H, W, 3), True), _t(g['min_sdf'].reshape(H, W), True)
    terms = functions.single_view_losses(engine, d, n, c('mask', (H, W)), q, c('gt_depth', (H, W)), c('gt_normal', (H, W, 3)), c('gt_mask', (H, W)),
                                         float(g['threshold']))
    assert _np(terms).tobytes() == out8[:4].tobytes()
    (terms * _t(np.asarray(g['weights'], np.float32))).sum().backward()
    return out8, _np(d.grad).reshape(-1), _np(n.grad).reshape(-1, 3), _np(q.grad).reshape(-1)


def _f3_check(tag, engine, g, hw):
    P = hw[0] * hw[1]
    r = lr.single(g['depth'], g['normal'], g['mask'], g['min_sdf'], g['gt_depth'], g['gt_normal'], g['gt_mask'], g['threshold'], g['weights'])
    got = _f3_run(engine, g, hw)
    out8 = got[0]
    assert out8[4:].tolist() == [float(c) for c in r['counts']], (tag, out8[4:], r['counts'])
    res = []
    for k in range(4):
        bar = lr.k_single_loss(k, P) * U * r['loss_A'][k]
        res.append(lr.ratio(abs(float(out8[k]) - r['losses'][k]), bar))
    grads = [lr.ratio(np.abs(a - r['g_' + name]), lr.K_GRAD[name] * U * r['A_' + name])
             for name, a in (('depth', got[1]), ('normal', got[2]), ('min_sdf', got[3]))]
    print('%s %dx%d counts %s: losses %s bars; g_depth %.3f g_normal %.3f g_min_sdf %.3f bars' % (
        tag, hw[0], hw[1], r['counts'].tolist(), ' '.join('%.3f' % v for v in res), grads[0], grads[1], grads[2]))
    assert max(res) <= 1.0 and max(grads) <= 1.0, (tag, res, grads)
    return r, got


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize('P', inp.F3_SIZES)
def test_single_view_random_forms_and_shapes(P, engine):
    """Random masks, the four forms (with / without gt_depth, gt_normal), both shapes of the size; run-to-run bytes."""
    for hw in inp.f3_shapes(P):
        for form in inp.F3_FORMS:
            g = inp.f3_random(P, *form)
            _, got = _f3_check('random %s' % (form,), engine, g, hw)
            assert _same(got, _f3_run(engine, g, hw)), 'not reproducible'
            if not form[0]:
                assert got[0][2] == 0 and got[0][6] == 0 and not got[1].any()
            if not form[1]:
                assert got[0][3] == 0 and got[0][7] == 0 and not got[2].any()


@pytest.mark.parametrize('P', inp.F3_SIZES)
def test_single_view_one_member(P, engine):
    """One member of one set, at pixel 0, 63, 64, 255, 256 or P - 1: the loss is that pixel's value, the count 1, the gradient zero elsewhere."""
    hw = inp.f3_shapes(P)[-1]
    for term in range(4):
        for pos in inp.positions(P):
            g = inp.f3_one_member(P, term, pos)
            r, got = _f3_check('one member of %s at %d' % (inp.SET_NAMES[term], pos), engine, g, hw)
            assert r['counts'].tolist() == [int(k == term) for k in range(4)] and r['value'][term][pos] != 0
            assert got[0][term] != 0 and [got[0][k] for k in range(4) if k != term] == [0, 0, 0]
            image = (got[3], got[3], got[1], got[2])[term]
            assert np.abs(image[pos]).max() > 0 and not np.delete(image, pos, 0).any()
            for other in {1, 2, 3} - {(3, 3, 1, 2)[term]}:
                assert not got[other].any()


@pytest.mark.parametrize('P', inp.F3_SIZES)
def test_single_view_full_and_empty(P, engine):
    hw = inp.f3_shapes(P)[-1]
    both, apart = inp.f3_full(P)
    r, _ = _f3_check('full depth and normal', engine, both, hw)
    assert r['counts'].tolist() == [0, 0, P, P]
    r, _ = _f3_check('full hinges', engine, apart, hw)
    assert r['counts'].tolist() == [max(1, P // 2), P - max(1, P // 2), 0, 0]
    r, got = _f3_check('empty', engine, inp.f3_empty(P), hw)
    assert not r['counts'].any() and got[0].tobytes() == np.zeros(8, np.float32).tobytes() and not any(a.any() for a in got[1:])


def test_single_view_special_values(engine):
    g, where = inp.f3_specials()
    hw = (1, inp.SPECIAL_P)
    r, got = _f3_check('specials', engine, g, hw)
    for (p, _), want in zip(inp.GT_DEPTH_SPECIALS, inp.GT_DEPTH_IN):
        assert bool(r['member'][2][p]) == want and (got[1][p] != 0) == want, p
    for p in where['equal_depth']:
        assert r['member'][2][p] and got[1][p] == 0
    for p in where['zero_normal']:
        assert not r['member'][3][p] and not got[2][p].any()
    for p in where['zero_gt_normal']:
        assert r['member'][3][p] and not got[2][p].any()
    g, ties = inp.f3_hinge_ties()
    r, got = _f3_check('hinge ties', engine, g, hw)
    for p, s in ties.items():
        on = (s > 0) if r['member'][0][p] else (s < 0)
        assert r['member'][0][p] != r['member'][1][p] and (got[3][p] != 0) == on, (p, s, got[3][p])


@pytest.mark.parametrize('P', (257, 513))
def test_single_view_poison(P, engine):
    """NaN and inf wherever depth, normal and min_sdf must not be read change no output byte."""
    hw = inp.f3_shapes(P)[-1]
    g = inp.f3_random(P, key='poison')
    bad, spots = inp.f3_poison(g)
    clean, dirty = _f3_run(engine, g, hw), _f3_run(engine, bad, hw)
    sel = {1: spots['depth'], 2: spots['normal'], 3: spots['min_sdf']}
    assert all(s.sum() >= P // 4 for s in sel.values())
    assert clean[0].tobytes() == dirty[0].tobytes()
    for k in (1, 2, 3):
        assert clean[k].tobytes() == dirty[k].tobytes(), k


def test_single_view_count_above_2_24(engine):
    """255 members in each of 66 818 blocks, 17 038 590 in all: the per-block counts are added as integers and converted once."""
    g = inp.f3_big()
    out8 = _f3_raw(engine, dict(g, depth=None, normal=None, gt_depth=None, gt_normal=None), 256, inp.BIG_BLOCKS)
    assert out8[4:].tolist() == [0.0, float(g['members']), 0.0, 0.0], out8
    t = float(np.float32(g['threshold']))
    bar = lr.k_single_loss(1, g['P']) * U * t
    print('17 038 590 members: mean hinge %.9g against %.9g, %.4f bars' % (out8[1], t, abs(float(out8[1]) - t) / bar))
    assert abs(float(out8[1]) - t) <= bar and out8[0] == 0 and out8[2] == 0 and out8[3] == 0


# ============================================================================================ f2
def _warp_run(engine, g):
    import torch
    from distr import binding, functions
    H, W = int(g['H']), int(g['W'])
    c = lambda k: _t(np.asarray(g[k], np.float32))
    z1, R1, T1, R2, T2 = (_t(np.asarray(g[k], np.float32), True) for k in ('zdepth1', 'R1', 'T1', 'R2', 'T2'))
    wcfg = binding.make_warp_cfg((H, W), g['K'], float(g['thres_depth']))
    K, Ki = inp.cfg_matrices(g)
    assert np.array(wcfg.K[:], np.float32).tobytes() == K.tobytes() and np.array(wcfg.K_inv[:], np.float32).tobytes() == Ki.tobytes()
    loss, keep, c1, c2 = functions.warp_loss(engine, wcfg, z1, _t(g['mask1']), c('zdepth2'), c('img1'), c('img2'), R1, T1, R2, T2)
    (loss * float(g.get('g_loss', 1.0))).backward()
    cam = np.concatenate([_np(t.grad).reshape(-1) for t in (R1, T1, R2, T2)])
    return dict(loss=_np(loss).reshape(1), keep=_np(keep), c1=_np(c1).reshape(-1, 3), c2=_np(c2).reshape(-1, 3), g_z=_np(z1.grad).reshape(-1), cam=cam)


def _warp_check(tag, engine, g, want_kept=1):
    """(e) first: the ambiguous pixels leave mask1; then everything is compared. Returns (restatement, outputs)."""
    g, r, share = inp.clear_ambiguous(g)
    assert share <= inp.AMBIGUOUS_CAP, (tag, share)
    P = int(g['H']) * int(g['W'])
    got = _warp_run(engine, g)
    assert got['keep'].dtype == np.uint8 and set(np.unique(got['keep'])) <= {0, 1}
    flips = int((got['keep'].astype(bool) != r['keep']).sum())
    assert flips == 0 and r['n_kept'] >= want_kept, (tag, flips, r['n_kept'])
    loss = float(got['loss'][0])
    if r['n_valid'] and not r['n_kept']:
        assert np.isnan(loss), (tag, loss)
        res_loss = 0.0
    else:
        res_loss = lr.ratio(abs(loss - float(r['loss'])), lr.k_warp_loss(P) * U * r['loss_A'])
    want_c1 = np.where(r['keep'][:, None], np.asarray(g['img1'], np.float32).reshape(-1, 3), np.float32(0))
    assert got['c1'].tobytes() == want_c1.tobytes(), tag
    res_c2 = lr.ratio(np.abs(got['c2'] - r['c2']), lr.K_COORD * U * np.where(r['keep'][:, None], r['c2_A'], 0.0))
    res_z = lr.ratio(np.abs(got['g_z'] - r['g_z']), U * r['A_z'])
    k = lr.k_warp_cam(P)
    res_cam = np.abs(got['cam'] - r['cam']) / np.maximum(k * U * r['cam_A'], 1e-300)
    res_cam = np.where((r['cam_A'] == 0) & (got['cam'] == 0), 0.0, res_cam)
    print('%s %dx%d valid %d kept %d cleared %.2f%%: loss %.3f c2 %.3f g_z1 %.3f bars; camera (k %d) R1 %.3f T1 %.3f R2 %.3f T2 %.3f bars' % (
        tag, g['H'], g['W'], r['n_valid'], r['n_kept'], 100 * share, res_loss, res_c2, res_z, k, res_cam[:9].max(), res_cam[9:12].max(),
        res_cam[12:21].max(), res_cam[21:].max()))
    assert res_loss <= 1.0 and res_c2 <= 1.0 and res_z <= 1.0 and res_cam.max() <= 1.0, (tag, res_loss, res_c2, res_z, res_cam.tolist())
    assert np.isfinite(got['g_z']).all() and np.isfinite(got['cam']).all()
    return r, got, g


def test_warp_border_scene(engine):
    """(a) view 1 reaches past view 2 on every side: the zero-padded corners of the colour sample and of its gradient."""
    g = dict(inp.warp_scene('border'), g_loss=0.37)
    r, got, g = _warp_check('border', engine, g, want_kept=2000)
    b = inp.border_pixels(r, g['H'], g['W'])
    assert all(len(b[k]) >= 8 for k in ('left', 'right', 'top', 'bottom', 'outside')) and len(b['corner']) >= 1
    out = b['outside']
    assert got['keep'][out].all() and not got['c2'][out].any() and not got['g_z'][out].any()
    for k in ('left', 'right', 'top', 'bottom', 'corner'):
        assert np.abs(got['g_z'][b[k]]).min() > 0, k
    again = _warp_run(engine, g)
    assert all(got[k].tobytes() == again[k].tobytes() for k in got), 'not reproducible'


@pytest.mark.parametrize('case', inp.one_hot_pixels(), ids=lambda c: '%s-%d' % c)
def test_warp_one_hot(case, engine):
    """(b) mask1 holds ONE pixel: every camera entry is that pixel's term alone, where float32 cancellation would show."""
    kind, pix = case
    g = inp.one_hot(inp.warp_scene(kind), pix)
    r, got, _ = _warp_check('one-hot %s %d' % case, engine, g)
    assert r['n_valid'] == 1 and r['keep'][pix] and np.count_nonzero(r['cam']) == 24 and np.count_nonzero(got['cam']) == 24 and got['g_z'][pix] != 0
    assert not np.delete(got['g_z'], pix).any() and not np.delete(got['c2'], pix, 0).any()


@pytest.mark.parametrize('hw', inp.WARP_SIZES, ids=lambda s: '%dx%d' % s)
def test_warp_sizes(hw, engine):
    """(c) one-pixel-wide images (grid_sample's round trip maps the thin axis to 0: no gradient along it), P = 255, 256, 257, and 65 blocks:
    the third round of eight sums and the last block's partial."""
    g = inp.warp_scene('inner', hw)
    r, got, g = _warp_check('size', engine, g, want_kept=hw[0] * hw[1] // 2)
    last = np.arange(256 * (lr.nblk(hw[0] * hw[1]) - 1), hw[0] * hw[1])
    assert np.abs(r['terms'][last][:, 16:]).max() > 0
    assert np.count_nonzero(got['cam']) == np.count_nonzero(r['cam']) == (20 if min(hw) == 1 else 24)


def test_warp_threshold_straddlers(engine):
    """(d) err^2 three and eight bounds either side of the threshold: the kept set is float64's, with no allowance."""
    g, pix, side = inp.straddle_case()
    r, got, _ = _warp_check('straddlers', engine, g, want_kept=600)
    assert (r['keep'][pix] == (side < 0)).all() and (got['keep'][pix] == (side < 0)).all()
    assert (side < 0).sum() >= 50 and (side > 0).sum() >= 50


def test_warp_exact_colour_ties(engine):
    """(d) both images the same constant per channel: inside view 2 every channel is tied by construction and the gradient is exactly
    zero, whatever sign(c1 - c2) comes to after the rounding of the four weights; at the border the zero padding breaks the tie."""
    g = inp.warp_scene('border', constant=True)
    r, got, g = _warp_check('ties', engine, g, want_kept=2000)
    tied = r['keep'] & r['flat'].all(1) & (r['outside'] == 0)
    assert tied.sum() >= 1000 and not got['g_z'][tied].any()
    assert np.abs(got['g_z'][r['keep'] & (r['outside'] > 0) & (r['outside'] < 4)]).min() > 0 and np.count_nonzero(got['cam']) == 24


def test_warp_degenerate(engine):
    """(f) no valid pixel: loss 0 and zero gradients; nothing kept: NaN loss, keep all 0, finite zero gradients."""
    g = inp.warp_scene('inner')
    none = dict(g, mask1=np.zeros(g['H'] * g['W'], np.uint8))
    r, got, _ = _warp_check('no valid pixel', engine, none, want_kept=0)
    assert r['n_valid'] == 0 and got['loss'].tobytes() == np.zeros(1, np.float32).tobytes()
    assert not got['keep'].any() and not got['g_z'].any() and not got['cam'].any() and not got['c1'].any() and not got['c2'].any()
    r, got, _ = _warp_check('nothing kept', engine, inp.nothing_kept(g), want_kept=0)
    assert r['n_valid'] == g['H'] * g['W'] and r['n_kept'] == 0 and np.isnan(got['loss'][0])
    assert not got['keep'].any() and not got['g_z'].any() and not got['cam'].any() and not got['c1'].any() and not got['c2'].any()
