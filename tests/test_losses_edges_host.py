"""The restatement of the fused losses (tests/losses_restatement.py) checked on the CPU: against oracle/loss_oracle.py on the goldens G7, G8
and on the inputs of tests/test_gpu_losses_edges.py, its closed-form gradients against torch float64 autograd, a float32 evaluation of a
single pixel's camera terms against its own rounding bar, and every condition the GPU cases assume of their inputs."""
import os

import numpy as np
import pytest

import losses_edges_inputs as inp
import losses_restatement as lr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
U = lr.U


def _single(g, weights=None):
    return lr.single(g['depth'], g['normal'], g['mask'], g['min_sdf'], g.get('gt_depth'), g.get('gt_normal'), g['gt_mask'], g['threshold'],
                     g['weights'] if weights is None else weights)


def _oracle_single(g, dtype):
    import torch
    from oracle import loss_oracle
    shape = np.asarray(g['mask']).shape
    shape = (1,) + shape if len(shape) == 1 else shape                     # the oracle's norm runs over dim 2
    t = lambda k, s=(): None if g.get(k) is None else torch.from_numpy(np.asarray(g[k]).reshape(shape + s))
    f = lambda k, s=(): None if g.get(k) is None else t(k, s).to(dtype)
    d, n, q = (f(k, s).clone().requires_grad_(True) for k, s in (('depth', ()), ('normal', (3,)), ('min_sdf', ())))
    ref = loss_oracle.single_view_losses(d, n, t('mask'), q, f('gt_depth'), f('gt_normal', (3,)), t('gt_mask'), float(np.float32(g['threshold'])))
    total = sum(float(w) * v for w, v in zip(np.asarray(g['weights'], np.float32), ref))
    if total.requires_grad:
        total.backward()
    grad = lambda v: np.zeros(tuple(v.shape)) if v.grad is None else v.grad.numpy().astype(np.float64)
    return np.array([float(v) for v in ref]), grad(d).reshape(-1), grad(n).reshape(-1, 3), grad(q).reshape(-1)


def _f3_inputs():
    out = []
    for P in inp.F3_SIZES:
        out += [('random %d %s' % (P, f), inp.f3_random(P, *f)) for f in inp.F3_FORMS]
        out += [('both %d' % P, inp.f3_full(P)[0]), ('apart %d' % P, inp.f3_full(P)[1]), ('empty %d' % P, inp.f3_empty(P))]
    return out + [('specials', inp.f3_specials()[0])]


def test_single_restatement_equals_autograd_and_oracle():
    """Closed-form gradients = float64 autograd of the oracle's text (1e-12); losses and gradients = the float32 oracle at float32 bars;
    on G7 = the reference's own numbers."""
    import torch
    for tag, g in _f3_inputs():
        r = _single(g)
        l64, d64, n64, q64 = _oracle_single(g, torch.float64)
        assert np.abs(r['losses'] - l64).max() <= 1e-12 * max(1.0, np.abs(l64).max()), tag
        for a, b in ((r['g_depth'], d64), (r['g_normal'], n64), (r['g_min_sdf'], q64)):
            assert np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1e-30), tag
        l32, d32, n32, q32 = _oracle_single(g, torch.float32)
        assert np.allclose(l32, r['losses'], rtol=2e-5, atol=1e-9), tag
        for a, b in ((r['g_depth'], d32), (r['g_normal'], n32), (r['g_min_sdf'], q32)):
            assert np.abs(a - b).max() <= 1e-5 * max(np.abs(b).max(), 1e-30), tag
        assert np.all(r['A_normal'] >= np.abs(r['g_normal']) * (1 - 1e-12)) and np.all(r['loss_A'] >= np.abs(r['losses']) * (1 - 1e-12))
    g = dict(np.load(os.path.join(GOLDEN, 'g7_single_losses.npz')))
    r = _single(g)
    assert np.allclose(r['losses'], g['losses'], rtol=2e-6, atol=1e-9)
    for name in ('g_depth', 'g_normal', 'g_min_sdf'):
        assert np.abs(r[name].reshape(-1) - g[name].reshape(-1)).max() <= 2e-6 * np.abs(g[name]).max(), name


def test_single_rules_float64_cannot_decide():
    """The kernel's rules, pinned: hinge sub-gradient 0 at min_sdf == threshold, gt_depth in (0, 1e5), the float32 norm test, sign(0) = 0,
    the mean over an empty set."""
    g, where = inp.f3_specials()
    r = _single(g)
    assert [bool(r['member'][2][p]) for p, _ in inp.GT_DEPTH_SPECIALS] == list(inp.GT_DEPTH_IN)
    assert all(r['member'][2][p] and r['g_depth'][p] == 0 for p in where['equal_depth'])
    assert not r['member'][3][list(where['zero_normal'])].any() and r['member'][3][list(where['zero_gt_normal'])].all()
    assert not r['g_normal'][list(where['zero_gt_normal'])].any()
    # the gradient cancels where the normals are (anti)parallel: the bar is against the terms
    for key in ('parallel', 'antiparallel', 'nearly'):
        p = list(where[key])
        assert np.all(np.abs(r['g_normal'][p]) <= 1e-3 * r['A_normal'][p]) and np.all(r['A_normal'][p] > 0), key
    tiny = dict(g, normal=np.full_like(g['normal'], 1e-30))       # |n|^2 underflows in float32: not in the set, as the kernel has it
    assert not _single(tiny)['member'][3].any()
    g, ties = inp.f3_hinge_ties()
    r = _single(g)
    for p, s in ties.items():
        assert r['member'][0][p] != r['member'][1][p]
        assert (r['g_min_sdf'][p] != 0) == ((s > 0) if r['member'][0][p] else (s < 0)), (p, s)
    e = _single(inp.f3_empty(513))
    assert not e['counts'].any() and not e['losses'].any() and not e['g_depth'].any() and not e['g_normal'].any() and not e['g_min_sdf'].any()


def test_single_input_conditions():
    for P in inp.F3_SIZES:
        for f in inp.F3_FORMS:
            r = _single(inp.f3_random(P, *f))
            if P >= 63:
                assert all(r['counts'][k] > 0 for k in range(4) if (k < 2 or f[k - 2])), (P, f, r['counts'])
            assert r['member'][1][-1] and r['value'][1][-1] > 0                   # the last block holds a member with a value
            assert r['counts'][2] == 0 or f[0]
            assert r['counts'][3] == 0 or f[1]
        for term in range(4):
            for pos in inp.positions(P):
                r = _single(inp.f3_one_member(P, term, pos))
                assert r['counts'].tolist() == [int(k == term) for k in range(4)] and r['member'][term][pos] and r['value'][term][pos] != 0
                assert abs(r['losses'][term] - r['value'][term][pos]) == 0
        both, apart = inp.f3_full(P)
        assert _single(both)['counts'].tolist() == [0, 0, P, P] and _single(apart)['counts'][:2].sum() == P
        assert not _single(inp.f3_empty(P))['counts'].any()
    assert inp.positions(16641) == [0, 63, 64, 255, 256, 16640] and inp.positions(1) == [0] and inp.positions(64) == [0, 63]
    assert lr.nblk(16641) == 66
    for P in (257, 513):
        _, spots = inp.f3_poison(inp.f3_random(P, key='poison'))
        assert all(s.sum() >= P // 4 for s in spots.values())
    big = inp.f3_big()
    assert big['members'] > 2 ** 24 and float(np.float32(big['members'])) == big['members'] and big['P'] < 2 ** 26
    assert int((big['mask'] != 0).sum()) == big['members'] and big['mask'].reshape(-1, 256).sum(1).max() == 255
    # what the float32 sum of the per-block counts did: 255 added 66 818 times in float32 is not the count
    acc = np.float32(0)
    for _ in range(inp.BIG_BLOCKS):
        acc = np.float32(acc + np.float32(255))
    print('float32 sum of 66 818 x 255: %d, the count: %d' % (int(acc), big['members']))
    assert int(acc) != big['members']


# ============================================================================================ f2
def _torch_warp64(g):
    """renderer_warp.py:18-101 in torch float64 from the float32 inputs (the text of oracle/loss_oracle.py, widened) -> gradients by autograd."""
    import torch
    import torch.nn.functional as F
    H, W = int(g['H']), int(g['W'])
    K, Ki = (torch.from_numpy(a.astype(np.float64)) for a in inp.cfg_matrices(g))
    t = lambda k: torch.from_numpy(np.asarray(g[k], np.float32).astype(np.float64))
    z1, R1, T1, R2, T2 = (t(k).clone().requires_grad_(True) for k in ('zdepth1', 'R1', 'T1', 'R2', 'T2'))
    m1 = torch.from_numpy(np.asarray(g['mask1']).reshape(-1) != 0)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing='ij')
    homo = Ki @ torch.stack([xx.reshape(-1), yy.reshape(-1), torch.ones(H * W, dtype=torch.float64)], 0)
    calib = (homo / (torch.norm(homo, p=2, dim=0, keepdim=True) + lr.EPS))[2]
    rays = R1.t() @ homo
    rays = rays / (torch.norm(rays, p=2, dim=0, keepdim=True) + lr.EPS)
    pts = rays[:, m1] * z1.reshape(-1)[m1][None, :] + (-(R1.t() @ T1))[:, None]
    proj = K @ (R2 @ pts + T2[:, None])
    xy = proj[:2] / proj[2]

    def sample(img):
        grid = torch.stack([2.0 * xy[0] / max(W - 1, 1) - 1.0, 2.0 * xy[1] / max(H - 1, 1) - 1.0], -1)[None, :, None, :]
        return F.grid_sample(img, grid, mode='bilinear', padding_mode='zeros', align_corners=True)[0, :, :, 0]
    keep = (proj[2] - sample((t('zdepth2').reshape(-1) * calib).reshape(1, 1, H, W))[0]) ** 2 < float(np.float32(g['thres_depth']))
    a = t('img1').reshape(H * W, 3)[m1][keep]
    b = sample(t('img2').reshape(H, W, 3).permute(2, 0, 1)[None]).t()[keep]
    loss = torch.mean(torch.abs(a - b))
    (loss * float(np.float32(g.get('g_loss', 1.0)))).backward()
    full = np.zeros(H * W, bool)
    full[np.nonzero(m1.numpy())[0][keep.numpy()]] = True
    return float(loss), full, z1.grad.numpy(), np.concatenate([v.grad.numpy().reshape(-1) for v in (R1, T1, R2, T2)])


def _warp_inputs():
    out = [('border', dict(inp.warp_scene('border'), g_loss=0.37)), ('inner', inp.warp_scene('inner')), ('ties', inp.warp_scene('border', constant=True)),
           ('straddlers', inp.straddle_case()[0])]
    out += [('size %dx%d' % hw, inp.warp_scene('inner', hw)) for hw in inp.WARP_SIZES]
    return out + [('one-hot %s %d' % c, inp.one_hot(inp.warp_scene(c[0]), c[1])) for c in inp.one_hot_pixels()]


def test_warp_restatement_equals_autograd():
    """Loss, kept set, g_z1 and the 24 camera entries of the closed form = torch float64 autograd through grid_sample, 1e-10 of the largest
    entry, on every GPU case after its ambiguous pixels are cleared (a pixel on a grid line has two one-sided derivatives). The
    one-pixel-wide images included: grid_sample's round trip has no gradient along the thin axis."""
    for tag, g in _warp_inputs():
        g, r, share = inp.clear_ambiguous(g)
        loss, keep, gz, cam = _torch_warp64(g)
        assert np.array_equal(keep, r['keep']) and r['n_kept'] > 0, tag
        assert abs(loss - float(r['loss'])) <= 1e-12, tag
        assert np.abs(gz - r['g_z']).max() <= 1e-10 * max(np.abs(gz).max(), 1e-30), (tag, np.abs(gz - r['g_z']).max(), np.abs(gz).max())
        assert np.abs(cam - r['cam']).max() <= 1e-10 * np.abs(cam).max(), (tag, np.abs(cam - r['cam']).max())
        assert np.all(r['cam_A'] >= np.abs(r['cam']) * (1 - 1e-12)) and np.all(r['A_z'] >= np.abs(r['g_z']) * (1 - 1e-12))


def _oracle_warp32(g):
    import torch
    from oracle import loss_oracle
    t = lambda k: torch.from_numpy(np.asarray(g[k], np.float32)).clone().requires_grad_(True)
    c = lambda k: torch.from_numpy(np.asarray(g[k], np.float32))
    H, W = int(g['H']), int(g['W'])
    tz, tR1, tT1, tR2, tT2 = t('zdepth1'), t('R1'), t('T1'), t('R2'), t('T2')
    ol, okeep, oc1, oc2 = loss_oracle.warp_loss(g['K'], H, W, tz, torch.from_numpy(np.asarray(g['mask1'])), c('zdepth2'), c('img1').reshape(H, W, 3),
                                                c('img2').reshape(H, W, 3), tR1, tT1, tR2, tT2, float(g['thres_depth']))
    (ol * float(g.get('g_loss', 1.0))).backward()
    return float(ol), okeep.numpy(), oc2.numpy().reshape(-1, 3), tz.grad.numpy().reshape(-1), np.concatenate([v.grad.numpy().reshape(-1) for v in (tR1, tT1, tR2, tT2)])


def test_warp_restatement_equals_oracle_and_golden():
    """The float32 oracle on every GPU case (ambiguous pixels cleared) at the parity tests' float32 bars, and the reference's numbers of G8."""
    for tag, g in _warp_inputs():
        g, r, _ = inp.clear_ambiguous(g)
        loss, keep, c2, gz, cam = _oracle_warp32(g)
        assert np.array_equal(keep, r['keep']), tag
        assert abs(loss - float(r['loss'])) <= 1e-5 and np.abs(c2 - r['c2']).max() <= 2e-4, (tag, np.abs(c2 - r['c2']).max())
        assert np.abs(gz - r['g_z']).max() <= 5e-4 * np.abs(r['g_z']).max(), tag
        for s in (slice(0, 9), slice(9, 12), slice(12, 21), slice(21, 24)):
            assert np.abs(cam[s] - r['cam'][s]).max() <= 5e-4 * np.abs(r['cam'][s]).max(), (tag, s)
    g = dict(np.load(os.path.join(GOLDEN, 'g8_warp_loss.npz')))
    g, r, share = inp.clear_ambiguous(g)
    print('G8: %.2f%% of the valid pixels ambiguous' % (100 * share))
    if share == 0:
        assert np.array_equal(r['keep'], g['keep'] != 0) and abs(float(r['loss']) - float(g['loss_color'])) <= 2e-6
        assert np.abs(r['c2'] - g['color_valid_2'].reshape(-1, 3)).max() <= 2e-5
        got = np.concatenate([g[k].reshape(-1) for k in ('g_R1', 'g_T1', 'g_R2', 'g_T2')])
        assert np.abs(r['g_z'] - g['g_zdepth1']).max() <= 2e-4 * np.abs(g['g_zdepth1']).max() and np.abs(got - r['cam']).max() <= 2e-4 * np.abs(got).max()
    else:
        ref = inp.restate(dict(np.load(os.path.join(GOLDEN, 'g8_warp_loss.npz'))))
        assert (ref['keep'] != (np.load(os.path.join(GOLDEN, 'g8_warp_loss.npz'))['keep'] != 0)).sum() == 0


def test_warp_input_conditions():
    """What the GPU cases assume: border counts, non-empty sets, the share of ambiguous pixels under the cap, straddler margins."""
    for tag, g in _warp_inputs():
        g2, r, share = inp.clear_ambiguous(g)
        print('%s: %d valid, %d kept, %.2f%% ambiguous' % (tag, r['n_valid'], r['n_kept'], 100 * share))
        assert share <= inp.AMBIGUOUS_CAP and r['n_kept'] >= 1, tag
        raw = inp.restate(g)
        tie = raw['keep'][:, None] & (raw['m_color'] == 0) & ~raw['flat']
        assert not tie.any(), (tag, 'an exact colour tie in a channel that is not flat')
    g = inp.warp_scene('border')
    _, r, _ = inp.clear_ambiguous(g)
    b = inp.border_pixels(r, g['H'], g['W'])
    print('border scene:', {k: len(v) for k, v in b.items()})
    assert all(len(b[k]) >= 8 for k in ('left', 'right', 'top', 'bottom', 'outside')) and len(b['corner']) >= 4
    cx, cy = r['ix'][b['corner']] < 0, r['iy'][b['corner']] < 0
    assert {(bool(a), bool(c)) for a, c in zip(cx, cy)} == {(False, False), (False, True), (True, False), (True, True)}, 'one at each image corner'
    assert r['keep'].all() or r['ambiguous'].sum() == 0
    assert np.abs(np.asarray(g['img2']).reshape(g['H'], g['W'], 3)[[0, -1]]).min() > 0 and np.abs(np.asarray(g['img2']).reshape(g['H'], g['W'], 3)[:, [0, -1]]).min() > 0
    for k in ('left', 'right', 'top', 'bottom', 'corner'):
        assert np.abs(r['g_z'][b[k]]).min() > 0, k
    assert not r['g_z'][b['outside']].any() and not r['c2'][b['outside']].any() and r['keep'][b['outside']].all()
    for kind, pix in inp.one_hot_pixels():
        r = inp.restate(inp.one_hot(inp.warp_scene(kind), pix))
        assert r['n_kept'] == 1 and not r['ambiguous'].any() and np.count_nonzero(r['cam']) == 24 and r['g_z'][pix] != 0, (kind, pix)
    assert [c[1] for c in inp.one_hot_pixels()[:4]] == [0, 255, 256, 767]
    for hw in inp.WARP_SIZES:
        _, r, _ = inp.clear_ambiguous(inp.warp_scene('inner', hw))
        P = hw[0] * hw[1]
        last = np.arange(256 * (lr.nblk(P) - 1), P)
        assert np.abs(r['terms'][last][:, 16:]).max() > 0 and r['n_kept'] >= P // 2, hw
        assert np.count_nonzero(r['cam']) == (20 if min(hw) == 1 else 24), hw
    assert lr.nblk(128 * 129) == 65
    g, pix, side = inp.straddle_case()
    r = inp.restate(g)
    m = (r['err2'][pix] - float(np.float32(g['thres_depth']))) / r['b_thres'][pix]
    print('straddlers: %d pixels, |err^2 - thres| between %.2f and %.2f bounds' % (pix.size, np.abs(m).min(), np.abs(m).max()))
    assert np.all(np.sign(m) == side) and np.abs(m).min() >= 2.0 and np.abs(m).max() <= 10.0 and not r['ambiguous'][pix].any()
    assert (side < 0).sum() >= 50 and (side > 0).sum() >= 50 and np.array_equal(r['keep'][pix], side < 0)
    _, r, _ = inp.clear_ambiguous(inp.warp_scene('border', constant=True))
    assert (r['keep'] & r['flat'].all(1) & (r['outside'] == 0)).sum() >= 1000
    assert not r['g_z'][r['keep'] & r['flat'].all(1)].any()
    r = inp.restate(inp.nothing_kept(inp.warp_scene('inner')))
    assert r['n_valid'] == 768 and r['n_kept'] == 0 and np.isnan(r['loss']) and not r['cam'].any() and not r['ambiguous'].any()


def test_random_sphere_scenes_stay_under_the_cap():
    """The twelve random scenes of tests/test_gpu_parity.py::test_random_warp_losses_match_oracle (seeds 0 .. 11): the share of valid pixels
    the restatement calls ambiguous, against the cap of 3 %."""
    from oracle.gen_synth import sphere_view, procedural_images
    from distr import fixture
    shares = []
    for seed in range(12):
        rs = np.random.RandomState(31000 + seed)
        H, W = int(rs.randint(24, 160)), int(rs.randint(24, 160))
        K = np.array(fixture.make_intrinsic(H, W), dtype=np.float64)
        K[0, 0] *= rs.uniform(0.85, 1.2); K[1, 1] *= rs.uniform(0.85, 1.2); K[0, 2] += rs.uniform(-0.1, 0.1) * W; K[1, 2] += rs.uniform(-0.1, 0.1) * H
        az, el, dist = float(rs.uniform(-180, 180)), float(rs.uniform(-40, 40)), float(rs.uniform(1.4, 2.2))
        R1, T1 = fixture.make_camera(az, el, dist, float(rs.uniform(-10, 10)))
        R2, T2 = fixture.make_camera(az + float(rs.uniform(-60, 60)), el + float(rs.uniform(-25, 25)), dist * float(rs.uniform(0.85, 1.2)), float(rs.uniform(-10, 10)))
        rad, ctr = float(rs.uniform(0.35, 0.75)), tuple(float(v) for v in rs.uniform(-0.08, 0.08, 3))
        z1, hit1 = sphere_view(K, R1, T1, H, W, rad, ctr)
        z2, _ = sphere_view(K, R2, T2, H, W, rad, ctr)
        img1, img2 = procedural_images(H, W)
        g = dict(H=H, W=W, K=K, R1=R1, T1=T1, R2=R2, T2=T2, thres_depth=float(10 ** rs.uniform(-3.5, -1.5)), zdepth1=z1, mask1=hit1.astype(np.uint8), zdepth2=z2,
                 img1=img1, img2=img2)
        shares.append(inp.clear_ambiguous(g)[2])
    print('ambiguous share of the valid pixels, seeds 0 .. 11: ' + ' '.join('%.2f%%' % (100 * s) for s in shares))
    assert max(shares) <= inp.AMBIGUOUS_CAP


def test_single_pixel_camera_terms_in_float32():
    """One kept pixel's 24 camera terms and g_z1: formed in float64 and rounded once they are within 2^-24 of themselves by construction
    (what k_warp_bwd does); the same closed form evaluated in float32 numpy (what it did before) against its own count of roundings
    (lr.K_F32: 148 .. 210) times |the term|. The figures are printed for every pixel of the inner scene and the border scene."""
    for kind in ('inner', 'border'):
        g, r64, _ = inp.clear_ambiguous(inp.warp_scene(kind))
        r32 = inp.restate(g, dtype=np.float32)
        assert r32['terms'].dtype == np.float32 and r64['terms'].dtype == np.float64
        sel = r64['keep'] & r32['keep'] & (r64['outside'] < 4)
        t64, t32 = r64['terms'][sel], r32['terms'][sel].astype(np.float64)
        once = np.abs(t64.astype(np.float32).astype(np.float64) - t64)
        assert np.all(once <= U * np.abs(t64))
        k = np.concatenate([[lr.K_F32['g_R1']] * 9, [lr.K_F32['g_T1']] * 3, [lr.K_F32['g_R2']] * 9, [lr.K_F32['g_T2']] * 3])
        with np.errstate(divide='ignore', invalid='ignore'):
            ratio = np.where(t64 != 0, np.abs(t32 - t64) / (k * U * np.abs(t64)), 0.0).max(1)
            ratio1 = np.where(t64 != 0, np.abs(t32 - t64) / (U * np.abs(t64)), 0.0).max(1)
            gz = np.abs(r32['g_z'][sel].astype(np.float64) - r64['g_z'][sel]) / (U * np.maximum(r64['A_z'][sel], 1e-300))
        print('%s scene, %d single pixels, float32 closed form against float64: camera terms median %.3f, largest %.2f of their own bar (k 148 .. 210), '
              '%d above it; in units of the one-rounding bar the kernel is held to: median %.1f, largest %.0f; g_z1: median %.1f, largest %.0f' % (
                  kind, int(sel.sum()), float(np.median(ratio)), float(ratio.max()), int((ratio > 1).sum()), float(np.median(ratio1)), float(ratio1.max()),
                  float(np.median(gz)), float(gz.max())))
        assert np.median(ratio1) > 1.0            # a float32 evaluation does not meet the bar of terms rounded once


def test_rounding_counts():
    assert lr.k_single_loss(0, 1) == 12 and lr.k_single_loss(3, 16641) == 15 + 10 + 66
    assert lr.k_warp_loss(768) == 77 and lr.k_warp_cam(1) == 11 and lr.k_warp_cam(128 * 129) == 75
