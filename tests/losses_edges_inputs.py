"""The synthetic inputs of tests/test_gpu_losses_edges.py, made with numpy from fixed seeds. tests/test_losses_edges_host.py reads the same
ones and asserts every condition a GPU case relies on (set sizes, border counts, the share of ambiguous pixels), so that no GPU case can
pass because its inputs were empty. Everything is float32 (uint8 for masks)."""
import zlib

import numpy as np

from distr import fixture

import losses_restatement as lr

# ---------------------------------------------------------------------------------------------- f3
F3_SIZES = (1, 63, 64, 65, 255, 256, 257, 513, 256 * 65 + 1)
_RAGGED = {1: (1, 1), 63: (7, 9), 64: (8, 8), 65: (5, 13), 255: (15, 17), 256: (16, 16), 257: (257, 1), 513: (19, 27), 16641: (43, 387)}
F3_FORMS = ((True, True), (True, False), (False, True), (False, False))         # (with gt_depth, with gt_normal)
F3_POSITIONS = (0, 63, 64, 255, 256, -1)
THRESHOLD = 5e-5
BELOW_1E5 = float(np.nextafter(np.float32(1e5), np.float32(0)))
BIG_BLOCKS = 66818                                   # 255 members in each of 66 818 blocks: 17 038 590 = 2^24 + 261 374, even (a float32): 1025 additions above 2^24
SET_NAMES = ('mask_gt', 'mask_out', 'depth', 'normal')


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def f3_shapes(P):
    """1 x P, and the ragged H x W of the same P (P x 1 for a prime)."""
    return [(1, P)] if P == 1 else [(1, P), _RAGGED[P]]


def positions(P):
    return sorted({p % P for p in F3_POSITIONS if p < P})


def f3_random(P, with_depth=True, with_normal=True, key=0):
    """Random masks of density 1/2 (every set has about P / 4 members), 10 % zero normals, 5 % zero gt normals, 10 % invalid gt depth; pixel
    P - 1 is a member of mask_out with a non-zero value."""
    rs = np.random.RandomState(_seed('f3', P, key))
    thr = THRESHOLD
    g = dict(threshold=thr, depth=(1 + rs.rand(P)).astype(np.float32), normal=rs.standard_normal((P, 3)).astype(np.float32),
             mask=(rs.rand(P) < 0.5).astype(np.uint8) * rs.choice(np.array([1, 255], dtype=np.uint8), P),
             min_sdf=(4 * thr * rs.standard_normal(P)).astype(np.float32),
             gt_depth=np.where(rs.rand(P) < 0.9, 1 + rs.rand(P), 0).astype(np.float32), gt_normal=rs.standard_normal((P, 3)).astype(np.float32),
             gt_mask=(rs.rand(P) < 0.5).astype(np.uint8), weights=rs.uniform(0.1, 10.0, 4).astype(np.float32))
    g['normal'][rs.rand(P) < 0.1] = 0
    g['gt_normal'][rs.rand(P) < 0.05] = 0
    g['mask'][-1], g['gt_mask'][-1], g['min_sdf'][-1] = 255, 0, np.float32(-2 * thr)     # the last pixel (alone in its block at P = 513, 16 641) is in mask_out
    if not with_depth:
        g['gt_depth'] = None
    if not with_normal:
        g['gt_normal'] = None
    return g


def f3_full(P, key=0):
    """Every pixel in the depth and the normal set (both masks on), then the same data with the masks apart: every pixel in mask_gt
    (first half of the image) or mask_out (second half; P = 1: mask_gt). -> (both, apart)."""
    g = f3_random(P, key=('full', key))
    rs = np.random.RandomState(_seed('f3 full', P, key))
    g['gt_depth'] = (1 + rs.rand(P)).astype(np.float32)
    g['normal'] = (rs.standard_normal((P, 3)) + 0.1).astype(np.float32)
    both = dict(g, mask=np.ones(P, np.uint8), gt_mask=np.full(P, 255, np.uint8))
    first = np.arange(P) < max(1, P // 2)
    apart = dict(g, mask=(~first).astype(np.uint8), gt_mask=first.astype(np.uint8))
    return both, apart


def f3_empty(P, key=0):
    """Equal masks and no valid gt depth, zero normals: all four sets empty although both ground truths are given."""
    g = f3_random(P, key=('empty', key))
    g['gt_mask'] = (g['mask'] != 0).astype(np.uint8)
    g['gt_depth'] = np.zeros(P, np.float32)
    g['normal'] = np.zeros((P, 3), np.float32)
    return g


def f3_one_member(P, term, pos, key=0):
    """Random float data, both masks off everywhere but at `pos`, which belongs to set `term` alone (its value is not zero)."""
    g = f3_random(P, key=('one', key))
    g['mask'], g['gt_mask'] = np.zeros(P, np.uint8), np.zeros(P, np.uint8)
    g['gt_depth'] = np.abs(g['gt_depth']) + np.float32(0.5)
    if term == 0:
        g['gt_mask'][pos], g['min_sdf'][pos] = 1, np.float32(THRESHOLD) + np.float32(3e-4)
    elif term == 1:
        g['mask'][pos], g['min_sdf'][pos] = 1, np.float32(THRESHOLD) - np.float32(3e-4)
    else:
        g['mask'][pos] = g['gt_mask'][pos] = 1
        if term == 2:
            g['normal'][pos] = 0                      # not in the normal set
            g['depth'][pos] = g['gt_depth'][pos] + np.float32(0.25)
        else:
            g['gt_depth'][pos] = 0                    # not in the depth set
            g['normal'][pos], g['gt_normal'][pos] = (0.3, -0.5, 0.8), (0.1, 0.7, -0.2)
    return g


SPECIAL_P = 513
GT_DEPTH_SPECIALS = ((63, 0.0), (64, -1.0), (255, 1e5), (256, BELOW_1E5), (511, np.inf), (512, np.nan), (1, -0.0), (257, -np.inf))
GT_DEPTH_IN = (False, False, False, True, False, False, False, False)


def f3_specials():
    """P = 513, both masks on (depth and normal sets full but for the special pixels, which sit on wave and block boundaries):
    gt_depth at 0, -1, 1e5, nextafter(1e5, 0), inf, NaN; depth == gt_depth at pixels 0 and 320; zero normals at 62, 254; zero gt normals at
    65, 258; normals parallel (2, 253), antiparallel (66, 259) and nearly parallel (3, 510) to the gt normal.
    -> (inputs, dict of the pixel lists)."""
    P = SPECIAL_P
    g, _ = f3_full(P, key='specials')
    g['gt_normal'][~g['gt_normal'].any(1)] = (0.2, -0.4, 0.6)
    for p, v in GT_DEPTH_SPECIALS:
        g['gt_depth'][p] = v
    for p in (0, 320):
        g['depth'][p] = g['gt_depth'][p]
    g['normal'][[62, 254]] = 0
    g['gt_normal'][[65, 258]] = 0
    for p in (2, 253):
        g['normal'][p] = g['gt_normal'][p] * np.float32(1.75)
    for p in (66, 259):
        g['normal'][p] = g['gt_normal'][p] * np.float32(-0.375)
    for p in (3, 510):
        g['normal'][p] = g['gt_normal'][p] * np.float32(2.0) + np.float32(1e-4) * np.array([1, -1, 0.5], np.float32)
    return g, dict(equal_depth=(0, 320), zero_normal=(62, 254), zero_gt_normal=(65, 258), parallel=(2, 253), antiparallel=(66, 259), nearly=(3, 510))


def f3_hinge_ties():
    """P = 513, first half in mask_gt, second in mask_out; min_sdf == threshold and one ulp either side at pixels 0, 63, 64, 255 (mask_gt)
    and 256, 257, 511, 512 (mask_out). -> (inputs, {pixel: -1 / 0 / +1 ulp})."""
    _, g = f3_full(SPECIAL_P, key='ties')
    t = np.float32(THRESHOLD)
    up, down = np.nextafter(t, np.float32(1)), np.nextafter(t, np.float32(0))
    where = {0: 0, 63: 1, 64: -1, 255: 0, 256: 0, 257: 1, 511: -1, 512: 0}
    for p, s in where.items():
        g['min_sdf'][p] = (down, t, up)[s + 1]
    return g, where


def f3_poison(g):
    """NaN and inf (alternating, both signs of inf) written into depth, normal and min_sdf wherever the kernels must not read them:
    depth off the depth set, normal where the masks do not both hold, min_sdf off the two hinge sets. -> (poisoned copy, pixels per array)."""
    r = lr.single(g['depth'], g['normal'], g['mask'], g['min_sdf'], g['gt_depth'], g['gt_normal'], g['gt_mask'], g['threshold'])
    both = (np.asarray(g['mask']) != 0) & (np.asarray(g['gt_mask']) != 0)
    spots = dict(depth=~r['member'][2], normal=~both, min_sdf=~(r['member'][0] | r['member'][1]))
    bad = np.array([np.nan, np.inf, -np.inf], np.float32)
    out = dict(g)
    for name, sel in spots.items():
        a = np.array(g[name], copy=True)
        idx = np.nonzero(sel)[0]
        a[idx] = bad[idx % 3] if a.ndim == 1 else bad[idx % 3][:, None]
        out[name] = a
    return out, spots


def f3_big():
    """No gt depth or normal; every pixel but thread 255 of each block in mask_out (mask on, gt mask off), min_sdf = 0 (each value: the
    threshold). P = 66 818 * 256 = 17 105 408 < 2^26 with 17 038 590 members."""
    P = BIG_BLOCKS * 256
    mask = np.ones(P, np.uint8)
    mask[255::256] = 0
    return dict(P=P, mask=mask, gt_mask=np.zeros(P, np.uint8), min_sdf=np.zeros(P, np.float32), threshold=THRESHOLD, members=255 * BIG_BLOCKS)


# ---------------------------------------------------------------------------------------------- f2
PLANE_N, PLANE_O = np.array([0.25, -0.15, 1.0]) / np.linalg.norm([0.25, -0.15, 1.0]), np.array([0.02, -0.03, 0.1])
BORDER_HW, INNER_HW = (40, 56), (24, 32)
WARP_SIZES = ((1, 300), (300, 1), (15, 17), (16, 16), (1, 257), (128, 129))      # P = 255, 256, 257; 16 512 pixels: nblk = 65
AMBIGUOUS_CAP = 0.03


def _plane_depth(K, R, T, H, W):
    """Distance along the normalised ray of every pixel to the plane n . (X - o) = 0, float64."""
    Ki = np.linalg.inv(np.asarray(K, np.float64))
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    h = Ki @ np.stack([xx.reshape(-1), yy.reshape(-1), np.ones(H * W)])
    r = np.asarray(R, np.float64).T @ h
    d = r / np.linalg.norm(r, axis=0)
    c = -np.asarray(R, np.float64).T @ np.asarray(T, np.float64)
    return (PLANE_N @ (PLANE_O - c)) / (PLANE_N @ d)


def images(H, W, constant=False):
    """Two smooth positive images, non-zero everywhere (and so at the border of view 2). constant: both images the same constant per
    channel: every footprint inside view 2 is flat in every channel, an exact colour tie by construction."""
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    if constant:
        img = np.broadcast_to(np.array([0.75, 0.5, 0.25]), (H, W, 3))
        return img.astype(np.float32).copy(), img.astype(np.float32).copy()
    img1 = np.stack([0.5 + 0.4 * np.sin(xx / 3.0 + yy / 7.0), 0.5 + 0.4 * np.cos(yy / 4.0 - xx / 9.0), 0.45 + 0.3 * np.sin(xx / 5.0) * np.cos(yy / 6.0)], -1)
    img2 = np.stack([0.5 + 0.4 * np.sin(xx / 3.0 + yy / 7.0 + 0.7), 0.5 + 0.4 * np.cos(yy / 4.0 - xx / 9.0 - 0.3), 0.55 + 0.3 * np.sin(xx / 5.0 + 0.4) * np.cos(yy / 6.0)], -1)
    return img1.astype(np.float32), img2.astype(np.float32)


def warp_scene(kind, hw=None, constant=False):
    """A plane seen by two cameras; zdepth1 and zdepth2 are the analytic ray lengths, rounded to float32.
    'border': view 2 is nearer to the plane, so view 1 reaches past view 2 on all four sides; the threshold (16) keeps every point, also
    those whose footprint lies wholly outside view 2 (depth sample 0, err^2 = pr2^2 < 16).
    'inner': view 2 is farther away, every footprint is inside; threshold 1e-3 against an err of the bilinear interpolation, ~1e-5."""
    H, W = hw or (BORDER_HW if kind == 'border' else INNER_HW)
    K = fixture.make_intrinsic(H, W)
    if min(H, W) == 1:                               # a one-pixel-wide image: a usable focal length along the thin side too
        K[0, 0] = K[1, 1] = float(max(H, W))
    R1, T1 = fixture.make_camera(-12.0, 8.0, 1.7, 4.0)
    R2, T2 = fixture.make_camera(-11.0, 7.5, 1.7 / 1.12, 5.0) if kind == 'border' else fixture.make_camera(-9.0, 6.0, 2.3, 7.0)
    img1, img2 = images(H, W, constant)
    g = dict(kind=kind, H=H, W=W, K=K, R1=R1.astype(np.float32), T1=T1.astype(np.float32), R2=R2.astype(np.float32), T2=T2.astype(np.float32),
             thres_depth=16.0 if kind == 'border' else 1e-3, zdepth1=_plane_depth(K, R1, T1, H, W).astype(np.float32),
             zdepth2=_plane_depth(K, R2, T2, H, W).astype(np.float32), mask1=np.ones(H * W, np.uint8), img1=img1, img2=img2, g_loss=1.0)
    return g


def cfg_matrices(g):
    """(K, K_inv) as the float32 matrices binding.make_warp_cfg hands to the library."""
    K = np.asarray(g['K'], np.float64)
    return K.astype(np.float32), np.linalg.inv(K).astype(np.float32)


def restate(g, dtype=np.float64):
    K, Ki = cfg_matrices(g)
    return lr.warp(int(g['H']), int(g['W']), K, Ki, g['thres_depth'], g['zdepth1'], g['mask1'], g['zdepth2'], g['img1'], g['img2'], g['R1'], g['T1'],
                   g['R2'], g['T2'], g.get('g_loss', 1.0), dtype=dtype)


def clear_ambiguous(g):
    """(e): the case with the mask bit of every ambiguous pixel cleared, its restatement, and the share of valid pixels cleared."""
    r = restate(g)
    n_valid, n_amb = r['n_valid'], int(r['ambiguous'].sum())
    if n_amb == 0:
        return g, r, 0.0
    g2 = dict(g, mask1=np.where(r['ambiguous'], 0, np.asarray(g['mask1']).reshape(-1)).astype(np.uint8))
    r2 = restate(g2)
    assert not r2['ambiguous'].any()
    return g2, r2, n_amb / float(n_valid)


def one_hot(g, pix):
    m = np.zeros(int(g['H']) * int(g['W']), np.uint8)
    m[pix] = 1
    return dict(g, mask1=m)


def border_pixels(r, H, W):
    """Kept pixels of the border scene by where their footprint leaves view 2: {'left', 'right', 'top', 'bottom'}: one or two corners
    outside across that side only; 'corner': three outside; 'outside': all four."""
    ix, iy, out, keep = r['ix'], r['iy'], r['outside'], r['keep']
    part = keep & ((out == 1) | (out == 2))
    inx, iny = (ix >= 0) & (ix < W - 1), (iy >= 0) & (iy < H - 1)
    return dict(left=np.nonzero(part & (ix < 0) & iny)[0], right=np.nonzero(part & (ix >= W - 1) & iny)[0], top=np.nonzero(part & (iy < 0) & inx)[0],
                bottom=np.nonzero(part & (iy >= H - 1) & inx)[0], corner=np.nonzero(keep & (out == 3))[0], outside=np.nonzero(keep & (out == 4))[0])


def one_hot_pixels():
    """(scene kind, pixel) of the one-hot runs (b): pixels 0, 255, 256 and P - 1 of the inner scene (768 pixels, three blocks), and of the
    border scene one pixel on each side and the first corner pixel."""
    P = INNER_HW[0] * INNER_HW[1]
    out = [('inner', p) for p in (0, 255, 256, P - 1)]
    g = warp_scene('border')
    b = border_pixels(restate(g), g['H'], g['W'])
    return out + [('border', int(b[k][len(b[k]) // 2])) for k in ('left', 'right', 'top', 'bottom')] + [('border', int(b['corner'][0]))]


STRADDLE_BOUNDS = (3.0, 8.0)


def straddle_case():
    """(d): the inner scene with the view-1 depth of every 7th pixel moved so that err^2 lies 3 or 8 bounds (b_thres of the restatement)
    below or above the threshold; the restatement decides, and no pixel of them is ambiguous. -> (inputs, pixels, wanted side +-1)."""
    g = warp_scene('inner')
    P = g['H'] * g['W']
    pix = np.arange(3, P, 7)
    side = np.where(np.arange(pix.size) % 2 == 0, 1.0, -1.0)
    dist = np.where((np.arange(pix.size) // 2) % 2 == 0, STRADDLE_BOUNDS[0], STRADDLE_BOUNDS[1])
    thres = float(np.float32(g['thres_depth']))
    z = g['zdepth1'].astype(np.float64)
    z[pix] += np.sqrt(thres)                         # err = pr2 - d2 grows with the point's depth: start near err^2 = thres
    f = lambda zz: restate(dict(g, zdepth1=zz.astype(np.float32)))
    for _ in range(6):
        r0 = f(z)
        target = thres + side * dist * r0['b_thres'][pix]
        z1 = z.copy()
        z1[pix] += 1e-4
        slope = (f(z1)['err2'][pix] - r0['err2'][pix]) / 1e-4
        z[pix] -= (r0['err2'][pix] - target) / slope
    return dict(g, zdepth1=z.astype(np.float32)), pix, side


def nothing_kept(g):
    """(f): view 2 five units farther away: every point fails the depth test."""
    return dict(g, zdepth2=(g['zdepth2'] + np.float32(5.0)).astype(np.float32), thres_depth=1e-3)
