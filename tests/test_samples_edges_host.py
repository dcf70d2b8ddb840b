"""The restatement of the list stages (tests/samples_restatement.py) checked on the CPU: its closed-form camera terms against torch
float64 autograd of its own points, its points in float32 against float64 at the bar the GPU tests hold the kernels to (so a correct f32
implementation is known to meet that bar on those inputs), and the validity rule on the special values."""
import numpy as np
import pytest

import samples_edges_inputs as inp
import samples_restatement as sr


def _autograd_terms(mode, Ki, M, RT, depth, index, W, g, normal, draws):
    import torch
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    rt = t(RT).requires_grad_(True)
    p = sr.points(mode, t(Ki), t(M), rt, t(depth), index, W, t(normal), t(draws), xp=torch)
    (p * t(g)).sum().backward()
    return rt.grad.numpy()


@pytest.mark.parametrize('mode,number', [(sr.SURFACE, 1), (sr.FREESPACE, 1), (sr.FREESPACE, 3)])
def test_camera_terms_equal_autograd(mode, number):
    """camera_terms = d/dRT of sum(g_xyz . points(RT)) by torch float64 autograd, 1e-12 of the largest entry; M is a rotation times a
    diagonal scale, so M^T M is not the identity."""
    H, W = 13, 17
    rs = np.random.RandomState(5)
    Ki, M = (a.astype(np.float64) for a in inp.geometry(H, W))
    assert np.abs(M.T @ M - np.eye(3)).max() > 0.1
    RT = inp.cameras(1)[0].astype(np.float64)
    depth = inp.depth_with_n_valid(rs, H * W, 150).astype(np.float64)
    index = sr.valid(depth[None].astype(np.float32))[0][0]
    N = index.size
    assert N == 150
    normal = inp.normals(rs, H * W).astype(np.float64)
    draws = (inp.draws(rs, mode, number, N)).astype(np.float64)
    m = 2 if mode == sr.SURFACE else number
    g = rs.uniform(0.5, 1.5, (m * N, 3)) * rs.choice([-1.0, 1.0], (m * N, 3))
    got = sr.camera_terms(mode, Ki, M, RT, depth, index, W, g, draws)
    want = _autograd_terms(mode, Ki, M, RT, depth, index, W, g, normal if mode == sr.SURFACE else None, draws)
    err = np.abs(got['g_RT'] - want).max() / np.abs(want).max()
    print('%s number %d: camera_terms against autograd %.3e' % (mode, number, err))
    assert err <= 1e-12
    assert np.all(got['A_RT'] >= np.abs(got['g_RT']) * (1 - 1e-12))
    assert got['terms'].shape == (N, 12) and np.allclose(got['terms'].sum(0), got['sum'], rtol=1e-12, atol=0)


def test_color_terms_equal_autograd():
    import torch
    H, W = 13, 17
    rs = np.random.RandomState(6)
    Ki, M = (a.astype(np.float64) for a in inp.geometry(H, W))
    RT = inp.cameras(1)[0].astype(np.float64)
    z = rs.uniform(0.8, 2.0, H * W)
    index = np.sort(rs.choice(H * W, 120, replace=False))
    g = rs.uniform(0.5, 1.5, (120, 3)) * rs.choice([-1.0, 1.0], (120, 3))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    R, T = t(RT[:, :3]).requires_grad_(True), t(RT[:, 3]).requires_grad_(True)
    (sr.surface_points(t(Ki), t(M), R, T, t(z), index, W, xp=torch) * t(g)).sum().backward()
    got = sr.camera_terms_color(Ki, M, RT[:, :3], RT[:, 3], z, index, W, g)
    scale = max(np.abs(R.grad.numpy()).max(), np.abs(T.grad.numpy()).max())
    assert np.abs(got['g_R'] - R.grad.numpy()).max() <= 1e-12 * scale and np.abs(got['g_T'] - T.grad.numpy()).max() <= 1e-12 * scale


@pytest.mark.parametrize('case', inp.POINT_CASES, ids=lambda c: '%s-%d-%d' % c)
def test_f32_points_meet_the_points_bar(case):
    """The inputs of the GPU module's point-list cases: the restatement evaluated in float32 numpy stays within the points bar of its
    float64 evaluation."""
    mode, number, N = case
    P = inp.H_B * inp.W_B
    v = inp.point_case(mode, number, [N])
    Ki, M = inp.geometry(inp.H_B, inp.W_B)
    index = sr.valid(v['depth'])[0][0]
    assert index.size == N
    w = lambda a: None if a is None else a.astype(np.float64)
    args = (v['RT'][0], v['depth'][0], index, inp.W_B, None if v['normal'] is None else v['normal'][0], v['draws'][0])
    p32 = sr.points(mode, Ki, M, *args)
    p64 = sr.points(mode, w(Ki), w(M), *[a if a is index or isinstance(a, int) else w(a) for a in args])
    assert p32.dtype == np.float32 and p64.dtype == np.float64 and p32.shape == ((2 if mode == sr.SURFACE else number) * N, 3)
    err, bar = float(np.abs(p32 - p64).max()), sr.points_bar(p64)
    print('%s number %d N %d: f32 against f64 %.3e (bar %.3e)' % (mode, number, N, err, bar))
    assert err <= bar


def test_f32_points_meet_the_points_bar_large_and_color():
    """The same for the 3 x 174 763 case (all valid, number 1) and for the colour stage's points."""
    H, W = inp.BIG_HW
    v = inp.big_case()
    Ki, M = inp.geometry(H, W)
    w = lambda a: a.astype(np.float64)
    index = np.arange(H * W)
    p32 = sr.points(sr.FREESPACE, Ki, M, v['RT'][0], v['depth'][0], index, W, None, v['draws'][0])
    p64 = sr.points(sr.FREESPACE, w(Ki), w(M), w(v['RT'][0]), w(v['depth'][0]), index, W, None, w(v['draws'][0]))
    assert np.abs(p32 - p64).max() <= sr.points_bar(p64)
    R, T = v['RT'][0][:, :3], v['RT'][0][:, 3]
    c32 = sr.surface_points(Ki, M, R, T, v['depth'][0], index, W)
    c64 = sr.surface_points(w(Ki), w(M), w(R), w(T), w(v['depth'][0]), index, W)
    assert c32.dtype == np.float32 and np.abs(c32 - c64).max() <= sr.points_bar(c64)


def _camera_ratios(mode, number, N, seed):
    """The camera sums of one point-list case against float64, in units of rounding_bar, largest over the twelve entries of g_RT:
    (a pixel's terms in float64 rounded once to float32 and summed in float32 -- what k_samp_cam_bwd does; everything in float32 -- what it
    did before, against the count that belonged to it, 46 + m + 1 roundings; the same against B). The point gradients are random
    directions of length 0.5 .. 1.5 (a decoder is not needed)."""
    rs = np.random.RandomState(seed)
    v = inp.point_case(mode, number, [N])
    Ki, M = inp.geometry(inp.H_B, inp.W_B)
    index = sr.valid(v['depth'])[0][0]
    m = 2 if mode == sr.SURFACE else number
    g = rs.standard_normal((m * N, 3))
    g = (g / np.linalg.norm(g, axis=1, keepdims=True) * rs.uniform(0.5, 1.5, (m * N, 1))).astype(np.float32)
    w = lambda a: a.astype(np.float64)
    c32 = sr.camera_terms(mode, Ki, M, v['RT'][0], v['depth'][0], index, inp.W_B, g, v['draws'][0], dtype=np.float32)
    c64 = sr.camera_terms(mode, w(Ki), w(M), w(v['RT'][0]), w(v['depth'][0]), index, inp.W_B, w(g), w(v['draws'][0]))
    assert c32['terms'].dtype == np.float32 and c64['terms'].dtype == np.float64
    once = sr.compose(c64['terms'].astype(np.float32).sum(0, dtype=np.float32), c64['R'], c64['T'])
    old_k = (47 + m) * 2.0 ** -24
    err = np.abs(c32['g_RT'] - c64['g_RT'])
    return (float((np.abs(once - c64['g_RT']) / sr.rounding_bar(c64['A_RT'], 'samples', N)).max()),
            float((err / (old_k * c64['A_RT'])).max()), float((err / (old_k * c64['B_RT'])).max()))


@pytest.mark.parametrize('mode,number', [(sr.SURFACE, 1), (sr.FREESPACE, 1), (sr.FREESPACE, 3), (sr.FREESPACE, 64)])
def test_camera_sums_meet_the_rounding_bar_on_the_cpu(mode, number):
    """Per-pixel terms formed in float64 and rounded once stay within k 2^-24 A at every list size, a single pixel included (200 draws of
    its point gradient). A float32 evaluation of the whole closed form does so only where a sum holds many pixels: for ONE pixel,
    g_r = g_d / e - (g_d . r) r / (rn e^2) is a difference that can be small against its two parts, and 5 to 12 per cent of single pixels
    are off by more than the 47 + m roundings that evaluation has (the figures are printed; with B for A every one stays below). That is
    why the kernel forms the terms in float64."""
    for N in inp.NS[1:]:
        once, f32, _ = _camera_ratios(mode, number, N, 1)
        print('%s number %d N %d: terms rounded once %.3f bars; all float32 %.3f of its own bar' % (mode, number, N, once, f32))
        assert once <= 1.0 and f32 <= 1.0
    single = np.array([_camera_ratios(mode, number, 1, s) for s in range(200)])
    print('%s number %d N 1, 200 draws of the point gradient: terms rounded once, largest %.3f bars; all float32: median %.3f, largest %.2f, '
          'above its bar %d; with B for A: largest %.3f' % (mode, number, float(single[:, 0].max()), float(np.median(single[:, 1])),
                                                          float(single[:, 1].max()), int((single[:, 1] > 1.0).sum()), float(single[:, 2].max())))
    assert single[:, 0].max() <= 1.0 and single[:, 2].max() <= 1.0


def test_valid_on_the_special_values():
    below = np.nextafter(np.float32(1e5), np.float32(0))
    d = np.array([[np.nan, np.inf, -np.inf, -1.0, 0.0, -0.0, 1e5, below, 1e-45, 1.0, np.float32(1e5) + np.float32(0.0078125)]], dtype=np.float32)
    assert d[0, 8] > 0 and d[0, 8] < np.finfo(np.float32).tiny          # a subnormal
    assert below < np.float32(1e5) and np.float32(1e5) == 100000.0
    index, counts = sr.valid(d)
    assert counts == [3] and index[0].tolist() == [7, 8, 9]
    got =sr.valid(np.array([inp.SPECIALS], dtype=np.float32))[0][0].tolist()
    assert got == [i for i, ok in enumerate(inp.SPECIALS_VALID) if ok]


def test_rounding_count():
    assert sr.rounding_count('samples', 0) == 29 and sr.rounding_count('samples', 1) == 29 and sr.rounding_count('samples', 524288) == 29
    assert sr.rounding_count('samples', 524289) == 30
    assert sr.rounding_count('color', 2049) == 44 and sr.rounding_count('color', 524289) == 45
