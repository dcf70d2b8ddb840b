"""The list stages around the decoder at their block edges: the depth samples (csrc/distr_samples.hpp: k_samp_count, k_samp_top_scan,
k_samp_compact, k_samp_points, k_samp_epilogue, k_samp_cam_bwd, k_samp_cam_fin) and the colour stage without lights
(csrc/distr_color_batch.hpp: k_cb_count, k_cb_compact, k_cb_points, k_cb_cam_bwd, k_cb_cam_fin) against the float64 restatement of
tests/samples_restatement.py, on synthetic inputs (tests/samples_edges_inputs.py; no render). The lit colour stage (the shading terms of
k_cb_cam_bwd) stays with tests/test_gpu_color_batch.py.

A. Compaction: counts and index lists, exactly, at P = 1, 2047, 2048, 2049 (the pixel block of 2048), 524 287, 524 288, 524 289 and
   1 048 577 (the first and second carry of the top scan's 256-block rounds), three views per call, six patterns over three calls.
B. Point list and epilogue at 72 x 64 with N = 1 .. 4097 valid pixels at random positions: every coordinate within
   4 2^-23 max(1, max |p|) of float64; the outputs byte for byte the decoder on the returned list (-+ eta).
C. Camera gradient: g_latent byte for byte the library's own decoder backward on the returned list; g_RT (g_R, g_T) within
   rounding_bar = k 2^-24 A of the closed form, entry by entry (k counted from the kernels: 29 for the depth samples, whose kernel forms a
   pixel's twelve terms in float64 and rounds them once, 30 with 257 camera blocks; 44 / 45 for the colour stage; samples_restatement's
   docstring has the count). A bar of k 2^-24 A sees a single dropped pixel as long as that pixel holds more than two bars of some entry
   (the sums' own residuals are a few per cent of a bar): every case prints that figure for its last pixel and the pixels at list entries
   2047 and 2048, and where it is two bars or less (SURFACE: the two list entries of a pixel carry upstream gradients of random sign)
   runs a one-hot backward for that pixel. At N = 524 289 (257 camera blocks: the second pass of cam_fin's loop) the sum cannot show one
   pixel; one-hot upstream gradients at list entries 0, 2047, 2048, 524 287, 524 288 do, and at N - 1 and 2048 for N = 2049 and 4097.
   The colour stage's large view gets one-hot runs at list entries 2048 and 524 288 on this module's own account; they are held to
   k 2^-24 B (samples_restatement: the bar that covers ONE pixel evaluated in float32, as k_cb_cam_bwd does).

Residuals of the unchanged library (MI355X) are recorded in profiles/samples_edges.md; every test prints its own.
"""
import numpy as np
import pytest

import samples_edges_inputs as inp
import samples_restatement as sr

pytestmark = pytest.mark.gpu

CS = 32                     # colour code length
_cache = {}


def _t(a, grad=False):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().requires_grad_(grad)


def _np(t):
    return t.detach().cpu().numpy()


def _same(a, b):
    a, b = _np(a), _np(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _w(a):
    return None if a is None else np.asarray(a).astype(np.float64)


def _samples_cfg(H, W, mode, number=1, clamp=None):
    """(cfg, K_inv, M): the two as the float32 values inside cfg, widened."""
    from distr import binding
    cfg = binding.make_samples_cfg((H, W), inp.intrinsic(H, W), inp.transform(), clamp, mode, number)
    Ki, M = inp.geometry(H, W)
    assert np.array(cfg.K_inv[:], dtype=np.float32).tobytes() == Ki.tobytes() and np.array(cfg.M[:], dtype=np.float32).tobytes() == M.tobytes()
    return cfg, _w(Ki), _w(M)


def _render_cfg(H, W):
    from distr import binding
    cfg = binding.make_cfg((H, W), inp.intrinsic(H, W), march_step=30, buffer_size=2, transform_matrix=inp.transform())
    Ki, M = inp.geometry(H, W)
    assert np.array(cfg.K_inv[:], dtype=np.float32).tobytes() == Ki.tobytes() and np.array(cfg.M[:], dtype=np.float32).tobytes() == M.tobytes()
    return cfg, _w(Ki), _w(M)


@pytest.fixture(scope='module')
def color_engine():
    """(engine of the synthetic colour decoder, its colour code (1, CS))."""
    from distr import fixture, functions
    Wc, bc, code = fixture.make_color_decoder_weights(color_size=CS)
    return functions.ColorEngine(device_index=0, weights=(Wc, bc)), code


def _codes(base, V, key):
    rs = np.random.RandomState(inp._seed('codes', key))
    return (base + 0.05 * np.abs(base).max() * rs.standard_normal((V, base.shape[1]))).astype(np.float32)


# ------------------------------------------------------------------------------------------ A. compaction
@pytest.mark.parametrize('hw', inp.COMPACTION_SIZES, ids=lambda s: '%dx%d' % s)
def test_depth_compaction(hw, engine):
    from distr import functions
    H, W = hw
    P = H * W
    cfg, _, _ = _samples_cfg(H, W, sr.SURFACE)
    for call in range(3):
        names = inp.call_patterns(call)
        depth = np.stack([inp.depth_pattern(n, P) for n in names])
        want_index, want_counts = sr.valid(depth)
        _, index, counts = functions.depth_samples_count(engine, cfg, _t(depth.reshape(3, H, W)))
        assert counts == want_counts, (hw, names, counts, want_counts)
        index = _np(index)
        for v in range(3):
            assert np.array_equal(index[v, :counts[v]], want_index[v]), (hw, names[v])


@pytest.mark.parametrize('hw', inp.COMPACTION_SIZES, ids=lambda s: '%dx%d' % s)
def test_color_compaction(hw, color_engine, fixture_decoder):
    """The colour stage's totals and index lists against nonzero(mask); masks hold 0 / 1 / 255. The image is zero off the mask."""
    from distr import functions
    eng, code = color_engine
    H, W = hw
    P = H * W
    cfg, _, _ = _render_cfg(H, W)
    RT = inp.cameras(3)
    z = _t(np.random.RandomState(inp._seed('z', P)).uniform(0.8, 2.0, (3, P)).astype(np.float32))
    for call in range(3):
        names = inp.call_patterns(call)
        mask = np.stack([inp.mask_pattern(n, P) for n in names])
        rgb, saved = functions.color_stage_forward(eng, cfg, _t(code), _t(fixture_decoder[2]), _t(RT[:, :, :3]), _t(RT[:, :, 3]), z, _t(mask), want_lists=True)
        totals, index = _np(saved['totals']), _np(saved['index'])
        for v in range(3):
            want = np.nonzero(mask[v])[0]
            assert totals[v] == want.size, (hw, names[v], totals[v], want.size)
            assert np.array_equal(index[v, :want.size], want), (hw, names[v])
        assert not rgb.reshape(3, P, 3)[_t(mask == 0)].any(), (hw, names)


# ------------------------------------------------------------------------------------------ B, C: the depth samples
def _samples_run(engine, latent, H, W, mode, number, case, per_view_codes, key):
    """One call through functions.*: count, forward, backward with the full upstream gradient; the library's own decoder forward and
    backward on the returned list. Everything the assertions need, kept for the tests that share the case."""
    import torch
    from distr import functions
    P = H * W
    cfg, Ki, M = _samples_cfg(H, W, mode, number)
    V = case['depth'].shape[0]
    d, index, counts = functions.depth_samples_count(engine, cfg, _t(case['depth'].reshape(V, H, W)))
    m = 2 if mode == sr.SURFACE else number
    seg = [m * c for c in counts]
    lat = _t(_codes(latent, V, key) if per_view_codes else latent, True)
    RT = _t(case['RT'], True)
    flat = np.concatenate([a.reshape(-1) for a in case['draws']])
    if mode == sr.SURFACE:
        per_view, xyz = functions.samples_call(engine, cfg, lat, RT, d, _t(case['normal']), _t(flat), index, counts)
        outs = [torch.cat(o) for o in per_view]
    else:
        outs, xyz = functions.freespace_call(engine, cfg, lat, RT, d, _t(flat), index, counts)
    out = torch.cat(outs)
    g = _t(inp.upstream(key, sum(seg)))
    g_lat, g_RT = torch.autograd.grad(out, (lat, RT), g, retain_graph=True)
    if per_view_codes:
        f = functions.mlp_eval_multi(engine, lat.detach(), xyz, seg, None).reshape(-1)
    else:
        f = functions.mlp_eval(engine, lat.detach(), xyz, None).reshape(-1)
    if mode == sr.SURFACE:                              # [f(p + o) - eta | f(p - o) + eta] per view, in f32
        parts, at = [], 0
        for c, eta in zip(counts, case['draws']):
            e = _t(eta)
            parts += [f[at:at + c] - e, f[at + c:at + 2 * c] + e]
            at += 2 * c
        f = torch.cat(parts)
    g_rows, g_xyz = functions.mlp_backward_multi(engine, lat.detach(), xyz, seg, g, None)
    index = _np(index)
    return dict(mode=mode, m=m, V=V, W=W, Ki=Ki, M=M, case=case, counts=counts, seg=seg, index=[index[v, :counts[v]] for v in range(V)],
                outs=outs, out=out, xyz=_np(xyz), lat=lat, RT=RT, f=f, g_lat=g_lat, g_RT=_np(g_RT), g_rows=g_rows, g_xyz=_np(g_xyz),
                per_view_codes=per_view_codes, engine=engine, key=key)


def _view_args(run, v):
    c = run['case']
    return (run['mode'], run['Ki'], run['M'], _w(c['RT'][v]), _w(c['depth'][v]), run['index'][v], run['W'])


def _check_points(run):
    at = 0
    for v in range(run['V']):
        c = run['case']
        want = sr.points(*_view_args(run, v), _w(None if c['normal'] is None else c['normal'][v]), _w(c['draws'][v]))
        got = run['xyz'][at:at + run['seg'][v]]
        at += run['seg'][v]
        assert got.shape == want.shape
        if want.size:
            err, bar = float(np.abs(got - want).max()), sr.points_bar(want)
            print('%s view %d (N %d): points differ from float64 by %.3e (bar %.3e)' % (run['key'], v, run['counts'][v], err, bar))
            assert err <= bar, (run['key'], v, err, bar)
    assert at == run['xyz'].shape[0]
    assert _same(run['out'], run['f']), '%s: the outputs are not the decoder on the returned list' % (run['key'],)
    for v in range(run['V']):
        assert run['outs'][v].numel() == run['seg'][v]


def _ratio(err, bar):
    """Largest err / bar over the entries; an entry whose bar is zero has to be exact."""
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(np.nanmax(np.where(bar > 0, err / bar, np.where(err > 0, np.inf, 0.0))))


def _camera_check(tag, run, v, g_xyz_view, got, one_hot=False):
    """got (3, 4) against the closed form on g_xyz_view, entry by entry at the rounding bar k 2^-24 A. Returns the terms and the bar."""
    c = run['case']
    N = run['counts'][v]
    ct = sr.camera_terms(*_view_args(run, v), _w(g_xyz_view), _w(c['draws'][v]))
    bar, bar_b = (sr.rounding_bar(ct[key], 'samples', N) for key in ('A_RT', 'B_RT'))
    err = np.abs(got - ct['g_RT'])
    print('%s view %d (N %d, k %d): largest |g_RT - closed form| %.3f bars (%.3e A); with B for A %.3f bars' % (
        tag, v, N, sr.rounding_count('samples', N), _ratio(err, bar), float((err / np.maximum(ct['A_RT'], 1e-300)).max()), _ratio(err, bar_b)))
    assert np.all(err <= bar), (tag, v, _ratio(err, bar), _ratio(err, bar_b))
    if one_hot:
        assert np.abs(ct['g_RT']).max() > 0 and np.abs(got).max() > 0, (tag, 'the one-hot gradient reaches no camera entry')
    return ct, bar


def _check_camera(run):
    g_lat = _np(run['g_lat'])
    rows = _np(run['g_rows'])
    if run['per_view_codes'] or run['V'] == 1:
        assert g_lat.tobytes() == rows.tobytes(), '%s: g_latent is not the decoder backward\'s rows' % (run['key'],)
    at = 0
    for v in range(run['V']):
        N, n = run['counts'][v], run['seg'][v]
        ct, bar = _camera_check(run['key'], run, v, run['g_xyz'][at:at + n], run['g_RT'][v])
        at += n
        if N == 0:
            assert not run['g_RT'][v].any() and not rows[v].any(), '%s: the empty view has a gradient' % (run['key'],)
            continue
        # the last pixel and the pixels around list entry 2048: either the sum fails without the pixel (its share of some entry is above
        # twice the bar; the sum's own residual is below one bar), or a one-hot run shows it alone (SURFACE: the two list entries of a
        # pixel carry upstream gradients of random sign and may cancel)
        for i in sorted({N - 1, min(N - 1, sr.MTILE - 1), min(N - 1, sr.MTILE)}):
            share = sr.pixel_share(ct, i, bar)
            print('%s view %d: list pixel %d holds %.1f bars of its largest entry' % (run['key'], v, i, share))
            if share <= 2.0:
                _one_hot(run, v, [i])


def _one_hot(run, v, entries):
    """Backward with the upstream gradient on ONE list entry of view v (entry i of draw 0): g_RT is that pixel's term alone."""
    import torch
    from distr import functions
    off = sum(run['seg'][:v])
    for i in sorted(set(entries)):
        assert inp.off_axis(run['Ki'], run['index'][v][i], run['W']), (run['key'], i, 'a one-hot pixel next to the principal point')
        g = torch.zeros(sum(run['seg']), dtype=torch.float32, device='cuda')
        g[off + i] = float(inp.upstream(('one-hot', run['key'], i), 1)[0])
        g_RT = _np(torch.autograd.grad(run['out'], run['RT'], g, retain_graph=True)[0])
        g_xyz = _np(functions.mlp_backward_multi(run['engine'], run['lat'].detach(), _t(run['xyz']), run['seg'], g, None, need_latent=False)[1])
        assert np.abs(g_xyz[off + i]).max() > 0 and np.count_nonzero(np.abs(g_xyz).max(1)) == 1
        _camera_check('%s one-hot %d' % (run['key'], i), run, v, g_xyz[off:off + run['seg'][v]], g_RT[v], one_hot=True)
        assert not np.delete(g_RT, v, 0).any()


def _point_run(engine, fixture_decoder, case):
    key = ('points',) + tuple(case)
    if key not in _cache:
        mode, number, N = case
        _cache[key] = _samples_run(engine, fixture_decoder[2], inp.H_B, inp.W_B, mode, number, inp.point_case(mode, number, [N]), False, key)
    return _cache[key]


def _batch_run(engine, fixture_decoder, mode, number, name):
    key = ('batch', mode, number, name)
    if key not in _cache:
        _cache[key] = _samples_run(engine, fixture_decoder[2], inp.H_B, inp.W_B, mode, number, inp.point_case(mode, number, inp.BATCHES[name]), True, key)
    return _cache[key]


_case_id = lambda c: '%s-%d-%d' % c
BATCH_CASES = [(mode, number, name) for mode, number in ((sr.SURFACE, 1), (sr.FREESPACE, 3)) for name in sorted(inp.BATCHES)]


@pytest.mark.parametrize('case', inp.POINT_CASES, ids=_case_id)
def test_point_list_and_epilogue(case, engine, fixture_decoder):
    run = _point_run(engine, fixture_decoder, case)
    assert run['counts'] == [case[2]]
    _check_points(run)


@pytest.mark.parametrize('case', inp.POINT_CASES, ids=_case_id)
def test_camera_gradient(case, engine, fixture_decoder):
    _check_camera(_point_run(engine, fixture_decoder, case))


@pytest.mark.parametrize('case', [c for c in inp.POINT_CASES if c[2] in (2049, 4097)], ids=_case_id)
def test_camera_gradient_one_hot(case, engine, fixture_decoder):
    N = case[2]
    _one_hot(_point_run(engine, fixture_decoder, case), 0, (N - 1, sr.MTILE))


@pytest.mark.parametrize('case', BATCH_CASES, ids=lambda c: '%s-%d-%s' % c)
def test_batch_point_list_and_epilogue(case, engine, fixture_decoder):
    """Three views with a code each: (4097, 300, 2048) valid pixels, and (257, 0, 2049) -- the empty view owns no list entries."""
    run = _batch_run(engine, fixture_decoder, *case)
    assert run['counts'] == list(inp.BATCHES[case[2]])
    _check_points(run)


@pytest.mark.parametrize('case', BATCH_CASES, ids=lambda c: '%s-%d-%s' % c)
def test_batch_camera_gradient(case, engine, fixture_decoder):
    """Views that need 3, 1 and 1 camera blocks (nblk_cam comes from the largest, cam_fin takes each view's own), and 1, 0 and 2."""
    _check_camera(_batch_run(engine, fixture_decoder, *case))


def _big_run(engine, fixture_decoder):
    if 'big' not in _cache:
        H, W = inp.BIG_HW
        _cache['big'] = _samples_run(engine, fixture_decoder[2], H, W, sr.FREESPACE, 1, inp.big_case(), False, ('big',))
    return _cache['big']


def test_large_view_full_gradient(engine, fixture_decoder):
    """3 x 174 763 pixels, all valid: 257 pixel blocks (a second round of the top scan) and 257 camera blocks (a second pass of cam_fin)."""
    run = _big_run(engine, fixture_decoder)
    assert run['counts'] == [inp.BIG_HW[0] * inp.BIG_HW[1]] and np.array_equal(run['index'][0], np.arange(run['counts'][0]))
    _check_points(run)
    g_lat, rows = _np(run['g_lat']), _np(run['g_rows'])
    assert g_lat.tobytes() == rows.tobytes()
    _camera_check('big', run, 0, run['g_xyz'], run['g_RT'][0])


def test_large_view_one_hot(engine, fixture_decoder):
    _one_hot(_big_run(engine, fixture_decoder), 0, inp.ONE_HOT_BIG)


# ------------------------------------------------------------------------------------------ B, C: the colour stage without lights
def _color_run(color_engine, fixture_decoder, H, W, masks, key):
    import torch
    from distr import functions
    eng, code = color_engine
    P, V = H * W, masks.shape[0]
    cfg, Ki, M = _render_cfg(H, W)
    rs = np.random.RandomState(inp._seed('color', key))
    z = rs.uniform(0.8, 2.0, (V, P)).astype(np.float32)
    RT = inp.cameras(V)
    cc, sc = _t(_codes(code, V, key), True), _t(_codes(fixture_decoder[2], V, key), True)
    R, T = _t(RT[:, :, :3], True), _t(RT[:, :, 3], True)
    zt, mt = _t(z), _t(masks)
    rgb = functions.ColorStageFunction.apply(cc, sc, R, T, None, eng, cfg, zt, mt, None, None, False)
    g = _t(inp.upstream(key, V * P * 3).reshape(V, H, W, 3))
    g_c, g_s, g_R, g_T = torch.autograd.grad(rgb, (cc, sc, R, T), g, retain_graph=True)
    rgb2, saved = functions.color_stage_forward(eng, cfg, cc.detach(), sc.detach(), R.detach(), T.detach(), zt, mt, want_lists=True)
    assert _same(rgb, rgb2)
    counts = [int(c) for c in _np(saved['totals'])]
    index = [_np(saved['index'][v, :counts[v]]).astype(np.int64) for v in range(V)]
    xyz = torch.cat([saved['xyz'][v, :counts[v]] for v in range(V)])
    g_list = torch.cat([g[v].reshape(P, 3)[_t(index[v])] for v in range(V)])
    col = functions.color_eval_multi(eng, cc.detach(), sc.detach(), xyz, counts)
    g_rows, g_xyz = functions.color_backward_multi(eng, cc.detach(), sc.detach(), xyz, counts, g_list)
    return dict(V=V, P=P, W=W, Ki=Ki, M=M, RT=RT, z=z, masks=masks, counts=counts, index=index, rgb=_np(rgb).reshape(V, P, 3), xyz=_np(xyz), col=_np(col),
                g_c=_np(g_c), g_s=_np(g_s), g_R=_np(g_R), g_T=_np(g_T), g_rows=_np(g_rows), g_xyz=_np(g_xyz), key=key,
                graph=(rgb, R, T), codes=(cc.detach(), sc.detach()), xyz_t=xyz, engine=eng)


def _color_one_hot(run, entries):
    """Backward of a one-view run with the upstream gradient on the three colours of ONE list entry: g_R, g_T are that pixel's term alone.
    Added on this module's own account (the sum over 524 289 pixels cannot show the one pixel of the 257th block), so held to k 2^-24 B."""
    import torch
    from distr import functions
    rgb, R, T = run['graph']
    N, P = run['counts'][0], run['P']
    for i in entries:
        pix = int(run['index'][0][i])
        g = torch.zeros(1, P, 3, dtype=torch.float32, device='cuda')
        g[0, pix] = _t(inp.upstream(('color one-hot', run['key'], i), 3))
        g_R, g_T = torch.autograd.grad(rgb, (R, T), g.reshape(rgb.shape), retain_graph=True)
        g_list = torch.zeros(N, 3, dtype=torch.float32, device='cuda')
        g_list[i] = g[0, pix]
        g_xyz = _np(functions.color_backward_multi(run['engine'], *run['codes'], run['xyz_t'], [N], g_list, need_codes=False)[1])
        assert np.abs(g_xyz[i]).max() > 0 and np.count_nonzero(np.abs(g_xyz).max(1)) == 1
        ct = sr.camera_terms_color(run['Ki'], run['M'], _w(run['RT'][0, :, :3]), _w(run['RT'][0, :, 3]), _w(run['z'][0]), run['index'][0], run['W'], _w(g_xyz))
        got = np.concatenate([_np(g_R).reshape(3, 3), _np(g_T).reshape(3, 1)], 1)
        err = np.abs(got - ct['g_RT'])
        bar, bar_b = (sr.rounding_bar(ct[key], 'color', N) for key in ('A_RT', 'B_RT'))
        print('%s one-hot %d: largest |g_R, g_T - closed form| %.3f bars; with B for A %.3f bars' % (run['key'], i, _ratio(err, bar), _ratio(err, bar_b)))
        assert np.all(err <= bar_b) and np.abs(got).max() > 0 and np.abs(ct['g_RT']).max() > 0, (run['key'], i, _ratio(err, bar_b))


def _check_color(run, share=True):
    at = 0
    for v in range(run['V']):
        N = run['counts'][v]
        want_index = np.nonzero(run['masks'][v])[0]
        assert N == want_index.size and np.array_equal(run['index'][v], want_index)
        R, T = _w(run['RT'][v, :, :3]), _w(run['RT'][v, :, 3])
        got, gx = run['xyz'][at:at + N], run['g_xyz'][at:at + N]
        want = sr.surface_points(run['Ki'], run['M'], R, T, _w(run['z'][v]), want_index, run['W'])
        if N:
            err, bar = float(np.abs(got - want).max()), sr.points_bar(want)
            print('%s view %d (N %d): points differ from float64 by %.3e (bar %.3e)' % (run['key'], v, N, err, bar))
            assert err <= bar
        assert run['rgb'][v][want_index].tobytes() == run['col'][at:at + N].tobytes(), 'the image is not the colour decoder on the returned list'
        assert not np.delete(run['rgb'][v], want_index, 0).any()
        ct = sr.camera_terms_color(run['Ki'], run['M'], R, T, _w(run['z'][v]), want_index, run['W'], _w(gx))
        got_RT = np.concatenate([run['g_R'][v].reshape(3, 3), run['g_T'][v].reshape(3, 1)], 1)
        bar, bar_b = (sr.rounding_bar(ct[key], 'color', N) for key in ('A_RT', 'B_RT'))
        err = np.abs(got_RT - ct['g_RT'])
        print('%s view %d (N %d, k %d): largest |g_R, g_T - closed form| %.3f bars (%.3e A); with B for A %.3f bars' % (
            run['key'], v, N, sr.rounding_count('color', N), _ratio(err, bar), float((err / np.maximum(ct['A_RT'], 1e-300)).max()), _ratio(err, bar_b)))
        assert np.all(err <= bar), (run['key'], v, _ratio(err, bar))
        rows = np.concatenate([run['g_s'][v], run['g_c'][v]])
        assert rows.tobytes() == run['g_rows'][v].tobytes(), '%s: the code gradient is not the colour decoder backward\'s row' % (run['key'],)
        if N == 0:
            assert not got_RT.any() and not rows.any()
        elif share:
            for i in sorted({N - 1, min(N - 1, sr.MTILE - 1), min(N - 1, sr.MTILE)}):
                print('%s view %d: list pixel %d holds %.1f bars of its largest entry' % (run['key'], v, i, sr.pixel_share(ct, i, bar)))
                assert sr.pixel_share(ct, i, bar) > 2.0, (run['key'], v, i)     # the sum fails without this pixel
        at += N


def _masks(counts, key):
    rs = np.random.RandomState(inp._seed('masks', key))
    P = inp.H_B * inp.W_B
    out = np.zeros((len(counts), P), dtype=np.uint8)
    for v, n in enumerate(counts):
        out[v, rs.choice(P, n, replace=False)] = rs.choice(np.array([1, 255], dtype=np.uint8), n)
    return out


@pytest.mark.parametrize('counts', [(N,) for N in inp.NS] + [inp.BATCHES[k] for k in sorted(inp.BATCHES)], ids=lambda c: '-'.join(str(n) for n in c))
def test_color_stage_points_and_camera_gradient(counts, color_engine, fixture_decoder):
    key = ('color',) + tuple(counts)
    _check_color(_color_run(color_engine, fixture_decoder, inp.H_B, inp.W_B, _masks(counts, key), key))


def test_color_stage_large_view(color_engine, fixture_decoder):
    """The 3 x 174 763 view, every pixel on the mask: 257 camera blocks in k_cb_cam_fin; the 257th holds list entry 524 288 alone."""
    H, W = inp.BIG_HW
    run = _color_run(color_engine, fixture_decoder, H, W, np.full((1, H * W), 255, dtype=np.uint8), ('color-big',))
    _check_color(run, share=False)
    _color_one_hot(run, (sr.MTILE, H * W - 1))
